"""Every kernel instantiation the launchers can pick, one by one, against the CPU oracle.

`fbs_kernel_catalog` lists them (csrc/fbs_select.cpp).  For each name tests/helpers.py:recipe knows a parameter set, a batch
size and the launcher knobs that lead to it (tests/test_select.py checks that on the CPU, through the selection itself); this module
runs the launch, asserts that the launcher really took that instantiation (the per-kernel profile table), and compares the
output ciphertexts with the oracle's word for word -- all of them for small batches, a subsample that covers both ends and
the crafted ciphertexts for large ones.  A catalog entry without a recipe here fails the suite, so a new launcher branch
cannot ship unchecked."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import CUS, recipe

pytestmark = pytest.mark.gpu

TABLES = [[0, 1, 1, 0, 1, 0, 0], [0, 1, 2, 3, 2, 1, 0], [0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1]]
def catalog():
    from tfhe_fbs_map_amd import _native
    return _native.kernel_catalog()


def pytest_generate_tests(metafunc):
    if "kernel_name" in metafunc.fixturenames:
        metafunc.parametrize("kernel_name", catalog())


def run_case(name, rec):
    from tfhe_fbs_map_amd import Params, _native as nat
    n = 8 if rec["log_n"] < 12 else 4
    prm = Params(n=n, log_n_poly=rec["log_n"], k=rec.get("k", 1), l_bsk=rec["l"], beta_bsk=rec["beta"], t_ksk=4, gamma_ksk=4 if rec["log_n"] < 12 else 3, p_msg=7,
                 sigma_lwe=1 << 6, sigma_glwe=1 << 4, bsk_group=rec["group"])
    ctx, o = nat.Context(prm, seed=21), orc.Oracle(prm, seed=21)
    ctx.tune(**rec["knobs"])
    count = rec["count"]
    rng = np.random.default_rng(count)
    ids = rng.integers(0, len(TABLES), count).astype(np.uint32)
    msgs = np.array([rng.integers(0, len(TABLES[i])) for i in ids])
    cts = ctx.encrypt(msgs, nonce0=3)
    crafted = sorted({1 % count, count // 2, count - 2})
    cts[crafted[0], :-1] = 0                                 # a trivial ciphertext: every rotation amount is zero
    cts[crafted[-1], :] = orc.Q - 1                          # maximal residues
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = ctx.bootstrap_batch(ctx.tvset(TABLES), cts, ids)
    launched = ctx.profile_kernels()
    assert name in launched, (name, sorted(launched))
    if count <= 64:
        pick = np.arange(count)
    else:                                                    # both ends, the crafted ones, every sub-slot of the first workgroups, a spread
        pick = np.unique(np.concatenate([np.arange(8), np.arange(count - 8, count), crafted, rng.integers(0, count, 12)]))
    ref, _ = o.bootstrap_batch(cts[pick], TABLES, ids[pick])
    assert np.array_equal(got[pick], ref), name
    assert got.max() < orc.Q
    ctx.close()


def test_every_catalog_entry_has_a_recipe():
    missing = [k for k in catalog() if recipe(k) is None]
    assert not missing, missing
    assert len(set(catalog())) == len(catalog()) >= 160


def test_instantiation_against_the_oracle(kernel_name):
    run_case(kernel_name, recipe(kernel_name))


def test_cu_count_matches_the_recipes():
    from tfhe_fbs_map_amd import Params, _native as nat
    ctx = nat.Context(Params(n=4, log_n_poly=8, p_msg=7), seed=1)
    assert ctx.stat("cu_count") == CUS, "the batch sizes of the recipes assume 256 CUs"
