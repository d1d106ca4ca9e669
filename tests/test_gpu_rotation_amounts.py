"""Every blind-rotation kernel on PLANTED rotation amounts, word for word against the CPU oracle.

Each of these kernels treats a step whose amounts are zero as a special case, and a skipped step is not a no-op: the whole-CU kernels
re-issue the next step's key request, the kernels with several bootstraps per workgroup still meet the workgroup's barriers, and
k_blind_rotate_glwe alternates its landing sets by the steps a bootstrap EXECUTES.  The kernels of two key bits per step also form
e2 = (e0 + e1) mod 2N and take a wave-uniform sign from each exponent.  Random toy ciphertexts never skip a single step (both
amounts of a pair are zero with probability 1 / (2N)^2), so the amounts are chosen here: tests/helpers.py, planted_amount_rows --
first, last, interleaved and all-but-one steps skipped, against e0 + e1 = 2N, e = N, (0, x), (x, 0) and wrap-around.

No key is touched.  At bits = log2(2N) fbs_refresh_compact_dev unpacks its fields, unrounded, into the rows the blind rotation
reads and calls the same launcher selection as fbs_bootstrap_batch_dev, through the identity table: `pack` of the chosen fields runs
any kernel on exactly those amounts.  One case per entry of fbs_kernel_catalog that is a rotation, at the recipe that reaches it
(tests/helpers.py:recipe; tests/test_select.py checks the recipes on the CPU), n = 16 steps; row f of a launch is planted row
f % 60, and 5 lists are coprime with 1, 2, 3 and 4 bootstraps per workgroup (3: k_blind_rotate_glwe at k = 3, N <= 512), so every
list meets every sub-slot and the ragged last workgroup.  Semantic rows must decrypt to their message on every entry but the six
whose template arguments force one gadget level of at most 9 bits (tests/helpers.py, planted_output_margin).  tests/test_rotation_amounts_reference.py checks the lists and the reference itself without a GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (PLANTED_DEFAULT_KNOBS, PLANTED_MARGIN, PLANTED_ROWS, PLANTED_STEPS, planted_amount_rows, planted_output_margin,
                           planted_set, recipe)
from tests.test_gpu_compact import pack
from tests.test_gpu_device_io import dev, host

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A                                    # (above q: no ciphertext word)
FAMILIES = {"k_blind_rotate", "k_blind_rotate_pairs", "k_blind_rotate_cu", "k_blind_rotate_cu_pairs", "k_blind_rotate_pairs_k2",
            "k_blind_rotate_cu_k2", "k_blind_rotate_glwe"}


def rotation_entries():
    from tfhe_fbs_map_amd import _native
    return [k for k in _native.kernel_catalog() if k.startswith("k_blind_rotate")]   # (the key-switch entries are no rotations)


def pytest_generate_tests(metafunc):
    if "kernel_name" in metafunc.fixturenames:
        metafunc.parametrize("kernel_name", rotation_entries())


def set_of(rec):
    return (rec["log_n"], rec.get("k", 1), rec["l"], rec["beta"], rec["group"])


@pytest.fixture(scope="module")
def planted():
    """per parameter set: context, oracle on the context's keys, the 60 planted rows, their messages and the oracle's 60 outputs
    (computed once, never written to)"""
    from tfhe_fbs_map_amd import Params, _native as nat
    made = {}

    def get(log_n, k, l, beta, group):
        key = (log_n, k, l, beta, group)
        if key not in made:
            prm = planted_set(*key)                              # (n = 16 at every size: key generation at N = 4096 stays under a second)
            ctx = nat.Context(Params(**prm), seed=33)
            keys = ctx.export_keys()
            o = orc.Oracle(prm, seed=33, keygen=False)
            o.set_keys(**keys)
            fields, meta = planted_amount_rows(1 << log_n, PLANTED_STEPS, group, keys["sk_lwe"], prm["p_msg"])
            tv, post = o.build_tv(list(range(prm["p_msg"])))     # the identity table
            with ThreadPoolExecutor(8) as pool:                  # (the oracle's calls are re-entrant and run outside the interpreter's lock)
                ref = np.stack(list(pool.map(lambda row: o.sample_extract(o.blind_rotate(row, tv), post), fields)))
            ref.setflags(write=False)
            made[key] = (ctx, o, fields, np.array(meta["msg"]), ref, planted_output_margin(prm) >= PLANTED_MARGIN)
        return made[key]

    yield get
    for entry in made.values():
        entry[0].close()


def refresh_planted(ctx, fields, count):
    """rows f % 60 of `fields`, f < count, through fbs_refresh_compact_dev at log2(2N) bits -> [count][D + 1]; the buffer is two rows
    longer than the launch, and those rows stay as they were"""
    import torch
    b = ctx.params.log_n_poly + 1
    words = pack(fields[np.arange(count) % PLANTED_ROWS].astype(np.uint64), b)
    assert words.shape == (count, ctx.compact_words(b))
    d_c = torch.full((count + 2, ctx.params.ct_words), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.refresh_compact_dev(dev(words).data_ptr(), count, d_c.data_ptr(), bits=b)
    ctx.sync()
    out = host(d_c)
    assert (out[count:] == SENTINEL).all(), "wrote past the last ciphertext"
    return out[:count]


def test_every_rotation_entry_has_a_case():
    names = rotation_entries()
    missing = [k for k in names if recipe(k) is None]
    assert not missing, missing
    assert len(set(names)) == len(names) >= 155
    assert {k.split("<")[0] for k in names} == FAMILIES


def test_planted_amounts_against_the_oracle(planted, kernel_name):
    rec = recipe(kernel_name)
    assert rec is not None, "no recipe reaches %s: it would ship without planted amounts" % kernel_name
    ctx, o, fields, msg, ref, usable = planted(*set_of(rec))
    ctx.tune(**{**PLANTED_DEFAULT_KNOBS, **rec["knobs"]})        # (the context is shared: the knobs are set per case)
    count = rec["count"]
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = refresh_planted(ctx, fields, count)
    launched = ctx.profile_kernels()
    ctx.profile(False)
    assert kernel_name in launched, (kernel_name, sorted(launched))
    rows = np.arange(count) % PLANTED_ROWS
    wrong = np.flatnonzero((got != ref[rows]).any(axis=1))       # ALL rows, word for word
    assert wrong.size == 0, (kernel_name, "ciphertexts", wrong[:8].tolist(), "lists", sorted(set((wrong % 5).tolist())))
    assert got.max() < orc.Q
    semantic = msg[rows] >= 0
    dec = ctx.decrypt(got)
    assert np.array_equal(dec, o.decrypt(ref)[rows])
    if usable:
        assert np.array_equal(dec[semantic], msg[rows][semantic]), kernel_name


@pytest.mark.parametrize("shape", [(10, 1, 3, 7, 1), (11, 1, 1, 20, 2), (10, 2, 1, 20, 2), (9, 3, 2, 8, 2), (8, 4, 2, 8, 2), (12, 1, 2, 10, 2)])
def test_the_rows_the_rotation_reads_are_the_planted_ones(planted, shape):
    """the construction itself: what the unpack of fbs_refresh_compact_dev leaves for the blind rotation (fbs_compact_fields_dev is
    that unpack alone) at log2(2N) bits is the planted fields, every one of them"""
    import torch
    ctx, _, fields, _, _, _ = planted(*shape)
    b = ctx.params.log_n_poly + 1
    d_f = torch.full((PLANTED_ROWS, ctx.params.n + 1), 0x5A5A, dtype=torch.int32, device="cuda")
    ctx.compact_fields_dev(dev(pack(fields.astype(np.uint64), b)).data_ptr(), PLANTED_ROWS, d_f.data_ptr(), bits=b)
    ctx.sync()
    assert np.array_equal(host(d_f, np.uint32), fields)


def test_planted_amounts_through_a_program(planted):
    """The refresh group of fbs_eval_sources (csrc/fbs_eval.cpp) reads the same amounts: a chain whose one input is an
    FBS_SRC_COMPACT source at log2(2N) bits carrying the planted rows, on the k = 2, N = 1024 set of two key bits per step.  The
    program returns its input wire, a copy of it (1 x the input) and the identity bootstrap of the copy: the first level's inputs
    are the direct refresh, word for word, and the level itself is the oracle's bootstrap of them -- on the twelve-wave kernel and
    on the kernel of three waves per bootstrap."""
    from tfhe_fbs_map_amd import _native as nat
    ctx, o, fields, msg, ref, usable = planted(10, 2, 1, 20, 2)
    assert usable
    p, b, T = ctx.params.p_msg, ctx.params.log_n_poly + 1, PLANTED_ROWS
    identity = list(range(p))
    prog = nat.Program(ctx, ctx.tvset([identity]), 1, kind=[0, 1], arg0=[0, 1], arg1=[1, 0], const_coef=[0, 0], term_coef=[1],
                       term_src=[0], out_wire=[0, 1, 2])
    words = pack(fields.astype(np.uint64), b)
    level, _ = o.bootstrap_batch(ref, [identity])
    semantic = msg >= 0
    for knobs, kernel in ((dict(), "k_blind_rotate_cu_k2"), (dict(br_k2_shape=3), "k_blind_rotate_pairs_k2<10,1>")):
        ctx.tune(**{**PLANTED_DEFAULT_KNOBS, **knobs})
        ctx.profile(True)
        ctx.profile_read(reset=True)
        got = prog.eval_sources([("compact", words, b)], T)
        launched = ctx.profile_kernels()
        ctx.profile(False)
        assert kernel in launched and launched[kernel]["launches"] >= 2, (kernel, launched)   # the refresh group and the level
        assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref), kernel
        assert np.array_equal(got[0], refresh_planted(ctx, fields, T)), kernel
        assert np.array_equal(got[2], level), kernel
        assert np.array_equal(ctx.decrypt(got[2])[semantic], msg[semantic])
    ctx.tune(**PLANTED_DEFAULT_KNOBS)
