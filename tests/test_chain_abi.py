"""Chained evaluation without a GPU (include/fbs_exec.h, "chained evaluation"): the new entries are declared, exported and bound;
output files carry out_norm2 and files without it still load; `plan_chain` resolves names and refuses what it must; the noise rules
(`params.refresh_*`) hold the link to the consuming program's margin at every parameter set the golden fixtures are chosen at; and
`client_choice` with no further programs is the choice a Client always made."""
import ctypes

import numpy as np
import pytest

from tests.test_compact_abi import _fixture_choices

ENTRIES = ("fbs_compact_fields_dev", "fbs_refresh_compact_dev", "fbs_eval_sources")
ADDER = "adder8__search_p15"
A_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    for meth in ("compact_fields_dev", "refresh_compact_dev"):
        assert callable(getattr(_native.Context, meth)), meth
    assert callable(_native.Program.eval_sources)
    # the ctypes image of fbs_input_src: kind, bits, refresh, (pad), nonce0, data
    assert ctypes.sizeof(_native._InputSrc) == 32 and _native._InputSrc.nonce0.offset == 16 and _native._InputSrc.data.offset == 24


def _adder():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(ADDER)
    return parse_fbs(rec["fbs"], inputs=rec["program_inputs"])


def _key_params(env):
    from tfhe_fbs_map_amd import ExecConfig
    from tfhe_fbs_map_amd.split import client_choice
    return client_choice(env, ExecConfig(), [env])


def test_outputs_round_trip_with_and_without_out_norm2(tmp_path):
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedOutputs
    rng = np.random.default_rng(0)
    cts = rng.integers(0, 2**46, (3, 5, 17), dtype=np.uint64)
    words = rng.integers(0, 2**63, (3, 5, 4), dtype=np.uint64)
    n2 = np.array([1.0, 0.0, 5.0])
    for obj in (EncryptedOutputs(["x", "y", "z"], 5, cts, bytes(range(8)), n2), CompactOutputs(["x", "y", "z"], 5, 11, words, bytes(8), n2),
                EncryptedOutputs(["x", "y", "z"], 5, cts, bytes(8)), CompactOutputs(["x", "y", "z"], 5, 11, words, bytes(8))):
        path = str(tmp_path / "o.npz")
        obj.save(path)
        back = type(obj).load(path)
        if obj.out_norm2 is None:   # a file of the format before chains: loads as it did, with no record
            assert back.out_norm2 is None
            with np.load(path) as z:
                assert "out_norm2" not in z.files
        else:
            assert np.array_equal(back.out_norm2, n2)
        assert back.output_names == obj.output_names and back.T == 5 and back.fingerprint == obj.fingerprint
    bad = CompactOutputs(["x", "y", "z"], 5, 11, words, bytes(8), np.array([1.0, 2.0]))
    bad.save(str(tmp_path / "bad.npz"))
    with pytest.raises(ValueError, match="out_norm2"):
        CompactOutputs.load(str(tmp_path / "bad.npz"))


def _sources(prm, T=4, fp=bytes(8), out_norm2=1.0, compact=True):
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedInputs, EncryptedOutputs, compact_words
    names = [f"s{i}" for i in range(8)] + ["cout"]
    b = prm.log_n_poly + 1
    if compact:
        acc = CompactOutputs(names, T, b, np.zeros((9, T, compact_words(prm, b)), np.uint64), fp, np.full(9, float(out_norm2)))
    else:
        acc = EncryptedOutputs(names, T, np.zeros((9, T, prm.ct_words), np.uint64), fp, np.full(9, float(out_norm2)))
    fresh = EncryptedInputs([f"b{i}" for i in range(8)], T, 100, np.zeros((8, T), np.uint64), fp)
    return acc, fresh


def test_plan_chain_resolves_names():
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    acc, fresh = _sources(prm)
    links, T = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    assert T == 4 and [ln.name for ln in links] == env.lower()["input_names"]
    for i in range(8):
        assert (links[i].kind, links[i].source, links[i].index, links[i].refresh) == ("compact", 0, i, True)
        assert (links[8 + i].kind, links[8 + i].source, links[8 + i].index, links[8 + i].refresh) == ("seeded", 1, i, False)
    # a full link from a bootstrap output goes in as it is; from a linear combination (out_norm2 > 1) it is refreshed
    for o2, refresh in ((1.0, False), (0.0, False), (2.0, True)):
        acc, fresh = _sources(prm, out_norm2=o2, compact=False)
        links, _ = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
        assert all(ln.kind == "full" and ln.refresh == refresh for ln in links[:8]), o2
    # one source holding everything, in another order of sources
    acc, fresh = _sources(prm)
    links, _ = plan_chain(prm, fuse, bytes(8), env, [fresh, acc], rename=A_FROM_S)
    assert links[0].source == 1 and links[8].source == 0


def test_plan_chain_refusals():
    from tfhe_fbs_map_amd import ExecConfig
    from tfhe_fbs_map_amd.params import choose_params
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedInputs, plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    acc, fresh = _sources(prm)
    with pytest.raises(ValueError, match="no source holds"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh])
    with pytest.raises(ValueError, match="no source holds"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename={**A_FROM_S, "a3": "nothing"})
    with pytest.raises(ValueError, match="not inputs"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename={**A_FROM_S, "zz": "s0"})
    with pytest.raises(ValueError, match="ambiguous"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh, acc], rename=A_FROM_S)
    twice = EncryptedInputs(["b0", "b0"], 4, 0, np.zeros((2, 4), np.uint64), bytes(8))
    with pytest.raises(ValueError, match="ambiguous"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh, twice], rename=A_FROM_S)
    other, _ = _sources(prm, fp=bytes(range(8)))
    with pytest.raises(ValueError, match="another server key"):
        plan_chain(prm, fuse, bytes(8), env, [other, fresh], rename=A_FROM_S)
    longer, _ = _sources(prm, T=5)
    with pytest.raises(ValueError, match="T = 4 samples where the others have 5"):
        plan_chain(prm, fuse, bytes(8), env, [longer, fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="cannot be evaluated"):
        plan_chain(prm.replace(p_msg=3), fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    old = CompactOutputs(acc.output_names, 4, acc.bits, acc.words, bytes(8))
    with pytest.raises(ValueError, match="saved without out_norm2"):
        plan_chain(prm, fuse, bytes(8), env, [old, fresh], rename=A_FROM_S)
    narrow = CompactOutputs(acc.output_names, 4, acc.bits + 1, acc.words, bytes(8), acc.out_norm2)
    with pytest.raises(ValueError, match="do not fit"):
        plan_chain(prm, fuse, bytes(8), env, [narrow, fresh], rename=A_FROM_S)
    noisy, _ = _sources(prm, out_norm2=1e4)
    with pytest.raises(ValueError, match="refresh would keep"):
        plan_chain(prm, fuse, bytes(8), env, [noisy, fresh], rename=A_FROM_S)
    # a key chosen for a program of norm2 1 leaves the adder (norm2 70) below ExecConfig().min_margin
    small = choose_params(prm.p_msg, 1.0, glwe_dims=(1, 2, 3))
    acc1, fresh1 = _sources(small)
    with pytest.raises(ValueError, match="own margin"):
        plan_chain(small, False, bytes(8), env, [acc1, fresh1], rename=A_FROM_S)
    assert ExecConfig().min_margin == 6.0


def test_refresh_margin_rules_on_every_fixture_set():
    from tfhe_fbs_map_amd.params import (DEFAULT_GLWE_DIMS, choose_params, compact_output_skew, margin_sigmas, refresh_input_variance,
                                         refresh_margin, refresh_margin_needed, variances)
    pairs = _fixture_choices()
    assert len(pairs) > 10
    for p, norm2 in pairs:
        try:
            prm = choose_params(p, norm2, glwe_dims=DEFAULT_GLWE_DIMS)
        except ValueError:
            prm = choose_params(p, norm2, floor_margin=4.0, glwe_dims=DEFAULT_GLWE_DIMS)
        b = prm.log_n_poly + 1
        skewed = margin_sigmas(prm, 1.0) * (1 - 4 * p * compact_output_skew(prm))
        assert refresh_margin(prm, b, 1.0) == pytest.approx(skewed, rel=1e-9, abs=1e-9), (p, norm2)
        assert refresh_margin(prm, None, 1.0) == pytest.approx(skewed, rel=1e-9, abs=1e-9), (p, norm2)
        # at w = log2(2N), out_norm2 = 1 every program's link is admitted
        assert refresh_margin(prm, b, 1.0) >= refresh_margin_needed(prm, norm2) * (1 - 1e-12), (p, norm2)
        # wider compact links carry one more modulus switch; noisier producers leave less
        v_br, v_ks, v_ms = variances(prm)
        assert refresh_input_variance(prm, b + 3, 1.0) > refresh_input_variance(prm, b, 1.0)
        assert refresh_input_variance(prm, None, 2.0) == pytest.approx(2 * v_br + v_ks + v_ms, rel=1e-12)
        for bits in (b, b + 3, None):
            m = [refresh_margin(prm, bits, o2) for o2 in (0.5, 1.0, 2.0, 8.0, 64.0)]
            assert all(x > y for x, y in zip(m, m[1:])), (p, norm2, bits)
        # a linear combination noisier than the consumer's norm2 is below the consumer's margin; one at it is not
        assert refresh_margin(prm, None, norm2 * 1.01 + 0.01) < refresh_margin_needed(prm, norm2)
        assert refresh_margin(prm, None, norm2) >= refresh_margin_needed(prm, norm2) * (1 - 1e-12)


def test_lincomb_link_above_the_consumer_norm2_is_refused():
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    norm2 = env.stats()["norm2_linprod"]
    acc, fresh = _sources(prm, out_norm2=norm2, compact=False)
    links, _ = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    assert all(ln.refresh for ln in links[:8])
    acc, fresh = _sources(prm, out_norm2=norm2 + 1, compact=False)
    with pytest.raises(ValueError, match="refresh would keep"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)


def test_client_choice_without_programs_is_the_old_choice():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.fbs_exec_env import min_fbs_size
    from tfhe_fbs_map_amd.split import client_choice
    for name in ("adder8__search_p15", "adder8__search_p7", "full_adder__search_p7", "aes_sbox__search_p15"):
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        for cfg in (ExecConfig(), ExecConfig(fuse_tables=True), ExecConfig(fuse_tables=False)):
            want = cfg.choose_params_fuse(env, min_fbs_size(env.lower()["tables"]))
            assert client_choice(env, cfg) == want, name
    # with programs: the largest p and norm2 over all of them, no shared rotations unless asked
    small, big = (parse_fbs(load_fixture(n)["fbs"], inputs=load_fixture(n)["program_inputs"]) for n in ("full_adder__search_p7", ADDER))
    prm, fuse = client_choice(small, ExecConfig(), [big])
    p = max(min_fbs_size(e.lower()["tables"]) for e in (small, big))
    assert prm == ExecConfig().params_choice(p, max(e.stats()["norm2_linprod"] for e in (small, big))) and fuse is False
    assert client_choice(small, ExecConfig(fuse_tables=True), [big])[1] is True
