"""Folded state without a GPU (include/fbs_exec.h, "folded state"): the entries are declared, exported and bound; `fold_choice` at
the default sets; a `ServerKey` without a fold key is written as it always was and one with a fold key round-trips; `FoldedOutputs`
round-trips; `plan_chain` links a folded source unrefreshed at the default set and refreshed where the fold's factor breaks the
rule; a host client cannot make the key and says where it is made."""
import ctypes
import math
import zipfile

import numpy as np
import pytest

from tests.test_chain_abi import A_FROM_S, _adder, _key_params

ENTRIES = ("fbs_fold_keygen", "fbs_fold_key_sizes", "fbs_export_fold_key", "fbs_import_fold_key", "fbs_fold_dev", "fbs_state_fold",
           "fbs_state_fold_dev", "fbs_state_unfold_dev", "fbs_debug_fold_front_dev")
ONE_LEVEL = [(15, 70), (8, 30), (4, 10), (3, 11), (2, 4)]
TWO_LEVELS = [(15, 281), (7, 20), (31, 70)]


def test_entries_are_declared_exported_and_bound_in_the_gpu_library_only():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _client_native, _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
        assert name not in _client_native.EXPORTED_SYMBOLS, name
    for meth in ("fold_keygen", "fold_key_sizes", "export_fold_key", "import_fold_key", "fold_dev", "fold"):
        assert callable(getattr(_native.Context, meth)), meth
    assert callable(_native.DeviceState.fold) and callable(_native.DeviceState.unfold)
    assert "fold" not in str(_native.kernel_catalog())                            # no rotation or key-switch launch among them


@pytest.mark.parametrize("p,norm2", ONE_LEVEL + TWO_LEVELS)
def test_fold_choice_at_the_default_sets(p, norm2):
    from tfhe_fbs_map_amd import params as P
    prm = P.choose_params(p, norm2, glwe_dims=(1, 2, 3))
    t_f, gamma_f = P.fold_choice(prm, norm2, 6.0)
    assert t_f == (1 if (p, norm2) in ONE_LEVEL else 2) and 1 <= gamma_f and t_f * gamma_f <= 31
    # the margin recomputed with v_br (1 + factor) in place of v_br
    v_br, v_ks, v_ms = P.variances(prm)
    factor = P.folded_state_factor(prm, t_f, gamma_f)
    assert factor == pytest.approx(P.folded_state_variance(prm, t_f, gamma_f) / v_br)
    kept = (1.0 / (4.0 * p)) / math.sqrt(norm2 * v_br * (1.0 + factor) + v_ks + v_ms)
    assert kept >= 6.0 and kept == pytest.approx(P.folded_margin(prm, norm2, t_f, gamma_f))
    assert factor <= 0.028 if t_f == 1 else factor <= 0.016                        # what the fold costs: under 3 % of a rotation
    for g in range(1, 31 // t_f + 1):                                              # the gamma_f of least variance at that level count
        assert P.folded_state_variance(prm, t_f, gamma_f) <= P.folded_state_variance(prm, t_f, g)
    if t_f == 2:                                                                   # ... and one level did not reach the margin
        assert all(P.folded_margin(prm, norm2, 1, g) < 6.0 for g in range(1, 32))
    D = prm.k * prm.N
    assert P.folded_state_skew(prm) == pytest.approx(D * 507903 / 2.0 ** 46)


def test_fold_choice_takes_the_last_resort_where_nothing_reaches_the_margin():
    from tfhe_fbs_map_amd import params as P
    prm = P.choose_params(15, 70, glwe_dims=(1, 2, 3))
    assert P.margin_sigmas(prm, 70) < 6.5                                          # no fold can lift the margin above the set's own
    got = P.fold_choice(prm, 70, 6.5)
    every = [(t, g) for t in range(1, 32) for g in range(1, 31 // t + 1)]
    assert all(P.folded_margin(prm, 70, t, g) < 6.5 for t, g in every)
    best = min(every, key=lambda tg: P.folded_state_variance(prm, *tg))
    assert P.folded_state_variance(prm, *got) == P.folded_state_variance(prm, *best) and got[0] * got[1] <= 31


def _toy_key(**more):
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.split import ServerKey, seeded_key_sizes
    prm = Params(n=4, log_n_poly=8, k=1, l_bsk=1, beta_bsk=10, t_ksk=2, gamma_ksk=4, p_msg=3, sigma_lwe=16, sigma_glwe=4)
    nb, nk = seeded_key_sizes(prm)
    rng = np.random.default_rng(1)
    return prm, ServerKey(prm, False, bytes(range(32)), rng.integers(0, 2 ** 46, nb, dtype=np.uint64),
                          rng.integers(0, 2 ** 46, nk, dtype=np.uint64), **more)


def _members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i.filename)) for i in z.infolist()]


def test_server_key_without_a_fold_key_is_written_as_before_and_with_one_round_trips(tmp_path):
    from dataclasses import asdict
    from tfhe_fbs_map_amd.split import FORMAT_VERSION, _PARAM_FIELDS, ServerKey
    prm, key = _toy_key()
    assert key.fold_bodies is None and key.fold_levels == 0 and key.fold_factor is None
    key.save(str(tmp_path / "key.npz"))
    # the file of a key as it was written before there were fold keys: these members, in this order, with these bytes
    np.savez(str(tmp_path / "old.npz"), kind=np.array("server_key"), format_version=np.array(FORMAT_VERSION),
             params=np.array([int(asdict(prm)[f]) for f in _PARAM_FIELDS], np.int64), fuse_tables=np.array(False),
             mask_key=np.frombuffer(key.mask_key, np.uint8), fingerprint=np.frombuffer(key.fingerprint, np.uint8),
             bsk_bodies=key.bsk_bodies, ksk_bodies=key.ksk_bodies)
    assert _members(str(tmp_path / "key.npz")) == _members(str(tmp_path / "old.npz"))
    back = ServerKey.load(str(tmp_path / "key.npz"))
    assert back.fold_bodies is None and back.fold_levels == back.fold_base_bits == 0
    D, N = prm.k * prm.N, prm.N
    bodies = np.random.default_rng(2).integers(0, 2 ** 46, D * 2 * N, dtype=np.uint64)
    _, folded = _toy_key(fold_bodies=bodies, fold_levels=2, fold_base_bits=9)
    folded.save(str(tmp_path / "folded.npz"))
    back = ServerKey.load(str(tmp_path / "folded.npz"))
    assert np.array_equal(back.fold_bodies, bodies) and (back.fold_levels, back.fold_base_bits) == (2, 9)
    assert back.fold_factor == folded.fold_factor > 0 and back.packing_bodies is None and back.fingerprint == key.fingerprint
    names = [n for n, _ in _members(str(tmp_path / "folded.npz"))]
    assert names[:8] == [n for n, _ in _members(str(tmp_path / "old.npz"))] and names[8:] == ["fold_bodies.npy", "fold_levels.npy", "fold_base_bits.npy"]
    for bad in (dict(fold_bodies=bodies[:-1], fold_levels=2, fold_base_bits=9), dict(fold_bodies=bodies, fold_levels=2, fold_base_bits=16),
                dict(fold_bodies=bodies, fold_levels=0, fold_base_bits=9)):
        with pytest.raises(ValueError, match="fold"):
            _toy_key(**bad)


def test_folded_outputs_round_trip(tmp_path):
    from tfhe_fbs_map_amd.split import FoldedOutputs, folded_words
    prm, _ = _toy_key()
    T, names = 200, ["x", "y", "z"]
    count = folded_words(prm, len(names) * T)
    assert count == 3 * 2 * 256                                                    # 600 ciphertexts: three samples of (k + 1) N words
    words = np.random.default_rng(3).integers(0, 2 ** 46, count, dtype=np.uint64)
    obj = FoldedOutputs(names, T, words, bytes(range(8)), np.array([1.0, 0.0, 1.0]), 0.02)
    obj.save(str(tmp_path / "f.npz"))
    back = FoldedOutputs.load(str(tmp_path / "f.npz"))
    assert back.output_names == names and back.T == T and back.fingerprint == bytes(range(8)) and back.fold_factor == 0.02
    assert np.array_equal(back.words, words) and np.array_equal(back.out_norm2, [1.0, 0.0, 1.0]) and not back.on_device
    with np.load(str(tmp_path / "f.npz"), allow_pickle=False) as z:               # no pickle in the file
        assert str(z["kind"]) == "folded_outputs"
    with pytest.raises(ValueError, match="folded_outputs"):                          # a file of another kind
        FoldedOutputs.load(_other_kind(tmp_path))


def _other_kind(tmp_path):
    from tfhe_fbs_map_amd.split import EncryptedOutputs
    path = str(tmp_path / "e.npz")
    EncryptedOutputs(["x"], 1, np.zeros((1, 1, 257), np.uint64), bytes(8), np.ones(1)).save(path)
    return path


def _folded(prm, T=4, fp=bytes(8), out_norm2=1.0, factor=0.02):
    from tfhe_fbs_map_amd.split import EncryptedInputs, FoldedOutputs, folded_words
    names = [f"s{i}" for i in range(8)] + ["cout"]
    acc = FoldedOutputs(names, T, np.zeros(folded_words(prm, 9 * T), np.uint64), fp, np.full(9, float(out_norm2)), factor)
    fresh = EncryptedInputs([f"b{i}" for i in range(8)], T, 100, np.zeros((8, T), np.uint64), fp)
    return acc, fresh


def test_plan_chain_links_a_folded_source_unrefreshed_at_the_default_set():
    from tfhe_fbs_map_amd.params import fold_choice, folded_state_factor
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    norm2 = (env.fusion_stats(prm.p_msg) if fuse else env.stats())["norm2_linprod"]
    factor = folded_state_factor(prm, *fold_choice(prm, norm2, 6.0))
    assert 0 < factor < 0.03
    acc, fresh = _folded(prm, factor=factor)
    links, T = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    assert T == 4
    for i in range(8):
        assert (links[i].kind, links[i].source, links[i].index, links[i].refresh) == ("folded", 0, i, False)
        assert links[i].noise == pytest.approx(1.0 + factor) and links[i].margin is None
        assert (links[8 + i].kind, links[8 + i].refresh) == ("seeded", False)
    # a constant's row: 0 + factor; a linear combination's (out_norm2 > 1) is refreshed, like any full link
    acc, fresh = _folded(prm, out_norm2=0.0, factor=factor)
    assert all(ln.noise == pytest.approx(factor) and not ln.refresh for ln in plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)[0][:8])
    acc, fresh = _folded(prm, out_norm2=2.0, factor=factor)
    links, _ = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    assert all(ln.kind == "folded" and ln.refresh and ln.noise == 1.0 and ln.margin is not None for ln in links[:8])
    # words that do not fit, another key, another T
    bad, _ = _folded(prm, factor=factor)
    bad.words = bad.words[:-1]
    with pytest.raises(ValueError, match="folded words"):
        plan_chain(prm, fuse, bytes(8), env, [bad, fresh], rename=A_FROM_S)
    other, _ = _folded(prm, fp=bytes([1] * 8), factor=factor)
    with pytest.raises(ValueError, match="another server key"):
        plan_chain(prm, fuse, bytes(8), env, [other, fresh], rename=A_FROM_S)


def test_plan_chain_refreshes_a_folded_link_whose_factor_breaks_the_rule():
    """a made-up fold key -- one level of 31 bits -- whose factor takes the program below its margin: the link is refreshed, under the
    full-link rule at out_norm2 + factor, and refused where even the refresh would not keep the margin"""
    from tfhe_fbs_map_amd.params import folded_margin, folded_state_factor, refresh_margin, refresh_margin_needed
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    norm2 = (env.fusion_stats(prm.p_msg) if fuse else env.stats())["norm2_linprod"]
    factor = 0.5
    assert folded_margin(prm, norm2, 1, 19) >= 6.0
    v_gamma = next(g for g in range(20, 32) if folded_margin(prm, norm2, 1, g) < 6.0)          # such keys exist: a wider digit
    assert folded_state_factor(prm, 1, v_gamma) > folded_state_factor(prm, 1, 19)
    acc, fresh = _folded(prm, factor=factor)
    links, _ = plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)
    need = refresh_margin_needed(prm, norm2)
    for ln in links[:8]:
        assert (ln.kind, ln.refresh, ln.noise) == ("folded", True, 1.0)
        assert ln.margin == pytest.approx(refresh_margin(prm, None, 1.0 + factor)) and ln.margin >= need * (1.0 - 1e-12)
    acc, fresh = _folded(prm, factor=1e6)
    with pytest.raises(ValueError, match="fold factor"):
        plan_chain(prm, fuse, bytes(8), env, [acc, fresh], rename=A_FROM_S)


def test_a_host_client_names_the_gpu_library():
    from tfhe_fbs_map_amd.split import Client
    with pytest.raises(NotImplementedError, match="libfbsexec"):
        Client(_adder(), host=True, folding=True)
