"""What tests/test_gpu_fold.py stands on, checked without a GPU (the counterpart of tests/test_packed_reference.py): the fast
form of the fold's definition (tests/fold_reference.py) is the schoolbook restatement word for word; the planted words reach the
edges they claim; the definition is what sample extraction undoes -- big-key encryptions made by the host library, folded here
under a fold key made here from the exported GLWE key, expanded by fbs_pub_expand and decrypted by the host library come back as
their messages, with a phase error inside the noise model."""
import math

import numpy as np
import pytest

from tests import fold_reference as F
from tests import helpers as H

_HOST = {}


def host_ctx(log_n=8, k=1, n=12):
    if (log_n, k, n) not in _HOST:
        from tfhe_fbs_map_amd import HostContext
        ctx = HostContext(F.fold_toy(log_n, k, n), seed=31)
        ctx.keygen_seeded()
        _HOST[log_n, k, n] = ctx
    return _HOST[log_n, k, n]


@pytest.mark.parametrize("t_f,gamma_f", [(3, 10), (1, 31), (2, 15)])
def test_fast_reference_is_the_schoolbook_restatement(t_f, gamma_f):
    ctx = host_ctx()
    prm = ctx.params
    key = F.python_fold_key(prm, ctx.export_keys()["sk_glwe"], t_f, gamma_f, seed=t_f)
    cts = F.planted_cts(prm.k * prm.N, 5, t_f, gamma_f, seed=3)                    # one sample of five ciphertexts
    slow = F.fold_reference(cts, key, t_f, gamma_f, slow=True)
    fast = F.fold_reference(cts, key, t_f, gamma_f)
    assert slow.shape == ((prm.k + 1) * prm.N,) and int(slow.max()) < H.Q
    assert np.array_equal(fast, slow)


def test_prefix_sums_are_the_definition():
    """fold_prefixes adds the samples of the parts of a batch: word for word the definition on each prefix"""
    ctx = host_ctx()
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    key = F.python_fold_key(prm, ctx.export_keys()["sk_glwe"], 3, 10, seed=2)
    big = F.planted_cts(D, N + 1, 3, 10, seed=4, N=N)
    got = F.fold_prefixes(big, key, 3, 10)
    assert sorted(got) == [1, N - 1, N, N + 1]
    for count, words in got.items():
        assert np.array_equal(words, F.fold_reference(big[:count], key, 3, 10)), count
        assert set(F.planted_rows(count, N)) <= set(F.planted_rows(N + 1, N))      # every prefix ends on a planted ciphertext


def test_negacyclic_by_bits_is_the_schoolbook_product():
    rng = np.random.default_rng(5)
    a = rng.integers(0, H.Q, (3, 256), dtype=np.uint64)
    a[0, :4] = [0, H.Q - 1, 1, H.Q - 1]
    s = rng.integers(0, 2, 256)
    got = F.negacyclic_by_bits(a, s)
    for r in range(3):
        assert np.array_equal(got[r], H.negacyclic(s.astype(np.int64), a[r])), r


@pytest.mark.parametrize("t_f,gamma_f", F.FOLD_KEYS + F.FOLD_EDGE_KEYS)
def test_planted_words_reach_the_edges_they_claim(t_f, gamma_f):
    tg, r, B = t_f * gamma_f, 46 - t_f * gamma_f, 1 << gamma_f
    named = F.planted_mask_words(t_f, gamma_f)
    assert {"zero", "qm1", "tie", "below_tie", "all_low", "all_high", "top_half"} <= set(named) and ("wraps" in named) == (r >= 20)
    rounded = {name: int(F.round_mask(w, t_f, gamma_f)) for name, w in named.items()}
    digits = {name: [int(d) for d in H.balanced_digits(a, t_f, gamma_f)] for name, a in rounded.items()}
    assert digits["all_low"] == [-B // 2] * t_f and digits["all_high"] == [B // 2 - 1] * t_f
    assert digits["top_half"] == [-B // 2] + [0] * (t_f - 1)
    chain = (B // 2) + sum((B // 2 - 1) << (gamma_f * v) for v in range(1, t_f))   # the carry through every level, dropped at the top
    assert rounded["all_low"] == chain
    assert (rounded["zero"], rounded["tie"], rounded["below_tie"]) == (0, 1, 0) and named["tie"] - named["below_tie"] == 1
    if r >= 20:
        assert rounded["wraps"] == 0 and rounded["qm1"] == 0 and int(F.round_mask(named["wraps"] - 1, t_f, gamma_f)) == (1 << tg) - 1
    D = 256
    for count in (1, 255, 256, 257):
        cts = F.planted_cts(D, count, t_f, gamma_f, seed=count)
        assert cts.shape == (count, D + 1) and int(cts.max()) < H.Q
        assert int(cts[0, D]) == 0 and (count < 2 or int(cts[1, D]) == H.Q - 1)
        if count >= 4:
            assert set(named.values()) <= set(int(x) for x in cts[F.planted_rows(count, 256)][:, :32].reshape(-1))
            d = H.balanced_digits(F.round_mask(cts[:, :D], t_f, gamma_f), t_f, gamma_f)
            for v in range(t_f):
                assert (d[v] == -B // 2).any() and (d[v] == B // 2 - 1).any(), v


@pytest.mark.parametrize("t_f,gamma_f", [(3, 10), (1, 19)])
def test_definition_is_what_sample_extraction_undoes(t_f, gamma_f):
    from tfhe_fbs_map_amd import _public_native
    from tfhe_fbs_map_amd.params import folded_state_skew, folded_state_variance
    ctx = host_ctx()
    prm = ctx.params
    p, N, D = prm.p_msg, prm.N, prm.k * prm.N
    sk = ctx.export_keys()["sk_glwe"]
    key = F.python_fold_key(prm, sk, t_f, gamma_f, seed=9)
    count = N + 5
    msgs = np.random.default_rng(t_f).integers(0, 2 * p, count)
    msgs[:2 * p] = np.arange(2 * p)
    cts = ctx.encrypt(msgs, nonce0=11)
    glwe = F.fold_reference(cts, key, t_f, gamma_f)
    assert glwe.size == _public_native.sample_words(prm, count)
    back = _public_native.expand(prm, glwe, count)
    assert back.shape == (count, D + 1) and np.array_equal(ctx.decrypt(back), msgs)
    # the phase of coefficient j is the source's phase plus the fold's noise: measured against the source's own phase
    src_phase = [(int(ct[D]) - sum(int(a) for a, s in zip(ct[:D], sk) if s)) % H.Q for ct in cts]
    err = F.phase_errors(glwe, prm, count, sk, src_phase) / float(H.Q)
    # rounding with q treated as 2^46 reads every mask word a as a q / 2^46: a deterministic shift of sum_(s_i = 1) a_i (1 - q / 2^46),
    # bounded by params.folded_state_skew; at this toy set's sigma_glwe = 4 it is larger than the noise, so it is taken off first
    shift = (cts[:, :D].astype(np.float64) @ np.asarray(sk, np.float64)) / float(H.Q) * (1.0 - H.Q / 2.0 ** 46)
    assert 0.0 <= float(shift.min()) and float(shift.max()) <= folded_state_skew(prm)
    assert float(np.abs(err).max()) <= folded_state_skew(prm) + 6.0 * math.sqrt(folded_state_variance(prm, t_f, gamma_f))
    err = err - shift
    sigma = math.sqrt(folded_state_variance(prm, t_f, gamma_f))
    assert float(np.abs(err).max()) < 6.0 * sigma and 0.5 < float(err.var()) / sigma ** 2 < 1.25, (float(err.var()), sigma ** 2)
