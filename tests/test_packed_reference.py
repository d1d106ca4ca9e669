"""What tests/test_gpu_pack_shapes.py stands on, checked without a GPU: the fast form of the packing definition (the oracle's NTT
products, tests/helpers.py) is the schoolbook restatement word for word; the planted fields reach the edges they claim; the
definition is the one the host decode undoes (messages encrypted in Python under the exported small key come back through
reference_pack and HostContext.decrypt_packed); the restated shapes are the ones the sources instantiate; the restated word count
is the binding's."""
import math
import os
import re

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ALL_KEYS = H.PACK_KEYS + H.PACK_EDGE_KEYS
_HOST = {}


def host_ctx(log_n=8, k=2, n=6):
    """a host context keyed with fbs_keygen_seeded for the toy set of a shape, made once per module"""
    if (log_n, k, n) not in _HOST:
        from tfhe_fbs_map_amd import HostContext
        ctx = HostContext(H.pack_toy(log_n, k, n), seed=29)
        ctx.keygen_seeded()
        _HOST[log_n, k, n] = ctx
    return _HOST[log_n, k, n]


# ---- 1. the fast form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", [(3, 10), (1, 31)])
def test_fast_reference_is_the_schoolbook_restatement(t_p, gamma_p):
    ctx = host_ctx()
    prm = ctx.params
    ctx.packing_keygen(t_p, gamma_p)
    key = ctx.export_packing_key(full=True)["full"]
    fields = H.planted_pack_fields(prm.n, prm.N - 1, t_p, gamma_p, seed=3)           # one sample, its last coefficient unused
    slow = H.sample_residues(fields, key, t_p, gamma_p, "host")
    assert np.array_equal(H.sample_residues(fields, key, t_p, gamma_p, "host", fast=True), slow) and int(slow.max()) < H.Q
    for bits in (prm.log_n_poly + 1, 17, 31):
        want = H.reference_pack(fields, key, t_p, gamma_p, bits, "host")
        assert want.size == H.packed_count(prm.k, prm.N, prm.N - 1, bits)
        assert np.array_equal(H.reference_pack(fields, key, t_p, gamma_p, bits, "host", fast=True), want), bits


# ---- 2. the planted fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", ALL_KEYS)
def test_planted_fields_reach_the_edges_they_claim(t_p, gamma_p):
    n, N = 6, 256
    tg, r, B = t_p * gamma_p, 31 - t_p * gamma_p, 1 << gamma_p
    named = H.planted_mask_fields(t_p, gamma_p)
    assert set(named) == {"zero", "ones", "all_low", "all_high", "top_half"} | ({"tie", "below_tie"} if r > 0 else set())
    assert all(0 <= m < 1 << 31 for m in named.values())
    rounded = {name: int(H.rounded_mask_fields(m, t_p, gamma_p)) for name, m in named.items()}
    digits = {name: [int(d) for d in H.balanced_digits(a, t_p, gamma_p)] for name, a in rounded.items()}
    value = lambda ds: sum(d << (gamma_p * (t_p - 1 - v)) for v, d in enumerate(ds))
    assert digits["all_low"] == [-B // 2] * t_p and digits["all_high"] == [B // 2 - 1] * t_p
    assert digits["top_half"] == [-B // 2] + [0] * (t_p - 1)
    # the carry chain: the lowest gamma bits B/2, every higher group B/2 - 1; its carry leaves the top and is dropped
    chain = (B // 2) + sum((B // 2 - 1) << (gamma_p * v) for v in range(1, t_p))
    assert rounded["all_low"] == chain and value(digits["all_low"]) == chain - (1 << tg)
    assert value(digits["top_half"]) == rounded["top_half"] - (1 << tg)
    assert rounded["zero"] == 0 and digits["zero"] == [0] * t_p
    if r > 0:
        assert rounded["ones"] == 0                                                  # rounds up to 2^(t gamma) and wraps
        assert named["tie"] - named["below_tie"] == 1 and (rounded["tie"], rounded["below_tie"]) == (1, 0)
    else:
        assert rounded["ones"] == (1 << 31) - 1 and value(digits["ones"]) == -1      # all ones: -1 after the dropped carry
    lift = lambda m: (m * H.Q + (1 << 30)) >> 31
    assert [lift(m) - (m << 15) for m in (2114, 2115)] == [0, -1] and lift((1 << 31) - 1) < H.Q
    for count in (N - 1, N, N + 1, N + 3):
        fields = H.planted_pack_fields(n, count, t_p, gamma_p, seed=count)
        assert fields.shape == (count, n + 1) and fields.dtype == np.uint32 and int(fields.max()) < 1 << 31
        assert np.array_equal(fields, H.planted_pack_fields(n, count, t_p, gamma_p, seed=count))
        spots = H.planted_positions(count)
        assert spots == [0, 1, count - 2, count - 1]
        for i in range(n):
            assert set(int(x) for x in fields[spots, i]) <= set(named.values())
        assert set(int(x) for x in fields[spots, :n].reshape(-1)) == set(named.values())          # every value, in some column
        assert set(H.PACK_BODY_FIELDS) <= set(int(x) for x in fields[:, n])
        # per sample of the batch the digits are what the kernels see: every level meets both ends of its range, and a dropped carry
        a = H.rounded_mask_fields(fields[:, :n], t_p, gamma_p)
        d = H.balanced_digits(a, t_p, gamma_p)
        assert int(d.min()) == -B // 2 and int(d.max()) == B // 2 - 1
        for v in range(t_p):
            assert (d[v] == -B // 2).any() and (d[v] == B // 2 - 1).any(), v
        total = sum(d[v] << (gamma_p * (t_p - 1 - v)) for v in range(t_p))
        assert np.array_equal(total % (1 << tg), a) and (total == a - (1 << tg)).any() and (total == a).any()
    one = H.planted_pack_fields(n, 1, t_p, gamma_p, seed=1)                          # a single ciphertext: one value a column
    assert one.shape == (1, n + 1) and set(int(x) for x in one[0, :n]) <= set(named.values()) and int(one[0, n]) == 0


# ---- 3. the definition is what the host decode undoes ----------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", H.PACK_KEYS)
def test_definition_decrypts_on_the_host(t_p, gamma_p):
    """small-key encryptions made here, at 31 bits under the exported sk_lwe, on planted mask fields: reference_pack and then
    fbs_decrypt_packed return the messages, at key parameters and widths where the noise model leaves the selector's 6 sigma"""
    from tfhe_fbs_map_amd.params import packed_output_margin
    ctx = host_ctx()
    prm = ctx.params
    p, n, N = prm.p_msg, prm.n, prm.N
    ctx.packing_keygen(t_p, gamma_p)
    key = ctx.export_packing_key(full=True)["full"]
    sk = ctx.export_keys()["sk_lwe"].astype(np.int64)
    assert sk.shape == (n,) and set(sk) <= {0, 1} and sk.any()
    count = N + 5
    rng = np.random.default_rng(t_p)
    msgs = rng.integers(0, 2 * p, count)
    msgs[:2 * p] = np.arange(2 * p)
    fields = H.planted_pack_fields(n, count, t_p, gamma_p, seed=7)
    encoded = ((msgs.astype(np.int64) << 31) + p) // (2 * p)                         # round(m 2^31 / 2p)
    fields[:, n] = (fields[:, :n].astype(np.int64) @ sk + encoded) % (1 << 31)
    for bits in (prm.log_n_poly + 1, 17, 31):
        margin = packed_output_margin(prm, t_p, gamma_p, bits)
        assert margin >= H.PLANTED_MARGIN, (bits, margin)
        words = H.reference_pack(fields, key, t_p, gamma_p, bits, "host", fast=True)
        assert np.array_equal(ctx.decrypt_packed(words, count, bits), msgs), bits
        phase = H.decode_phases(words, prm, count, bits, ctx.export_keys()["sk_glwe"])
        err = (phase / float(1 << bits) - msgs / (2.0 * p) + 0.5) % 1.0 - 0.5
        assert float(np.abs(err).max()) < 1.0 / (4 * p), bits


# ---- 4. the shapes -----------------------------------------------------------------------------------------------------------------
def test_pack_shapes_are_the_ones_the_sources_instantiate():
    from tfhe_fbs_map_amd.params import glwe_shape_built
    glwe = re.search(r"^#define FBS_GLWE_SHAPES\(X\) (.*)$", open(os.path.join(CSRC, "fbs_select.hpp")).read(), flags=re.M).group(1)
    pack = re.search(r"^#define FBS_PACK_SHAPES\(X\) (.*)$", open(os.path.join(CSRC, "fbs_pack.hip")).read(), flags=re.M).group(1)
    assert pack.count("FBS_GLWE_SHAPES(X)") == 1
    pairs = re.findall(r"X\((\d+), (\d+)\)", pack.replace("FBS_GLWE_SHAPES(X)", glwe))
    assert re.sub(r"X\(\d+, \d+\)|\s", "", pack.replace("FBS_GLWE_SHAPES(X)", glwe)) == ""          # nothing else on the lines
    built = sorted((int(L), int(K1) - 1) for L, K1 in pairs)
    assert built == sorted(H.PACK_SHAPES) and len(set(H.PACK_SHAPES)) == len(H.PACK_SHAPES) == 13
    for log_n, k in H.PACK_SHAPES:
        assert 8 <= log_n <= 12 and (k == 1 or glwe_shape_built(log_n, k)), (log_n, k)
        prm = H.pack_toy(log_n, k, 6)
        assert (prm.log_n_poly, prm.k, prm.n) == (log_n, k, 6)


# ---- 5. the word count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,k", H.PACK_SHAPES)
def test_restated_word_count_is_the_bindings(log_n, k):
    from tfhe_fbs_map_amd import HostContext
    ctx = HostContext(H.pack_toy(log_n, k, 6), seed=1)
    N = 1 << log_n
    for count in (0, 1, N - 1, N, N + 1, N + 3, 2 * N + 3, 8192 // N * N + N + 3):
        for bits in (log_n + 1, 17, 31):
            assert ctx.packed_words(count, bits) == H.packed_count(k, N, count, bits), (count, bits)
    assert H.packed_sample_count(k, N, N, 31) == (k + 1) * N * 31 // 64 and math.log2(N) == log_n
    ctx.close()
