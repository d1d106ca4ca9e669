"""Folded state on the GPU (include/fbs_exec.h, "folded state"; csrc/fbs_fold.hip): k_fold_front, k_pack_accumulate with n := D and
k_fold_finish, word for word against the definition restated in tests/fold_reference.py (held to the schoolbook product and to
decryption by tests/test_fold_reference.py).  Ciphertext words are arbitrary canonical residues, so the planted words (the rounding
tie, the word that rounds up and wraps, both ends of every digit, the carry dropped at the top, body words 0 and q - 1) go in as
they are.  Every comparison is exact; every output buffer is two samples longer than needed and the rest must keep its sentinel;
every source buffer carries 64 rows of 0xFF..FF past `count` that must change nothing."""
import math

import numpy as np
import pytest

from tests import fold_reference as F
from tests.test_gpu_device_io import dev, host

pytestmark = pytest.mark.gpu

Q = F.Q
E_INVALID, E_STATE = -1, -3
SENTINEL = 0x5A5A5A5A5A5A5A5A
_CTX, _KEY = {}, {}


def keyed(log_n, k):
    """a context keyed with fbs_keygen_seeded for the toy set of a shape (n = 12), made once per module"""
    if (log_n, k) not in _CTX:
        from tfhe_fbs_map_amd import Context
        ctx = Context(F.fold_toy(log_n, k), seed=17, keygen=False)
        ctx.keygen_seeded()
        _CTX[log_n, k] = ctx
    return _CTX[log_n, k]


def fold_key(ctx, t_f, gamma_f):
    """makes (t_f, gamma_f) the context's fold key; returns the whole key [D][t_f][k+1][N]"""
    prm = ctx.params
    ctx.fold_keygen(t_f, gamma_f)
    assert (ctx.stat("fold_key"), ctx.stat("fold_levels"), ctx.stat("fold_base_bits")) == (1, t_f, gamma_f)
    memo = (prm.log_n_poly, prm.k, t_f, gamma_f)
    if memo not in _KEY:
        _KEY.clear()                                                               # (one whole key at a time: up to 150 MB)
        _KEY[memo] = ctx.export_fold_key(full=True)["full"]
        assert _KEY[memo].shape == (prm.k * prm.N, t_f, prm.k + 1, prm.N)
    return _KEY[memo]


def shipped(prm):
    from tfhe_fbs_map_amd.params import fold_choice
    return fold_choice(prm)


def fold_dev(ctx, cts, offset=0):
    """fbs_fold_dev on host ciphertexts, 64 rows of all-ones words behind them, the source `offset` words into its allocation"""
    import torch
    prm = ctx.params
    count = cts.shape[0]
    buf = np.full(offset + (count + 64) * prm.ct_words, 0xFFFFFFFFFFFFFFFF, np.uint64)
    buf[offset:offset + count * prm.ct_words] = cts.reshape(-1)
    d_c = dev(buf)
    W = -(-count // prm.N) * (prm.k + 1) * prm.N
    d_w = torch.full((W + 2 * (prm.k + 1) * prm.N,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fold_dev(d_c.data_ptr() + 8 * offset, count, d_w.data_ptr())
    ctx.sync()
    out = host(d_w)
    assert (out[W:] == np.uint64(SENTINEL)).all(), "words written past the batch"
    return out[:W]


# ---- a. every transform class, the fills, both keys ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["3x10", "shipped"])
@pytest.mark.parametrize("log_n,k", F.FOLD_SHAPES)
def test_every_shape_folds_planted_words_word_for_word(log_n, k, which):
    ctx = keyed(log_n, k)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    assert (prm.log_n_poly, prm.k, prm.n) == (log_n, k, 12)
    t_f, gamma_f = shipped(prm) if which == "shipped" else (3, 10)
    if log_n == 11:
        if which == "3x10":
            t_f, gamma_f = 1, 10                                                   # N = 2048 is held at one level
        assert t_f == 1
    key = fold_key(ctx, t_f, gamma_f)
    big = F.planted_cts(D, N + 1, t_f, gamma_f, seed=100 * log_n + k, N=N)
    for count, want in F.fold_prefixes(big, key, t_f, gamma_f).items():
        assert want.size == -(-count // N) * (k + 1) * N
        got = fold_dev(ctx, big[:count], offset=count & 1)
        assert np.array_equal(got, want), (count, int((got != want).sum()))


# ---- b. edge key parameters, every slicing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_f,gamma_f", F.FOLD_EDGE_KEYS)
def test_edge_key_parameters(t_f, gamma_f):
    """r = 46 - t_f gamma_f = 15 with the widest digit (|d| <= 2^30) and with the most levels (31 of one bit), and r = 16"""
    ctx = keyed(8, 2)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    key = fold_key(ctx, t_f, gamma_f)
    cts = F.planted_cts(D, N + 1, t_f, gamma_f, seed=t_f, N=N)
    assert np.array_equal(fold_dev(ctx, cts), F.fold_prefixes(cts, key, t_f, gamma_f)[N + 1])


def test_every_slicing_gives_the_same_words():
    ctx = keyed(8, 2)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    key = fold_key(ctx, 3, 10)
    cts = F.planted_cts(D, N + 1, 3, 10, seed=5, N=N)
    want = F.fold_prefixes(cts, key, 3, 10)[N + 1]
    try:
        for slices in (1, 2, 5, 31, 32, 1000, 0):                                  # (1000 is cut to min(32, D); 0: by launch size)
            ctx.tune(pack_slices=slices)
            assert np.array_equal(fold_dev(ctx, cts), want), slices
    finally:
        ctx.tune(pack_slices=0)


# ---- c. passes, scratch, the state entries -----------------------------------------------------------------------------------------
def test_two_passes_and_a_second_call_that_grows_no_scratch():
    ctx = keyed(8, 1)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    key = fold_key(ctx, 3, 10)
    count = 8192 + N + 3                                                           # a pass of 8192, then one of two samples
    cts = np.random.default_rng(8).integers(0, Q, (count, D + 1), dtype=np.uint64)
    got = fold_dev(ctx, cts)
    growths = ctx.stat("scratch_growths")
    assert np.array_equal(fold_dev(ctx, cts), got) and ctx.stat("scratch_growths") == growths
    sw = (prm.k + 1) * N
    assert np.array_equal(got[:8192 // N * sw], fold_dev(ctx, cts[:8192]))        # a pass is the fold of its ciphertexts
    assert np.array_equal(got[8192 // N * sw:], fold_dev(ctx, cts[8192:]))
    assert np.array_equal(got[-2 * sw:], F.fold_reference(cts[8192:], key, 3, 10))  # ... and the second pass the definition
    assert np.array_equal(got[:sw], F.fold_reference(cts[:N], key, 3, 10))


def test_state_fold_is_fold_dev_of_the_full_fetch():
    import torch
    ctx = keyed(8, 2)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    fold_key(ctx, 3, 10)
    rows, T = 3, N // 2 + 7                                                        # rows 1 and 2: N + 14 ciphertexts, two samples
    cts = F.planted_cts(D, rows * T, 3, 10, seed=6, N=N).reshape(rows, T, D + 1)
    with ctx.state(rows, T) as st:
        st.put(cts)
        assert np.array_equal(st.fetch(), cts)
        for row0, n_rows in ((0, 3), (1, 2), (2, 1), (1, 0)):
            want = fold_dev(ctx, cts[row0:row0 + n_rows].reshape(-1, D + 1)) if n_rows else np.zeros(0, np.uint64)
            assert np.array_equal(st.fold(row0, n_rows), want), (row0, n_rows)
            on_card = st.fold(row0, n_rows, device=True)
            assert isinstance(on_card, torch.Tensor) and on_card.is_cuda and np.array_equal(host(on_card), want)
        growths = ctx.stat("scratch_growths")
        st.fold()
        assert ctx.stat("scratch_growths") == growths


# ---- d. the front kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,k", [(8, 1), (10, 2)])
@pytest.mark.parametrize("offset", [0, 1])
def test_front_kernel_alone(log_n, k, offset):
    """D + 1 = 257 and 2049 words a ciphertext; the source on a 16-byte line and 8 bytes off it (within a batch the rows alternate
    anyway: D + 1 is odd); rows behind `count` are not read"""
    import torch
    ctx = keyed(log_n, k)
    prm = ctx.params
    N, D = prm.N, prm.k * prm.N
    assert D + 1 == {8: 257, 10: 2049}[log_n]
    for tg, count in ((30, N + 3), (19, 1), (31, N)):
        cols = -(-count // N) * N
        cts = F.planted_cts(D, count, 1, tg, seed=tg, N=N)
        buf = np.full(offset + (count + 64) * (D + 1), 0xFFFFFFFFFFFFFFFF, np.uint64)
        buf[offset:offset + count * (D + 1)] = cts.reshape(-1)
        d_c = dev(buf)
        d_f = torch.full(((D + 2) * cols + 2 * N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.debug_fold_front_dev(d_c.data_ptr() + 8 * offset, count, cols, tg, d_f.data_ptr())
        ctx.sync()
        out = host(d_f, np.uint32)
        assert (out[(D + 2) * cols:] == 0x5A5A5A5A).all()
        fields = out[:D * cols].reshape(D, cols)
        bodies = out[D * cols:(D + 2) * cols].view(np.uint64)
        assert np.array_equal(fields[:, :count], F.round_mask(cts[:, :D], 1, tg).T.astype(np.uint32)), (tg, count)
        assert np.array_equal(bodies[:count], cts[:, D]) and not fields[:, count:].any() and not bodies[count:].any()


# ---- e. round trip, device and host paths -------------------------------------------------------------------------------------------
def test_fold_then_unfold_decrypts_to_the_source():
    ctx = keyed(10, 2)
    prm = ctx.params
    p, N = prm.p_msg, prm.N
    ctx.fold_keygen(*shipped(prm))
    rows, T = 3, N // 2 + 5
    msgs = np.random.default_rng(3).integers(0, 2 * p, (rows, T))
    with ctx.state(rows, T) as src, ctx.state(rows, T) as back, ctx.state(rows, T) as back2:
        src.put(ctx.encrypt(msgs.reshape(-1), nonce0=7).reshape(rows, T, -1))
        on_card = src.fold(device=True)
        words = src.fold()
        assert np.array_equal(host(on_card), words)                                # folded on the device = through the host path
        back.unfold(on_card)
        back2.unfold(words)
        got = back.fetch()
        assert np.array_equal(got, back2.fetch())
        assert np.array_equal(ctx.decrypt(got.reshape(-1, prm.ct_words)).reshape(rows, T), msgs)
        back.unfold(src.fold(1, 2, device=True), 0, 2)                             # rows 1, 2 into rows 0, 1
        assert np.array_equal(ctx.decrypt(back.fetch(0, 2).reshape(-1, prm.ct_words)).reshape(2, T), msgs[1:])


def test_keys_made_on_the_device_are_the_hosts_and_an_imported_key_folds_the_same():
    from tfhe_fbs_map_amd import Context
    prm = F.fold_toy(8, 2)
    a = Context(prm, seed=17, keygen=False)
    a.keygen_seeded()
    a.fold_keygen(2, 9)
    on_host = a.export_fold_key()
    a.tune(keys_on_device=1)
    a.fold_keygen(2, 9)
    assert np.array_equal(a.export_fold_key()["fold_bodies"], on_host["fold_bodies"])
    cts = F.planted_cts(prm.k * prm.N, prm.N + 1, 2, 9, seed=2, N=prm.N)
    want = fold_dev(a, cts)
    server = Context.evaluation_only(prm, **a.export_seeded_keys())
    server.import_fold_key(2, 9, on_host["fold_bodies"])
    assert np.array_equal(fold_dev(server, cts), want)
    a.keygen_seeded()                                                              # a keygen drops the fold key, as the packing key
    assert a.stat("fold_key") == 0
    server.close()
    a.close()


# ---- f. noise ------------------------------------------------------------------------------------------------------------------------
def test_noise_at_the_default_set_is_inside_the_model():
    """2 N fresh encryptions of zero at the default k = 2, N = 1024 set, folded; the phase errors under the exported GLWE key; their
    variance minus the encryptions' own sigma_glwe^2 against params.folded_state_variance, in the band of the compact and packed
    noise tests"""
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, fold_choice, folded_state_variance
    prm = choose_params(15, 70, glwe_dims=(1, 2, 3))
    assert (prm.k, prm.N) == (2, 1024)
    t_f, gamma_f = fold_choice(prm, 70)
    assert t_f == 1
    ctx = Context(prm, seed=23, keygen=False)
    ctx.tune(keys_on_device=1)
    ctx.keygen_seeded()
    ctx.fold_keygen(t_f, gamma_f)
    count = 2 * prm.N
    cts = ctx.encrypt(np.zeros(count, np.int64), nonce0=1)
    glwe = fold_dev(ctx, cts)
    sk = ctx.export_keys()["sk_glwe"]
    err = F.phase_errors(glwe, prm, count, sk, np.zeros(count, np.int64)) / float(Q)
    own = (prm.sigma_glwe / float(Q)) ** 2
    model = folded_state_variance(prm, t_f, gamma_f)
    ratio = (float(err.var()) - own) / model
    print("folded-state noise: measured / model = %.3f (variance %.3e, model %.3e, sigma_glwe^2 %.3e, mean %.3e)"
          % (ratio, float(err.var()), model, own, float(err.mean())))
    ctx.close()
    assert 0.5 <= ratio <= 1.25, ratio


# ---- g. refusals -----------------------------------------------------------------------------------------------------------------------
def _code(call):
    from tfhe_fbs_map_amd import FbsError
    try:
        call()
    except FbsError as e:
        return e.code
    return 0


def test_refusals_write_nothing_and_leave_the_context_usable():
    import torch
    from tfhe_fbs_map_amd import Context, _native as nat
    lib = nat.lib
    prm = F.fold_toy(8, 2)
    N, D = prm.N, prm.k * prm.N
    cts = F.planted_cts(D, N + 2, 2, 7, seed=1, N=N)
    d_c = dev(cts)
    d_w = torch.full((4 * (prm.k + 1) * N,), 0x5A5A, dtype=torch.int64, device="cuda")
    out = np.full(4 * (prm.k + 1) * N, 7, np.uint64)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_w == 0x5A5A).all()) and bool((out == 7).all())

    plain = Context(prm, seed=3)                                                   # ordinary keys: no fold key to make, none to fold with
    assert _code(lambda: plain.fold_keygen(2, 7)) == E_STATE
    assert _code(lambda: plain.fold_dev(d_c.data_ptr(), N + 2, d_w.data_ptr())) == E_STATE
    assert plain.stat("fold_key") == 0 and untouched()
    plain.close()
    client = Context(prm, seed=3, keygen=False)
    assert _code(lambda: client.fold_keygen(2, 7)) == E_STATE                      # no keys at all
    client.keygen_seeded()
    assert _code(lambda: client.fold_dev(d_c.data_ptr(), N + 2, d_w.data_ptr())) == E_STATE           # seeded keys, still no fold key
    assert _code(lambda: client.fold_key_sizes()) == E_STATE and _code(lambda: client.export_fold_key()) == E_STATE
    for t_f, gamma_f in ((4, 8), (1, 32), (2, 16), (3, 0), (0, 5), (32, 1)):
        assert _code(lambda: client.fold_keygen(t_f, gamma_f)) == E_INVALID, (t_f, gamma_f)
    assert client.stat("fold_key") == 0
    client.fold_keygen(2, 7)
    good = fold_dev(client, cts)
    exported = client.export_fold_key()
    assert client.fold_key_sizes() == client.fold_key_sizes(2) == (D * 2 * N, D * 2 * (prm.k + 1) * N)
    assert _code(lambda: client.fold_keygen(4, 8)) == E_INVALID and client.stat("fold_levels") == 2   # the key in place stays
    assert _code(lambda: client.fold_dev(d_c.data_ptr(), N + 2, d_w.data_ptr() + 8)) == E_INVALID     # 8 bytes off a 16-byte line
    assert _code(lambda: client.fold_dev(d_c.data_ptr(), 2 ** 62, d_w.data_ptr())) == E_INVALID       # count (D + 1) words overflow
    assert _code(lambda: client._check(lib.fbs_fold_dev(client._h, None, 3, d_w.data_ptr(), None))) == E_INVALID
    other = Context(prm, seed=4, keygen=False)
    other.keygen_seeded()
    other.fold_keygen(2, 7)
    with client.state(2, 5) as st, other.state(2, 5) as foreign:
        st.put(cts[:10].reshape(2, 5, D + 1))
        for row0, rows in ((0, 3), (2, 1), (3, 0)):                                # rows past the state
            assert _code(lambda: client._check(lib.fbs_state_fold(client._h, st._h, row0, rows, out.ctypes.data))) == E_INVALID
            assert _code(lambda: client._check(lib.fbs_state_fold_dev(client._h, st._h, row0, rows, d_w.data_ptr()))) == E_INVALID
            assert _code(lambda: client._check(lib.fbs_state_unfold_dev(client._h, st._h, row0, rows, d_w.data_ptr()))) == E_INVALID
        for entry in (lib.fbs_state_fold_dev, lib.fbs_state_unfold_dev):           # a state of another context
            assert _code(lambda: client._check(entry(client._h, foreign._h, 0, 1, d_w.data_ptr()))) == E_INVALID
        assert _code(lambda: client._check(lib.fbs_state_fold(client._h, foreign._h, 0, 1, out.ctypes.data))) == E_INVALID
        assert _code(lambda: client._check(lib.fbs_state_fold(client._h, st._h, 0, 1, None))) == E_INVALID
        assert np.array_equal(st.fetch(), cts[:10].reshape(2, 5, D + 1)) and untouched()
    other.close()
    # an evaluation-only context: no fold keygen; non-canonical bodies leave its key in place
    server = Context.evaluation_only(prm, **client.export_seeded_keys())
    assert _code(lambda: server.fold_keygen(2, 7)) == E_STATE
    server.import_fold_key(2, 7, exported["fold_bodies"])
    bad = exported["fold_bodies"].copy()
    bad[-1] = Q
    assert _code(lambda: server.import_fold_key(2, 7, bad)) == E_INVALID
    assert _code(lambda: server.import_fold_key(2, 16, exported["fold_bodies"])) == E_INVALID
    assert server.stat("fold_levels") == 2 and untouched()
    assert np.array_equal(fold_dev(server, cts), good) and np.array_equal(fold_dev(client, cts), good)
    server.close()
    client.close()


def test_gadget_key_refusals_word_for_word():
    """(call, code, text) of every refusal of the fold key's entries and of the imports of both keys, as the library said them before
    the packing and fold keys were given one code path (tests/test_client_lib.py pins the packing key's on the client library)"""
    from tfhe_fbs_map_amd import Context, FbsError, _native as nat
    lib = nat.lib
    prm = F.fold_toy(8, 2)
    N, D = prm.N, prm.k * prm.N

    def refused(call, code, text):
        with pytest.raises(FbsError) as e:
            call()
        assert (e.value.code, str(e.value)) == (code, f"libfbsexec error {code}: {text}"), (code, text, str(e.value))

    def raw(ctx, entry, *args):
        return lambda: ctx._check(entry(ctx._h, *args))

    no_keys, eval_only = "fbs_keygen has not run", "this context holds evaluation keys only"
    ctx = Context(prm, seed=5, keygen=False)                                       # no keys at all
    good = np.zeros(D * 2 * N, np.uint64)
    refused(lambda: ctx.fold_keygen(2, 7), E_STATE, no_keys)
    refused(lambda: ctx.import_fold_key(2, 7, good), E_STATE, no_keys)
    refused(lambda: ctx.import_packing_key(2, 7, good[:prm.n * 2 * N]), E_STATE, no_keys)
    refused(lambda: ctx.fold_key_sizes(0), E_STATE, "the context has no fold key")
    refused(raw(ctx, lib.fbs_export_fold_key, good.ctypes.data, None), E_STATE, "the context has no fold key")
    refused(lambda: ctx.fold_key_sizes(32), E_INVALID, "fold key needs 1 <= t_f <= 31")
    ctx.keygen()                                                                   # plain keys, not seeded ones
    refused(lambda: ctx.fold_keygen(2, 7), E_STATE, "a fold key goes with seeded keys (fbs_keygen_seeded)")
    refused(lambda: ctx.import_fold_key(2, 7, good), E_STATE, "a fold key goes with seeded keys (fbs_import_seeded_keys)")
    refused(lambda: ctx.import_packing_key(2, 7, good[:prm.n * 2 * N]), E_STATE, "a packing key goes with seeded keys (fbs_import_seeded_keys)")
    ctx.keygen_seeded()
    for (t, g), text in (((0, 1), "fold key needs t_f >= 1 and gamma_f >= 1"), ((1, 0), "fold key needs t_f >= 1 and gamma_f >= 1"),
                         ((32, 1), "fold key needs t_f * gamma_f <= 31"), ((4, 8), "fold key needs t_f * gamma_f <= 31")):
        refused(lambda: ctx.fold_keygen(t, g), E_INVALID, text)
    refused(lambda: ctx.fold_key_sizes(0), E_STATE, "the context has no fold key")
    refused(lambda: ctx.fold_key_sizes(32), E_INVALID, "fold key needs 1 <= t_f <= 31")
    refused(raw(ctx, lib.fbs_export_fold_key, good.ctypes.data, None), E_STATE, "the context has no fold key")
    d_c = dev(np.zeros((2, D + 1), np.uint64))
    refused(lambda: ctx.fold_dev(d_c.data_ptr(), 1, d_c.data_ptr()), E_STATE, "the context has no fold key (fbs_fold_keygen / fbs_import_fold_key)")
    refused(lambda: ctx.pack_dev(d_c.data_ptr(), 1, d_c.data_ptr(), 31), E_STATE,
            "the context has no packing key (fbs_packing_keygen / fbs_import_packing_key)")
    server = Context.evaluation_only(prm, **ctx.export_seeded_keys())              # no secret: no keygen of either kind
    refused(lambda: server.fold_keygen(2, 7), E_STATE, eval_only)
    refused(lambda: server.packing_keygen(2, 7), E_STATE, eval_only)
    bad = good.copy()
    bad[-1] = Q
    for noun, letter, entry, rows in (("fold", "f", lib.fbs_import_fold_key, D), ("packing", "p", lib.fbs_import_packing_key, prm.n)):
        bodies = good[:rows * 2 * N]
        refused(raw(server, entry, 2, 7, None), E_INVALID, "null argument")
        refused(raw(server, entry, 2, 7, bad[-rows * 2 * N:].ctypes.data), E_INVALID, f"{noun}-key body word is not a canonical residue")
        refused(raw(server, entry, 2, 16, bodies.ctypes.data), E_INVALID, f"{noun} key needs t_{letter} * gamma_{letter} <= 31")
        refused(raw(server, entry, 0, 7, bodies.ctypes.data), E_INVALID, f"{noun} key needs t_{letter} >= 1 and gamma_{letter} >= 1")
        assert server.stat(noun + "_key") == 0
    server.close()
    ctx.close()


@pytest.mark.parametrize("log_n,k", [(8, 2), (9, 1)])
def test_both_gadget_keys_on_one_context(log_n, k):
    """A packing key and a fold key on one context: each output is word for word what a context holding that key alone returns, also
    interleaved (the fields and accumulator scratch is shared); making or refusing one key leaves the other where it was; new seeded
    keys drop both.  Two samples, the second a one-coefficient tail.  At (9, 1) -- the other transform class, k = 1 -- the interleaving
    alone."""
    from tfhe_fbs_map_amd import Context
    prm = F.fold_toy(log_n, k)
    assert prm.n == 12
    N, D = prm.N, prm.k * prm.N
    cts = F.planted_cts(D, N + 1, 2, 9, seed=31, N=N)

    def keyed_with(packing, folding):
        ctx = Context(prm, seed=17, keygen=False)
        ctx.keygen_seeded()
        if packing:
            ctx.packing_keygen(2, 9)
        if folding:
            ctx.fold_keygen(2, 9)
        return ctx

    alone_p, alone_f = keyed_with(True, False), keyed_with(False, True)
    packed, folded = alone_p.pack(cts, 31), alone_f.fold(cts)
    assert packed.size == alone_p.packed_words(N + 1, 31) and folded.size == 2 * (k + 1) * N
    alone_p.close()
    alone_f.close()
    both = keyed_with(True, True)
    for _ in range(2):                                                             # pack, fold, pack, fold
        assert np.array_equal(both.pack(cts, 31), packed)
        assert np.array_equal(both.fold(cts), folded)
    if (log_n, k) != (8, 2):
        both.close()
        return
    pack_key, fold_key_ = both.export_packing_key(), both.export_fold_key()
    assert (both.stat("packing_key"), both.stat("packing_levels"), both.stat("packing_base_bits")) == (1, 2, 9)
    assert (both.stat("fold_key"), both.stat("fold_levels"), both.stat("fold_base_bits")) == (1, 2, 9)

    def same(a, b):
        return a.keys() == b.keys() and all(np.array_equal(a[name], b[name]) for name in a)

    both.fold_keygen(3, 7)                                                         # a new fold key: the packing key stays
    assert both.stat("fold_levels") == 3 and both.stat("packing_levels") == 2 and same(both.export_packing_key(), pack_key)
    assert np.array_equal(both.pack(cts, 31), packed) and not np.array_equal(both.fold(cts), folded)
    both.fold_keygen(2, 9)
    assert same(both.export_fold_key(), fold_key_) and np.array_equal(both.fold(cts), folded)
    both.packing_keygen(3, 7)                                                      # and the other way round
    assert both.stat("packing_levels") == 3 and both.stat("fold_levels") == 2 and same(both.export_fold_key(), fold_key_)
    assert np.array_equal(both.fold(cts), folded) and not np.array_equal(both.pack(cts, 31), packed)
    both.packing_keygen(2, 9)
    assert same(both.export_packing_key(), pack_key) and np.array_equal(both.pack(cts, 31), packed)
    assert _code(lambda: both.import_fold_key(2, 16, fold_key_["fold_bodies"])) == E_INVALID           # t gamma > 31: nothing moves
    assert same(both.export_packing_key(), pack_key) and same(both.export_fold_key(), fold_key_)
    assert np.array_equal(both.pack(cts, 31), packed) and np.array_equal(both.fold(cts), folded)
    both.keygen_seeded()                                                           # new keys drop both
    assert both.stat("packing_key") == both.stat("fold_key") == 0
    both.close()
