"""The packing kernels of csrc/fbs_pack.hip (k_pack_transpose, k_pack_accumulate, k_pack_finish) at every (k, N) they are
instantiated for, word for word against the definition (tests/helpers.py: the oracle's NTT products, held to the schoolbook
restatement and to the host decode by tests/test_packed_reference.py).  The fields are planted (planted_pack_fields: the wrap and
the tie of the mask rounding, both ends of every digit, the carry dropped at the top, the body fields where pack_lift_body's floor
term changes sign) and go in through fbs_debug_pack_fields_dev, which is fbs_pack_dev without its key switch; fbs_pack_dev itself
is tied to the hook once per shape, at the default 128-bit set's real size, and across more than one pass.  Every comparison is
exact; every output buffer is two samples longer than needed and the rest must keep its sentinel; the fields buffer carries 64 rows
of 0xFFFFFFFF past `count` that must change nothing."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_compact import compact_on_device, unpack
from tests.test_gpu_device_io import dev, host

pytestmark = pytest.mark.gpu

Q = H.Q
E_INVALID, E_STATE = -1, -3
SENTINEL = 0x5A5A5A5A5A5A5A5A
EDGE_SHAPES = [(8, 1), (11, 1), (12, 1), (9, 3), (10, 2)]   # PolyNtt at 4 and 8 and 16 words a lane, the two classes above N = 1024
_CTX = {}


def keyed(log_n, k, n=6):
    """a context keyed with fbs_keygen_seeded for the toy set of a shape, made once per module"""
    if (log_n, k, n) not in _CTX:
        from tfhe_fbs_map_amd import Context
        ctx = Context(H.pack_toy(log_n, k, n), seed=17, keygen=False)
        ctx.keygen_seeded()
        _CTX[log_n, k, n] = ctx
    return _CTX[log_n, k, n]


def packing_key(ctx, t_p, gamma_p):
    ctx.packing_keygen(t_p, gamma_p)
    assert (ctx.stat("packing_key"), ctx.stat("packing_levels"), ctx.stat("packing_base_bits")) == (1, t_p, gamma_p)
    return ctx.export_packing_key(full=True)["full"]


def words_out(ctx, count, bits):
    """(device buffer of sentinels, words of the batch): the buffer is two full samples longer"""
    import torch
    W = ctx.packed_words(count, bits)
    pad = 2 * ctx.packed_words(ctx.params.N, bits)
    return torch.full((W + pad,), SENTINEL, dtype=torch.int64, device="cuda"), W


def checked(d_w, W):
    out = host(d_w)
    assert (out[W:] == np.uint64(SENTINEL)).all(), "words written past the batch"
    return out[:W]


def hook(ctx, fields, bits):
    """fbs_debug_pack_fields_dev on fields [count][n + 1], 64 rows of 0xFFFFFFFF behind them"""
    import torch
    count, n1 = fields.shape
    assert n1 == ctx.params.n + 1 and int(fields.max()) < 1 << 31
    buf = np.full((count + 64, n1), 0xFFFFFFFF, np.uint32)
    buf[:count] = fields
    d_f = torch.from_numpy(buf.view(np.int32)).cuda()
    d_w, W = words_out(ctx, count, bits)
    ctx.debug_pack_fields_dev(d_f.data_ptr(), count, d_w.data_ptr(), bits)
    ctx.sync()
    return checked(d_w, W)


def pack_dev(ctx, cts, bits):
    """fbs_pack_dev on host ciphertexts"""
    d_c = dev(cts)
    d_w, W = words_out(ctx, cts.shape[0], bits)
    ctx.pack_dev(d_c.data_ptr(), cts.shape[0], d_w.data_ptr(), bits)
    ctx.sync()
    return checked(d_w, W)


def random_cts(prm, count, seed):
    return np.random.default_rng(seed).integers(0, Q, (count, prm.ct_words), dtype=np.uint64)


def switched_fields(ctx, cts):
    """what step 1 leaves: the fields of fbs_compact_dev at 31 bits"""
    return unpack(compact_on_device(ctx, cts, 31), ctx.params.n, 31).astype(np.uint32)


# ---- a. every shape --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", H.PACK_KEYS)
@pytest.mark.parametrize("log_n,k", H.PACK_SHAPES)
def test_every_shape_packs_planted_fields_word_for_word(log_n, k, t_p, gamma_p):
    ctx = keyed(log_n, k)
    prm = ctx.params
    N, n = prm.N, prm.n
    assert (prm.log_n_poly, prm.k, n) == (log_n, k, 6)
    key = packing_key(ctx, t_p, gamma_p)
    tag = (log_n, k, n)
    try:
        for count in (1, N - 1, N, N + 1):
            fields = H.planted_pack_fields(n, count, t_p, gamma_p, seed=100 * log_n + count % 7)
            for bits in (log_n + 1, 31) + ((17,) if count == N + 1 else ()):
                want = H.reference_pack(fields, key, t_p, gamma_p, bits, tag, fast=True)
                assert want.size == ctx.packed_words(count, bits) == H.packed_count(k, N, count, bits)
                assert np.array_equal(hook(ctx, fields, bits), want), (count, bits)
        want = H.reference_pack(fields, key, t_p, gamma_p, 17, tag, fast=True)        # count N + 1: two samples, the second of one
        for slices in (1, 2, 5, 32, 0):                                                 # (32 is cut to n)
            ctx.tune(pack_slices=slices)
            assert np.array_equal(hook(ctx, fields, 17), want), slices
    finally:
        ctx.tune(pack_slices=0)


@pytest.mark.parametrize("log_n,k", H.PACK_SHAPES)
def test_pack_dev_is_the_hook_on_its_own_key_switch(log_n, k):
    ctx = keyed(log_n, k)
    prm = ctx.params
    packing_key(ctx, 1, 27)
    cts = random_cts(prm, prm.N + 3, seed=log_n + k)
    fields = switched_fields(ctx, cts)
    for bits in (log_n + 1, 31):
        assert np.array_equal(pack_dev(ctx, cts, bits), hook(ctx, fields, bits)), bits


# ---- b. edge key parameters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", H.PACK_EDGE_KEYS)
@pytest.mark.parametrize("log_n,k", EDGE_SHAPES)
def test_edge_key_parameters(log_n, k, t_p, gamma_p):
    """r = 31 - t_p gamma_p = 0 with the widest digit (|d| <= 2^30) and with the most levels (31 of one bit), and r = 1"""
    ctx = keyed(log_n, k)
    prm = ctx.params
    key = packing_key(ctx, t_p, gamma_p)
    count = prm.N + 1
    fields = H.planted_pack_fields(prm.n, count, t_p, gamma_p, seed=log_n + t_p)
    for bits in (log_n + 1, 31):
        want = H.reference_pack(fields, key, t_p, gamma_p, bits, (log_n, k, prm.n), fast=True)
        assert np.array_equal(hook(ctx, fields, bits), want), bits


# ---- c. tiles of the transposition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64])
def test_transposition_tiles(n):
    """n + 1 = 64: one exactly full column of tiles; n + 1 = 65: a second column that holds the body alone"""
    ctx = keyed(8, 1, n)
    prm = ctx.params
    assert prm.bsk_group == 1
    key = packing_key(ctx, 1, 27)
    count = prm.N + 3
    fields = H.planted_pack_fields(n, count, 1, 27, seed=n)
    want = H.reference_pack(fields, key, 1, 27, 9, (8, 1, n), fast=True)
    assert np.array_equal(hook(ctx, fields, 9), want)
    ctx.close()
    del _CTX[8, 1, n]


# ---- d. the default set at its real size -------------------------------------------------------------------------------------------
def test_default_set_at_its_real_size():
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, packing_choice
    prm = choose_params(15, 70, glwe_dims=(1, 2))
    assert (prm.k, prm.N, prm.n) == (2, 1024, 734) and (prm.n + 1) % 64 == 31
    t_p, gamma_p, bits = packing_choice(prm, 70, 1.0)
    assert (t_p, gamma_p) == (1, 27)
    ctx = Context(prm, seed=13, keygen=False, device_keys=True)
    ctx.keygen_seeded()
    key = packing_key(ctx, t_p, gamma_p)
    count = prm.N + 3
    fields = H.planted_pack_fields(prm.n, count, t_p, gamma_p, seed=5)
    want = H.reference_pack(fields, key, t_p, gamma_p, bits, "default", fast=True)
    assert np.array_equal(hook(ctx, fields, bits), want)
    cts = random_cts(prm, count, seed=6)
    assert np.array_equal(pack_dev(ctx, cts, bits), hook(ctx, switched_fields(ctx, cts), bits))
    ctx.close()


# ---- e. more than one pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,t_p,gamma_p", [(8, 3, 10), (12, 1, 27)])
def test_more_than_one_pass(log_n, t_p, gamma_p):
    from tfhe_fbs_map_amd import Context
    ctx = Context(H.pack_toy(log_n, 1, 6), seed=19, keygen=False)
    ctx.keygen_seeded()
    prm = ctx.params
    N, bits = prm.N, log_n + 1
    key = packing_key(ctx, t_p, gamma_p)
    whole = max(ctx.stat("ms_capacity"), 8192) // N * N
    count = whole + N + 3
    cts = random_cts(prm, count, seed=log_n)
    got = pack_dev(ctx, cts, bits)
    assert ctx.stat("ms_capacity") < count                                             # so the call took two passes
    growths = ctx.stat("scratch_growths")
    again = pack_dev(ctx, cts, bits)
    assert ctx.stat("scratch_growths") == growths and np.array_equal(again, got)
    with ctx.state(1, count) as st:
        st.put(cts.reshape(1, count, prm.ct_words))
        assert np.array_equal(st.fetch_packed(bits), got)
    fields = switched_fields(ctx, cts)
    want = H.reference_pack(fields, key, t_p, gamma_p, bits, ("passes", log_n), fast=True)
    assert want.size == got.size and np.array_equal(got, want)
    # and the hook takes one pass and no more, refused with nothing written
    import torch
    from tfhe_fbs_map_amd import FbsError
    d_f = torch.zeros((count, prm.n + 1), dtype=torch.int32, device="cuda")
    d_w, W = words_out(ctx, count, bits)
    with pytest.raises(FbsError) as e:
        ctx.debug_pack_fields_dev(d_f.data_ptr(), count, d_w.data_ptr(), bits)
    assert e.value.code == E_INVALID and "one pass" in str(e.value)
    ctx.sync()
    assert (host(d_w) == np.uint64(SENTINEL)).all()
    ctx.close()


# ---- the hook refuses what fbs_pack_dev refuses --------------------------------------------------------------------------------------
def test_hook_refusals_write_nothing():
    import torch
    from tfhe_fbs_map_amd import Context, FbsError
    prm = H.pack_toy(8, 2, 6)
    fields = H.planted_pack_fields(prm.n, prm.N + 2, 2, 7, seed=1)
    d_f = torch.from_numpy(fields.view(np.int32)).cuda()
    d_w = torch.full((4096,), SENTINEL, dtype=torch.int64, device="cuda")

    def code(ctx, bits=9, d_fields=d_f.data_ptr(), d_words=d_w.data_ptr()):
        try:
            ctx.debug_pack_fields_dev(d_fields, prm.N + 2, d_words, bits)
        except FbsError as e:
            return e.code
        return 0

    ctx = Context(prm, seed=3, keygen=False)
    assert code(ctx) == E_STATE                                                        # no keys
    ctx.keygen_seeded()
    assert code(ctx) == E_STATE                                                        # seeded keys, no packing key
    ctx.packing_keygen(2, 7)
    for bad in (8, 32, 0):
        assert code(ctx, bits=bad) == E_INVALID
    assert code(ctx, d_fields=0) == E_INVALID and code(ctx, d_words=0) == E_INVALID
    ctx.sync()
    assert (host(d_w) == np.uint64(SENTINEL)).all()
    key = ctx.export_packing_key(full=True)["full"]
    assert np.array_equal(hook(ctx, fields, 9), H.reference_pack(fields, key, 2, 7, 9, "refusals", fast=True))
    ctx.close()
