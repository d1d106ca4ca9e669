"""The mapped fold on the GPU (include/fbs_exec.h, "encrypted-index reads"; k_fold_front_mapped of csrc/fbs_fold.hip): by definition
fbs_fold_mapped_dev is WORD FOR WORD fbs_fold_dev of the materialised array (tests/lookup_reference.py, materialise), and that is
all that is compared here -- the plain fold itself is held to the definition by tests/test_gpu_fold.py.

Shapes: N = 256 at k = 1 and 4, 512 at k = 3, 1024 at k = 2 (the toy sets of tests/fold_reference.py).  Maps: the box map at p = 3
and p = 7 with len < p (none-values, the negated half box), the identity (the plain fold of the sources), all-negated, and a map
with indices past the sources (which read source 0).  Counts 1, N - 1, N, N + 1; the source array starts at both 16-byte
alignments; 64 rows of all-ones words lie behind the sources and map entries that name source 0 behind the map, and neither may
show; the output is two samples longer than needed and the rest must keep its sentinel."""
import numpy as np
import pytest

from tests import lookup_reference as L
from tests.test_gpu_device_io import dev, host
from tests.test_gpu_fold import E_INVALID, E_STATE, Q, SENTINEL, fold_dev, keyed

pytestmark = pytest.mark.gpu

SHAPES = [(8, 1), (8, 4), (9, 3), (10, 2)]
KINDS = ["box_p3", "box_p7", "identity", "negated", "out_of_range"]
_SRC = {}


def sources(ctx):
    """N + 1 random ciphertexts of a shape, made once"""
    prm = ctx.params
    key = (prm.log_n_poly, prm.k)
    if key not in _SRC:
        _SRC[key] = np.random.default_rng([31, *key]).integers(0, Q, (prm.N + 1, prm.ct_words), dtype=np.uint64)
        _SRC[key].setflags(write=False)
    return _SRC[key]


def the_map(kind, count, N, n_src):
    if kind.startswith("box"):
        p, length = (3, 2) if kind == "box_p3" else (7, 5)
        box = L.lookup_map(p, N, length, base=1, stride=3)                        # sources 1, 4, 7, ..: a stride, a base
        assert L.MAP_NONE in box and (1 | L.MAP_NEG) in box
        return np.tile(box, 2)[:count]
    ids = np.arange(count, dtype=np.uint32)
    if kind == "identity":
        return ids
    if kind == "negated":
        return ids | np.uint32(L.MAP_NEG)
    rng = np.random.default_rng(count)
    m = rng.integers(0, n_src, count, dtype=np.uint32)
    m[::3] = rng.integers(n_src, L.MAP_NEG, len(m[::3]), dtype=np.uint32)        # past the sources: source 0
    m[1::5] |= np.uint32(L.MAP_NEG)
    m[0] = 0x7FFFFFFE                                                             # the largest index that is not the none-value's
    if count > 2:
        m[2] = 0xFFFFFFFE                                                         # ... negated: minus source 0
    return m


def fold_mapped(ctx, cts, fmap, offset):
    import torch
    prm = ctx.params
    n_src, count = cts.shape[0], len(fmap)
    buf = np.full(offset + (n_src + 64) * prm.ct_words, 0xFFFFFFFFFFFFFFFF, np.uint64)
    buf[offset:offset + n_src * prm.ct_words] = cts.reshape(-1)
    d_c = dev(buf)
    d_m = torch.from_numpy(np.concatenate([np.asarray(fmap, np.uint32), np.zeros(64, np.uint32)]).view(np.int32)).cuda()
    W = -(-count // prm.N) * (prm.k + 1) * prm.N
    d_w = torch.full((W + 2 * (prm.k + 1) * prm.N,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fold_mapped_dev(d_c.data_ptr() + 8 * offset, n_src, d_m.data_ptr(), count, d_w.data_ptr())
    ctx.sync()
    out = host(d_w)
    assert (out[W:] == np.uint64(SENTINEL)).all(), "words written past the batch"
    return out[:W]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_n,k", SHAPES)
def test_mapped_fold_is_the_fold_of_the_materialised_array(log_n, k, kind):
    ctx = keyed(log_n, k)
    ctx.fold_keygen(3, 10)
    N = ctx.params.N
    cts = sources(ctx)
    for at, count in enumerate((1, N - 1, N, N + 1)):
        n_src = len(cts) if kind in ("identity", "negated") else 17
        fmap = the_map(kind, count, N, n_src)
        offset = (at + KINDS.index(kind)) & 1                                     # both alignments for every kind and every count parity
        got = fold_mapped(ctx, cts[:n_src], fmap, offset)
        want = fold_dev(ctx, L.materialise(cts[:n_src], fmap), offset=at & 1)
        assert np.array_equal(got, want), (kind, count, int((got != want).sum()))
        if kind == "identity":
            assert np.array_equal(got, fold_dev(ctx, cts[:count]))
        assert got.max() < Q


def test_two_passes_take_their_part_of_the_map():
    """8192 positions a pass at N = 256: the second pass reads the map from where the first stopped, the sources from their start"""
    ctx = keyed(8, 1)
    ctx.fold_keygen(3, 10)
    N = ctx.params.N
    cts = sources(ctx)[:9]
    count = 8192 + N + 3
    fmap = np.random.default_rng(4).integers(0, 9, count, dtype=np.uint32)
    fmap[8192:8192 + N] = L.lookup_map(7, N, 7, base=2, stride=1)
    got = fold_mapped(ctx, cts, fmap, 0)
    assert np.array_equal(got, fold_dev(ctx, L.materialise(cts, fmap)))


def test_refusals_write_nothing():
    import torch
    from tfhe_fbs_map_amd import Context, FbsError
    from tests import fold_reference as F
    ctx = keyed(8, 1)
    ctx.fold_keygen(3, 10)
    prm = ctx.params
    d_c = dev(sources(ctx)[:4].copy())
    d_m = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_w = torch.full((4 * prm.N + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    for args, code, text in (((d_c.data_ptr(), 4, d_m.data_ptr(), 8, d_w.data_ptr() + 8), E_INVALID, "16-byte aligned"),
                             ((d_c.data_ptr(), 0, d_m.data_ptr(), 8, d_w.data_ptr()), E_INVALID, "source ciphertexts"),
                             ((d_c.data_ptr(), 1 << 31, d_m.data_ptr(), 8, d_w.data_ptr()), E_INVALID, "source ciphertexts"),
                             ((0, 4, d_m.data_ptr(), 8, d_w.data_ptr()), E_INVALID, ""),
                             ((d_c.data_ptr(), 4, 0, 8, d_w.data_ptr()), E_INVALID, "")):
        with pytest.raises(FbsError) as e:
            ctx.fold_mapped_dev(*args)
        assert e.value.code == code and text in str(e.value), args
    ctx.fold_mapped_dev(d_c.data_ptr(), 4, d_m.data_ptr(), 0, d_w.data_ptr())      # nothing to fold: nothing done
    bare = Context(F.fold_toy(8, 1), seed=18, keygen=False)
    bare.keygen_seeded()
    with pytest.raises(FbsError) as e:
        bare.fold_mapped_dev(d_c.data_ptr(), 4, d_m.data_ptr(), 8, d_w.data_ptr())
    assert e.value.code == E_STATE and "fold key" in str(e.value)
    bare.close()
    ctx.sync()
    assert (host(d_w) == np.uint64(SENTINEL)).all()
