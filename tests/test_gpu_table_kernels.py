"""The device primitives of encrypted tables (include/fbs_exec.h, "encrypted tables"; csrc/fbs_table.hip), word for word.

THE ROTATION THAT KEEPS ITS SAMPLE.  One case per rotation entry of fbs_kernel_catalog, at the recipe that reaches it (tests/helpers.py:
recipe, planted_set, n = 16), through fbs_rotate_compact_dev at bits = log2(2N) with FBS_ROTATE_NEGATE: the fields of a row are its
rotation amounts, k_ms_negate turns every one of the n + 1 into (2N - a) mod 2N, and the kernel leaves its WHOLE accumulator,
(k + 1) N canonical residues, through the accumulator exit.  The rows, the three genuine mapped-fold tables, the ids in device memory
(id 3 is out of range and reads table 0) and the subset REF_ROWS are those of tests/test_gpu_lookup_kernels.py; the reference is
tests/lookup_reference.py:blind_rotate_from on the negated row, computed once per parameter set.  Every word of every row f with
f % 60 in the subset is compared, and every other row must equal the row 60 before it.  The planted lists skip steps (zero must stay
zero) and, at two key bits a step, hold pairs whose negated sum wraps.  Without the flag, sample extraction of the output must be
fbs_lookup_compact_dev's ciphertext, word for word.

THE SUM OF SAMPLES.  k_glwe_add against numpy modulo q at N = 256 (k = 1, 4), 512 (k = 3) and 1024 (k = 2), 1, 2 and 7 sources, the
words q - 1 + q - 1, targets nobody names unchanged, and the refusals of the host (a target twice, a target out of range, sources
that overlap the targets), which write nothing."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests import lookup_reference as L
from tests import table_reference as R
from tests.helpers import PLANTED_DEFAULT_KNOBS, PLANTED_ROWS, PLANTED_STEPS, planted_amount_rows, planted_set, recipe
from tests.test_gpu_compact import pack
from tests.test_gpu_device_io import dev, host
from tests.test_gpu_lookup_kernels import N_TABLES, REF_ROWS, lookup_planted, table_of
from tests.test_gpu_rotation_amounts import SENTINEL, rotation_entries, set_of

pytestmark = pytest.mark.gpu

Q = orc.Q


def pytest_generate_tests(metafunc):
    if "kernel_name" in metafunc.fixturenames:
        metafunc.parametrize("kernel_name", rotation_entries())


def rotate_planted(ctx, fields, tables, count, negate):
    """rows f % 60 of `fields`, f < count, through fbs_rotate_compact_dev at log2(2N) bits -> [count][(k + 1) N]; the buffer is two
    samples longer than the launch, and those stay as they were"""
    import torch
    prm = ctx.params
    b = prm.log_n_poly + 1
    words = pack(fields[np.arange(count) % PLANTED_ROWS].astype(np.uint64), b)
    d_t = dev(np.array(tables))
    d_of = torch.from_numpy(table_of(np.arange(count)).astype(np.int32)).cuda()
    d_g = torch.full((count + 2, (prm.k + 1) * prm.N), SENTINEL, dtype=torch.int64, device="cuda")
    assert d_t.data_ptr() % 16 == 0 and d_g.data_ptr() % 16 == 0
    ctx.rotate_compact_dev(d_t.data_ptr(), len(tables), d_of.data_ptr(), dev(words).data_ptr(), count, d_g.data_ptr(), bits=b, negate=negate)
    ctx.sync()
    out = host(d_g)
    assert (out[count:] == SENTINEL).all(), "wrote past the last sample"
    return out[:count]


def extract0(samples, k, N):
    """sample extraction of coefficient 0 of [count][(k + 1) N] -> [count][k N + 1]"""
    s = np.asarray(samples, np.uint64).reshape(len(samples), k + 1, N)
    out = np.empty((len(s), k * N + 1), np.uint64)
    for c in range(k):
        out[:, c * N] = s[:, c, 0]
        out[:, c * N + 1:(c + 1) * N] = ((np.uint64(Q) - s[:, c, :0:-1]) % np.uint64(Q))
    out[:, k * N] = s[:, k, 0]
    return out


@pytest.fixture(scope="module")
def planted():
    """per parameter set: context, oracle on its keys, the 60 planted rows, the three tables, and the reference samples of REF_ROWS
    under the NEGATED amounts (computed once, never written to); ref=False: the context alone"""
    from tfhe_fbs_map_amd import Params, _native as nat
    ctxs, made = {}, {}

    def get(log_n, k, l, beta, group, ref=True):
        key = (log_n, k, l, beta, group)
        if key not in ctxs:
            ctxs[key] = nat.Context(Params(**planted_set(*key)), seed=33)
        if not ref:
            return ctxs[key]
        if key not in made:
            prm, ctx = planted_set(*key), ctxs[key]
            o = orc.Oracle(prm, seed=33, keygen=False)
            o.set_keys(**ctx.export_keys())
            N = 1 << log_n
            fields, _ = planted_amount_rows(N, PLANTED_STEPS, group, o.keys()["sk_lwe"], prm["p_msg"])
            tables, _ = L.encrypted_tables(o, prm, N_TABLES, seed=11)
            L._keys_of(o)                                        # (before the threads share it)
            eff = [int(t) if t < N_TABLES else 0 for t in table_of(REF_ROWS)]
            with ThreadPoolExecutor(8) as pool:
                ref = np.stack(list(pool.map(lambda jt: L.blind_rotate_from(o, R.negated_amounts(fields[jt[0]], N), tables[jt[1]]),
                                             zip(REF_ROWS, eff))))
            ref.setflags(write=False)
            tables.setflags(write=False)
            made[key] = (ctx, o, fields, tables, ref)
        return made[key]

    yield get
    for ctx in ctxs.values():
        ctx.close()


def test_negation_keeps_zero_and_wraps_pairs():
    """what the planted rows put in front of k_ms_negate: skipped steps, whose amounts must stay zero, and pairs whose negated
    amounts sum past 2N, so that the kernels' own third exponent is derived from the negated pair"""
    for group in (1, 2):
        fields, _ = planted_amount_rows(1024, PLANTED_STEPS, group, np.ones(PLANTED_STEPS, np.int64), 7)
        neg = R.negated_amounts(fields, 1024)
        assert ((fields == 0) == (neg == 0)).all() and (fields[REF_ROWS] == 0).any() and int(neg.max()) < 2048
        assert np.array_equal(R.negated_amounts(neg, 1024), fields)
        assert {int(fields[j, PLANTED_STEPS]) for j in REF_ROWS} >= {1023, 1024, 2047}       # the raw bodies N - 1, N, 2N - 1
        if group == 2:
            pairs = neg[REF_ROWS, :PLANTED_STEPS].reshape(len(REF_ROWS), -1, 2).astype(np.int64)
            sums = pairs.sum(axis=2)
            assert (sums > 2048).any() and (sums == 2048).any() and ((pairs[..., 0] == 0) != (pairs[..., 1] == 0)).any()


def test_whole_negated_rotation_against_the_reference(planted, kernel_name):
    rec = recipe(kernel_name)
    assert rec is not None, "no recipe reaches %s" % kernel_name
    ctx, _, fields, tables, ref = planted(*set_of(rec))
    ctx.tune(**{**PLANTED_DEFAULT_KNOBS, **rec["knobs"]})        # (the context is shared: the knobs are set per case)
    count = rec["count"]
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = rotate_planted(ctx, fields, tables, count, negate=True)
    launched = ctx.profile_kernels()
    ctx.profile(False)
    assert kernel_name in launched, (kernel_name, sorted(launched))
    assert got.max() < Q
    rows = np.arange(count) % PLANTED_ROWS
    at = {j: i for i, j in enumerate(REF_ROWS)}
    held = np.array([f for f in range(count) if rows[f] in at])
    want = ref[[at[j] for j in rows[held]]]
    wrong = held[(got[held] != want).any(axis=1)]                # ALL (k + 1) N words of every row of the subset
    assert wrong.size == 0, (kernel_name, "rows", wrong[:8].tolist(), "lists", sorted(set((wrong % 5).tolist())))
    if count > PLANTED_ROWS:                                     # ... and every other row through the row 60 before it
        again = np.flatnonzero((got[PLANTED_ROWS:] != got[:-PLANTED_ROWS]).any(axis=1)) + PLANTED_ROWS
        assert again.size == 0, (kernel_name, "repeats", again[:8].tolist())
    # without the flag: the sample whose coefficient 0 the lookup extracts
    plain = rotate_planted(ctx, fields, tables, count, negate=False)
    assert np.array_equal(extract0(plain, ctx.params.k, ctx.params.N), lookup_planted(ctx, fields, tables, count)), kernel_name


def test_rotation_of_big_key_indices_runs_the_key_switch_first(planted):
    """fbs_rotate_dev: the key switch and modulus switch of fbs_lookup_dev, the amounts negated, the rotation from the table -- the
    oracle's switch and the reference's rotation, word for word; and without the flag the sample fbs_lookup_dev extracts from"""
    import torch
    ctx, o, _, tables, _ = planted(10, 2, 1, 20, 2)
    ctx.tune(**PLANTED_DEFAULT_KNOBS)
    prm = ctx.params
    p, count = prm.p_msg, 9
    cts = ctx.encrypt(np.arange(count) % p, nonce0=5)
    ids = (np.arange(count) // 2) % 4
    eff = np.where(ids < N_TABLES, ids, 0)
    d_t, d_in = dev(np.array(tables)), dev(cts)
    d_of = torch.from_numpy(ids.astype(np.int32)).cuda()
    outs = {}
    for negate in (True, False):
        d_g = torch.full((count + 2, (prm.k + 1) * prm.N), SENTINEL, dtype=torch.int64, device="cuda")
        ctx.rotate_dev(d_t.data_ptr(), N_TABLES, d_of.data_ptr(), d_in.data_ptr(), count, d_g.data_ptr(), negate=negate)
        ctx.sync()
        got = host(d_g)
        assert (got[count:] == SENTINEL).all()
        outs[negate] = got[:count]
    ms = [o.modswitch(o.keyswitch(ct)) for ct in cts]
    want = np.stack([L.blind_rotate_from(o, R.negated_amounts(m, prm.N), tables[t]) for m, t in zip(ms, eff)])
    assert np.array_equal(outs[True], want)
    d_c = torch.full((count, prm.ct_words), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.lookup_dev(d_t.data_ptr(), N_TABLES, d_of.data_ptr(), d_in.data_ptr(), count, d_c.data_ptr())
    ctx.sync()
    assert np.array_equal(extract0(outs[False], prm.k, prm.N), host(d_c))


def test_rotation_refusals_write_nothing(planted):
    import torch
    from tfhe_fbs_map_amd import FbsError, _native as nat
    ctx, _, fields, tables, _ = planted(8, 4, 2, 8, 2)
    prm = ctx.params
    b = prm.log_n_poly + 1
    d_t, d_w = dev(np.array(tables)), dev(pack(fields[:4].astype(np.uint64), b))
    d_g = torch.full((6, (prm.k + 1) * prm.N), SENTINEL, dtype=torch.int64, device="cuda")
    d_c = dev(ctx.encrypt(np.arange(4), nonce0=9))
    lib, h = nat.lib, ctx._h
    for call, text in ((lambda: ctx.rotate_compact_dev(d_t.data_ptr() + 8, 3, 0, d_w.data_ptr(), 4, d_g.data_ptr(), bits=b), "16-byte aligned"),
                       (lambda: ctx.rotate_compact_dev(d_t.data_ptr(), 3, 0, d_w.data_ptr(), 4, d_g.data_ptr() + 8, bits=b), "d_glwe_out must be 16-byte aligned"),
                       (lambda: ctx.rotate_compact_dev(d_t.data_ptr(), 0, 0, d_w.data_ptr(), 4, d_g.data_ptr(), bits=b), "at least one table"),
                       (lambda: ctx.rotate_compact_dev(d_t.data_ptr(), 3, 0, d_w.data_ptr(), 4, d_g.data_ptr(), bits=b - 1), "compact width"),
                       (lambda: ctx._check(lib.fbs_rotate_compact_dev(h, d_t.data_ptr(), 3, None, d_w.data_ptr(), 4, b, 2, d_g.data_ptr(), None)), "unknown flag"),
                       (lambda: ctx._check(lib.fbs_rotate_dev(h, d_t.data_ptr(), 3, None, d_c.data_ptr(), 4, 6, d_g.data_ptr(), None)), "unknown flag"),
                       (lambda: ctx.rotate_dev(d_t.data_ptr(), 3, 0, d_c.data_ptr(), 4, d_g.data_ptr() + 8), "d_glwe_out must be 16-byte aligned"),
                       (lambda: ctx.rotate_dev(d_t.data_ptr(), 0, 0, d_c.data_ptr(), 4, d_g.data_ptr()), "at least one table")):
        with pytest.raises(FbsError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value)
    ctx.rotate_compact_dev(d_t.data_ptr(), 3, 0, d_w.data_ptr(), 0, d_g.data_ptr(), bits=b, negate=True)   # nothing to turn: nothing done
    ctx.sync()
    assert (host(d_g) == SENTINEL).all()


# ---- k_glwe_add -----------------------------------------------------------------------------------------------------------------------
ADD_SHAPES = {(8, 1): (8, 1, 3, 7, 1), (8, 4): (8, 4, 2, 8, 2), (9, 3): (9, 3, 2, 8, 2), (10, 2): (10, 2, 1, 20, 2)}


@pytest.mark.parametrize("shape", sorted(ADD_SHAPES))
def test_glwe_add_is_the_sum_modulo_q(planted, shape):
    import torch
    from tfhe_fbs_map_amd import FbsError
    ctx = planted(*ADD_SHAPES[shape], ref=False)
    prm = ctx.params
    words = (prm.k + 1) * prm.N
    rng = np.random.default_rng([7, words])
    n_dst = 9
    for count in (1, 2, 7):
        dst = rng.integers(0, Q, (n_dst, words), dtype=np.uint64)
        src = rng.integers(0, Q, (count, words), dtype=np.uint64)
        dst[0, :3], dst[0, -2:] = Q - 1, Q - 1                                   # q - 1 + q - 1 at both ends of a sample
        src[0, :3], src[0, -2:] = Q - 1, Q - 1
        dst[1, 0], src[0, 5] = 0, 0
        dst_of = np.append(0, rng.permutation(np.arange(1, n_dst))[:count - 1]).astype(np.uint32)   # source 0 -> target 0, no order
        d_dst = torch.cat([dev(dst), torch.full((1, words), SENTINEL, dtype=torch.int64, device="cuda")])
        d_src = dev(src)
        ctx.glwe_add_dev(d_dst.data_ptr(), n_dst, dst_of, d_src.data_ptr())
        ctx.sync()
        got = host(d_dst)
        want = dst.copy()
        want[dst_of] = (dst[dst_of] + src) % np.uint64(Q)
        assert (got[n_dst] == SENTINEL).all() and np.array_equal(got[:n_dst], want), (shape, count)
        assert int(got[0, 0]) == Q - 2
        untouched = np.setdiff1d(np.arange(n_dst), dst_of)
        assert untouched.size == n_dst - count and np.array_equal(got[untouched], dst[untouched])
        assert np.array_equal(host(d_src), src)
    # refusals: the host checks the targets, and nothing is written
    d_dst, d_src = dev(dst), dev(src)
    for bad, text in (([0, 3, 3], "written twice"), ([0, n_dst, 2], "is past the"), ([1, 2, 0xFFFFFFFF], "is past the")):
        with pytest.raises(FbsError) as e:
            ctx.glwe_add_dev(d_dst.data_ptr(), n_dst, bad, d_src.data_ptr())
        assert e.value.code == -1 and text in str(e.value), bad
    with pytest.raises(FbsError) as e:
        ctx.glwe_add_dev(d_dst.data_ptr() + 8, n_dst - 1, [0], d_src.data_ptr())
    assert "16-byte aligned" in str(e.value)
    with pytest.raises(FbsError) as e:
        ctx.glwe_add_dev(d_dst.data_ptr(), 2, [0, 1, 1], d_src.data_ptr())
    assert "more sources than targets" in str(e.value)
    for inside in (d_dst.data_ptr() + words * 8, d_dst.data_ptr() + (n_dst - 1) * words * 8):       # the sources within the targets
        with pytest.raises(FbsError) as e:
            ctx.glwe_add_dev(d_dst.data_ptr(), n_dst, [0], inside)
        assert e.value.code == -1 and "overlap" in str(e.value)
    ctx.glwe_add_dev(d_dst.data_ptr(), n_dst, [], d_src.data_ptr())
    ctx.sync()
    assert np.array_equal(host(d_dst), dst) and np.array_equal(host(d_src), src)
