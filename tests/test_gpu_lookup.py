"""Encrypted-index reads end to end (include/fbs_exec.h, "encrypted-index reads").  At the level of a context: tables laid out by
fbs_fold_mapped_dev under the box map of fbs_lookup_map, read by fbs_lookup_dev with encrypted indices, decrypted; the noise of such
a read at the default set against the model of params.lookup_output_norm2.  Through `Client` and `Server` (cases a to f): resident
tables read by resident indices with `Server.lookup` -- per-sample, shared and sample-axis tables, planes that share a key switch,
two digits, fbs_state_lookup word for word against the device entries, the refusals.  The resident rows are fresh encryptions
under the client's key restored into the server (`Server.restore`); results are read with the client's own context, since
`Client.decrypt` names outputs by a program's."""
import numpy as np
import pytest

from tests.helpers import PLANTED_FAMILIES, planted_set
from tests.test_gpu_compact import pack
from tests.test_gpu_device_io import dev, host

pytestmark = pytest.mark.gpu

Q = 0x3FFFFFF84001


def upload_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def fold_tables(ctx, cts, fmap):
    """fbs_fold_mapped_dev of host ciphertexts under a host map of whole samples -> device tensor [len(fmap) / N][k+1][N]"""
    import torch
    prm = ctx.params
    assert len(fmap) % prm.N == 0
    d_c, d_m = dev(cts), upload_u32(fmap)
    d_t = torch.zeros((len(fmap) // prm.N, prm.k + 1, prm.N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fold_mapped_dev(d_c.data_ptr(), len(cts), d_m.data_ptr(), len(fmap), d_t.data_ptr())
    ctx.sync()
    return d_t


def lookup(ctx, d_tables, index_cts, table_of=None):
    import torch
    count = len(index_cts)
    d_i = dev(index_cts)
    d_of = None if table_of is None else upload_u32(table_of)
    d_o = torch.zeros((count, ctx.params.ct_words), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.lookup_dev(d_tables.data_ptr(), d_tables.shape[0], 0 if d_of is None else d_of.data_ptr(), d_i.data_ptr(), count, d_o.data_ptr())
    ctx.sync()
    return host(d_o)


@pytest.fixture(scope="module")
def ctx():
    from tfhe_fbs_map_amd import Context, Params
    c = Context(Params(**planted_set(**PLANTED_FAMILIES["k2_n1024_g2"])), seed=41, keygen=False)
    c.keygen_seeded()
    c.fold_keygen(2, 10)
    yield c
    c.close()


@pytest.mark.parametrize("length", [7, 5])
def test_every_sample_reads_its_own_table_by_its_own_index(ctx, length):
    """T = 8 samples, each with a table of its own (`length` entries of 0 .. p - 1) and every index value: entry index, or 0 past
    the table's length (the none-value: a zero phase)"""
    from tfhe_fbs_map_amd import _native as nat
    p, N, T = ctx.params.p_msg, ctx.params.N, 8
    rng = np.random.default_rng(length)
    entries = rng.integers(0, p, (T, length))
    cts = ctx.encrypt(entries.reshape(-1), nonce0=100)
    fmap = np.concatenate([nat.lookup_map(p, N, length, base=s * length) for s in range(T)])
    d_t = fold_tables(ctx, cts, fmap)
    for x in range(p):
        index = ctx.encrypt(np.full(T, x), nonce0=1000 + 10 * x)
        want = entries[:, x] if x < length else np.zeros(T, np.int64)
        assert np.array_equal(ctx.decrypt(lookup(ctx, d_t, index)), want), x          # no ids: index i reads table i


def test_a_shared_table_and_a_table_along_a_stride(ctx):
    """one table read by every query (ids all 0), and the same entries taken with a stride from an interleaved source array"""
    from tfhe_fbs_map_amd import _native as nat
    p, N = ctx.params.p_msg, ctx.params.N
    entries = np.array([3, 1, 4, 1, 5, 2, 6])
    other = np.array([6, 6, 0, 2, 2, 5, 3])
    inter = np.stack([entries, other], axis=1).reshape(-1)                               # entry e of table t at source 2 e + t
    cts = ctx.encrypt(inter, nonce0=300)
    d_t = fold_tables(ctx, cts, np.concatenate([nat.lookup_map(p, N, p, base=t, stride=2) for t in (0, 1)]))
    xs = np.arange(2 * p) % p
    index = ctx.encrypt(xs, nonce0=400)
    assert np.array_equal(ctx.decrypt(lookup(ctx, d_t, index, np.zeros(2 * p, np.uint32))), entries[xs])
    assert np.array_equal(ctx.decrypt(lookup(ctx, d_t, index, np.ones(2 * p, np.uint32))), other[xs])
    assert np.array_equal(ctx.decrypt(lookup(ctx, d_t, index, np.full(2 * p, 9, np.uint32))), entries[xs])   # id past the set: table 0


def test_noise_at_the_default_set_is_inside_the_model():
    """2 N lookups at the default k = 2, N = 1024 set, fold key at its fold_choice: four tables whose N entries each are fresh
    encryptions of zero (the identity map), read at 512 coefficients each by noise-free indices.  The indices are CHOSEN rotation
    amounts (fbs_lookup_compact_dev at log2(2N) bits: random a~_i, b~ = sum a~_i s_i + r): a trivial ciphertext of 0 has a zero
    mask, every step would be skipped and no rotation noise measured.  Phases under the exported key; their variance over
    v_br (fold_factor + 1) + sigma_glwe^2 in the band of the compact, packed and fold noise tests."""
    import torch
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, fold_choice, folded_state_factor, lookup_output_norm2, variances
    prm = choose_params(15, 70, glwe_dims=(1, 2, 3))
    assert (prm.k, prm.N) == (2, 1024)
    t_f, gamma_f = fold_choice(prm, 70)
    c = Context(prm, seed=29, keygen=False)
    c.tune(keys_on_device=1)
    c.keygen_seeded()
    c.fold_keygen(t_f, gamma_f)
    N, n, tables, per = prm.N, prm.n, 4, 512
    cts = c.encrypt(np.zeros(tables * N, np.int64), nonce0=1)
    d_t = fold_tables(c, cts, np.arange(tables * N, dtype=np.uint32))
    keys = c.export_keys()
    sk = np.asarray(keys["sk_lwe"], np.int64)
    rng = np.random.default_rng(3)
    count = tables * per
    fields = rng.integers(0, 2 * N, (count, n + 1))
    r = np.tile(2 * np.arange(per), tables)                                             # coefficient read: even ones, each once per table
    fields[:, n] = (fields[:, :n] @ sk + r) % (2 * N)
    b = prm.log_n_poly + 1
    d_w = dev(pack(fields.astype(np.uint64), b))
    d_of = upload_u32(np.repeat(np.arange(tables), per))
    d_o = torch.zeros((count, prm.ct_words), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.lookup_compact_dev(d_t.data_ptr(), tables, d_of.data_ptr(), d_w.data_ptr(), count, d_o.data_ptr(), bits=b)
    c.sync()
    out = host(d_o)
    big = np.asarray(keys["sk_glwe"], np.uint64)
    D = prm.k * N
    phase = (out[:, D].astype(object) - ((out[:, :D] * big).sum(axis=1) % np.uint64(Q)).astype(object)) % Q   # (2048 words below 2^46: no overflow)
    err = np.array([(int(x) + Q // 2) % Q - Q // 2 for x in phase], np.float64) / float(Q)
    ff = folded_state_factor(prm, t_f, gamma_f)
    v_br = variances(prm)[0]
    model = v_br * (lookup_output_norm2(0.0, ff)) + (prm.sigma_glwe / float(Q)) ** 2
    ratio = float(err.var()) / model
    print("lookup noise: measured / model = %.3f (variance %.3e, model %.3e of which v_br %.3e, fold factor %.4f, mean %.3e)"
          % (ratio, float(err.var()), model, v_br, ff, float(err.mean())))
    c.close()
    assert 0.5 <= ratio <= 1.25, ratio


# ---- through Client and Server: resident tables read by resident indices (Server.lookup, fbs_state_lookup) ---------------------------
T8 = 8


def _served():
    from tests.test_gpu_fold_chain import _setup
    _, _, client, server = _setup()
    return client, server


def _resident(client, server, names, values, T=T8, nonce0=None):
    """rows `names` holding fresh encryptions of values [len(names)][T] under the client's key, resident on the server"""
    from tfhe_fbs_map_amd.split import EncryptedOutputs
    values = np.asarray(values, np.int64).reshape(len(names), T)
    cts = client.ctx.encrypt(values.reshape(-1), nonce0=nonce0).reshape(len(names), T, client.params.ct_words)
    return server.restore(EncryptedOutputs(list(names), T, cts, client.fingerprint, np.ones(len(names))))


def _read(client, res):
    return client.ctx.decrypt(res.fetch().cts)


def test_a_every_sample_reads_its_own_table_by_its_own_index():
    """(a) T = 8 samples, each with a different table and index; every index value; an index past the table reads 0"""
    from tfhe_fbs_map_amd.params import lookup_output_norm2
    client, server = _served()
    p = client.params.p_msg
    length = p - 1
    rng = np.random.default_rng(5)
    entries = rng.integers(0, p, (length, T8))
    names = ["e%d" % e for e in range(length)]
    with _resident(client, server, names, entries, nonce0=5000) as table:
        for shift in range(p):
            idx = (np.arange(T8) + shift) % p
            with _resident(client, server, ["i"], idx[None], nonce0=6000 + 100 * shift) as index:
                with server.lookup(table, [names], index, "i") as res:
                    want = np.where(idx < length, entries[np.minimum(idx, length - 1), np.arange(T8)], 0)
                    assert np.array_equal(_read(client, res)[0], want), shift
                    assert res.T == T8 and res.output_names == ["lookup0"] and res.fingerprint == server.key.fingerprint
                    assert res.out_norm2[0] == pytest.approx(lookup_output_norm2(1.0, server.key.fold_factor))
        assert server.ctx.stat("lookup_tables") == T8 and server.ctx.stat("lookup_scratch_words") >= T8 * (client.params.k + 1) * client.params.N


def test_b_a_shared_table_and_a_table_along_the_samples():
    """(b) table.T == 1 and axis "samples" (T_table = len) give the same cleartext answers; the tables folded are `planes`"""
    client, server = _served()
    p = client.params.p_msg
    rng = np.random.default_rng(6)
    entries = rng.integers(0, p, p)
    idx = np.arange(T8) % p
    names = ["e%d" % e for e in range(p)]
    with _resident(client, server, ["i"], idx[None], nonce0=7000) as index:
        with _resident(client, server, names, entries[:, None], T=1, nonce0=7100) as shared:
            with server.lookup(shared, [names], index, "i") as res:
                assert np.array_equal(_read(client, res)[0], entries[idx])
            assert server.ctx.stat("lookup_tables") == 1
        with _resident(client, server, ["row", "other"], np.stack([entries, (entries + 1) % p]), T=p, nonce0=7200) as along:
            with server.lookup(along, ["row", "other"], index, "i", out_names=["x", "y"], axis="samples") as res:
                got = _read(client, res)
                assert np.array_equal(got[0], entries[idx]) and np.array_equal(got[1], (entries[idx] + 1) % p)
                assert res.output_names == ["x", "y"]
            assert server.ctx.stat("lookup_tables") == 2


def test_c_two_planes_read_by_one_index_share_its_key_switch():
    """(c) the planes of one index launch ONE key switch: as many key-switch launches for two planes as for one; both decrypt"""
    client, server = _served()
    p = client.params.p_msg
    rng = np.random.default_rng(7)
    entries = rng.integers(0, p, (2, p, T8))
    idx = rng.integers(0, p, T8)
    a, b = ["a%d" % e for e in range(p)], ["b%d" % e for e in range(p)]
    with _resident(client, server, a + b, entries.reshape(2 * p, T8), nonce0=8000) as table, \
            _resident(client, server, ["i"], idx[None], nonce0=8100) as index:
        counts = []
        for planes in ([a], [a, b]):
            server.ctx.profile(True)
            server.ctx.profile_read(reset=True)
            with server.lookup(table, planes, index, "i") as res:
                got = _read(client, res)
            prof = server.ctx.profile_read(reset=True)
            server.ctx.profile(False)
            counts.append((prof["keyswitch"]["launches"], prof["blind_rotate"]["launches"]))
            for m in range(len(planes)):
                assert np.array_equal(got[m], entries[m, idx, np.arange(T8)]), m
        assert counts[0][0] == counts[1][0] >= 1 and counts[1][1] >= 1, counts


def test_d_two_digits():
    """(d) E = p + 2 entries read by two digits: every (d1, d0) that names an entry decrypts to it; one past them reads 0"""
    from tfhe_fbs_map_amd.params import lookup_output_norm2
    client, server = _served()
    p = client.params.p_msg
    E = p + 2
    rng = np.random.default_rng(8)
    entries = rng.integers(0, p, (E, T8))
    names = ["e%d" % e for e in range(E)]
    alive = server.ctx.stat("states_alive")
    with _resident(client, server, names, entries, nonce0=9000) as table:
        for start in range(0, E + 1, T8):
            which = np.minimum(start + np.arange(T8), E)                          # (E itself: d1 = 1, d0 = 2, past the entries)
            with _resident(client, server, ["d0", "d1"], np.stack([which % p, which // p]), nonce0=9100 + 10 * start) as index:
                with server.lookup(table, [names], index, ["d0", "d1"]) as res:
                    want = np.where(which < E, entries[np.minimum(which, E - 1), np.arange(T8)], 0)
                    assert np.array_equal(_read(client, res)[0], want), start
                    assert res.out_norm2[0] == pytest.approx(lookup_output_norm2(1.0, server.key.fold_factor, 2))
    assert server.ctx.stat("states_alive") == alive                              # the round's temporary state is gone


def test_e_the_state_entry_is_the_device_entries_on_hand_built_tables():
    """(e) fbs_state_lookup, word for word, against fbs_lookup_dev fed the fbs_fold_mapped_dev tables built by hand"""
    from tfhe_fbs_map_amd import _native as nat
    client, server = _served()
    prm, ctx = client.params, server.ctx
    p, N = prm.p_msg, prm.N
    length = p - 1
    rng = np.random.default_rng(9)
    entries = rng.integers(0, p, (2 * length, T8))
    idx = rng.integers(0, p, T8)
    names = ["e%d" % e for e in range(2 * length)]
    with _resident(client, server, names, entries, nonce0=10000) as table, _resident(client, server, ["j", "i"], np.stack([idx, idx]), nonce0=10100) as index:
        rows = np.arange(2 * length, dtype=np.uint32).reshape(2, length)[::-1].copy()          # plane 0: rows length .., plane 1: rows 0 ..
        out = table.state.lookup(rows, index.state, 1)
        got = out.fetch()
        out.close()
        cts, ind = table.state.fetch(), index.state.fetch()[1]
        fmap = np.concatenate([nat.lookup_map(p, N, length, base=int(rows[m, 0]) * T8 + s, stride=T8) for m in range(2) for s in range(T8)])
        d_t = fold_tables(ctx, cts.reshape(-1, prm.ct_words), fmap)
        want = lookup(ctx, d_t, np.concatenate([ind, ind]))                                      # table m T + s, read by index s
        assert np.array_equal(got.reshape(-1, prm.ct_words), want)
        assert np.array_equal(client.ctx.decrypt(got)[0], np.where(idx < length, entries[length + np.minimum(idx, length - 1), np.arange(T8)], 0))


def test_f_refusals():
    from tfhe_fbs_map_amd import Client, ExecConfig, FbsError, Server
    client, server = _served()
    p = client.params.p_msg
    names = ["e%d" % e for e in range(p + 1)]
    table = _resident(client, server, names, np.zeros((p + 1, T8), np.int64), nonce0=11000)
    index = _resident(client, server, ["i"], np.zeros((1, T8), np.int64), nonce0=11100)
    try:
        with pytest.raises(ValueError, match="more than 1 digit"):
            server.lookup(table, [names], index, "i")                              # len > p
        with pytest.raises(ValueError, match="no row named"):
            server.lookup(table, [["nope"]], index, "i")
        with pytest.raises(FbsError) as e:                                         # ... and the entry itself
            table.state.lookup(np.arange(p + 1, dtype=np.uint32)[None], index.state, 0)
        assert e.value.code == -1 and "at most p entries" in str(e.value)
        other = Server(client.server_key())                                        # another server's state
        try:
            foreign = _resident(client, other, ["i"], np.zeros((1, T8), np.int64), nonce0=11200)
            with pytest.raises(ValueError, match="resident on another server"):
                server.lookup(table, [names[:p]], foreign, "i")
            foreign.close()
        finally:
            other.ctx.close()
        bare = Client(client.env, ExecConfig(seed=7), programs=[client.env])      # no fold key
        plain = Server(bare.server_key())
        try:
            t2 = _resident(bare, plain, names[:p], np.zeros((p, T8), np.int64), nonce0=11300)
            i2 = _resident(bare, plain, ["i"], np.zeros((1, T8), np.int64), nonce0=11400)
            with pytest.raises(ValueError, match="no fold key"):
                plain.lookup(t2, [names[:p]], i2, "i")
            with pytest.raises(FbsError) as e:
                t2.state.lookup(np.arange(p, dtype=np.uint32)[None], i2.state, 0)
            assert e.value.code == -3 and "fold key" in str(e.value)
        finally:
            plain.ctx.close()
        index.close()                                                              # a closed state
        with pytest.raises(ValueError, match="not an open ResidentOutputs"):
            server.lookup(table, [names[:p]], index, "i")
    finally:
        table.close()
        index.close()
