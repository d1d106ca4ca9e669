"""Writable encrypted tables end to end (include/fbs_exec.h, "encrypted tables"), through the adder8 `Client` and `Server` of
tests/test_gpu_fold_chain.py (its 128-bit set: k = 2, N = 1024, p = 10, so tables of 5 entries), T = 8, spread 2: tables made once by `Server.table`, read, added to and set by encrypted indices (cases a to h), fbs_table_write and
fbs_table_read word for word against the context-level entries they are made of; and at the default (15, 70) set (i) the noise of
three adds against `params.table_write_norm2` and (j) the noise of a unit box's fold against its share of the fold factor.  The resident rows are fresh encryptions under the client's key restored into the server, as in
tests/test_gpu_lookup.py; an index of entry i holds spread * i."""
import numpy as np
import pytest

from tests.test_gpu_compact import pack
from tests.test_gpu_device_io import dev, host
from tests.test_gpu_lookup import Q, T8, _read, _resident, _served, fold_tables, lookup

pytestmark = pytest.mark.gpu

S = 2                                                                            # spread


def _entries(client, tab):
    """every entry of every table, decrypted: [len][planes][T]"""
    out = []
    for res in tab.entries():
        with res:
            out.append(_read(client, res))
    return np.stack(out)


def _table(client, server, entries, nonce0, T=T8, max_value=None):
    """a one-plane `ResidentTable` of entries [len][T]"""
    names = ["e%d" % e for e in range(len(entries))]
    with _resident(client, server, names, entries, T=T, nonce0=nonce0) as rows:
        return server.table(rows, [names], spread=S, max_value=max_value)


def test_a_every_index_value_reads_its_entry():
    """(a) per-sample tables: after create, every index value reads its entry; the state the tables were made of is closed"""
    from tfhe_fbs_map_amd.params import table_read_norm2
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    entries = np.random.default_rng(1).integers(0, p, (length, T8))
    with _table(client, server, entries, 20000) as tab:
        assert (tab.table.stat("tables"), tab.table.stat("len"), tab.table.stat("spread"), tab.table.stat("writes")) == (T8, length, S, 0)
        assert tab.out_norm2.shape == tab.max_value.shape == tab.writes.shape == (T8,)                   # one figure a table
        assert np.allclose(tab.out_norm2, 1.0 + server.key.fold_factor) and (tab.max_value == p - 1).all() and tab.fingerprint == server.key.fingerprint
        assert tab.fetch().shape == (T8, client.params.k + 1, client.params.N) and server.ctx.stat("tables_alive") >= 1
        for shift in range(length):
            which = (np.arange(T8) + shift) % length
            with _resident(client, server, ["i"], S * which[None], nonce0=20100 + 100 * shift) as index, tab.read(index, "i") as res:
                assert np.array_equal(_read(client, res)[0], entries[which, np.arange(T8)]), shift
                assert res.out_norm2[0] == pytest.approx(table_read_norm2(tab.out_norm2.max())) and res.output_names == ["plane0"]
        assert np.array_equal(_entries(client, tab)[:, 0], entries)


def test_b_three_adds_each_sample_its_own_value_at_its_own_index():
    """(b) every sample adds a different value at a different encrypted index, three times; entries() decrypts to the cleartext array,
    untouched entries included"""
    from tfhe_fbs_map_amd.params import table_write_norm2
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    rng = np.random.default_rng(2)
    want = rng.integers(0, 3, (length, T8))
    with _table(client, server, want, 21000, max_value=2) as tab:
        norm2, bound = float(tab.out_norm2[0]), 2
        for turn in range(3):
            which = rng.integers(0, length, T8)
            value = rng.integers(0, 3, T8)
            with _resident(client, server, ["i", "v"], np.stack([S * which, value]), nonce0=21100 + 100 * turn) as iv:
                tab.add(iv, "i", iv, "v", max_value=2)
            want[which, np.arange(T8)] += value
            norm2, bound = table_write_norm2(norm2, 1.0, server.key.fold_factor), bound + 2
            assert np.allclose(tab.out_norm2, norm2) and (tab.max_value == bound).all() and (tab.writes == turn + 1).all()
            assert tab.table.stat("writes") == turn + 1
            assert np.array_equal(_entries(client, tab)[:, 0], want), turn
        assert (tab.max_value == 8).all() and 8 <= p - 1 and want.max() <= 8 and server.ctx.stat("table_scratch_words") >= 2 * T8 * (client.params.k + 1) * client.params.N


def test_c_a_histogram_in_a_shared_table():
    """(c) one shared table of zeros made of the SERVER's own data (`PlainInputs`: no client ciphertext, no noise), one index of one
    sample at a time, repeated adds of 1: the counts"""
    from tfhe_fbs_map_amd.split import PlainInputs
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    draws = [3, 0, 3, length - 1, 3, 0, 1]
    bins = ["bin%d" % e for e in range(length)]
    with server.table(PlainInputs(bins, None, np.zeros(length, np.int64)), [bins], spread=S) as hist:
        assert hist.table.stat("tables") == 1 and hist.T == 1 and (hist.max_value == 0).all()
        assert np.allclose(hist.out_norm2, server.key.fold_factor)                 # trivial ciphertexts: the fold's noise and no other
        assert not hist.fetch()[:, :client.params.k].any()                         # ... in fact none at all: zero masks meet no key row
        for j, x in enumerate(draws):
            with _resident(client, server, ["i", "one"], [[S * x], [1]], T=1, nonce0=22100 + 10 * j) as iv:
                hist.add(iv, "i", iv, "one", max_value=1)
        assert np.array_equal(_entries(client, hist)[:, 0, 0], np.bincount(draws, minlength=length))
        assert (hist.max_value == len(draws)).all() and (hist.writes == len(draws)).all()
        # read by eight queries at once: a shared table takes any number of readers
        which = np.arange(T8) % length
        with _resident(client, server, ["i"], S * which[None], nonce0=22900) as index, hist.read(index, "i") as res:
            assert np.array_equal(_read(client, res)[0], np.bincount(draws, minlength=length)[which])


def test_d_set_then_read_at_every_index_twice_on_one_entry():
    """(d) set replaces whatever the entry held; a second set of the same entry replaces the first"""
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    rng = np.random.default_rng(4)
    want = rng.integers(0, p, (length, T8))
    with _table(client, server, want, 23000) as tab:
        which = rng.integers(0, length, T8)
        for turn in range(2):
            value = rng.integers(0, p, T8)
            with _resident(client, server, ["i", "v"], np.stack([S * which, value]), nonce0=23100 + 100 * turn) as iv:
                tab.set(iv, "i", iv, "v", max_value=p - 1)
            want[which, np.arange(T8)] = value
            for shift in range(length):
                at = (np.arange(T8) + shift) % length
                with _resident(client, server, ["i"], S * at[None], nonce0=23300 + 1000 * turn + 10 * shift) as index, tab.read(index, "i") as res:
                    assert np.array_equal(_read(client, res)[0], want[at, np.arange(T8)]), (turn, shift)
        assert (tab.max_value == p - 1).all() and (tab.writes == 2).all()


def test_e_two_planes_share_the_key_switch_of_their_index():
    """(e) two planes read and written by one index launch as many key switches as one plane does"""
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    rng = np.random.default_rng(5)
    entries = rng.integers(0, 4, (2, length, T8))
    a, b = ["a%d" % e for e in range(length)], ["b%d" % e for e in range(length)]
    which, va, vb = rng.integers(0, length, T8), rng.integers(0, 4, T8), rng.integers(0, 4, T8)
    with _resident(client, server, a + b, entries.reshape(2 * length, T8), nonce0=24000) as rows, \
            _resident(client, server, ["i", "va", "vb"], np.stack([S * which, va, vb]), nonce0=24100) as iv:
        counts = []
        for planes, values in (([a], ["va"]), ([a, b], ["va", "vb"])):
            with server.table(rows, planes, spread=S, max_value=3) as tab:
                server.ctx.profile(True)
                server.ctx.profile_read(reset=True)
                tab.add(iv, "i", iv, values, max_value=3)
                with tab.read(iv, "i") as res:
                    got = _read(client, res)
                prof = server.ctx.profile_read(reset=True)
                server.ctx.profile(False)
                counts.append((prof["keyswitch"]["launches"], prof["blind_rotate"]["launches"]))
                for m, v in enumerate((va, vb)[:len(planes)]):
                    assert np.array_equal(got[m], entries[m, which, np.arange(T8)] + v), m
        assert counts[0][0] == counts[1][0] >= 2 and counts[1][1] >= 2, counts


def test_f_a_write_is_the_context_level_sequence_word_for_word():
    """(f) fbs_table_write (add) against fbs_fold_mapped_dev of hand-built unit-box maps, fbs_rotate_dev with the negated amounts and
    fbs_glwe_add_dev; (g) fbs_table_read against fbs_lookup_dev on fbs_table_words"""
    import torch
    from tfhe_fbs_map_amd import _native as nat
    client, server = _served()
    prm, ctx = client.params, server.ctx
    p, N, ctw = prm.p_msg, prm.N, prm.ct_words
    length = p // S
    rng = np.random.default_rng(6)
    entries = rng.integers(0, 3, (2 * length, T8))
    names = ["e%d" % e for e in range(2 * length)]
    which = rng.integers(0, length, T8)
    with _resident(client, server, names, entries, nonce0=25000) as rows, \
            _resident(client, server, ["v1", "i", "v0"], np.stack([rng.integers(0, 3, T8), S * which, rng.integers(0, 3, T8)]), nonce0=25100) as iv:
        with server.table(rows, [names[length:], names[:length]], spread=S, max_value=2) as tab:
            # (g) the read: table m T + s by index s
            before = tab.fetch()
            ind = iv.state.fetch()[1]
            with tab.read(iv, "i") as res:
                got = res.state.fetch()
            want = lookup(ctx, dev(before), np.concatenate([ind, ind]))
            assert np.array_equal(got.reshape(-1, ctw), want)
            assert np.array_equal(client.ctx.decrypt(got)[0], entries[length + which, np.arange(T8)])
            # (f) the add: plane 0 takes row "v0" (row 2 of the state), plane 1 row "v1" (row 0)
            tab.add(iv, "i", iv, ["v0", "v1"], max_value=2)
            after = tab.fetch()
            cts = iv.state.fetch().reshape(-1, ctw)
            fmap = np.concatenate([nat.table_map(p, N, S, 1, base=row * T8 + s) for row in (2, 0) for s in range(T8)])
            d_units = fold_tables(ctx, cts, fmap)
            d_turned = torch.zeros((2 * T8, (prm.k + 1) * N), dtype=torch.int64, device="cuda")
            d_index = dev(np.concatenate([ind, ind]))
            torch.cuda.synchronize()
            ctx.rotate_dev(d_units.data_ptr(), 2 * T8, 0, d_index.data_ptr(), 2 * T8, d_turned.data_ptr(), negate=True)
            d_tab = dev(before.reshape(2 * T8, -1))
            ctx.glwe_add_dev(d_tab.data_ptr(), 2 * T8, np.arange(2 * T8), d_turned.data_ptr())
            ctx.sync()
            assert np.array_equal(host(d_tab), after.reshape(2 * T8, -1))
            assert not np.array_equal(before, after)


def test_h_refusals():
    from tfhe_fbs_map_amd import Client, ExecConfig, FbsError, Server
    client, server = _served()
    p = client.params.p_msg
    length = p // S
    names = ["e%d" % e for e in range(length + 1)]
    rows = _resident(client, server, names, np.zeros((length + 1, T8), np.int64), nonce0=26000)
    one = _resident(client, server, names[:length], np.zeros((length, 1), np.int64), T=1, nonce0=26100)
    iv = _resident(client, server, ["i", "v"], np.zeros((2, T8), np.int64), nonce0=26200)
    tab = shared = None
    try:
        with pytest.raises(ValueError, match="more than p = %d boxes hold" % p):   # len > floor(p / spread)
            server.table(rows, [names], spread=S)
        with pytest.raises(FbsError) as e:                                         # ... and the entry itself
            server.ctx.table(rows.state, np.arange(length + 1, dtype=np.uint32)[None], S)
        assert e.value.code == -1 and "floor(p / spread)" in str(e.value)
        with pytest.raises(ValueError, match="no row named"):
            server.table(rows, [["nope"]])
        shared = server.table(one, [names[:length]], spread=S, max_value=0)
        with pytest.raises(ValueError, match="a shared table is written by an index of one sample, not 8"):
            shared.add(iv, "i", iv, "v", max_value=1)                              # a shared table and T > 1
        with pytest.raises(FbsError) as e:
            shared.table.write(iv.state, 0, iv.state, [1])
        assert e.value.code == -1 and "a shared table is written by an index state of one sample" in str(e.value)
        tab = server.table(rows, [names[:length]], spread=S, max_value=p - 3)
        with pytest.raises(ValueError, match="above p - 1 = %d: it would not decrypt" % (p - 1)):
            tab.add(iv, "i", iv, "v", max_value=3)                                 # bound overflow
        tab.out_norm2[:] = 1e6
        with pytest.raises(ValueError, match="noise budget is spent"):
            tab.add(iv, "i", iv, "v", max_value=1)                                 # noise budget spent
        assert not tab.writes.any() and tab.table.stat("writes") == 0                         # ... and nothing was written
        bare = Client(client.env, ExecConfig(seed=7), programs=[client.env])      # no fold key
        plain = Server(bare.server_key())
        try:
            r2 = _resident(bare, plain, names[:length], np.zeros((length, T8), np.int64), nonce0=26300)
            with pytest.raises(ValueError, match="no fold key"):
                plain.table(r2, [names[:length]])
            with pytest.raises(FbsError) as e:
                plain.ctx.table(r2.state, np.arange(length, dtype=np.uint32)[None], S)
            assert e.value.code == -3 and "fold key" in str(e.value)
        finally:
            plain.ctx.close()
        tab.close()                                                                # a freed table
        for call in (lambda: tab.read(iv, "i"), lambda: tab.add(iv, "i", iv, "v", max_value=0), tab.entries, tab.fetch):
            with pytest.raises(ValueError, match="the resident table is closed"):
                call()
    finally:
        for res in (rows, one, iv, tab, shared):
            if res is not None:
                res.close()


@pytest.fixture(scope="module")
def default_ctx():
    """a context at the default (15, 70) set, k = 2, N = 1024, with a fold key at its fold_choice: the two noise tests' own"""
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, fold_choice
    prm = choose_params(15, 70, glwe_dims=(1, 2, 3))
    assert (prm.k, prm.N) == (2, 1024)
    t_f, gamma_f = fold_choice(prm, 70)
    c = Context(prm, seed=31, keygen=False)
    c.tune(keys_on_device=1)
    c.keygen_seeded()
    c.fold_keygen(t_f, gamma_f)
    yield c, prm, t_f, gamma_f, c.export_keys()
    c.close()


def _phase_errors(words, sk_glwe, k, N):
    """the phases of GLWE samples [count][k+1][N] under the key, centred, in torus units: [count][N]"""
    from oracle import tfhe_oracle as orc
    S_glwe = np.asarray(sk_glwe, np.uint64).reshape(k, N)
    err = []
    for w in words:
        phase = w[k].copy()
        for cc in range(k):
            phase = (phase + np.uint64(Q) - orc.polymul_ntt(w[cc], S_glwe[cc])) % np.uint64(Q)
        err.append(((phase.astype(np.int64) + Q // 2) % Q - Q // 2).astype(np.float64) / float(Q))
    return np.stack(err)


def test_i_noise_of_three_adds_at_the_default_set(default_ctx):
    """(i) four tables whose N entries each are fresh encryptions of zero (the identity map); three adds each of folded
    zero-encryptions, turned by CHOSEN noise-free amounts (fbs_rotate_compact_dev at log2(2N) bits with the negate flag: random a~_i,
    b~ = sum a~_i s_i + r) and summed in by fbs_glwe_add_dev.  The tables' phases under the exported GLWE key against
    v_br table_write_norm2 (three writes of noise-free values onto the fold, every fold a whole sample) + 4 sigma_glwe^2,
    in the band of the lookup, fold and packing noise tests (measured 0.920, profiles/tables/README.md)."""
    import torch
    from tfhe_fbs_map_amd.params import folded_state_factor, table_write_norm2, variances
    c, prm, t_f, gamma_f, keys = default_ctx
    N, n, k, tables, adds = prm.N, prm.n, prm.k, 4, 3
    ident = np.arange(tables * N, dtype=np.uint32)
    d_tab = fold_tables(c, c.encrypt(np.zeros(tables * N, np.int64), nonce0=1), ident).reshape(tables, -1)
    sk = np.asarray(keys["sk_lwe"], np.int64)
    rng = np.random.default_rng(3)
    b = prm.log_n_poly + 1
    for turn in range(adds):
        d_units = fold_tables(c, c.encrypt(np.zeros(tables * N, np.int64), nonce0=(turn + 2) * (1 << 20)), ident)
        fields = rng.integers(0, 2 * N, (tables, n + 1))
        fields[:, n] = (fields[:, :n] @ sk + rng.integers(0, 2 * N, tables)) % (2 * N)
        d_w = dev(pack(fields.astype(np.uint64), b))
        d_turned = torch.zeros((tables, (k + 1) * N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c.rotate_compact_dev(d_units.data_ptr(), tables, 0, d_w.data_ptr(), tables, d_turned.data_ptr(), bits=b, negate=True)
        c.glwe_add_dev(d_tab.data_ptr(), tables, np.arange(tables), d_turned.data_ptr())
    c.sync()
    err = _phase_errors(host(d_tab).reshape(tables, k + 1, N), keys["sk_glwe"], k, N).reshape(-1)
    ff = folded_state_factor(prm, t_f, gamma_f)
    v_br = variances(prm)[0]
    norm2 = ff
    for _ in range(adds):
        norm2 = table_write_norm2(norm2, 0.0, ff)
    model = v_br * norm2 + (adds + 1) * (prm.sigma_glwe / float(Q)) ** 2
    ratio = float(err.var()) / model
    print("table noise after %d adds: measured / model = %.3f (variance %.3e, model %.3e of which v_br %.3e, fold factor %.4f, mean %.3e)"
          % (adds, ratio, float(err.var()), model, v_br, ff, float(err.mean())))
    assert 0.5 <= ratio <= 1.25, ratio


def test_j_the_fold_of_a_unit_box_against_the_fold_factor(default_ctx):
    """(j) what a write's fold adds, measured where nothing else is: 64 unit boxes (fbs_table_map at len = 1, spread 2) of fresh
    encryptions of zero, folded and not rotated.  A unit box has filled = about s N / p sources where a whole sample has N, and the
    finer figure would be `folded_state_variance` x filled / N.  It does NOT hold: measured / that figure is 0.33 on the coefficients
    the map leaves empty and 5.4 on the filled ones, where a written value lies, outside the band 0.5 .. 1.25 on both sides
    (profiles/tables/README.md).  The model's own two terms say why -- the key noise is a sum over the sources, the rounding of a
    ciphertext's mask words stays whole at its own coefficient -- and their split is printed for the record.  So
    `table_write_norm2` counts the fold whole, which is safe, and the upper side alone is asserted: against the whole fold the
    filled coefficients measured 0.73, the empty ones 0.044."""
    from tfhe_fbs_map_amd import _native as nat
    from tfhe_fbs_map_amd.params import folded_state_variance
    c, prm, t_f, gamma_f, keys = default_ctx
    N, k, p, boxes = prm.N, prm.k, prm.p_msg, 64
    unit = nat.table_map(p, N, S, 1)
    filled = int((unit != nat.MAP_NONE).sum())
    assert filled in (S * N // p, S * N // p + 1)
    fmap = np.concatenate([nat.table_map(p, N, S, 1, base=t) for t in range(boxes)])
    words = host(fold_tables(c, c.encrypt(np.zeros(boxes, np.int64), nonce0=9 << 20), fmap)).reshape(boxes, k + 1, N)
    err = _phase_errors(words, keys["sk_glwe"], k, N)
    empty, full = float(err[:, unit == nat.MAP_NONE].var()), float(err[:, unit != nat.MAP_NONE].var())
    v_fold = folded_state_variance(prm, t_f, gamma_f) + (prm.sigma_glwe / float(Q)) ** 2
    rounding = (prm.k * N / 2.0) * 2.0 ** (-2 * t_f * gamma_f) / 12.0            # folded_state_variance's second term
    key_noise = folded_state_variance(prm, t_f, gamma_f) - rounding
    fill = filled / N
    print("unit-box fold noise, %d of %d coefficients filled: variance on the empty coefficients %.3e, on the filled %.3e; against the "
          "whole fold (%.3e) %.3f and %.3f; against fold x fill %.3f and %.3f; against the two terms apart (key noise %.3e x fill; that + "
          "rounding %.3e) %.3f and %.3f"
          % (filled, N, empty, full, v_fold, empty / v_fold, full / v_fold, empty / (v_fold * fill), full / (v_fold * fill), key_noise, rounding,
             empty / (key_noise * fill), full / (key_noise * fill + rounding)))
    assert full / v_fold <= 1.25 and empty / v_fold <= 1.25, (full / v_fold, empty / v_fold)
