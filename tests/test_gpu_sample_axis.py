"""Sample-axis operations on the GPU (include/fbs_exec.h, "sample-axis operations"): fbs_eval_resident_mapped over state rows read
through an index is fbs_eval_sources over the same ciphertexts gathered on the host, word for word -- into the host and into a
state, refreshed, mixed with the other source kinds, chunked -- and leaves fbs_eval_resident what it was; fbs_state_sum_groups is
the word-wise sum modulo q, canonical at the largest group; counts, a shifted operand and a tree reduction decrypt to their
cleartext values; and what must be refused is, with nothing written."""
import ctypes as C

import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import load_fixture, subsample
from tests.test_gpu_device_io import SETS

pytestmark = pytest.mark.gpu

E_INVALID = -1
NONE = 0xFFFFFFFF
ADDER = "adder8__search_p15"
A_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}
B_FROM_S = {f"b{i}": f"s{i}" for i in range(8)}
B_NAMES = [f"b{i}" for i in range(8)]
T_SRC, T = 37, 23


def _pair(name):
    from tfhe_fbs_map_amd import Context
    client = Context(SETS[name](), seed=11, keygen=False)
    client.keygen_seeded()
    return client, Context.evaluation_only(client.params, **client.export_seeded_keys())


def _load(ctx, low):
    from tfhe_fbs_map_amd import _native as nat
    tv = ctx.tvset(low["tables"])
    prog = nat.Program(ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"],
                       low["term_coef"], low["term_src"], low["out_wire"])
    prog._tv = tv
    return prog


def _program(ctx, name):
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    return rec, low, _load(ctx, low)


def trivial_body(prm, m):
    """the body of the trivial ciphertext of message m: m Delta mod q, Delta = 2 round(q / 4p) (the header's FBS_SRC_PLAIN)"""
    p = int(prm.p_msg)
    return int(m) * (2 * ((orc.Q + 2 * p) // (4 * p))) % orc.Q


def gathered(prm, row, index, fill):
    """row [T_src][D+1] read through `index` on the host: sample s is row[index[s]], or the trivial ciphertext of `fill`"""
    index = np.asarray(index, np.int64)
    none = index == NONE
    out = row[np.where(none, 0, index)].copy()
    out[none] = 0
    out[none, -1] = trivial_body(prm, fill)
    return out


def sample_maps(n_in):
    """one index [T] into T_SRC samples and one fill per input: indices that repeat and run backwards, both parities next to each
    other (so that source and destination agree in their 16-byte alignment for some samples and not for others), FBS_SAMPLE_NONE at
    the first and at the last sample under fill 1 (input 2) and under fill 0 (input 3), and in the middle (input 5)"""
    rng = np.random.default_rng(5)
    index = rng.integers(0, T_SRC, (n_in, T)).astype(np.uint32)
    index[0] = np.arange(T_SRC - 1, T_SRC - 1 - T, -1)          # backwards from the last sample
    index[1] = 7                                                 # one sample for all
    index[4] = (np.arange(T) // 3 * 5) % T_SRC                   # runs of three, then a jump
    fills = [0] * n_in
    for i, fill in ((2, 1), (3, 0)):
        index[i, 0] = index[i, -1] = NONE
        fills[i] = fill
    index[5, 11], fills[5] = NONE, 1
    return index, fills


class Adder8:
    """adder8 at a toy set: the outputs of one seeded evaluation at T_SRC samples (9 rows of bits) in a state; the inputs of a
    second evaluation at T samples read rows of it (7 of the 9 rows feed two inputs) through a sample map each.  What that
    evaluation must return is fbs_eval_sources over ("full", ...) links gathered on the host: computed once per feed."""

    def __init__(self, name):
        self.client, self.server = _pair(name)
        self.prm = self.server.params
        self.rec, self.low, self.prog = _program(self.server, "adder8__search_p7")
        ins, _ = subsample(self.rec, T_SRC)
        self.n_in = len(self.low["input_names"])
        msgs = np.stack([np.asarray(ins[k], np.int64) for k in self.low["input_names"]])
        bodies, nonce0 = self.client.encrypt_seeded(msgs, nonce0=5)
        self.first = self.prog.eval_seeded(bodies, T_SRC, nonce0)                    # [9][T_SRC][D+1]
        self.rows = [(5 * i + 3) % 9 for i in range(self.n_in)]
        self.index, self.fills = sample_maps(self.n_in)
        self.state = self.server.state(9, T_SRC).put(self.first)
        # further inputs of the call's own T: seeded bodies, compact words, plaintext messages
        self.msgs = msgs[:, :T].copy()
        self.bodies, self.nonce0 = self.client.encrypt_seeded(self.msgs, nonce0=1 << 20)
        self.bits = self.prm.log_n_poly + 3
        self.words = self.prog.eval_seeded_compact(self.bodies, T, self.nonce0, self.bits)

    def host_link(self, i, refresh=False):
        return ("full", gathered(self.prm, self.first[self.rows[i]], self.index[i], self.fills[i]), refresh)

    def state_link(self, i, refresh=False, state=None):
        return ("state", state or self.state, self.rows[i], refresh, self.index[i], self.fills[i])

    def feeds(self, refresh=lambda i: False, mixed=False, state=None):
        """-> (the feed with mapped state rows, the same with those rows gathered on the host as full links)"""
        dev, host = [], []
        for i in range(self.n_in):
            other = None
            if mixed and i % 4 == 0:
                other = ("seeded", self.bodies[i], self.nonce0 + i * T)
            elif mixed and i % 4 == 1:
                other = ("compact", self.words[i % 9], self.bits)
            elif mixed and i % 4 == 2:
                other = ("plain", self.msgs[i].copy()) if i % 8 == 2 else ("plain", 1)
            dev.append(other or self.state_link(i, refresh(i), state))
            host.append(other or self.host_link(i, refresh(i)))
        return dev, host


@pytest.fixture(scope="module", params=["k1_n1024", "k3"])
def adder8(request):
    a = Adder8(request.param)
    yield a
    a.server.close()
    a.client.close()


def test_the_maps_are_what_the_test_needs(adder8):
    index, fills = adder8.index, adder8.fills
    assert adder8.prm.ct_words % 2 == 1 and len(set(adder8.rows)) == 9 and len(adder8.rows) == 16
    real = index[index != NONE]
    assert real.max() < T_SRC and (index == NONE).sum() == 5
    assert (np.diff(index[0].astype(np.int64)) == -1).all() and len(set(index[1])) == 1 and len(set(index[4])) < T
    # D + 1 is odd: source sample j and destination sample s agree in alignment when j and s have one parity (up to the row's own
    # offset, which is constant along a row), so every input needs both equal and unequal parities among its samples
    for i in range(adder8.n_in):
        live = index[i] != NONE
        par = (index[i][live].astype(np.int64) + np.arange(T)[live]) % 2
        if i != 0:                     # (input 0 runs backwards by one: s + j is constant -- one case along the row, by design)
            assert 0 < par.sum() < par.size, i
    assert index[2, 0] == index[2, -1] == NONE and fills[2] == 1 and index[3, 0] == index[3, -1] == NONE and fills[3] == 0


def test_mapped_rows_are_gathered_full_sources_word_for_word(adder8):
    a, prog, server = adder8, adder8.prog, adder8.server
    dev, host = a.feeds()
    want = prog.eval_sources(host, T)
    assert np.array_equal(prog.eval_resident(dev, T), want)
    with server.state(prog.n_outputs, T) as out:
        assert prog.eval_resident(dev, T, out_state=out) is out        # every input resident: queued, not waited for
        assert np.array_equal(out.fetch(), want)
    # compact outputs of the mapped call
    assert np.array_equal(prog.eval_resident(dev, T, a.bits), prog.eval_sources(host, T, a.bits))
    # refreshed: word for word the refreshed gathered links; the trivial samples refresh like any other
    third = lambda i: i % 3 == 0
    dev_r, host_r = a.feeds(third)
    want_r = prog.eval_sources(host_r, T)
    assert np.array_equal(prog.eval_resident(dev_r, T), want_r) and not np.array_equal(want_r, want)
    assert np.array_equal(a.client.decrypt(want_r), a.client.decrypt(want))
    with server.state(prog.n_outputs, T) as out:
        prog.eval_resident(dev_r, T, out_state=out)
        assert np.array_equal(out.fetch(), want_r)
    assert np.array_equal(a.state.fetch(), a.first)                    # the input state is only read
    assert server.stat("states_alive") == 1


def test_mapped_rows_mix_with_the_other_source_kinds(adder8):
    a, prog, server = adder8, adder8.prog, adder8.server
    dev, host = a.feeds(lambda i: i == 7, mixed=True)
    assert sorted({s[0] for s in dev}) == ["compact", "plain", "seeded", "state"] and sum(len(s) == 6 for s in dev) == 4
    want = prog.eval_sources(host, T)
    assert np.array_equal(prog.eval_resident(dev, T), want)
    with server.state(prog.n_outputs, T) as out:
        prog.eval_resident(dev, T, out_state=out)
        assert np.array_equal(out.fetch(), want)
    # mapped and unmapped rows in one call: the unmapped ones come from a state of the call's T
    with server.state(9, T).put(a.first[:, :T]) as short:
        both = [("state", short, a.rows[i], False) if i % 2 else a.state_link(i) for i in range(a.n_in)]
        same = [("full", a.first[a.rows[i], :T], False) if i % 2 else a.host_link(i) for i in range(a.n_in)]
        assert np.array_equal(prog.eval_resident(both, T), prog.eval_sources(same, T))


def every_link_shape(a, state, short):
    """-> (a feed with every shape of device-side link in one call, the same over host-gathered full links): by i mod 6 an
    unmapped row of `short` (a state of the call's T), a message per sample, two mapped rows of `state` (inputs 2 and 3: their
    maps have FBS_SAMPLE_NONE at sample 0 and at sample T - 1), a seeded input, one message for all.  A chunked call reads the maps
    at s0 + q, the messages at q, in slots of stride Tc > tc in the last chunk."""
    dev, host = [], []
    for i in range(a.n_in):
        kind, refresh = i % 6, i % 5 == 0
        if kind == 0:
            dev.append(("state", short, a.rows[i], refresh))
            host.append(("full", a.first[a.rows[i], :T], refresh))
        elif kind in (2, 3):
            dev.append(a.state_link(i, refresh, state))
            host.append(a.host_link(i, refresh))
        else:
            other = {1: ("plain", a.msgs[i].copy()), 4: ("seeded", a.bodies[i], a.nonce0 + i * T), 5: ("plain", 1)}[kind]
            dev.append(other)
            host.append(other)
    for i in (2, 3):
        assert len(dev[i]) == 6 and dev[i][4][0] == dev[i][4][T - 1] == NONE
    assert {i % 6 for i in range(a.n_in)} == set(range(6))
    return dev, host


@pytest.mark.parametrize("feed", ["mapped", "every_link_shape"])
def test_chunks_slice_the_index(adder8, monkeypatch, feed):
    from tfhe_fbs_map_amd import Context
    a = adder8
    mapped = lambda state: a.feeds(lambda i: i % 5 == 0, state=state)
    host = mapped(None)[1] if feed == "mapped" else every_link_shape(a, a.state, a.state)[1]
    want = a.prog.eval_sources(host, T)
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")
    assert 2 * 2**20 * 0.6 / (a.prog.n_slots * a.prm.ct_words * 8) < T / 3          # three chunks or more
    fresh = Context.evaluation_only(a.client.params, **a.client.export_seeded_keys())
    _, _, prog = _program(fresh, "adder8__search_p7")
    state = fresh.state(9, T_SRC).put(a.first)
    short = fresh.state(9, T).put(a.first[:, :T])
    dev = mapped(state)[0] if feed == "mapped" else every_link_shape(a, state, short)[0]
    assert np.array_equal(prog.eval_resident(dev, T), want)
    out = fresh.state(prog.n_outputs, T)
    prog.eval_resident(dev, T, out_state=out)
    assert np.array_equal(out.fetch(), want)
    monkeypatch.delenv("FBS_WIRE_BUDGET_MB")
    fresh.close()
    assert out.closed and state.closed and short.closed


def test_the_identity_map_is_the_unmapped_call_and_the_old_entry_is_unchanged(adder8):
    a, prog = adder8, adder8.prog
    want = prog.eval_sources([("full", a.first[r], False) for r in a.rows], T_SRC)
    old = [("state", a.state, r, False) for r in a.rows]                               # the 4-tuple feed: fbs_eval_resident
    assert np.array_equal(prog.eval_resident(old, T_SRC), want)
    ident = [("state", a.state, r, False, np.arange(T_SRC, dtype=np.uint32), 0) for r in a.rows]
    assert np.array_equal(prog.eval_resident(ident, T_SRC), want)
    with a.server.state(prog.n_outputs, T_SRC) as out:
        prog.eval_resident(old, T_SRC, out_state=out)
        assert np.array_equal(out.fetch(), want)
        prog.eval_resident(ident, T_SRC, out_state=out)
        assert np.array_equal(out.fetch(), want)


def _sums(block, group):
    """[rows][T][W] uint64 -> [rows][ceil(T / group)][W]: exact integer sums of runs of `group` samples, modulo q"""
    big = block.astype(object)
    Tn = -(-block.shape[1] // group)
    out = np.stack([big[:, j * group:(j + 1) * group].sum(axis=1) % orc.Q for j in range(Tn)], axis=1)
    return out.astype(np.uint64)


@pytest.mark.parametrize("group", [1, 2, 3, 7])
def test_group_sums_word_for_word(adder8, group):
    server, ctw = adder8.server, adder8.prm.ct_words
    rng = np.random.default_rng(group)
    pattern = rng.integers(0, orc.Q, (5, T_SRC, ctw), dtype=np.uint64)
    Tn = -(-T_SRC // group)
    assert group == 1 or T_SRC % group                                                # a ragged last group
    before = rng.integers(0, orc.Q, (6, Tn, ctw), dtype=np.uint64)
    with server.state(5, T_SRC).put(pattern) as src, server.state(6, Tn).put(before) as dst:
        for row0, rows, dst_row0 in ((1, 3, 2), (2, 2, 1), (0, 0, 3)):
            want = before.copy()
            want[dst_row0:dst_row0 + rows] = _sums(pattern[row0:row0 + rows], group)
            assert src.sum_groups(group, row0, rows, out=dst, out_row0=dst_row0) is dst
            got = dst.fetch()
            assert got.max() < orc.Q and np.array_equal(got, want), (group, row0)     # the other rows are as they were
            dst.put(before)
        assert np.array_equal(src.fetch(), pattern)
        with src.sum_groups(group) as made:                                            # a new state for every row
            assert (made.rows, made.T) == (5, Tn) and np.array_equal(made.fetch(), _sums(pattern, group))
    assert server.stat("states_alive") == 1


def test_the_largest_sums_are_canonical():
    """every word q - 1, 4096 + 5 samples in groups of 4096: the sums pass 2^58, and the results are 4096 (q - 1) mod q = q - 4096
    and 5 (q - 1) mod q = q - 5 only if the accumulator is reduced, once, at the end"""
    from tfhe_fbs_map_amd import Context
    server = Context(SETS["k1_n1024"](), seed=3, keygen=False)
    group, T_ = 4096, 4096 + 5
    ctw = server.params.ct_words
    with server.state(1, T_).put(np.full((1, T_, ctw), orc.Q - 1, np.uint64)) as src, src.sum_groups(group) as out:
        got = out.fetch()
    assert got.shape == (1, 2, ctw)
    assert (got[0, 0] == (group * (orc.Q - 1)) % orc.Q).all() and (got[0, 1] == (5 * (orc.Q - 1)) % orc.Q).all()
    assert int(got[0, 0, 0]) == orc.Q - 4096 and int(got[0, 1, 0]) == orc.Q - 5
    server.close()


AND = """m1 = 1 * a + 1 * b
m2 = Bootstrap(m1, [0, 0, 1])
Output both = m2
"""


def test_counting_matches_in_groups():
    """how many of each 7 rows have both bits set, counted on the server: the client decrypts 4 counts, not 28 bits"""
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    from tfhe_fbs_map_amd.split import EncryptedOutputs
    T_ = 28
    env = parse_fbs(AND, inputs=["a", "b"])
    client = Client(env, ExecConfig(seed=2, fbs_size=15, params=SETS["k1_n1024"]()))
    assert client.params.p_msg == 15
    server = Server(client.server_key())
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 2, T_), rng.integers(0, 2, T_)
    b[7:14] = a[7:14] = 1                                                             # one group in which all seven match
    bits = server.run(env, client.encrypt({"a": a, "b": b}), resident=True)
    assert np.array_equal(client.decrypt(bits.fetch())["both"], a & b)
    counts = bits.sum_groups(7)
    assert counts.T == 4 and np.array_equal(counts.out_norm2, bits.out_norm2 * 7) and counts.compact_bits is None
    got = counts.fetch()
    assert isinstance(got, EncryptedOutputs) and got.cts.shape[:2] == (1, 4)
    want = (a & b).reshape(4, 7).sum(axis=1)
    assert want[1] == 7 and np.array_equal(client.decrypt(got)["both"], want)
    with pytest.raises(ValueError, match="above p - 1 = 14"):
        bits.sum_groups(15)
    with pytest.raises(ValueError, match="pass bits"):
        counts.fetch(compact=True)
    assert server.ctx.stat("states_alive") == 2
    counts.close()
    bits.close()
    assert server.ctx.stat("states_alive") == 0
    server.ctx.close()
    client.ctx.close()


@pytest.fixture(scope="module")
def adder128():
    """adder8 under its default 128-bit key, for the two tests that decrypt a sum"""
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture(ADDER)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=7), programs=[env])
    server = Server(client.server_key())
    yield rec, env, client, server
    server.ctx.close()
    client.ctx.close()


def _bits_of(x, names):
    return {n: (np.asarray(x) >> i) & 1 for i, n in enumerate(names)}


def _value(out):
    return sum(np.asarray(out[f"s{i}"]).astype(np.int64) << i for i in range(8))


def test_fold_sums_five_numbers(adder128):
    rec, env, client, server = adder128
    x = np.array([200, 17, 255, 90, 3])
    zero = np.zeros(5, np.int64)
    first = {**_bits_of(x, [f"a{i}" for i in range(8)]), **_bits_of(zero, B_NAMES)}
    state = server.run(env, client.encrypt(first), resident=True)
    assert np.array_equal(_value(client.decrypt(state.fetch())), x)
    total = server.fold(env, state, A_FROM_S, B_FROM_S)                                # 5 -> 3 -> 2 -> 1: the fill pairs twice
    assert total.T == 1 and total.output_names == state.output_names and not state.closed
    assert _value(client.decrypt(total.fetch()))[0] == int(x.sum()) % 256 == 53
    assert server.ctx.stat("states_alive") == 2                                        # the input state and the result
    # one sample folds to a copy of itself
    copy = server.fold(env, total, A_FROM_S, B_FROM_S)
    assert copy.T == 1 and copy.state is not total.state and np.array_equal(copy.fetch().cts, total.fetch().cts)
    for st in (copy, total, state):
        st.close()
    assert server.ctx.stat("states_alive") == 0


def test_a_shifted_state_is_the_previous_sample(adder128):
    rec, env, client, server = adder128
    T_ = 9
    rng = np.random.default_rng(4)
    x, b = rng.integers(0, 256, T_), rng.integers(0, 256, T_)
    first = {**_bits_of(x, [f"a{i}" for i in range(8)]), **_bits_of(np.zeros(T_, np.int64), B_NAMES)}
    with server.run(env, client.encrypt(first), resident=True) as state:
        out = server.run_chain(env, [state.shift(1, fill=0), client.encrypt(_bits_of(b, B_NAMES), names=B_NAMES)], rename=A_FROM_S)
        got = _value(client.decrypt(out))
        assert got[0] == b[0] and np.array_equal(got[1:], (x[:-1] + b[1:]) % 256)
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**_bits_of(np.concatenate([[0], x[:-1]]), [f"a{i}" for i in range(8)]), **_bits_of(b, B_NAMES)})
        assert np.array_equal(np.broadcast_to(client.decrypt(out)["cout"], (T_,)), np.broadcast_to(clear["cout"], (T_,)))
    assert server.ctx.stat("states_alive") == 0


def test_refusals_write_nothing(adder8):
    from tfhe_fbs_map_amd import FbsError, _native as nat
    a, prog, server, lib = adder8, adder8.prog, adder8.server, nat.lib
    ctw, n_out, p = a.prm.ct_words, adder8.prog.n_outputs, int(a.prm.p_msg)
    pattern = np.random.default_rng(9).integers(0, orc.Q, (n_out, T, ctw), dtype=np.uint64)
    out_state = server.state(n_out, T).put(pattern)
    host = np.full((n_out, T, ctw), 7, np.uint64)
    index = np.ascontiguousarray(a.index)
    seeded = nat._InputSrc(nat.SRC_SEEDED, 0, 0, a.nonce0, a.bodies[4].ctypes.data)

    def code(entry=None, fill=None, no_index=(), seeded_input=None, map_it=True, to_host=False):
        idx = index.copy()
        srcs, res, maps = (nat._InputSrc * a.n_in)(), (nat._ResidentSrc * a.n_in)(), (nat._SampleMap * a.n_in)()
        if entry is not None:
            idx[entry[0], entry[1]] = entry[2]
        for i, r in enumerate(a.rows):
            res[i] = nat._ResidentSrc(a.state._h.value, r, 0)
            maps[i] = nat._SampleMap(None if i in no_index else idx[i].ctypes.data, a.fills[i])
        if fill is not None:
            maps[fill[0]].fill = fill[1]
        if seeded_input is not None:
            res[seeded_input] = nat._ResidentSrc(None, 0, 0)
            srcs[seeded_input] = seeded
            if not map_it:
                maps[seeded_input].index = None
        try:
            server._check(lib.fbs_eval_resident_mapped(server._h, prog._h, C.byref(srcs), C.byref(res), C.byref(maps), T, 0,
                                                       host.ctypes.data if to_host else None, None if to_host else out_state._h))
        except FbsError as e:
            return e.code
        return 0
    assert code(entry=(6, 9, T_SRC)) == E_INVALID                        # an index entry equal to T_src
    assert "reads sample 37" in lib.fbs_last_error(server._h).decode()
    assert code(entry=(15, T - 1, NONE - 1)) == E_INVALID
    assert code(fill=(2, -1)) == E_INVALID and code(fill=(9, 2 * p)) == E_INVALID
    assert "outside [0, 2p)" in lib.fbs_last_error(server._h).decode()
    assert code(seeded_input=4) == E_INVALID                             # a map on a seeded input
    assert "not a state row" in lib.fbs_last_error(server._h).decode()
    assert code(no_index=(8,)) == E_INVALID                              # a NULL index with T_src != T: the old rule, the old message
    assert "its state holds 37 samples a row, the call has 23" in lib.fbs_last_error(server._h).decode()
    assert code(entry=(6, 9, T_SRC), to_host=True) == E_INVALID
    assert (host == 7).all() and np.array_equal(out_state.fetch(), pattern)
    # group sums
    foreign, same_T = a.client.state(9, T_SRC), server.state(9, T_SRC)
    sums = server.state(9, -(-T_SRC // 4)).put(np.zeros((9, -(-T_SRC // 4), ctw), np.uint64))
    for args in ((a.state, 0, 9, 4, same_T, 0),                          # a wrong dst T
                 (a.state, 0, 9, 5, sums, 0),
                 (a.state, 0, 9, 1, a.state, 0),                         # src == dst
                 (a.state, 0, 9, 0, sums, 0), (a.state, 0, 9, 65537, sums, 0),
                 (foreign, 0, 9, 4, sums, 0), (a.state, 0, 9, 4, foreign, 0),   # a state of another context
                 (a.state, 1, 9, 4, sums, 0), (a.state, 0, 9, 4, sums, 1), (a.state, 10, 0, 4, sums, 0)):   # rows past either state's rows
        src, row0, rows, group, dst, dst_row0 = args
        assert lib.fbs_state_sum_groups(server._h, src._h, row0, rows, group, dst._h, dst_row0) == E_INVALID, args[1:4] + args[5:]
    with pytest.raises(ValueError, match="outside"):
        a.state.sum_groups(0)
    assert not sums.fetch().any() and np.array_equal(a.state.fetch(), a.first) and np.array_equal(out_state.fetch(), pattern)
    # the context still evaluates, and the same calls with the offending argument put right go through
    assert lib.fbs_state_sum_groups(server._h, a.state._h, 0, 9, 4, sums._h, 0) == 0
    assert np.array_equal(sums.fetch(), _sums(a.first, 4))
    assert code(seeded_input=4, map_it=False) == 0
    want = prog.eval_sources([("seeded", a.bodies[4], a.nonce0) if i == 4 else a.host_link(i) for i in range(a.n_in)], T)
    assert np.array_equal(out_state.fetch(), want)
    assert code() == 0 and np.array_equal(out_state.fetch(), prog.eval_sources(a.feeds()[1], T))
    for st in (out_state, foreign, same_T, sums):
        st.close()
    assert server.stat("states_alive") == 1 and a.client.stat("states_alive") == 0
