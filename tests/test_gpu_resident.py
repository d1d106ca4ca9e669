"""Resident state on the GPU (include/fbs_exec.h, "resident state"): fbs_eval_resident over state rows is fbs_eval_sources over the
same ciphertexts as full links, word for word, into the host and into a state, mixed with seeded and compact sources, chunked too;
the gather and the scatter are the identity at the odd ciphertext stride and leave every other row alone; fbs_state_fetch at a
width is fbs_compact_dev of the full fetch; a 32-hop adder8 accumulator whose state never leaves the card but to be checked
decrypts to the cleartext running sum after every hop without growing scratch; a chain is handed to a second server through a
compact file and goes on resident there; and what must be refused is, with nothing written."""
import ctypes as C

import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import load_fixture, subsample
from tests.test_gpu_compact import compact_on_device, unpack
from tests.test_gpu_device_io import SETS

pytestmark = pytest.mark.gpu

E_INVALID = -1
ADDER = "adder8__search_p15"
A_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}
B_NAMES = [f"b{i}" for i in range(8)]
T = 37


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


def _adder_setup(seed=7):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture(ADDER)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=seed), programs=[env])
    return rec, env, client, Server(client.server_key())


def _hop_inputs(rng, T):
    return {f"b{i}": rng.integers(0, 2, T) for i in range(8)}


def _same(got, clear, T, what):
    for k in clear:
        assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (what, k)


class Adder8:
    """adder8 at the toy k = 1, N = 1024 set: the outputs of one seeded evaluation (9 rows of bits) in a state, the inputs of a
    second evaluation taken from those rows in a shuffled order in which rows repeat, and that evaluation's outputs by the
    host-source path (fbs_eval_sources over ("full", ...) links, held to the oracle by tests/test_gpu_chain.py): computed once"""

    def __init__(self):
        self.client, self.server = _pair("k1_n1024")
        self.rec, self.low, self.prog = _program(self.server, "adder8__search_p7")
        ins, _ = subsample(self.rec, T)
        self.n_in = len(self.low["input_names"])
        msgs = np.stack([np.asarray(ins[k], np.int64) for k in self.low["input_names"]])
        self.bodies, self.nonce0 = self.client.encrypt_seeded(msgs, nonce0=5)
        self.first = self.prog.eval_seeded(self.bodies, T, self.nonce0)          # [9][T][D+1]
        self.rows = [(5 * i + 3) % 9 for i in range(self.n_in)]                  # 16 inputs over 9 rows: 7 rows feed two inputs
        self.full_feed = [("full", self.first[r], False) for r in self.rows]
        self.want = self.prog.eval_sources(self.full_feed, T)
        self.state = self.server.state(9, T).put(self.first)

    def state_feed(self, refresh=lambda i: False, state=None):
        return [("state", state or self.state, r, refresh(i)) for i, r in enumerate(self.rows)]


@pytest.fixture(scope="module")
def adder8():
    a = Adder8()
    yield a
    a.server.close()
    a.client.close()


def test_state_rows_are_full_sources_word_for_word(adder8):
    a, prog, server = adder8, adder8.prog, adder8.server
    assert len(set(a.rows)) == 9 and len(a.rows) == 16
    assert np.array_equal(a.state.fetch(), a.first)
    assert (server.stat("states_alive"), server.stat("state_bytes")) == (1, a.first.nbytes)
    # into the host, and into a state
    assert np.array_equal(prog.eval_resident(a.state_feed(), T), a.want)
    with server.state(prog.n_outputs, T) as out:
        assert prog.eval_resident(a.state_feed(), T, out_state=out) is out
        assert np.array_equal(out.fetch(), a.want)
        assert np.array_equal(out.fetch(3, 2), a.want[3:5])
        assert server.stat("states_alive") == 2
    assert server.stat("states_alive") == 1
    # state, seeded and compact sources in one call, against the same call with the state rows as full links
    b = server.params.log_n_poly + 1
    words = prog.eval_seeded_compact(a.bodies, T, a.nonce0, b + 2)
    def mixed(state_rows):
        feed = []
        for i in range(a.n_in):
            if i % 3 == 0:
                feed.append(("seeded", a.bodies[i], a.nonce0 + i * T))
            elif i % 3 == 1:
                feed.append(("compact", words[i % 9], b + 2))
            else:
                feed.append(("state", a.state, a.rows[i], False) if state_rows else a.full_feed[i])
        return feed
    want_mixed = prog.eval_sources(mixed(False), T)
    assert np.array_equal(prog.eval_resident(mixed(True), T), want_mixed)
    assert np.array_equal(prog.eval_resident(mixed(True), T, b), prog.eval_sources(mixed(False), T, b))
    with server.state(prog.n_outputs, T) as out:
        prog.eval_resident(mixed(True), T, out_state=out)         # a compact host source: this one blocks
        assert np.array_equal(out.fetch(), want_mixed)
        only = [("seeded", a.bodies[i], a.nonce0 + i * T) if i % 2 else ("state", a.state, a.rows[i], False) for i in range(a.n_in)]
        prog.eval_resident(only, T, out_state=out)                # state and seeded sources only: queued, not waited for
        assert np.array_equal(out.fetch(), prog.eval_sources([s if i % 2 else a.full_feed[i] for i, s in enumerate(only)], T))
    # refreshed rows: word for word the refreshed full links, and the messages of the unrefreshed ones
    odd = lambda i: i % 2 == 1
    refreshed = prog.eval_resident(a.state_feed(odd), T)
    assert np.array_equal(refreshed, prog.eval_sources([("full", a.first[r], odd(i)) for i, r in enumerate(a.rows)], T))
    assert not np.array_equal(refreshed, a.want)
    assert np.array_equal(a.client.decrypt(refreshed), a.client.decrypt(a.want))
    # repeated calls of one shape do not grow scratch
    growths = server.stat("scratch_growths")
    with server.state(prog.n_outputs, T) as out:
        for _ in range(3):
            prog.eval_resident(a.state_feed(odd), T, out_state=out)
            prog.eval_resident(a.state_feed(), T, out_state=out)
        assert np.array_equal(out.fetch(), a.want)
    assert server.stat("scratch_growths") == growths
    assert np.array_equal(a.state.fetch(), a.first)               # the input state is only read


PASS_THROUGH = """m1 = 1 * a + 1 * b
m2 = Bootstrap(m1, [0, 1, 0])
Output pc = c
Output pa = a
Output k = 1
Output pb = b
Output s = m1
Output t = m2
"""


@pytest.mark.parametrize("T_", [1, 3])
def test_gather_and_scatter_are_the_identity_at_the_odd_stride(adder8, T_):
    """D + 1 words a ciphertext and an odd T: ciphertext (row, sample) starts on an odd multiple of 8 bytes whenever row * T + sample is
    odd, in the state and -- at another parity -- in the wire slots; a program that passes inputs through moves them by the gather
    and the scatter alone"""
    from tfhe_fbs_map_amd import parse_fbs
    server = adder8.server
    ctw = server.params.ct_words
    assert ctw % 2 == 1
    low = parse_fbs(PASS_THROUGH, inputs=["a", "b", "c"]).lower()
    assert low["input_names"] == ["a", "b", "c"] and low["out_wire"][:4] == [2, 0, -2, 1]
    prog = _load(server, low)
    rng = np.random.default_rng(T_)
    pattern = rng.integers(0, orc.Q, (6, T_, ctw), dtype=np.uint64)
    src = server.state(6, T_).put(pattern)
    out = server.state(6, T_).put(pattern[::-1])
    feed = [("state", src, 3, False), ("state", src, 0, False), ("state", src, 2, False)]        # a, b, c; rows 1, 4, 5 are not named
    prog.eval_resident(feed, T_, out_state=out)
    got = out.fetch()
    assert np.array_equal(got[0], pattern[2]) and np.array_equal(got[1], pattern[3]) and np.array_equal(got[3], pattern[0])
    assert np.array_equal(got[4], (pattern[3] + pattern[0]) % np.uint64(orc.Q))
    assert not got[2, :, :-1].any() and (got[2, :, -1] == got[2, 0, -1]).all() and got[2, 0, -1] != 0   # the trivial ciphertext of 1
    assert np.array_equal(got, prog.eval_sources([("full", pattern[r], False) for r in (3, 0, 2)], T_))
    assert np.array_equal(src.fetch(), pattern)
    # and once more from the state just written, into a third: rows 0, 1, 3 of `out` come through unchanged
    third = server.state(6, T_).put(pattern)
    prog.eval_resident([("state", out, 1, False), ("state", out, 3, False), ("state", out, 0, False)], T_, out_state=third)
    again = third.fetch()
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and np.array_equal(again[3], got[3])
    assert np.array_equal(out.fetch(), got)
    # a put into the middle of a state leaves its other rows alone
    src.put(pattern[4:6], row0=1)
    assert np.array_equal(src.fetch(), np.concatenate([pattern[:1], pattern[4:6], pattern[3:]]))
    for st in (src, out, third):
        st.close()
    prog.close()
    assert server.stat("states_alive") == 1


def test_chunked_is_unchunked(adder8, monkeypatch):
    from tfhe_fbs_map_amd import Context
    a = adder8
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")
    assert 2 * 2**20 * 0.6 / (a.prog.n_slots * a.server.params.ct_words * 8) < T / 3          # three chunks or more
    fresh = Context.evaluation_only(a.client.params, **a.client.export_seeded_keys())
    _, _, prog = _program(fresh, "adder8__search_p7")
    state = fresh.state(9, T).put(a.first)
    assert np.array_equal(prog.eval_resident(a.state_feed(state=state), T), a.want)
    out = fresh.state(prog.n_outputs, T)
    prog.eval_resident(a.state_feed(state=state), T, out_state=out)
    assert np.array_equal(out.fetch(), a.want)
    half = [("seeded", a.bodies[i], a.nonce0 + i * T) if i % 2 else ("state", state, a.rows[i], i % 4 == 0) for i in range(a.n_in)]
    prog.eval_resident(half, T, out_state=out)
    monkeypatch.delenv("FBS_WIRE_BUDGET_MB")
    want = a.prog.eval_sources([s if i % 2 else ("full", a.first[a.rows[i]], i % 4 == 0) for i, s in enumerate(half)], T)
    assert np.array_equal(out.fetch(), want)
    fresh.close()
    assert out.closed and state.closed


def test_fetch_at_a_width_is_compact_dev_of_the_full_fetch():
    client, server = _pair("k3")
    rec, low, prog = _program(server, "edge_outputs")
    T_ = 9
    ins, _ = subsample(rec, T_)
    msgs = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]]).reshape(len(low["input_names"]), T_)
    bodies, nonce0 = client.encrypt_seeded(msgs, nonce0=33)
    seeded = [("seeded", bodies[i], nonce0 + i * T_) for i in range(len(msgs))]
    n, b = server.params.n, server.params.log_n_poly + 1
    with server.state(prog.n_outputs, T_) as out:
        prog.eval_resident(seeded, T_, out_state=out)
        full = out.fetch()
        assert np.array_equal(full, prog.eval_seeded(bodies, T_, nonce0))
        for bits in (b, b + 2):
            words = out.fetch(bits=bits)
            assert words.shape == (prog.n_outputs, T_, server.compact_words(bits))
            assert np.array_equal(words.reshape(-1, words.shape[-1]), compact_on_device(server, full, bits)), bits
            assert np.array_equal(words, prog.eval_seeded_compact(bodies, T_, nonce0, bits)), bits
            assert np.array_equal(out.fetch(2, 3, bits=bits), words[2:5])
            for o, w in enumerate(low["out_wire"]):
                if w < 0:   # a constant output: zero mask fields
                    assert not unpack(words[o], n, bits)[:, :n].any(), (bits, o)
            assert np.array_equal(client.decrypt_compact(words, bits), client.decrypt(full))
    assert sum(w < 0 for w in low["out_wire"]) == 2
    server.close()
    client.close()


def test_adder8_accumulator_32_resident_hops():
    """the accumulator of tests/test_gpu_chain.py with the state on the card: acc <- acc + b over 32 hops; the client decrypts a
    full fetch after even hops and a compact one after odd hops"""
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedOutputs, ResidentOutputs
    T_ = 16
    rec, env, client, server = _adder_setup()
    rng = np.random.default_rng(1)
    first = {**{f"a{i}": rng.integers(0, 2, T_) for i in range(8)}, **_hop_inputs(rng, T_)}
    acc = server.run(env, client.encrypt(first), resident=True)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    _same(client.decrypt(acc.fetch()), clear, T_, "first")
    _same(client.decrypt(acc.fetch(compact=True)), clear, T_, "first, compact")   # (the packed staging exists from here on)
    growths = None
    for hop in range(32):
        fresh = _hop_inputs(rng, T_)
        nxt = server.run_chain(env, [acc, client.encrypt(fresh, names=B_NAMES)], rename=A_FROM_S, resident=True)
        acc.close()
        acc = nxt
        assert isinstance(acc, ResidentOutputs) and acc.T == T_ and acc.out_norm2 is not None
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T_,)) for i in range(8)}, **fresh})
        got = acc.fetch() if hop % 2 == 0 else acc.fetch(compact=True)
        assert isinstance(got, EncryptedOutputs if hop % 2 == 0 else CompactOutputs)
        if hop % 2:
            assert got.bits == server.compact_bits(env)
        _same(client.decrypt(got), clear, T_, hop)
        assert server.ctx.stat("states_alive") == 1
        if hop == 0:      # the first chained hop; nothing grows after it
            growths = server.ctx.stat("scratch_growths")
        else:
            assert server.ctx.stat("scratch_growths") == growths, hop
    acc.close()
    assert server.ctx.stat("states_alive") == 0 and server.ctx.stat("state_bytes") == 0


def test_a_chain_is_handed_over_compact_and_goes_on_resident(tmp_path):
    from tfhe_fbs_map_amd import Server, ServerKey
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedOutputs
    T_ = 8
    rec, env, client, server_a = _adder_setup(seed=4)
    rng = np.random.default_rng(3)
    first = {**{f"a{i}": rng.integers(0, 2, T_) for i in range(8)}, **_hop_inputs(rng, T_)}
    key, mid, full = (str(tmp_path / f) for f in ("key.npz", "mid.npz", "full.npz"))
    client.server_key().save(key)
    acc = server_a.run(env, client.encrypt(first), resident=True)
    acc.fetch(compact=True).save(mid)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    server_b = Server(ServerKey.load(key))
    with pytest.raises(ValueError, match="another server"):
        server_b.run_chain(env, [acc, client.encrypt(_hop_inputs(rng, T_), names=B_NAMES)], rename=A_FROM_S, resident=True)
    acc.close()
    with pytest.raises(ValueError, match="closed"):
        server_a.run_chain(env, [acc, client.encrypt(_hop_inputs(rng, T_), names=B_NAMES)], rename=A_FROM_S, resident=True)
    with pytest.raises(ValueError, match="closed"):
        acc.fetch()
    server_a.ctx.close()
    state = CompactOutputs.load(mid)                  # a compact link: the first hop on the second server refreshes it
    for hop in range(3):
        fresh = _hop_inputs(rng, T_)
        nxt = server_b.run_chain(env, [state, client.encrypt(fresh, names=B_NAMES)], rename=A_FROM_S, resident=True)
        if hop:
            state.close()
        state = nxt
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T_,)) for i in range(8)}, **fresh})
        _same(client.decrypt(state.fetch(compact=True)), clear, T_, hop)
    # a full fetch saved to disk goes back into device memory and links as before
    state.fetch().save(full)
    state.close()
    state = server_b.restore(EncryptedOutputs.load(full))
    assert server_b.ctx.stat("states_alive") == 1
    fresh = _hop_inputs(rng, T_)
    out = server_b.run_chain(env, [state, client.encrypt(fresh, names=B_NAMES)], rename=A_FROM_S)     # resident in, host out
    clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T_,)) for i in range(8)}, **fresh})
    _same(client.decrypt(out), clear, T_, "restored")
    with pytest.raises(ValueError, match="pass bits"):
        state.fetch(compact=True)
    server_b.ctx.close()
    assert state.closed
    state.close()


def test_refusals_write_nothing(adder8):
    from tfhe_fbs_map_amd import FbsError, _native as nat
    a, prog, server, lib = adder8, adder8.prog, adder8.server, nat.lib
    ctw, n_out = server.params.ct_words, adder8.prog.n_outputs
    pattern = np.random.default_rng(9).integers(0, orc.Q, (n_out, T, ctw), dtype=np.uint64)
    out_state = server.state(n_out, T).put(pattern)
    host = np.full((n_out, T, ctw), 7, np.uint64)
    longer, short, foreign = server.state(9, T + 1), server.state(n_out - 1, T), a.client.state(9, T)
    srcs = (nat._InputSrc * a.n_in)()

    def code(res=None, T_=T, out_bits=0, to_host=False, to_state=True, state=out_state):
        arr = (nat._ResidentSrc * a.n_in)()
        for i, r in enumerate(a.rows):
            arr[i] = nat._ResidentSrc(a.state._h.value, r, 0)
        for i, (st, row) in (res or {}).items():
            arr[i] = nat._ResidentSrc(st._h.value if st is not None else None, row, 0)
        try:
            server._check(lib.fbs_eval_resident(server._h, prog._h, C.byref(srcs), C.byref(arr), T_, out_bits,
                                                host.ctypes.data if to_host else None, state._h if to_state else None))
        except FbsError as e:
            return e.code
        return 0
    assert code({3: (a.state, 9)}) == E_INVALID                          # a row past the state's rows
    assert code({3: (a.state, 0xFFFFFFFF)}) == E_INVALID
    assert code({0: (longer, 0)}) == E_INVALID                           # a state whose T differs from the call's
    assert code(T_=T + 1) == E_INVALID
    assert code(state=short) == E_INVALID                                # an out_state with rows != n_outputs
    assert code({5: (out_state, 1)}) == E_INVALID                        # an out_state that is also an input state
    assert code(to_host=True) == E_INVALID                               # both
    assert code(to_state=False) == E_INVALID                             # neither
    assert code(out_bits=server.params.log_n_poly + 1) == E_INVALID      # compact outputs into a state
    assert code({2: (foreign, 0)}) == E_INVALID                          # a state of another context
    assert code(state=foreign) == E_INVALID
    assert code({4: (None, 0)}) == E_INVALID                             # no state: srcs[4] is read, and its data is null
    assert code(to_host=True, to_state=False, out_bits=5) == E_INVALID   # what fbs_eval_sources refuses
    assert (host == 7).all() and np.array_equal(out_state.fetch(), pattern)
    # fetch and put
    for args in ((out_state, n_out, 1, 0), (out_state, 0, n_out + 1, 0), (foreign, 0, 1, 0), (out_state, 0, 1, 5), (out_state, 0, 1, 32)):
        st, row0, rows, bits = args
        assert lib.fbs_state_fetch(server._h, st._h, row0, rows, bits, host.ctypes.data) == E_INVALID, args[1:]
    bad = pattern.copy()
    bad[2, 5, 17] = orc.Q
    assert lib.fbs_state_put(server._h, out_state._h, 0, n_out, bad.ctypes.data) == E_INVALID
    assert "canonical" in lib.fbs_last_error(server._h).decode()
    assert lib.fbs_state_put(server._h, out_state._h, 1, n_out, pattern.ctypes.data) == E_INVALID
    assert (host == 7).all() and np.array_equal(out_state.fetch(), pattern)
    # counts are checked before anything is sized; a state the device cannot hold is a device error, and the context goes on
    h = C.c_void_p()
    for rows, T_ in ((0, 4), (4, 0), ((1 << 28) + 1, 1), (1 << 20, 2**64 // (1 << 20) // 8)):
        assert lib.fbs_state_create(server._h, rows, T_, C.byref(h)) == E_INVALID and not h.value, (rows, T_)
    assert lib.fbs_state_create(server._h, 1 << 20, 1 << 20, C.byref(h)) == -2 and not h.value      # 2^40 ciphertexts
    alive = server.stat("states_alive")
    assert code() == 0 and np.array_equal(out_state.fetch(), a.want)
    rows_, T__ = C.c_size_t(), C.c_size_t()
    assert lib.fbs_state_info(longer._h, C.byref(rows_), C.byref(T__)) == 0 and (rows_.value, T__.value) == (9, T + 1)
    lib.fbs_state_destroy(None)
    for st in (out_state, longer, short, foreign):
        st.close()
        st.close()
    assert server.stat("states_alive") == alive - 3 and a.client.stat("states_alive") == 0
    with pytest.raises(ValueError, match="closed"):
        prog.eval_resident(a.state_feed(state=out_state), T)
    # closing the context closes its states: their own close() is then a no-op
    from tfhe_fbs_map_amd import Context
    ctx = Context.evaluation_only(a.client.params, **a.client.export_seeded_keys())
    st = ctx.state(2, 3)
    ctx.close()
    assert st.closed
    st.close()
