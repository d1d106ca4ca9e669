"""Plaintext server inputs on the GPU (include/fbs_exec.h, "chained evaluation", FBS_SRC_PLAIN): fbs_eval_sources over plain sources
is, word for word, fbs_eval_sources over the same inputs given as full links that hold the trivial ciphertexts of the header's formula
(built here in numpy: D zero words, then m * Delta mod q) -- at odd and even ciphertext indices, per sample and broadcast, mixed with
seeded inputs and alone, with full and compact outputs; an input wired to an output comes back as that trivial ciphertext; resident,
with state rows beside it, into a state, without growing scratch; in chunks; what must be refused is, with nothing written; and
through `split`: client-encrypted a, server-held b, the cleartext sum."""
import ctypes as C

import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import load_fixture, toy_k3

pytestmark = pytest.mark.gpu

E_INVALID = -1
P = 7
SPECIAL = (0, 1, P - 1, P, 2 * P - 1)
# four inputs, three bootstraps on two levels, a pass-through of a and of d, a constant and a linear combination among the outputs
PROGRAM = """m1 = 1 * a + 1 * b
m2 = Bootstrap(m1, [0, 1, 0])
m3 = 1 * c + 2 * d
m4 = Bootstrap(m3, [0, 1, 1, 0])
m5 = 1 * m2 + 1 * m4
m6 = Bootstrap(m5, [0, 1, 1])
Output x = m2
Output pa = a
Output y = m4
Output k = 1
Output z = m6
Output pd = d
Output s = m3
"""
INPUTS = ["a", "b", "c", "d"]


def _k1_n256():
    from tfhe_fbs_map_amd import Params
    return Params(n=12, log_n_poly=8, p_msg=P, sigma_lwe=1 << 8, sigma_glwe=1 << 8)


SETS = {"k1_n256": _k1_n256, "k3_n512": lambda: toy_k3(P)}
_MADE = {}


def made(name):
    """(client context, evaluation-only server context, lowered program, loaded program) of a toy set, once per module"""
    if name not in _MADE:
        from tfhe_fbs_map_amd import Context, _native as nat, parse_fbs
        client = Context(SETS[name](), seed=11, keygen=False)
        client.keygen_seeded()
        server = Context.evaluation_only(client.params, **client.export_seeded_keys())
        assert server.stat("has_secret") == 0 and server.params.ct_words % 2 == 1
        low = parse_fbs(PROGRAM, inputs=INPUTS).lower()
        assert low["input_names"] == INPUTS
        tv = server.tvset(low["tables"])
        prog = nat.Program(server, tv, 4, low["kind"], low["arg0"], low["arg1"], low["const_coef"], low["term_coef"], low["term_src"],
                           low["out_wire"])
        prog._tv = tv
        _MADE[name] = (client, server, low, prog)
    return _MADE[name]


def trivial(prm, msgs):
    """the header's formula: [count][D + 1], zero mask, body m * Delta mod q, Delta = 2 * round(q / 4p)"""
    p = prm.p_msg
    delta = 2 * ((orc.Q + 2 * p) // (4 * p))
    m = np.asarray(msgs, np.int64).reshape(-1)
    cts = np.zeros((m.size, prm.ct_words), np.uint64)
    cts[:, -1] = [int(v) * delta % orc.Q for v in m]
    return cts


def messages(T, shift):
    """[4][T] over the five special messages: every one of them appears, at T = 1 over the two shifts"""
    return np.array([[SPECIAL[(i + s + shift) % 5] for s in range(T)] for i in range(4)], np.int64)


def feeds(client, msgs, T, plain, broadcast, seeded):
    """-> (the feed with inputs `plain` as plain sources, the same with them as full links of trivial ciphertexts); the others seeded"""
    got, want = [], []
    for i in range(4):
        if i in plain:
            row = np.full(T, msgs[i, 0]) if broadcast else msgs[i]
            got.append(("plain", int(msgs[i, 0]) if broadcast else msgs[i].copy()))
            want.append(("full", trivial(client.params, row), False))
        else:
            src = ("seeded", seeded[0][i], seeded[1] + i * T)
            got.append(src)
            want.append(src)
    return got, want


@pytest.mark.parametrize("T", [1, 3, 65])
@pytest.mark.parametrize("name", list(SETS))
def test_plain_sources_are_trivial_full_links_word_for_word(name, T):
    client, server, low, prog = made(name)
    prm = server.params
    b = prm.log_n_poly + 1
    assert b < 17
    slots = [int(s) for s in prog.in_slot]
    assert {s % 2 for s in slots} == {0, 1}, slots          # plain inputs in an even and in an odd slot
    seen = set()
    for shift in (0, 1):
        msgs = messages(T, shift)
        seen |= set(msgs.reshape(-1).tolist())
        seeded = client.encrypt_seeded(msgs, nonce0=1000 * T + 7)
        seeded = (seeded[0].reshape(4, T), seeded[1])
        for plain in ((0, 1, 2, 3), (1, 3), (0, 2)):         # an all-plain program, and the two mixes with seeded inputs
            for broadcast in (False, True):
                got, want = feeds(client, msgs, T, plain, broadcast, seeded)
                for bits in (0, b, 17):
                    out, ref = prog.eval_sources(got, T, bits), prog.eval_sources(want, T, bits)
                    assert np.array_equal(out, ref), (name, T, shift, plain, broadcast, bits)
                if len(plain) == 4:                          # a pass-through returns the trivial ciphertext itself
                    full = prog.eval_sources(got, T)
                    for o, i in ((1, 0), (5, 3)):
                        assert low["out_wire"][o] == i
                        assert np.array_equal(full[o], trivial(prm, np.full(T, msgs[i, 0]) if broadcast else msgs[i])), (name, T, o)
                    assert np.array_equal(full[3], trivial(prm, np.ones(T)))      # and a constant output is written the same way
                    assert np.array_equal(client.decrypt(full[1]), (np.full(T, msgs[0, 0]) if broadcast else msgs[0]) % (2 * P))
    assert seen == set(SPECIAL)


@pytest.mark.parametrize("name", list(SETS))
def test_resident_with_plain_seeded_and_state_rows(name):
    client, server, low, prog = made(name)
    T = 65
    msgs = messages(T, 2)
    bodies, nonce0 = client.encrypt_seeded(msgs, nonce0=90_000)
    bodies = bodies.reshape(4, T)
    first = prog.eval_seeded(bodies, T, nonce0)                                   # [7][T][D + 1]: rows 0, 2, 4 are bootstrap outputs
    with server.state(7, T) as state, server.state(prog.n_outputs, T) as out:
        state.put(first)
        feed = [("plain", msgs[0].copy()), ("seeded", bodies[1], nonce0 + T), ("state", state, 4, False), ("plain", int(msgs[3, 0]))]
        want = prog.eval_sources([("full", trivial(server.params, msgs[0]), False), feed[1], ("full", first[4], False),
                                  ("full", trivial(server.params, np.full(T, msgs[3, 0])), False)], T)
        host = prog.eval_resident(feed, T)
        assert np.array_equal(host, want)
        assert prog.eval_resident(feed, T, out_state=out) is out                  # plain, seeded, resident: queued, not waited for
        assert np.array_equal(out.fetch(), host)
        growths = server.stat("scratch_growths")
        for _ in range(2):
            prog.eval_resident(feed, T, out_state=out)
            assert np.array_equal(prog.eval_sources([("plain", msgs[i].copy()) for i in range(4)], T)[1], trivial(server.params, msgs[0]))
        assert np.array_equal(out.fetch(), host)
        assert server.stat("scratch_growths") == growths
        assert np.array_equal(state.fetch(), first)


@pytest.mark.parametrize("name", list(SETS))
def test_chunked_is_unchunked(name, monkeypatch):
    client, server, low, prog = made(name)
    T = 150
    msgs = messages(T, 3)
    bodies, nonce0 = client.encrypt_seeded(msgs, nonce0=200_000)
    seeded = (bodies.reshape(4, T), nonce0)
    runs = []
    for plain, broadcast in (((0, 1, 2, 3), False), ((1, 3), False), ((0, 2), True)):
        got, _ = feeds(client, msgs, T, plain, broadcast, seeded)
        runs.append((got, prog.eval_sources(got, T), prog.eval_sources(got, T, 17)))
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "1")
    assert 0.6 * 2**20 / (prog.n_slots * server.params.ct_words * 8) < T         # two chunks or more
    with server.state(prog.n_outputs, T) as out:
        for got, full, compact in runs:
            assert np.array_equal(prog.eval_sources(got, T), full)
            assert np.array_equal(prog.eval_sources(got, T, 17), compact)
            prog.eval_resident(got, T, out_state=out)
            assert np.array_equal(out.fetch(), full)
    monkeypatch.delenv("FBS_WIRE_BUDGET_MB")


def test_refusals_write_nothing():
    from tfhe_fbs_map_amd import FbsError, _native as nat
    client, server, low, prog = made("k3_n512")
    T, ctw, lib = 3, server.params.ct_words, nat.lib
    msgs = messages(T, 0)
    keep = [np.ascontiguousarray(msgs[i]) for i in range(4)]
    good = [(3, 0, 0, 0, keep[i].ctypes.data) for i in range(4)]
    out = np.full((prog.n_outputs, T, ctw), 7, np.uint64)
    pattern = np.random.default_rng(5).integers(0, orc.Q, (prog.n_outputs, T, ctw), dtype=np.uint64)
    state = server.state(prog.n_outputs, T).put(pattern)

    def code(kinds, to_state=False):
        arr = (nat._InputSrc * 4)()
        for i, k in enumerate(kinds):
            arr[i] = nat._InputSrc(*k)
        try:
            if to_state:
                server._check(lib.fbs_eval_resident(server._h, prog._h, C.byref(arr), None, T, 0, None, state._h))
            else:
                server._check(lib.fbs_eval_sources(server._h, prog._h, C.byref(arr), T, 0, out.ctypes.data))
        except FbsError as e:
            return e.code
        return 0
    too_big, negative = np.array([0, 2 * P, 1], np.int64), np.array([0, 1, -1], np.int64)
    for to_state in (False, True):
        assert code(good[:2] + [(3, 0, 0, 0, too_big.ctypes.data)] + good[3:], to_state) == E_INVALID      # a message of 2p
        assert "outside [0, 2p)" in lib.fbs_last_error(server._h).decode()
        assert code([(3, 0, 0, 0, negative.ctypes.data)] + good[1:], to_state) == E_INVALID                 # a message of -1
        assert code(good[:3] + [(3, 1, 0, 0, too_big[1:].ctypes.data)], to_state) == E_INVALID              # ... as a broadcast message
        assert code(good[:1] + [(3, 0, 1, 0, keep[1].ctypes.data)] + good[2:], to_state) == E_INVALID       # refresh = 1
        assert code(good[:3] + [(3, 0, 0, 0, None)], to_state) == E_INVALID                                 # null data
        assert code(good[:3] + [(3, 2, 0, 0, keep[3].ctypes.data)], to_state) == E_INVALID                  # bits is 0 or 1
        assert code(good[:3] + [(4, 0, 0, 0, keep[3].ctypes.data)], to_state) == E_INVALID                  # the next kind is unknown
    assert (out == 7).all() and np.array_equal(state.fetch(), pattern)
    # the context then runs a good call, into the host and into the state
    want = prog.eval_sources([("full", trivial(server.params, msgs[i]), False) for i in range(4)], T)
    assert code(good) == 0 and np.array_equal(out, want)
    assert code(good, to_state=True) == 0 and np.array_equal(state.fetch(), want)
    state.close()


def test_split_client_encrypts_a_server_holds_b():
    from tfhe_fbs_map_amd import Client, ExecConfig, PlainInputs, Server, parse_fbs
    rec = load_fixture("adder8__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    T = 16
    a_names, b_names = [f"a{i}" for i in range(8)], [f"b{i}" for i in range(8)]
    client = Client(env, ExecConfig(seed=3))
    server = Server(client.server_key())
    assert server.ctx.stat("has_secret") == 0                                    # an evaluation-only server does all of it
    rng = np.random.default_rng(6)
    a = {n: rng.integers(0, 2, T) for n in a_names}
    per_sample = {n: rng.integers(0, 2, T) for n in b_names}
    constant = {n: (0xA5 >> i) & 1 for i, n in enumerate(b_names)}
    enc_a = client.encrypt(a, names=a_names)
    seeded_norm2 = server.run(env, client.encrypt({**a, **per_sample})).out_norm2
    for b, plain in ((per_sample, PlainInputs(b_names, T, per_sample)), (constant, PlainInputs(b_names, None, constant))):
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**a, **{n: np.broadcast_to(v, (T,)) for n, v in b.items()}})
        outs = [server.run_chain(env, [enc_a, plain]), server.run_chain(env, [plain, enc_a], compact=True), server.run(env, enc_a, plain=plain)]
        with server.run_chain(env, [enc_a, plain], resident=True) as res:
            outs.append(res.fetch())
            outs.append(res.fetch(compact=True))
            assert np.array_equal(res.out_norm2, seeded_norm2)
        for k, out in enumerate(outs):
            assert np.array_equal(out.out_norm2, seeded_norm2), k
            got = client.decrypt(out)
            for name in clear:
                assert np.array_equal(np.broadcast_to(got[name], (T,)), np.broadcast_to(clear[name], (T,))), (k, name)
    assert server.ctx.stat("has_secret") == 0
    server.ctx.close()
    client.ctx.close()
