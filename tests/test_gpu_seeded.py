"""Evaluation without the secret key (include/fbs_exec.h, "seeded keys and inputs"): a server context made from the mask key
and the key bodies holds exactly the client's full keys; the device seeded encryption and expansion are word for word the host
entries; fbs_eval_seeded computes what the oracle and fbs_eval compute on the expanded inputs; an evaluation-only context refuses
everything that needs the secret and writes nothing; and a Client / Server pair in two processes reproduces LutExecEnv.eval."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import assert_outputs_equal, load_fixture, oracle_eval_program, subsample, toy_k2
from tests.test_gpu_device_io import SETS, dev, host, messages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONCE_LIMIT = 1 << 55
E_INVALID, E_STATE = -1, -3
_PAIRS = {}


def pair(name):
    """(client context keyed with keygen_seeded, evaluation-only server context from its server key), once per module"""
    if name not in _PAIRS:
        from tfhe_fbs_map_amd import Context
        prm = SETS[name]()
        client = Context(prm, seed=11, keygen=False)
        client.keygen_seeded()
        server = Context.evaluation_only(prm, **client.export_seeded_keys())
        _PAIRS[name] = (client, server)
    return _PAIRS[name]


def server_full_keys(server):
    from tfhe_fbs_map_amd import _native as nat
    sizes = (C.c_size_t * 4)()
    server._check(nat.lib.fbs_key_sizes(server._h, C.byref(sizes)))
    bsk, ksk = np.empty(sizes[2], np.uint64), np.empty(sizes[3], np.uint64)
    server._check(nat.lib.fbs_export_keys(server._h, None, None, bsk.ctypes.data, ksk.ctypes.data))
    return bsk, ksk


def expand_on_device(ctx, bodies, nonce0):
    import torch
    bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1)
    d_b = dev(bodies) if bodies.size else torch.empty(0, dtype=torch.int64, device="cuda")
    d_c = torch.full((max(1, bodies.size), ctx.params.ct_words), 7, dtype=torch.int64, device="cuda")
    ctx.expand_seeded_dev(d_b.data_ptr(), bodies.size, nonce0, d_c.data_ptr())
    ctx.sync()
    return host(d_c)[:bodies.size]


@pytest.mark.parametrize("name", list(SETS))
def test_server_keys_and_seeded_io_match_the_client(name):
    client, server = pair(name)
    assert client.stat("has_secret") == 1 and client.stat("seeded_keys") == 1
    assert server.stat("has_secret") == 0 and server.stat("seeded_keys") == 1
    full = client.export_keys()
    bsk, ksk = server_full_keys(server)
    assert np.array_equal(bsk, full["bsk"]) and np.array_equal(ksk, full["ksk"])
    p = client.params.p_msg
    for count in (0, 1, 7, 1000, 4099):
        m = messages(count, p, seed=count) % (2 * p)
        for nonce0 in (0, NONCE_LIMIT - count - 1):
            on_dev, first = client.encrypt_seeded(m, nonce0=nonce0)
            on_host, _ = client.encrypt_seeded(m, nonce0=nonce0, device=False)
            assert first == nonce0 and on_dev.shape == m.shape and np.array_equal(on_dev, on_host), (name, count, nonce0)
            cts = client.expand_seeded(on_host, nonce0)
            assert np.array_equal(server.expand_seeded(on_host, nonce0), cts)
            assert np.array_equal(expand_on_device(server, on_host, nonce0), cts), (name, count, nonce0)
            assert np.array_equal(client.decrypt(cts), m)
    # (a ciphertext at an odd word offset: the expanded rows of odd index start on one)
    assert client.params.ct_words % 2 == 1


def _program(nat, ctx, name, fuse=False):
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    tv = ctx.tvset(low["tables"])
    prog = nat.Program(ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"],
                       low["term_coef"], low["term_src"], low["out_wire"], fuse_tables=fuse)
    prog._tv = tv
    return rec, low, prog


@pytest.mark.parametrize("set_name,name,fuse", [("k1_n1024", "adder8__search_p7", False), ("k2", "adder8__search_p7", True),
                                                ("k2", "edge_outputs", True), ("k3", "edge_outputs", False)])
def test_eval_seeded_equals_oracle_eval_and_goldens(set_name, name, fuse):
    from tfhe_fbs_map_amd import _native as nat
    client, server = pair(set_name)
    rec, low, prog = _program(nat, server, name, fuse)
    _, _, cprog = _program(nat, client, name, fuse)
    T = 9
    ins, expect = subsample(rec, T)
    bits = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]]).reshape(len(low["input_names"]), T)
    bodies, nonce0 = client.encrypt_seeded(bits, nonce0=33)
    got = prog.eval_seeded(bodies, T, nonce0)
    full_in = client.expand_seeded(bodies, nonce0)                     # [n_in][T][D+1]: input i, sample s on stream 33 + i T + s
    assert np.array_equal(got, cprog.eval(full_in, T))
    o = orc.Oracle(client.params, seed=11, keygen=False)
    o.set_keys(**client.export_keys())
    ops, outs = lut_oracle.read_fbs(rec["fbs"])
    wires = oracle_eval_program(o, ops, outs, {n: full_in[i] for i, n in enumerate(low["input_names"])}, fuse=fuse)
    dec = client.decrypt(got)
    for k, (out_name, src) in enumerate(outs):
        assert out_name == low["out_names"][k]
        if low["out_wire"][k] >= 0:
            assert np.array_equal(got[k], wires[src]), (name, out_name)
        e = expect[out_name]
        assert np.array_equal(dec[k], np.full(T, e) if np.ndim(e) == 0 else np.asarray(e)), (name, out_name)
    if name == "edge_outputs":
        assert any(w < 0 for w in low["out_wire"])


def test_eval_seeded_in_chunks(monkeypatch):
    from tfhe_fbs_map_amd import Context, _native as nat
    client, _ = pair("k1_n1024")
    T = 37
    rec, low, cprog = _program(nat, client, "adder8__search_p7")
    ins, _ = subsample(rec, T)
    bits = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]])
    bodies, nonce0 = client.encrypt_seeded(bits, nonce0=2)
    want = cprog.eval(client.expand_seeded(bodies, nonce0), T)
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")
    assert 2 * 2**20 * 0.6 / (cprog.n_slots * client.params.ct_words * 8) < T / 3
    server = Context.evaluation_only(client.params, **client.export_seeded_keys())   # fresh: its wire buffer has not grown
    _, _, prog = _program(nat, server, "adder8__search_p7")
    assert np.array_equal(prog.eval_seeded(bodies, T, nonce0), want)
    assert prog.eval_seeded(bodies[:, :0], 0, nonce0).shape == (cprog.n_outputs, 0, client.params.ct_words)


def _code(call):
    from tfhe_fbs_map_amd import FbsError
    try:
        call()
    except FbsError as e:
        return e.code
    return 0


def test_evaluation_only_context_refuses_what_needs_the_secret():
    import torch
    from tfhe_fbs_map_amd import _native as nat
    client, server = pair("k1_n1024")
    lib, h = nat.lib, server._h
    ctw, D = server.params.ct_words, server.params.big_dim
    m = np.arange(4, dtype=np.int64)
    cts = np.full((4, ctw), 5, np.uint64)
    out_m = np.full(4, 9, np.int64)
    bodies = np.full(4, 3, np.uint64)
    d_m = dev(m)
    d_c = torch.full((4, ctw), 123, dtype=torch.int64, device="cuda")
    d_o = torch.full((4,), 55, dtype=torch.int64, device="cuda")
    sk = np.full(max(server.params.n, D), 77, np.uint64)
    mk = np.full(32, 1, np.uint8)
    nonce = C.c_uint64(99)
    before = server.stat("next_nonce")
    calls = [
        lambda: server._check(lib.fbs_encrypt(h, m.ctypes.data, 4, 0, cts.ctypes.data)),
        lambda: server._check(lib.fbs_encrypt_fresh(h, m.ctypes.data, 4, cts.ctypes.data, C.byref(nonce))),
        lambda: server._check(lib.fbs_decrypt(h, cts.ctypes.data, 4, out_m.ctypes.data)),
        lambda: server._check(lib.fbs_encrypt_dev(h, d_m.data_ptr(), 4, 0, d_c.data_ptr(), None)),
        lambda: server._check(lib.fbs_encrypt_fresh_dev(h, d_m.data_ptr(), 4, d_c.data_ptr(), C.byref(nonce), None)),
        lambda: server._check(lib.fbs_decrypt_dev(h, d_c.data_ptr(), 4, d_o.data_ptr(), None)),
        lambda: server._check(lib.fbs_encrypt_seeded(h, m.ctypes.data, 4, 0, bodies.ctypes.data)),
        lambda: server._check(lib.fbs_encrypt_seeded_fresh(h, m.ctypes.data, 4, bodies.ctypes.data, C.byref(nonce))),
        lambda: server._check(lib.fbs_encrypt_seeded_dev(h, d_m.data_ptr(), 4, 0, d_o.data_ptr(), None)),
        lambda: server._check(lib.fbs_encrypt_seeded_fresh_dev(h, d_m.data_ptr(), 4, d_o.data_ptr(), C.byref(nonce), None)),
        lambda: server._check(lib.fbs_export_seeded_keys(h, mk.ctypes.data, sk.ctypes.data, sk.ctypes.data)),
        lambda: server._check(lib.fbs_export_keys(h, sk.ctypes.data, None, None, None)),
        lambda: server._check(lib.fbs_export_keys(h, None, sk.ctypes.data, None, None)),
    ]
    for i, call in enumerate(calls):
        assert _code(call) == E_STATE, i
        assert "evaluation keys only" in nat.lib.fbs_last_error(h).decode(), i
    rec, low, prog = _program(nat, server, "full_adder__search_p7")
    msgs = np.zeros((prog.n_inputs, 3), np.int64)
    assert _code(lambda: prog.eval_messages(msgs, nonce0=1)) == E_STATE
    assert _code(lambda: prog.eval_messages(msgs)) == E_STATE
    server.sync()
    assert (cts == 5).all() and (out_m == 9).all() and (bodies == 3).all() and (sk == 77).all() and (mk == 1).all()
    assert nonce.value == 99 and server.stat("next_nonce") == before
    assert bool((d_c == 123).all()) and bool((d_o == 55).all())
    # what does not need the secret works: the batch, fbs_eval and the level entries (through fbs_eval), keys without secrets
    tv = server.tvset([[0, 1, 1, 0, 1, 0, 0]])
    fresh = client.encrypt(np.arange(6) % 7, nonce0=3)
    assert np.array_equal(client.decrypt(server.bootstrap_batch(tv, fresh)), [[0, 1, 1, 0, 1, 0, 0][v] for v in np.arange(6) % 7])
    ins, expect = subsample(rec, 4)
    bits = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]])
    got = client.decrypt(prog.eval(client.encrypt(bits, nonce0=8), 4))
    for k, n in enumerate(low["out_names"]):
        assert np.array_equal(got[k], expect[n]), n
    bsk, _ = server_full_keys(server)
    assert bsk.size and server.stat("has_secret") == 0


def test_bad_import_keeps_the_old_keys_and_keygen_contexts_export_no_seeded_keys():
    from tfhe_fbs_map_amd import Context, _native as nat
    client, _ = pair("k2")
    key = client.export_seeded_keys()
    server = Context.evaluation_only(client.params, **key)
    rec, low, prog = _program(nat, server, "full_adder__search_p7")
    T = 5
    ins, _ = subsample(rec, T)
    bits = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]])
    bodies, nonce0 = client.encrypt_seeded(bits, nonce0=4)
    want = prog.eval_seeded(bodies, T, nonce0)
    q = (1 << 46) - 62 * (1 << 13) + 1
    for field, where in (("bsk_bodies", -1), ("ksk_bodies", 0)):
        bad = dict(key)
        bad[field] = key[field].copy()
        bad[field][where] = q
        assert _code(lambda: server.import_seeded_keys(**bad)) == E_INVALID
        assert "canonical" in nat.lib.fbs_last_error(server._h).decode()
    assert nat.lib.fbs_import_seeded_keys(server._h, None, key["bsk_bodies"].ctypes.data, key["ksk_bodies"].ctypes.data) == E_INVALID
    assert np.array_equal(prog.eval_seeded(bodies, T, nonce0), want)
    assert server.stat("has_secret") == 0 and server.stat("seeded_keys") == 1
    plain = Context(client.params, seed=11)                               # fbs_keygen: the same secrets, no seeded keys
    assert plain.stat("seeded_keys") == 0 and plain.stat("has_secret") == 1
    assert _code(plain.export_seeded_keys) == E_STATE
    assert np.array_equal(plain.export_keys()["sk_glwe"], client.export_keys()["sk_glwe"])
    # a full context decrypts what the seeded path produced on the same secrets
    assert np.array_equal(plain.decrypt(client.expand_seeded(bodies, nonce0)), bits)


def test_seeded_nonces_follow_the_rules_of_encrypt():
    client, server = pair("k1_n1024")
    m = messages(6, 7) % 14
    for device in (True, False):
        for nonce0, count in ((NONCE_LIMIT - 3, 4), (NONCE_LIMIT, 1)):
            assert _code(lambda: client.encrypt_seeded(np.zeros(count, np.int64), nonce0=nonce0, device=device)) == E_INVALID
    b1, f1 = client.encrypt_seeded(m)                                       # fresh, on the device
    mid = client.stat("next_nonce")
    client.encrypt(m[:5])                                                    # fbs_encrypt_fresh: the same counter
    b3, f3 = client.encrypt_seeded(m[:3], device=False)
    assert f1 >= NONCE_LIMIT and mid == f1 + 6 and f3 == mid + 5 and client.stat("next_nonce") == f3 + 3
    for b, f, mm in ((b1, f1, m), (b3, f3, m[:3])):
        cts = server.expand_seeded(b, f)
        assert np.array_equal(expand_on_device(server, b, f), cts)
        assert np.array_equal(client.decrypt(cts), mm)
    assert _code(lambda: server.expand_seeded(b1, (1 << 56) - 2)) == E_INVALID      # stream ids are 56 bits


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tfhe_fbs_map_amd import EncryptedInputs, Server, ServerKey, parse_fbs
from tests.helpers import load_fixture
rec = load_fixture(sys.argv[2])
env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
server = Server(ServerKey.load(sys.argv[3]))
assert server.ctx.stat("has_secret") == 0, "the server holds a secret"
server.run(env, EncryptedInputs.load(sys.argv[4])).save(sys.argv[5])
print("server done")
"""


@pytest.mark.parametrize("name", ["adder8__search_p7", "edge_outputs"])
def test_client_and_server_in_two_processes(name, tmp_path):
    from tfhe_fbs_map_amd import Client, EncryptedOutputs, ExecConfig, parse_fbs
    rec = load_fixture(name)
    ins, expect = subsample(rec, 24)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = ExecConfig(seed=3)
    client = Client(env, cfg)
    key_path, in_path, out_path = (str(tmp_path / f) for f in ("server_key.npz", "inputs.npz", "outputs.npz"))
    client.server_key().save(key_path)
    client.encrypt(ins).save(in_path)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, name, key_path, in_path, out_path], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "server done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = client.decrypt(EncryptedOutputs.load(out_path))
    assert_outputs_equal(got, expect)
    want = env.eval(ins, config=cfg)
    assert got.keys() == want.keys()
    for k in want:
        assert type(got[k]) is type(want[k]) and np.array_equal(got[k], want[k]), k
    assert client.params == cfg.last_choice["params"] and client.fuse_tables == cfg.last_choice["fuse_tables"]


def test_server_refuses_foreign_inputs_and_tables():
    from tfhe_fbs_map_amd import Client, EncryptedInputs, ExecConfig, LutExecEnv, Server, parse_fbs
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = ExecConfig(seed=4, reduced_noise=True)
    a, b = Client(env, cfg), Client(env, ExecConfig(seed=5, reduced_noise=True))
    server = Server(a.server_key())
    ins, expect = subsample(rec, 6)
    with pytest.raises(ValueError, match="another server key"):
        server.run(env, b.encrypt(ins))
    wide = LutExecEnv()
    x, y = wide.input("x"), wide.input("y")
    s = wide.linear([1] * 20, [x] * 10 + [y] * 10)
    wide.output("o", wide.bootstrap(s, [v % 2 for v in range(21)]))
    with pytest.raises(ValueError, match="at the server key.s p = %d" % a.params.p_msg):
        server.run(wide, EncryptedInputs(["x", "y"], 1, 0, np.zeros((2, 1), np.uint64), a.fingerprint))
    assert_outputs_equal(a.decrypt(server.run(env, a.encrypt(ins))), expect)
