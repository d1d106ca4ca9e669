"""Compact output ciphertexts on the GPU (include/fbs_exec.h, "compact outputs"): fbs_compact_dev is the oracle's key switch
followed by the rounding and packing of the format, word for word, on every key-switch family; the host and device decodes agree
with each other and with the decryption of the full ciphertexts; fbs_eval_seeded_compact is fbs_compact_dev of fbs_eval_seeded's
outputs (constants included, in chunks too); a Client / Server pair in two processes exchanges compact files; and the phase
noise of compact bootstrap outputs is what params.compact_output_variance says.

The word-for-word comparisons here run on the toy sets of tests/test_gpu_device_io.py (n = 12: one round of k_compact_pack, one
pass of 64 lanes in k_decrypt_compact, a 32-bit sum that never wraps).  Real key sizes (n up to 4096), planted rounding
boundaries and the definitions on Python integers are in tests/test_gpu_compact_wide.py and tests/test_compact_reference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import assert_outputs_equal, load_fixture, subsample
from tests.test_gpu_device_io import SETS, dev, host, keyed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -3
COMPACT_SETS = ("k1_n1024", "k1_n2048", "k2", "k3")
KNOBS = ({}, dict(ks_mfma=0), dict(ks_mfma=0, ks_fp=0))   # the GEMM; then the integer, lanes and FP64 kernels; then lanes only
COUNTS = (1, 64, 65, 1000, 8193)
_SWITCHED = {}


# ---- the format, restated in numpy ---------------------------------------------------------------------------------------
def round_fields(x, bits):
    """section 1: x [count][n+1] canonical residues (mask, body) -> fields [count][n+1] < 2^bits"""
    x = np.asarray(x, np.uint64)
    n = x.shape[1] - 1
    sh = np.uint64(46 - bits)
    m = ((x[:, :n] >> (sh - np.uint64(1))) + np.uint64(1)) >> np.uint64(1)
    eps = (x[:, :n].astype(np.int64) - (m << sh).astype(np.int64)).sum(axis=1)
    body = (x[:, n].astype(object) - (eps >> 1).astype(object)) % orc.Q          # eps >> 1: the floor of eps / 2
    body = np.array(body, dtype=np.uint64)
    mn = ((body >> (sh - np.uint64(1))) + np.uint64(1)) >> np.uint64(1)
    mask = np.uint64((1 << bits) - 1)
    return np.concatenate([m, mn[:, None]], axis=1) & mask


def pack(fields, bits):
    count, n1 = fields.shape
    W = -(-n1 * bits // 64)
    words = np.zeros((count, W), np.uint64)
    for j in range(n1):
        b = j * bits
        w, o = b // 64, b % 64
        f = fields[:, j].astype(np.uint64)
        words[:, w] |= f << np.uint64(o)
        if o + bits > 64:
            words[:, w + 1] |= f >> np.uint64(64 - o)
    return words


def unpack(words, n, bits):
    fields = np.zeros((words.shape[0], n + 1), np.uint64)
    mask = np.uint64((1 << bits) - 1)
    for j in range(n + 1):
        b = j * bits
        w, o = b // 64, b % 64
        v = words[:, w] >> np.uint64(o)
        if o + bits > 64:
            v |= words[:, w + 1] << np.uint64(64 - o)
        fields[:, j] = v & mask
    return fields


def switched(name, count):
    """(ciphertexts, their key switch by the oracle) for a set, made once per module"""
    if (name, count) not in _SWITCHED:
        ctx, o = keyed(name)
        p = ctx.params.p_msg
        cts = ctx.encrypt(np.random.default_rng(count).integers(0, 2 * p, count), nonce0=10 * count)
        _SWITCHED[(name, count)] = (cts, np.stack([o.keyswitch(c) for c in cts]))
    return _SWITCHED[(name, count)]


def compact_on_device(ctx, cts, bits):
    import torch
    cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, ctx.params.ct_words)
    W = ctx.compact_words(bits)
    d_w = torch.full((max(1, cts.shape[0]), W), 0x5A5A, dtype=torch.int64, device="cuda")
    ctx.compact_dev(dev(cts).data_ptr(), cts.shape[0], d_w.data_ptr(), bits=bits)
    ctx.sync()
    return host(d_w)[:cts.shape[0]]


@pytest.mark.parametrize("name", COMPACT_SETS)
def test_compact_dev_matches_the_oracle(name):
    ctx, o = keyed(name)
    w0 = ctx.params.log_n_poly + 1
    cts, x = switched(name, 64)
    # the restatement is anchored in the oracle's modulus switch at the blind rotation's width
    assert np.array_equal(round_fields(x, w0), np.stack([o.modswitch(r) for r in x]).astype(np.uint64))
    try:
        for knobs in KNOBS:
            ctx.tune(**{**dict(ks_mfma=1, ks_fp=1), **knobs})
            for count in COUNTS:
                cts, x = switched(name, count)
                before = ctx.stat("ms_capacity")
                for bits in (w0, w0 + 3, 31):
                    want = pack(round_fields(x, bits), bits)
                    got = compact_on_device(ctx, cts, bits)
                    assert got.shape == (count, ctx.compact_words(bits)) and np.array_equal(got, want), (name, knobs, count, bits)
                assert ctx.stat("ms_capacity") <= max(before, 8192)          # passes, not scratch grown with count
    finally:
        ctx.tune(ks_mfma=1, ks_fp=1)


def _code(call):
    from tfhe_fbs_map_amd import FbsError
    try:
        call()
    except FbsError as e:
        return e.code
    return 0


@pytest.mark.parametrize("name", COMPACT_SETS)
def test_decrypt_compact_host_device_and_full_agree(name):
    import torch
    from tfhe_fbs_map_amd import Context, _native as nat
    ctx, _ = keyed(name)
    p, w0 = ctx.params.p_msg, ctx.params.log_n_poly + 1
    rng = np.random.default_rng(3)
    tables = [[int(v) for v in rng.integers(0, 2 * p, p)] for _ in range(3)]
    msgs = rng.integers(0, p, 600)
    ids = rng.integers(0, 3, 600).astype(np.uint32)
    out = ctx.bootstrap_batch(ctx.tvset(tables), ctx.encrypt(msgs, nonce0=77), ids)
    full = ctx.decrypt(out)
    assert np.array_equal(full, [tables[i][m] for i, m in zip(ids, msgs)])
    for bits in (w0, w0 + 3, 31):
        words = compact_on_device(ctx, out, bits)
        on_host = ctx.decrypt_compact(words, bits, device=False)
        on_dev = ctx.decrypt_compact(words, bits, device=True)
        assert np.array_equal(on_host, full) and np.array_equal(on_dev, full), (name, bits)
    # refusals: out-of-range widths, and an evaluation-only context; nothing written
    lib, h = nat.lib, ctx._h
    words = compact_on_device(ctx, out[:4], w0)
    msgs_out = np.full(4, 9, np.int64)
    d_w = dev(words)
    d_m = torch.full((4,), 55, dtype=torch.int64, device="cuda")
    for bad in (w0 - 1, 32, 0):
        assert _code(lambda: ctx._check(lib.fbs_decrypt_compact(h, words.ctypes.data, 4, bad, msgs_out.ctypes.data))) == E_INVALID
        assert _code(lambda: ctx._check(lib.fbs_decrypt_compact_dev(h, d_w.data_ptr(), 4, bad, d_m.data_ptr(), None))) == E_INVALID
        assert _code(lambda: ctx._check(lib.fbs_compact_dev(h, dev(out[:4]).data_ptr(), 4, bad, d_w.data_ptr(), None))) == E_INVALID
        assert _code(lambda: ctx.compact_words(bad)) == E_INVALID
    client = Context(ctx.params, seed=21, keygen=False)
    client.keygen_seeded()
    server = Context.evaluation_only(ctx.params, **client.export_seeded_keys())
    sh = server._h
    assert _code(lambda: server._check(lib.fbs_decrypt_compact(sh, words.ctypes.data, 4, w0, msgs_out.ctypes.data))) == E_STATE
    assert _code(lambda: server._check(lib.fbs_decrypt_compact_dev(sh, d_w.data_ptr(), 4, w0, d_m.data_ptr(), None))) == E_STATE
    server.sync()
    assert (msgs_out == 9).all() and bool((d_m == 55).all()) and np.array_equal(host(d_w), words)
    # ... while it compacts (no secret needed) what the client then decodes
    c_out = client.bootstrap_batch(client.tvset(tables), client.encrypt(msgs[:50], nonce0=5), ids[:50])
    assert np.array_equal(client.decrypt_compact(compact_on_device(server, c_out, w0 + 1), w0 + 1), client.decrypt(c_out))
    server.close()
    client.close()


def _pair(name):
    from tfhe_fbs_map_amd import Context
    client = Context(SETS[name](), seed=11, keygen=False)
    client.keygen_seeded()
    return client, Context.evaluation_only(client.params, **client.export_seeded_keys())


def _program(ctx, name, fuse=False):
    from tfhe_fbs_map_amd import _native as nat, parse_fbs
    rec = load_fixture(name)
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    tv = ctx.tvset(low["tables"])
    prog = nat.Program(ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"],
                       low["term_coef"], low["term_src"], low["out_wire"], fuse_tables=fuse)
    prog._tv = tv
    return rec, low, prog


@pytest.mark.parametrize("set_name,name,fuse", [("k1_n1024", "adder8__search_p7", False), ("k2", "adder8__search_p7", True),
                                                ("k2", "edge_outputs", True), ("k3", "edge_outputs", False)])
def test_eval_seeded_compact_is_compact_dev_of_eval_seeded(set_name, name, fuse):
    client, server = _pair(set_name)
    rec, low, prog = _program(server, name, fuse)
    T = 9
    ins, expect = subsample(rec, T)
    bits_in = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]]).reshape(len(low["input_names"]), T)
    bodies, nonce0 = client.encrypt_seeded(bits_in, nonce0=33)
    full = prog.eval_seeded(bodies, T, nonce0)
    w0 = server.params.log_n_poly + 1
    for bits in (w0, 31):
        got = prog.eval_seeded_compact(bodies, T, nonce0, bits)
        assert got.shape == (prog.n_outputs, T, server.compact_words(bits))
        want = compact_on_device(server, full.reshape(-1, server.params.ct_words), bits).reshape(got.shape)
        assert np.array_equal(got, want), (name, bits)
        dec = client.decrypt_compact(got, bits)
        for k, out_name in enumerate(low["out_names"]):
            e = expect[out_name]
            assert np.array_equal(dec[k], np.full(T, e) if np.ndim(e) == 0 else np.asarray(e)), (name, out_name, bits)
    if name == "edge_outputs":
        assert any(w < 0 for w in low["out_wire"])
    assert prog.eval_seeded_compact(bodies[:, :0], 0, nonce0).shape == (prog.n_outputs, 0, server.compact_words())
    server.close()
    client.close()


def test_eval_seeded_compact_in_chunks(monkeypatch):
    from tfhe_fbs_map_amd import Context
    client, _ = _pair("k1_n1024")
    T = 37
    rec, low, cprog = _program(client, "adder8__search_p7")
    ins, expect = subsample(rec, T)
    bits_in = np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]])
    bodies, nonce0 = client.encrypt_seeded(bits_in, nonce0=2)
    w0 = client.params.log_n_poly + 1
    want = compact_on_device(client, cprog.eval_seeded(bodies, T, nonce0).reshape(-1, client.params.ct_words), w0 + 2)
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")
    assert 2 * 2**20 * 0.6 / (cprog.n_slots * client.params.ct_words * 8) < T / 3
    server = Context.evaluation_only(client.params, **client.export_seeded_keys())   # fresh: its scratch has not grown
    _, _, prog = _program(server, "adder8__search_p7")
    got = prog.eval_seeded_compact(bodies, T, nonce0, w0 + 2)
    assert np.array_equal(got.reshape(want.shape), want)
    dec = client.decrypt_compact(got, w0 + 2)
    for k, out_name in enumerate(low["out_names"]):
        assert np.array_equal(dec[k], expect[out_name]), out_name
    server.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tfhe_fbs_map_amd import EncryptedInputs, Server, ServerKey, parse_fbs
from tests.helpers import load_fixture
rec = load_fixture(sys.argv[2])
env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
server = Server(ServerKey.load(sys.argv[3]))
assert server.ctx.stat("has_secret") == 0, "the server holds a secret"
inputs = EncryptedInputs.load(sys.argv[4])
server.run(env, inputs).save(sys.argv[5])
server.run_compact(env, inputs).save(sys.argv[6])
print("server done")
"""


@pytest.mark.parametrize("name", ["adder8__search_p7", "edge_outputs"])
def test_client_and_server_exchange_compact_files(name, tmp_path):
    from tfhe_fbs_map_amd import Client, EncryptedOutputs, ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.split import CompactOutputs
    rec = load_fixture(name)
    ins, expect = subsample(rec, 24)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = ExecConfig(seed=3)
    client = Client(env, cfg)
    key_path, in_path, full_path, compact_path = (str(tmp_path / f) for f in ("key.npz", "in.npz", "full.npz", "compact.npz"))
    client.server_key().save(key_path)
    client.encrypt(ins).save(in_path)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, name, key_path, in_path, full_path, compact_path], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "server done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    compact = CompactOutputs.load(compact_path)
    assert compact.bits == client.params.log_n_poly + 1                  # a plain program keeps the blind rotation's width
    got = client.decrypt(compact)
    assert_outputs_equal(got, expect)
    want = env.eval(ins, config=cfg)
    assert got.keys() == want.keys()
    for k in want:
        assert type(got[k]) is type(want[k]) and np.array_equal(got[k], want[k]), k
    assert client.decrypt(EncryptedOutputs.load(full_path)).keys() == got.keys()
    assert os.path.getsize(compact_path) < os.path.getsize(full_path) / 10
    # what the client refuses: another key's outputs, another program's, a width that does not fit its parameters
    other = CompactOutputs(compact.output_names, compact.T, compact.bits, compact.words, bytes(8))
    with pytest.raises(ValueError, match="another server key"):
        client.decrypt(other)
    with pytest.raises(ValueError, match="another program"):
        client.decrypt(CompactOutputs(compact.output_names[::-1], compact.T, compact.bits, compact.words, compact.fingerprint))
    with pytest.raises(ValueError, match="do not fit"):
        client.decrypt(CompactOutputs(compact.output_names, compact.T, compact.bits + 1, compact.words, compact.fingerprint))


@pytest.mark.parametrize("which", ["k2", "k3"])
def test_compact_noise_is_the_model(which):
    """~20 000 bootstrap outputs at the 128-bit k = 2 set (p = 15) and k = 3 set (p = 7), compacted at log2(2N) and at 31 bits: the
    measured phase-error variance lies within 0.5x .. 1.25x of params.compact_output_variance (the bounds of test_gpu_k2's noise
    test)"""
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import DEFAULT_GLWE_DIMS, choose_params, compact_output_variance
    prm = choose_params(15, 70, glwe_dims=(1, 2)) if which == "k2" else choose_params(7, 10, glwe_dims=DEFAULT_GLWE_DIMS)
    assert prm.k == (2 if which == "k2" else 3)
    ctx = Context(prm, seed=13)
    sk = ctx.export_keys()["sk_lwe"].astype(bool)
    p, n = prm.p_msg, prm.n
    rng = np.random.default_rng(5)
    table = [int(v) for v in rng.integers(0, 2 * p, p)]
    B = 20480
    msgs = rng.integers(0, p, B)
    out = ctx.bootstrap_batch(ctx.tvset([table]), ctx.encrypt(msgs, nonce0=900))
    want = np.array([table[m] for m in msgs])
    delta = 2 * ((orc.Q + 2 * p) // (4 * p))                          # 2 round(q / 4p)
    for bits in (prm.log_n_poly + 1, 31):
        words = compact_on_device(ctx, out, bits)
        f = unpack(words, n, bits).astype(np.int64)
        phase = (f[:, n] - (f[:, :n] * sk).sum(axis=1)) % (1 << bits)
        err = phase / float(1 << bits) - want * (delta / orc.Q)
        err = (err + 0.5) % 1.0 - 0.5
        measured, predicted = float(np.mean(err ** 2)), compact_output_variance(prm, bits, 1.0)
        assert 0.5 * predicted < measured < 1.25 * predicted, (which, bits, measured, predicted)
        assert np.array_equal(ctx.decrypt_compact(words, bits), want)
    ctx.close()
