"""Chained evaluation on the GPU (include/fbs_exec.h, "chained evaluation"): fbs_compact_fields_dev is a numpy restatement of the
unpack and re-rounding at every width; fbs_refresh_compact_dev of fbs_compact_dev at log2(2N) is fbs_bootstrap_batch_dev through
the identity table, word for word; fbs_eval_sources with seeded sources is fbs_eval_seeded and fbs_eval_seeded_compact, chunked
too, refuses with codes and does not grow scratch when called again; a 32-hop adder8 accumulator over compact, full and mixed
links decrypts to the cleartext running sum after every hop; two processes hand a chain over through .npz files; and the noise
of refreshed inputs is what params says.

The restatement and the refresh are compared here at n = 12, on random words.  k_compact_unpack at real key sizes (several and
partial passes of 64 lanes, its grid-stride loop), a re-rounding error sum at its extremes and of either parity, and the refresh
at n = 734 are in tests/test_gpu_compact_wide.py; tests/test_compact_reference.py anchors `reround` in its definition."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import load_fixture, subsample
from tests.test_gpu_compact import _pair, _program, compact_on_device, pack, round_fields, switched, unpack
from tests.test_gpu_device_io import dev, host, keyed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
CHAIN_SETS = ("k2", "k3", "k1_n2048")   # k = 2 at N = 1024, k = 3 at N = 512, k = 1 at N = 2048
ADDER = "adder8__search_p15"


def reround(fields, n, bits, b):
    """the unpack's re-rounding from 2^bits to 2^b, restated: fields [count][n+1] < 2^bits -> [count][n+1] < 2^b"""
    f = np.asarray(fields, np.int64)
    if bits == b:
        return f.astype(np.uint64)
    sh = bits - b
    m = ((f[:, :n] >> (sh - 1)) + 1) >> 1
    eps = (f[:, :n] - (m << sh)).sum(axis=1)
    body = (f[:, n] - (eps >> 1)) % (1 << bits)
    mn = ((body >> (sh - 1)) + 1) >> 1
    return (np.concatenate([m, mn[:, None]], axis=1) & ((1 << b) - 1)).astype(np.uint64)


def fields_on_device(ctx, words, bits):
    import torch
    count = words.shape[0]
    d_f = torch.full((max(1, count), ctx.params.n + 1), 0x5A5A, dtype=torch.int32, device="cuda")
    ctx.compact_fields_dev(dev(words).data_ptr(), count, d_f.data_ptr(), bits=bits)
    ctx.sync()
    return host(d_f, np.uint32)[:count].astype(np.uint64)


def refresh_on_device(ctx, words, bits):
    import torch
    d_c = torch.full((max(1, words.shape[0]), ctx.params.ct_words), 0x5A5A, dtype=torch.int64, device="cuda")
    ctx.refresh_compact_dev(dev(words).data_ptr(), words.shape[0], d_c.data_ptr(), bits=bits)
    ctx.sync()
    return host(d_c)[:words.shape[0]]


@pytest.mark.parametrize("name", CHAIN_SETS)
def test_compact_fields_are_the_restatement(name):
    ctx, o = keyed(name)
    n, b = ctx.params.n, ctx.params.log_n_poly + 1
    cts, x = switched(name, 1000)
    for bits in range(b, 32):
        words = compact_on_device(ctx, cts, bits)
        assert np.array_equal(unpack(words, n, bits), round_fields(x, bits)), (name, bits)
        got = fields_on_device(ctx, words, bits)
        assert np.array_equal(got, reround(unpack(words, n, bits), n, bits, b)), (name, bits)
        if bits == b:   # what fbs_compact_dev packed: the fields the blind rotation reads
            assert np.array_equal(got, np.stack([o.modswitch(r) for r in x]).astype(np.uint64))


@pytest.mark.parametrize("name", CHAIN_SETS)
def test_refresh_is_the_identity_bootstrap(name):
    ctx, _ = keyed(name)
    p, b = ctx.params.p_msg, ctx.params.log_n_poly + 1
    identity = ctx.tvset([list(range(p))])
    for count in (1, 63, 256, 1500, 9000):   # below and above the launchers' cuts, and more than one pass of 8192
        msgs = np.random.default_rng(count).integers(0, p, count)
        cts = ctx.encrypt(msgs, nonce0=50_000 + count)
        want = ctx.bootstrap_batch(identity, cts)
        got = refresh_on_device(ctx, compact_on_device(ctx, cts, b), b)
        assert np.array_equal(got, want), (name, count)
        assert np.array_equal(ctx.decrypt(got), msgs)
        wide = refresh_on_device(ctx, compact_on_device(ctx, cts[:300], 31), 31)   # re-rounded: the same values
        assert np.array_equal(ctx.decrypt(wide), msgs[:300])


def _srcs(nat, kinds):
    arr = (nat._InputSrc * len(kinds))()
    for i, k in enumerate(kinds):
        arr[i] = nat._InputSrc(*k)
    return arr


def eval_dev_of_expansion(ctx, prog, bodies, T, nonce0):
    """fbs_eval_dev on what fbs_expand_seeded_dev makes of the bodies: the device entry keeps a load and a store of its own, and
    the expansion is one flat run of streams, so nothing here goes through the code the host-buffer entries share"""
    import torch
    bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1)
    ctw = ctx.params.ct_words
    d_in = torch.full((bodies.size, ctw), 7, dtype=torch.int64, device="cuda")
    ctx.expand_seeded_dev(dev(bodies).data_ptr(), bodies.size, nonce0, d_in.data_ptr())
    d_out = torch.full((prog.n_outputs, T, ctw), 7, dtype=torch.int64, device="cuda")
    prog.eval_dev(d_in.data_ptr(), T, d_out.data_ptr())
    ctx.sync()
    return host(d_out)


def host_entries_are_eval_dev_of_the_expansion(client, ctx, prog, bodies, T, nonce0):
    """fbs_eval_seeded and fbs_eval are eval_sources over sources they build themselves (input i at bodies + i T on stream
    nonce0 + i T, or at cts + i T (D + 1)): word for word what the device entry returns.  Returns those words."""
    want = eval_dev_of_expansion(ctx, prog, bodies, T, nonce0)
    assert np.array_equal(prog.eval_seeded(bodies, T, nonce0), want)
    assert np.array_equal(prog.eval(client.expand_seeded(bodies, nonce0), T), want)
    return want


def test_eval_sources_with_seeded_sources_is_eval_seeded(monkeypatch):
    from tfhe_fbs_map_amd import Context, FbsError, _native as nat
    client, server = _pair("k1_n1024")
    rec, low, prog = _program(server, "adder8__search_p7")
    T = 37
    ins, _ = subsample(rec, T)
    n_in = len(low["input_names"])
    bodies, nonce0 = client.encrypt_seeded(np.stack([np.asarray(ins[k], np.int64) for k in low["input_names"]]), nonce0=5)
    b = server.params.log_n_poly + 1
    seeded = [("seeded", bodies[i], nonce0 + i * T) for i in range(n_in)]
    full = prog.eval_seeded(bodies, T, nonce0)
    assert np.array_equal(host_entries_are_eval_dev_of_the_expansion(client, server, prog, bodies, T, nonce0), full)
    assert np.array_equal(prog.eval_sources(seeded, T), full)
    for bits in (b, b + 2):
        assert np.array_equal(prog.eval_sources(seeded, T, bits), prog.eval_seeded_compact(bodies, T, nonce0, bits))
    # bodies that are not one array: one copy per input, the same runs
    split_bodies = [np.array(bodies[i]) for i in range(n_in)]
    assert np.array_equal(prog.eval_sources([("seeded", split_bodies[i], nonce0 + i * T) for i in range(n_in)], T), full)
    # full links, plain and refreshed (key switch, modulus switch, identity rotation): the same messages
    expanded = client.expand_seeded(bodies, nonce0).reshape(n_in, T, -1)
    want = client.decrypt(full)
    assert np.array_equal(prog.eval_sources([("full", expanded[i], False) for i in range(n_in)], T), full)
    refreshed = prog.eval_sources([("full", expanded[i], i % 2 == 0) for i in range(n_in)], T)
    assert np.array_equal(client.decrypt(refreshed), want)
    # repeated calls of one shape do not grow scratch, with refreshed links too
    words = prog.eval_seeded_compact(bodies, T, nonce0, b)
    mixed = [("compact", words[i % 9], b) if i < 8 else seeded[i] for i in range(n_in)]
    first = prog.eval_sources(mixed, T)
    growths = server.stat("scratch_growths")
    for _ in range(3):
        assert np.array_equal(prog.eval_sources(mixed, T), first)
        prog.eval_sources(seeded, T, b)
    assert server.stat("scratch_growths") == growths
    # chunked: a wire budget far below T samples
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")
    assert 2 * 2**20 * 0.6 / (prog.n_slots * server.params.ct_words * 8) < T / 3
    fresh = Context.evaluation_only(client.params, **client.export_seeded_keys())
    _, _, cprog = _program(fresh, "adder8__search_p7")
    assert np.array_equal(cprog.eval_sources(seeded, T), full)
    assert np.array_equal(host_entries_are_eval_dev_of_the_expansion(client, fresh, cprog, bodies, T, nonce0), full)   # ragged chunks
    assert np.array_equal(cprog.eval_sources(seeded, T, b + 2), prog.eval_seeded_compact(bodies, T, nonce0, b + 2))
    assert np.array_equal(cprog.eval_sources(mixed, T), first)
    monkeypatch.delenv("FBS_WIRE_BUDGET_MB")
    # constant outputs and outputs that are inputs: the trivial-ciphertext store, two inputs' stream offsets
    erec, elow, eprog = _program(server, "edge_outputs")
    e_ins, e_expect = subsample(erec, 3)
    e_bodies, e_nonce0 = client.encrypt_seeded(np.stack([np.asarray(e_ins[k], np.int64) for k in elow["input_names"]]), nonce0=900)
    e_out = host_entries_are_eval_dev_of_the_expansion(client, server, eprog, e_bodies, 3, e_nonce0)
    for k, name in enumerate(elow["out_names"]):
        e = e_expect[name]
        assert np.array_equal(client.decrypt(e_out[k]), np.full(3, e) if np.ndim(e) == 0 else np.asarray(e)), name
    assert any(w < 0 for w in elow["out_wire"])
    # refusals: a code, and nothing written
    lib, h = nat.lib, server._h
    ctw = server.params.ct_words
    out = np.full((prog.n_outputs, T, ctw), 7, np.uint64)
    good = [(0, 0, 0, nonce0 + i * T, bodies[i].ctypes.data) for i in range(n_in)]

    def code(kinds, T_=T, out_bits=0):
        try:
            server._check(lib.fbs_eval_sources(h, prog._h, C.byref(_srcs(nat, kinds)), T_, out_bits, out.ctypes.data))
        except FbsError as e:
            return e.code
        return 0
    assert code([(5, 0, 0, 0, bodies[0].ctypes.data)] + good[1:]) == E_INVALID                  # unknown kind
    assert code(good[:3] + [(0, 0, 0, nonce0, None)] + good[4:]) == E_INVALID                   # null data
    for bad in (b - 1, 32, 0):
        assert code([(2, bad, 1, 0, words[0].ctypes.data)] + good[1:]) == E_INVALID              # compact width
    assert code(good, out_bits=b - 1) == E_INVALID                                               # output width
    assert code([(0, 0, 0, (1 << 56) - 3, bodies[0].ctypes.data)] + good[1:]) == E_INVALID       # streams past 2^56
    assert code([(1, 0, 0, 0, bodies[0].ctypes.data)] + good[1:], T_=(2**64 - 1) // 8 // ctw + 1) == E_INVALID   # T * words
    assert (out == 7).all()
    fresh.close()
    server.close()
    client.close()


def _adder_setup(T, seed=7):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture(ADDER)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=seed), programs=[env])
    server = Server(client.server_key())
    return rec, env, client, server


def _hop_inputs(rng, T):
    return {f"b{i}": rng.integers(0, 2, T) for i in range(8)}


A_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}


@pytest.mark.parametrize("mode", ["compact", "full", "mixed"])
def test_adder8_accumulator_32_hops(mode):
    """acc <- acc + b over 32 hops with the state kept on the server; the client decrypts after every hop"""
    T = 16
    rec, env, client, server = _adder_setup(T)
    rng = np.random.default_rng(1)
    b_names = [f"b{i}" for i in range(8)]
    first = {**{f"a{i}": rng.integers(0, 2, T) for i in range(8)}, **_hop_inputs(rng, T)}
    acc = server.run_compact(env, client.encrypt(first)) if mode == "compact" else server.run(env, client.encrypt(first))
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    for hop in range(32):
        got = client.decrypt(acc)
        for k in clear:
            assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (mode, hop, k)
        fresh = _hop_inputs(rng, T)
        compact = mode == "compact" or (mode == "mixed" and hop % 2 == 0)
        acc = server.run_chain(env, [acc, client.encrypt(fresh, names=b_names)], rename=A_FROM_S, compact=compact)
        assert acc.out_norm2 is not None and acc.T == T
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T,)) for i in range(8)}, **fresh})
    got = client.decrypt(acc)
    for k in clear:
        assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (mode, k)


def test_run_chain_refuses():
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedOutputs
    T = 4
    rec, env, client, server = _adder_setup(T, seed=9)
    rng = np.random.default_rng(2)
    ins = {**{f"a{i}": rng.integers(0, 2, T) for i in range(8)}, **_hop_inputs(rng, T)}
    acc = server.run_compact(env, client.encrypt(ins))
    b_in = client.encrypt(_hop_inputs(rng, T), names=[f"b{i}" for i in range(8)])
    with pytest.raises(ValueError, match="no source"):
        server.run_chain(env, [acc, b_in])
    with pytest.raises(ValueError, match="ambiguous"):
        server.run_chain(env, [acc, b_in, acc], rename=A_FROM_S)
    with pytest.raises(ValueError, match="another server key"):
        server.run_chain(env, [CompactOutputs(acc.output_names, T, acc.bits, acc.words, bytes(8), acc.out_norm2), b_in], rename=A_FROM_S)
    with pytest.raises(ValueError, match="saved without out_norm2"):
        server.run_chain(env, [CompactOutputs(acc.output_names, T, acc.bits, acc.words, acc.fingerprint), b_in], rename=A_FROM_S)
    full = server.run(env, client.encrypt(ins))
    noisy = EncryptedOutputs(full.output_names, T, full.cts, full.fingerprint, np.full(9, 1e4))
    with pytest.raises(ValueError, match="refresh would keep"):
        server.run_chain(env, [noisy, b_in], rename=A_FROM_S)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tfhe_fbs_map_amd import EncryptedInputs, Server, ServerKey, parse_fbs
from tfhe_fbs_map_amd.split import CompactOutputs
from tests.helpers import load_fixture
rec = load_fixture(sys.argv[2])
env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
server = Server(ServerKey.load(sys.argv[3]))
assert server.ctx.stat("has_secret") == 0, "the server holds a secret"
if sys.argv[4] == "A":
    server.run_compact(env, EncryptedInputs.load(sys.argv[5])).save(sys.argv[6])
else:
    a_from_s = {"a%d" % i: "s%d" % i for i in range(8)}
    server.run_chain(env, [CompactOutputs.load(sys.argv[5]), EncryptedInputs.load(sys.argv[6])], rename=a_from_s,
                     compact=True).save(sys.argv[7])
print("server done")
"""


def test_two_servers_hand_a_chain_over_through_files(tmp_path):
    from tfhe_fbs_map_amd import Client, ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.split import CompactOutputs
    T = 24
    rec = load_fixture(ADDER)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=4), programs=[env])
    rng = np.random.default_rng(3)
    first = {**{f"a{i}": rng.integers(0, 2, T) for i in range(8)}, **_hop_inputs(rng, T)}
    second = _hop_inputs(rng, T)
    key, in1, mid, in2, out = (str(tmp_path / f) for f in ("key.npz", "in1.npz", "mid.npz", "in2.npz", "out.npz"))
    client.server_key().save(key)
    client.encrypt(first).save(in1)
    client.encrypt(second, names=[f"b{i}" for i in range(8)]).save(in2)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    for args in (["A", in1, mid], ["B", mid, in2, out]):
        r = subprocess.run([sys.executable, str(script), ROOT, ADDER, key] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "server done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert CompactOutputs.load(mid).out_norm2 is not None
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T,)) for i in range(8)}, **second})
    got = client.decrypt(CompactOutputs.load(out))
    for k in clear:
        assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), k


def test_refreshed_input_noise_is_the_model():
    """12 288 compact links at the 128-bit k = 2 set (p = 15), at log2(2N) and 4 bits wider: the phase the refresh reads (the
    unpacked fields under the small key, modulo 2N) against params.refresh_input_variance, and the refreshed ciphertexts' phase
    under the GLWE key against one blind rotation's variance; both within 0.5x .. 1.25x"""
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import DEFAULT_GLWE_DIMS, choose_params, refresh_input_variance, variances
    prm = choose_params(15, 70, glwe_dims=DEFAULT_GLWE_DIMS)
    ctx = Context(prm, seed=17)
    keys = ctx.export_keys()
    s_lwe, s_glwe = keys["sk_lwe"].astype(np.int64), keys["sk_glwe"].astype(np.int64)
    p, n, b = prm.p_msg, prm.n, prm.log_n_poly + 1
    rng = np.random.default_rng(8)
    B = 12288
    msgs = rng.integers(0, p, B)
    outs = ctx.bootstrap_batch(ctx.tvset([list(range(p))]), ctx.encrypt(msgs, nonce0=700))   # bootstrap outputs: out_norm2 = 1
    delta = 2 * ((orc.Q + 2 * p) // (4 * p))
    for bits in (b, b + 4):
        words = compact_on_device(ctx, outs, bits)
        f = fields_on_device(ctx, words, bits).astype(np.int64)
        phase = (f[:, n] - (f[:, :n] * s_lwe).sum(axis=1)) % (1 << b)
        err = phase / float(1 << b) - msgs * (delta / orc.Q)
        err = (err + 0.5) % 1.0 - 0.5
        measured, predicted = float(np.mean(err ** 2)), refresh_input_variance(prm, bits, 1.0)
        assert 0.5 * predicted < measured < 1.25 * predicted, ("read", bits, measured, predicted)
        fresh = refresh_on_device(ctx, words, bits).astype(np.int64)
        D = prm.k * prm.N
        ph = (fresh[:, D] - (fresh[:, :D] * s_glwe).sum(axis=1)) % orc.Q
        err = ph / float(orc.Q) - msgs * (delta / orc.Q)
        err = (err + 0.5) % 1.0 - 0.5
        measured, predicted = float(np.mean(err ** 2)), variances(prm)[0]
        assert 0.5 * predicted < measured < 1.25 * predicted, ("refreshed", bits, measured, predicted)
        assert np.array_equal(ctx.decrypt(fresh.astype(np.uint64)), msgs)
    ctx.close()
