"""Public-key inputs on the GPU (include/fbs_exec.h, "public-key inputs"): k_expand_public is, word for word, the host expansion
fbs_pub_expand -- on real encryptions and on planted samples, at destinations of either alignment; fbs_state_put_public fills
exactly the rows it is given, refuses a non-canonical word with the state untouched and does not grow scratch twice; and through
`split`: a third party's public-key inputs beside seeded and plain ones give the golden outputs, in every output form."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import load_fixture, subsample
from tests.test_client_lib import SETS, toy_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = (1 << 46) - 62 * (1 << 13) + 1
E_INVALID = -1
GUARD = 0x5A5A5A5A5A5A5A5A
_MADE = {}


@pytest.fixture(scope="module", autouse=True)
def public_library():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc"), "client", "public"], timeout=900)


def made(name):
    """(parameter set, a GPU context with no key at all, an encryptor under a public key of a host context) once per module"""
    if name not in _MADE:
        from tfhe_fbs_map_amd import Context, HostContext, _public_native as pub
        prm = toy_sets()[name]
        holder = HostContext(prm, seed=21)
        holder.keygen_seeded()
        mask_key = holder.export_seeded_keys()["mask_key"]
        bodies = pub.keygen(prm, mask_key, holder.export_keys()["sk_glwe"], bytes(range(32)))
        ctx = Context(prm, seed=1, keygen=False)
        assert ctx.stat("has_secret") == 0 and ctx.params.ct_words % 2 == 1
        _MADE[name] = (prm, ctx, pub.Encryptor(prm, mask_key, bodies, bytes(32)), holder)
    return _MADE[name]


def planted(prm, kind, rng):
    """one sample [k+1][N] of the edge words: what the negation of zero, the wrap at i = t and i = t + 1, t = 0 and t = N - 1 meet"""
    shape = (prm.k + 1, prm.N)
    if kind == "zeros":
        return np.zeros(shape, np.uint64)
    if kind == "edge":                       # A'_c[0] = 0 and everything else q - 1
        s = np.full(shape, Q - 1, np.uint64)
        s[:prm.k, 0] = 0
        return s
    if kind == "three":
        return rng.choice(np.array([0, 1, Q - 1], np.uint64), shape)
    return rng.integers(0, Q, shape, dtype=np.uint64)


KINDS = ("zeros", "edge", "three", "random")


def expand_on_device(ctx, glwe, count, dst_off=0, src_off=0):
    """fbs_pub_expand_dev into a guarded buffer whose first ciphertext starts dst_off words after a 16-byte line, from samples that
    start src_off words after one"""
    import torch
    ctw = ctx.params.ct_words
    dev = torch.device("cuda", ctx.device)
    flat = np.ascontiguousarray(glwe, np.uint64).reshape(-1)
    d_g = torch.zeros(flat.size + 2, dtype=torch.int64, device=dev)
    d_g[src_off:src_off + flat.size] = torch.from_numpy(flat.view(np.int64)).to(dev)
    d_c = torch.full((count * ctw + 8,), GUARD, dtype=torch.int64, device=dev)
    assert d_g.data_ptr() % 16 == 0 and d_c.data_ptr() % 16 == 0
    lead = 2 + dst_off
    ctx.pub_expand_dev(d_g.data_ptr() + 8 * src_off, count, d_c.data_ptr() + 8 * lead, None)
    ctx.sync()
    out = d_c.cpu().numpy().view(np.uint64)
    assert (out[:lead] == GUARD).all() and (out[lead + count * ctw:] == GUARD).all()          # nothing before or after the batch
    return out[lead:lead + count * ctw].reshape(count, ctw)


@pytest.mark.parametrize("name", SETS)
def test_device_expansion_is_the_host_expansion_word_for_word(name):
    from tfhe_fbs_map_amd import _public_native as pub
    prm, ctx, enc, _ = made(name)
    N = prm.N
    rng = np.random.default_rng(3)
    for count in (1, N - 1, N, N + 1, 2 * N + 3):
        G = -(-count // N)
        real, _ = enc.encrypt(rng.integers(0, 2 * prm.p_msg, count))
        batches = [real] + [np.stack([planted(prm, KINDS[(r + g) % 4], rng) for g in range(G)]) for r in range(4)]
        for b, glwe in enumerate(batches):
            want = pub.expand(prm, glwe, count)
            for dst_off, src_off in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if b < 2 else ()):
                got = expand_on_device(ctx, glwe, count, dst_off, src_off)
                assert np.array_equal(got, want), (name, count, b, dst_off, src_off)
        # the planted properties themselves, on the device's words: a zero stays zero, the edge sample wraps where the header says
        zeros = expand_on_device(ctx, batches[1][:1], min(count, N))
        assert not zeros.any()
        edge = expand_on_device(ctx, batches[2][:1], min(count, N))
        for t in {0, min(count, N) - 1}:
            row = edge[t, :N]
            want = np.where(np.arange(N) == t, 0, np.where(np.arange(N) < t, Q - 1, 1)).astype(np.uint64)
            assert np.array_equal(row, want) and edge[t, -1] == Q - 1, (name, count, t)
    assert np.array_equal(ctx.pub_expand(real, count), pub.expand(prm, real, count))          # the convenience form
    ctx.pub_expand_dev(None, 0, None, None)                                                    # count = 0 does nothing


@pytest.mark.parametrize("T_of", [lambda N: N // 2 + 1, lambda N: 1, lambda N: 2 * N], ids=["T=N/2+1", "T=1", "T=2N"])
@pytest.mark.parametrize("name", SETS)
def test_put_public_fills_its_rows_and_no_others(name, T_of):
    from tfhe_fbs_map_amd import _public_native as pub
    prm, ctx, enc, holder = made(name)
    T = T_of(prm.N)
    rng = np.random.default_rng(T)
    before = rng.integers(0, Q, (5, T, prm.ct_words), dtype=np.uint64)
    msgs = rng.integers(0, 2 * prm.p_msg, (3, T))
    glwe, _ = enc.encrypt(msgs)
    want = pub.expand(prm, glwe, 3 * T).reshape(3, T, prm.ct_words)
    with ctx.state(5, T) as state:
        state.put(before)
        assert state.put_public(glwe, row0=1, rows=3) is state
        got = state.fetch()
        assert np.array_equal(got[1:4], want), (name, T)
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[4], before[4])
        assert np.array_equal(holder.decrypt(got[1:4]), msgs)
        # a row on its own, and the last row: the flattening starts at the row it is given
        one, _ = enc.encrypt(msgs[2])
        state.put_public(one, row0=4, rows=1)
        assert np.array_equal(state.fetch(row0=4, rows=1)[0], pub.expand(prm, one, T))
        assert np.array_equal(state.fetch(row0=0, rows=4), got[:4])


def test_put_public_refuses_a_non_canonical_word_and_leaves_the_state():
    from tfhe_fbs_map_amd import FbsError, _native as nat
    prm, ctx, enc, _ = made("k2_N256_g2")
    T = prm.N // 2 + 1
    rng = np.random.default_rng(8)
    before = rng.integers(0, Q, (5, T, prm.ct_words), dtype=np.uint64)
    glwe, _ = enc.encrypt(rng.integers(0, 2 * prm.p_msg, 3 * T))
    with ctx.state(5, T) as state:
        state.put(before)
        for index in (0, glwe.size - 1):
            for value in (Q, (1 << 64) - 1):
                bad = glwe.copy().reshape(-1)
                bad[index] = value
                with pytest.raises(FbsError) as e:
                    state.put_public(bad, row0=1, rows=3)
                assert e.value.code == E_INVALID and "sample word %d is not a canonical residue" % index in str(e.value)
        lib = nat.lib
        assert lib.fbs_state_put_public(ctx._h, state._h, 1, 3, None) == E_INVALID
        assert lib.fbs_state_put_public(ctx._h, state._h, 3, 3, glwe.ctypes.data) == E_INVALID and "rows past the end" in lib.fbs_last_error(ctx._h).decode()
        assert lib.fbs_state_put_public(ctx._h, None, 1, 3, glwe.ctypes.data) == E_INVALID
        assert lib.fbs_state_put_public(ctx._h, state._h, 1, 0, None) == 0                        # rows = 0 does nothing
        assert np.array_equal(state.fetch(), before)
        state.put_public(glwe, row0=1, rows=3)                                                    # and the context goes on
        assert not np.array_equal(state.fetch(row0=1, rows=3), before[1:4])


def test_put_public_does_not_grow_scratch_twice():
    prm, ctx, enc, _ = made("k1_N1024")
    T = 700
    glwe, _ = enc.encrypt(np.random.default_rng(4).integers(0, 2 * prm.p_msg, 3 * T))
    with ctx.state(3, T) as state:
        state.put_public(glwe)
        first = state.fetch()
        growths = ctx.stat("scratch_growths")
        state.put_public(glwe)
        state.put_public(glwe[:1], row0=2, rows=1)                                                # a smaller call of another shape
        assert ctx.stat("scratch_growths") == growths
        assert np.array_equal(state.fetch(row0=0, rows=2), first[:2])


# ---- three parties, end to end ---------------------------------------------------------------------------------------------------------
def test_three_parties_on_the_adder(tmp_path):
    from tfhe_fbs_map_amd import Client, ExecConfig, FbsError, PlainInputs, PublicEncryptor, PublicInputs, PublicKey, Server, parse_fbs
    from tfhe_fbs_map_amd.params import margin_sigmas, public_input_factor
    from tfhe_fbs_map_amd.split import output_noise_factors
    rec = load_fixture("adder8__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    T = 16
    ins, expect = subsample(rec, T)
    prm = toy_sets()["k3_N256_g2"]
    assert margin_sigmas(prm, env.stats()["norm2_linprod"]) > 12                                   # a toy set with margin to spare
    a_names, b_names = [f"a{i}" for i in range(8)], [f"b{i}" for i in range(7)]
    client = Client(env, ExecConfig(seed=3, fbs_size=7, params=prm), programs=[env])
    assert client.params == prm
    server = Server(client.server_key())
    assert server.ctx.stat("has_secret") == 0
    # the key holder publishes, the data owner encrypts on the host library alone, the server never sees a secret
    client.public_key().save(str(tmp_path / "public_key.npz"))
    sensor = PublicEncryptor(PublicKey.load(str(tmp_path / "public_key.npz")))
    sensor.encrypt(ins, a_names).save(str(tmp_path / "reading.npz"))
    reading = PublicInputs.load(str(tmp_path / "reading.npz"))
    seeded = client.encrypt(ins, names=b_names)
    plain = PlainInputs(["b7"], T, {"b7": np.asarray(ins["b7"])})
    low, factor = env.lower(), public_input_factor(prm)
    names = low["input_names"]

    def norm2_with(a_noise):
        return np.asarray(output_noise_factors(low, prm.p_msg, client.fuse_tables, [a_noise if n in a_names else 0.0 for n in names]))

    def check(out, a_noise, what):
        assert np.array_equal(out.out_norm2, norm2_with(a_noise)), what
        got = client.decrypt(out)
        for name, v in expect.items():
            assert np.array_equal(np.broadcast_to(got[name], (T,)), np.broadcast_to(v, (T,))), (what, name)

    check(server.run_chain(env, [reading, seeded, plain]), factor, "full")
    check(server.run_chain(env, [plain, seeded, reading], compact=True), factor, "compact")
    check(server.run(env, seeded, plain=plain, public=reading), factor, "run")
    with server.run_chain(env, [reading, seeded, plain], resident=True) as res:
        assert server.ctx.stat("states_alive") == 1                                               # the outputs'; the inputs' is gone
        check(res.fetch(compact=True), factor, "resident, compact")
        check(res.fetch(), factor, "resident")
    check(server.run_chain(env, [reading, seeded, plain], refresh_public=True), 1.0, "refreshed")
    with server.run_chain(env, [reading, seeded, plain], resident=True, refresh_public=True) as res:
        check(res.fetch(compact=True), 1.0, "refreshed, resident, compact")
    assert server.ctx.stat("states_alive") == 0

    # the temporary state is freed when the evaluation raises, and the server goes on
    broken = PublicInputs(a_names, T, reading.samples.copy(), reading.fingerprint)
    broken.samples[-1, -1, -1] = Q
    with pytest.raises(FbsError, match="not a canonical residue"):
        server.run_chain(env, [broken, seeded, plain])
    assert server.ctx.stat("states_alive") == 0
    with pytest.raises(ValueError, match="another server key"):
        server.run_chain(env, [PublicInputs(a_names, T, reading.samples, bytes(8)), seeded, plain])
    check(server.run_chain(env, [reading, seeded, plain]), factor, "after a refused source")
    assert server.ctx.stat("states_alive") == 0 and server.ctx.stat("has_secret") == 0
    server.ctx.close()
    client.ctx.close()
