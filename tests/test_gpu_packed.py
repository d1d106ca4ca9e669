"""Packed outputs on the GPU (include/fbs_exec.h, "packed outputs"): fbs_pack_dev is, word for word, the definition restated in
numpy (tests/helpers.py) on the oracle's schoolbook products, whatever the number of slices; the rows of the packing key decrypt
to s_i h_v within the sampler's bound; an evaluation-only context with the imported bodies packs the same words; fbs_decrypt_packed recovers bootstrap
outputs at every width and fbs_state_fetch_packed is fbs_pack_dev of the full fetch; a Client / Server pair runs a golden program
end to end; the phase noise is what params.packed_output_variance says; and what is refused is refused with nothing written."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import assert_outputs_equal, decode_phases, load_fixture, reference_pack, subsample
from tests.test_gpu_compact import compact_on_device, unpack
from tests.test_gpu_device_io import dev, host

pytestmark = pytest.mark.gpu

Q = orc.Q
E_INVALID, E_STATE = -1, -3
PACK_SETS = {"k1_n256": (1, 8, 24), "k2_n256": (2, 8, 24), "k3_n512": (3, 9, 24), "k1_n1024": (1, 10, 16)}
PACK_KEYS = ((1, 8), (2, 7), (3, 10))
_CTX = {}


def toy(k, log_n, n, p=3):
    from tfhe_fbs_map_amd import Params
    if k == 1:
        return Params(n=n, log_n_poly=log_n, k=1, l_bsk=2, beta_bsk=10, t_ksk=8, gamma_ksk=2, p_msg=p, sigma_lwe=1 << 8, sigma_glwe=4)
    return Params(n=n, log_n_poly=log_n, k=k, l_bsk=1, beta_bsk=21 if k == 2 else 18, t_ksk=8, gamma_ksk=2, p_msg=p,
                  sigma_lwe=1 << 8, sigma_glwe=4, bsk_group=2)


def client_ctx(name):
    """a context keyed with fbs_keygen_seeded for a toy set, made once per module"""
    if name not in _CTX:
        from tfhe_fbs_map_amd import Context
        ctx = Context(toy(*PACK_SETS[name]), seed=17, keygen=False)
        ctx.keygen_seeded()
        _CTX[name] = ctx
    return _CTX[name]


def planted_cts(prm, count, seed):
    """random canonical words with 0 and q - 1 planted in masks and bodies (they need not be valid encryptions)"""
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, Q, (count, prm.ct_words), dtype=np.uint64)
    cts[0, :3] = (0, Q - 1, 0)
    cts[0, -1] = Q - 1
    cts[min(1, count - 1), -1] = 0
    cts[count - 1, -2] = Q - 1
    return cts


# ---- 1. word for word ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_p,gamma_p", PACK_KEYS)
@pytest.mark.parametrize("name", list(PACK_SETS))
def test_pack_dev_is_the_definition_word_for_word(name, t_p, gamma_p):
    ctx = client_ctx(name)
    prm = ctx.params
    N, n = prm.N, prm.n
    ctx.packing_keygen(t_p, gamma_p)
    assert (ctx.stat("packing_key"), ctx.stat("packing_levels"), ctx.stat("packing_base_bits")) == (1, t_p, gamma_p)
    key = ctx.export_packing_key(full=True)["full"]
    cts = planted_cts(prm, 2 * N + 3, seed=N + t_p)
    fields = unpack(compact_on_device(ctx, cts, 31), n, 31)
    try:
        for count in (1, N - 1, N, N + 1, 2 * N + 3):
            for bits in (prm.log_n_poly + 1, 17, 31):
                want = reference_pack(fields[:count], key, t_p, gamma_p, bits, name)
                assert want.size == ctx.packed_words(count, bits)
                got = ctx.pack(cts[:count], bits)
                assert np.array_equal(got, want), (name, t_p, gamma_p, count, bits)
            want = reference_pack(fields[:count], key, t_p, gamma_p, 17, name)
            for slices in (1, 2, 5):
                ctx.tune(pack_slices=slices)
                assert np.array_equal(ctx.pack(cts[:count], 17), want), (name, t_p, gamma_p, count, slices)
            ctx.tune(pack_slices=0)
    finally:
        ctx.tune(pack_slices=0)


# ---- 2. key rows -----------------------------------------------------------------------------------------------------------------
def test_packing_key_rows_decrypt_and_leave_the_other_keys_alone():
    from tfhe_fbs_map_amd import Context
    prm = toy(2, 8, 24)
    ctx = Context(prm, seed=23, keygen=False)
    ctx.keygen_seeded()
    before = ctx.export_keys()
    seeded_before = ctx.export_seeded_keys()
    t_p, gamma_p = 3, 10
    ctx.packing_keygen(t_p, gamma_p)
    after = ctx.export_keys()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    for name, v in ctx.export_seeded_keys().items():
        assert bytes(v) == bytes(seeded_before[name]) if name == "mask_key" else np.array_equal(v, seeded_before[name]), name
    exported = ctx.export_packing_key(full=True)
    key = exported["full"]
    assert np.array_equal(key[:, :, prm.k].reshape(-1), exported["packing_bodies"]) and int(key.max()) < Q
    S = before["sk_glwe"].reshape(prm.k, prm.N)
    worst = 0
    for i in range(prm.n):
        for v in range(t_p):
            phase = key[i, v, prm.k].copy()
            for c in range(prm.k):
                phase = (phase + np.uint64(Q) - orc.polymul_schoolbook(key[i, v, c], S[c])) % np.uint64(Q)
            h = (Q + (1 << (gamma_p * (v + 1) - 1))) >> (gamma_p * (v + 1))            # round(q / 2^(gamma (v+1)))
            phase[0] = (int(phase[0]) - int(before["sk_lwe"][i]) * h) % Q
            centred = np.where(phase > Q // 2, phase.astype(np.int64) - Q, phase.astype(np.int64))
            worst = max(worst, int(np.abs(centred).max()))
    assert 0 < worst <= 6 * prm.sigma_glwe, worst
    ctx.close()


# ---- 3. server equals client -----------------------------------------------------------------------------------------------------
def test_an_evaluation_only_context_packs_the_same_words():
    from tfhe_fbs_map_amd import Context
    client = client_ctx("k2_n256")
    prm = client.params
    client.packing_keygen(2, 7)
    exported = client.export_packing_key()
    server = Context.evaluation_only(prm, **client.export_seeded_keys())
    assert server.stat("packing_key") == 0
    server.import_packing_key(2, 7, exported["packing_bodies"])
    assert (server.stat("packing_key"), server.stat("has_secret")) == (1, 0)
    cts = planted_cts(prm, prm.N + 9, seed=4)
    for bits in (prm.log_n_poly + 1, 20):
        assert np.array_equal(server.pack(cts, bits), client.pack(cts, bits)), bits
    server.close()


# ---- 4. decode -------------------------------------------------------------------------------------------------------------------
def test_decrypt_packed_and_the_packed_fetch_of_a_state():
    ctx = client_ctx("k2_n256")
    prm = ctx.params
    p, N = prm.p_msg, prm.N
    ctx.packing_keygen(3, 10)
    rows, T = 3, 87                                              # 261 = N + 5 outputs
    rng = np.random.default_rng(8)
    table = [int(v) for v in rng.permutation(p)]
    msgs = np.arange(rows * T) % p
    out = ctx.bootstrap_batch(ctx.tvset([table]), ctx.encrypt(msgs, nonce0=400))
    want = np.array([table[m] for m in msgs])
    assert set(want) == set(range(p)) and np.array_equal(ctx.decrypt(out), want)
    with ctx.state(rows, T) as st:
        st.put(out.reshape(rows, T, prm.ct_words))
        for bits in (prm.log_n_poly + 1, 17, 31):
            words = ctx.pack(out, bits)
            assert np.array_equal(ctx.decrypt_packed(words, rows * T, bits), want), bits
            assert np.array_equal(st.fetch_packed(bits), ctx.pack(st.fetch().reshape(-1, prm.ct_words), bits)), bits
        assert np.array_equal(st.fetch_packed(17, row0=1, rows=2), ctx.pack(out[T:], 17))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def test_client_and_server_end_to_end_with_packed_outputs(tmp_path):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, ServerKey, parse_fbs
    from tfhe_fbs_map_amd.split import PackedOutputs, packed_words
    rec = load_fixture("adder8__search_p15")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=5), packing=True)
    prm = client.params
    n_out = len(env.lower()["out_names"])
    T = prm.N // n_out + 7                                       # n_outputs * T: one full sample and a partial one
    assert prm.N < n_out * T < 2 * prm.N
    ins, expect = subsample(rec, T)
    key_path, out_path = str(tmp_path / "key.npz"), str(tmp_path / "packed.npz")
    client.server_key().save(key_path)
    key = ServerKey.load(key_path)
    assert (key.packing_levels, key.packing_base_bits) == tuple(client.packing[:2])
    assert np.array_equal(key.packing_bodies, client.server_key().packing_bodies)
    server = Server(key)
    assert server.ctx.stat("has_secret") == 0 and server.ctx.stat("packing_key") == 1
    inputs = client.encrypt(ins, nonce0=50)
    server.run_packed(env, inputs).save(out_path)
    packed = PackedOutputs.load(out_path)
    assert packed.bits == server.packed_bits(env) and packed.T == T
    assert len(packed.words) * 8 == packed_words(prm, n_out * T, packed.bits) * 8
    assert packed.words.size == (prm.k + 1) * prm.N * packed.bits // 64 + prm.k * prm.N * packed.bits // 64 + -(-(n_out * T - prm.N) * packed.bits // 64)
    got = client.decrypt(packed)
    assert_outputs_equal(got, expect)
    full = client.decrypt(server.run(env, inputs))
    assert got.keys() == full.keys()
    for name in full:
        assert type(got[name]) is type(full[name]) and np.array_equal(got[name], full[name]), name
    with server.run(env, inputs, resident=True) as res:
        again = res.fetch(packed=True)
        assert again.bits == packed.bits and np.array_equal(again.words, packed.words)
    with pytest.raises(ValueError, match="PackedOutputs"):
        server.run_chain(env, [packed])


# ---- 6. noise --------------------------------------------------------------------------------------------------------------------
def test_packed_noise_is_the_model():
    """20 480 bootstrap outputs at the 128-bit k = 2, N = 1024 set (p = 15), packed at packing_choice's parameters: the measured
    phase-error variance against params.packed_output_variance, inside the band the compact test uses (0.5x .. 1.25x).
    Measured on an MI355X: see DESIGN.md section 4 "Packed outputs"."""
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, packed_output_variance, packing_choice
    prm = choose_params(15, 70, glwe_dims=(1, 2))
    assert (prm.k, prm.N) == (2, 1024)
    t_p, gamma_p, bits = packing_choice(prm, 70, 1.0)
    ctx = Context(prm, seed=13, keygen=False)
    ctx.keygen_seeded()
    ctx.packing_keygen(t_p, gamma_p)
    sk_glwe = ctx.export_keys()["sk_glwe"]
    p = prm.p_msg
    rng = np.random.default_rng(5)
    table = [int(v) for v in rng.integers(0, 2 * p, p)]
    B = 20480
    msgs = rng.integers(0, p, B)
    out = ctx.bootstrap_batch(ctx.tvset([table]), ctx.encrypt(msgs, nonce0=900))
    want = np.array([table[m] for m in msgs])
    delta = 2 * ((Q + 2 * p) // (4 * p))
    words = ctx.pack(out, bits)
    phase = decode_phases(words, prm, B, bits, sk_glwe)
    err = phase / float(1 << bits) - want * (delta / Q)
    err = (err + 0.5) % 1.0 - 0.5
    measured, predicted = float(np.mean(err ** 2)), packed_output_variance(prm, t_p, gamma_p, bits, 1.0)
    print("packed noise: (t_p, gamma_p, bits) = %s measured %.4e predicted %.4e ratio %.3f" % ((t_p, gamma_p, bits), measured, predicted,
                                                                                             measured / predicted))
    assert np.array_equal(ctx.decrypt_packed(words, B, bits), want)
    assert 0.5 * predicted < measured < 1.25 * predicted, (t_p, gamma_p, bits, measured, predicted)
    ctx.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def _code(call):
    from tfhe_fbs_map_amd import FbsError
    try:
        call()
    except FbsError as e:
        return e.code
    return 0


def test_refusals_write_nothing_and_leave_the_context_usable():
    import torch
    from tfhe_fbs_map_amd import Context, _native as nat
    lib = nat.lib
    prm = toy(2, 8, 24)
    N, w0 = prm.N, prm.log_n_poly + 1
    cts = planted_cts(prm, N + 2, seed=1)
    d_c = dev(cts)
    d_w = torch.full((4096,), 0x5A5A, dtype=torch.int64, device="cuda")
    msgs = np.full(N + 2, 9, np.int64)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_w == 0x5A5A).all()) and bool((msgs == 9).all())

    # a context with ordinary keys: no packing key to make, none to pack with
    plain = Context(prm, seed=3)
    assert _code(lambda: plain.packing_keygen(2, 7)) == E_STATE
    assert _code(lambda: plain.pack_dev(d_c.data_ptr(), N + 2, d_w.data_ptr(), w0)) == E_STATE
    assert plain.stat("packing_key") == 0 and untouched()
    plain.close()
    client = Context(prm, seed=3, keygen=False)
    client.keygen_seeded()
    assert _code(lambda: client.pack_dev(d_c.data_ptr(), N + 2, d_w.data_ptr(), w0)) == E_STATE       # seeded keys, still no packing key
    for t_p, gamma_p in ((4, 8), (1, 32), (2, 16), (3, 0), (0, 5), (32, 1)):
        assert _code(lambda: client.packing_keygen(t_p, gamma_p)) == E_INVALID, (t_p, gamma_p)
    assert client.stat("packing_key") == 0
    client.packing_keygen(2, 7)
    good = client.pack(cts, w0)
    exported = client.export_packing_key()
    for bad in (w0 - 1, 32, 0):
        assert _code(lambda: client.pack_dev(d_c.data_ptr(), N + 2, d_w.data_ptr(), bad)) == E_INVALID
        assert _code(lambda: client.packed_words(5, bad)) == E_INVALID
        assert _code(lambda: client._check(lib.fbs_decrypt_packed(client._h, good.ctypes.data, N + 2, bad, msgs.ctypes.data))) == E_INVALID
    assert _code(lambda: client.packing_keygen(4, 8)) == E_INVALID and client.stat("packing_levels") == 2   # the key in place stays
    with client.state(2, 5) as st:
        out = np.full(64, 7, np.uint64)
        for row0, rows in ((0, 3), (2, 1), (3, 0)):
            assert _code(lambda: client._check(lib.fbs_state_fetch_packed(client._h, st._h, row0, rows, w0, out.ctypes.data))) == E_INVALID
        assert (out == 7).all()
    assert untouched()
    # an evaluation-only context: no packing keygen, no decode; non-canonical bodies leave its key in place
    server = Context.evaluation_only(prm, **client.export_seeded_keys())
    assert _code(lambda: server.packing_keygen(2, 7)) == E_STATE
    server.import_packing_key(2, 7, exported["packing_bodies"])
    bad_bodies = exported["packing_bodies"].copy()
    bad_bodies[-1] = Q
    assert _code(lambda: server.import_packing_key(2, 7, bad_bodies)) == E_INVALID
    assert _code(lambda: server.import_packing_key(2, 16, exported["packing_bodies"])) == E_INVALID
    assert _code(lambda: server._check(lib.fbs_decrypt_packed(server._h, good.ctypes.data, N + 2, w0, msgs.ctypes.data))) == E_STATE
    assert untouched()
    # ... and both contexts still work; a second identical call grows no scratch
    assert np.array_equal(server.pack(cts, w0), good)
    growths = server.stat("scratch_growths")
    assert np.array_equal(server.pack(cts, w0), good) and server.stat("scratch_growths") == growths
    assert np.array_equal(client.pack(cts, w0), good)
    server.close()
    client.close()
