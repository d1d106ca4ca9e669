"""The host client against the GPU: libfbsclient.so and libfbsexec.so write the same words for the same parameter set and seed, a
`Client(host=True)` and a GPU `Server` speak the whole protocol (full, compact and packed outputs, a resident chain), and its files
are those of a `Client(host=False)`."""
import io
import zipfile

import numpy as np
import pytest

from oracle import lut_oracle
from tests.helpers import load_fixture, subsample

pytestmark = pytest.mark.gpu

T = 16
A_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}
B_NAMES = [f"b{i}" for i in range(8)]


def _sets():
    from tfhe_fbs_map_amd import Params
    common = dict(n=12, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=4)
    return {"k1_N256": Params(log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, **common),
            "k2_N256_g2": Params(log_n_poly=8, k=2, l_bsk=1, beta_bsk=21, bsk_group=2, **common),
            "k3_N512_g2": Params(log_n_poly=9, k=3, l_bsk=1, beta_bsk=18, bsk_group=2, **common)}


# ---- 7. word identity of the two libraries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [23, bytes(range(7, 39))], ids=["seed64", "seed32bytes"])
@pytest.mark.parametrize("name", ["k1_N256", "k2_N256_g2", "k3_N512_g2"])
def test_both_libraries_write_the_same_words(name, seed):
    from tfhe_fbs_map_amd import Context, HostContext
    prm = _sets()[name]
    host, gpu = HostContext(prm, seed=seed), Context(prm, seed=seed, keygen=False)
    assert host.device_info == "host" and gpu.device_info.startswith("gfx950")
    host.keygen_seeded()
    gpu.keygen_seeded()
    a, b = host.export_seeded_keys(), gpu.export_seeded_keys()
    assert a["mask_key"] == b["mask_key"] and set(a) == set(b) == {"mask_key", "bsk_bodies", "ksk_bodies"}
    for k in ("bsk_bodies", "ksk_bodies"):
        assert a[k].size and np.array_equal(a[k], b[k]), k
    ka, kb = host.export_keys(), gpu.export_keys()
    for k in ka:                                                    # secrets and the expanded keys as well
        assert np.array_equal(ka[k], kb[k]), k
    host.packing_keygen(2, 7)
    gpu.packing_keygen(2, 7)
    pa, pb = host.export_packing_key(full=True), gpu.export_packing_key(full=True)
    assert (pa["packing_levels"], pa["packing_base_bits"]) == (pb["packing_levels"], pb["packing_base_bits"]) == (2, 7)
    assert np.array_equal(pa["packing_bodies"], pb["packing_bodies"]) and np.array_equal(pa["full"], pb["full"])
    msgs = np.arange(3 * 2 * prm.p_msg).reshape(3, -1) % (2 * prm.p_msg)
    for device in (True, False):                                    # the GPU library's device and host entries alike
        (x, fx), (y, fy) = host.encrypt_seeded(msgs, nonce0=1000), gpu.encrypt_seeded(msgs, nonce0=1000, device=device)
        assert fx == fy == 1000 and np.array_equal(x, y)
        (x, fx), (y, fy) = host.encrypt_seeded(msgs), gpu.encrypt_seeded(msgs, device=device)      # fresh: the same counter
        assert fx == fy and fx >= 1 << 55 and np.array_equal(x, y)
    assert host.stat("next_nonce") == gpu.stat("next_nonce") == (1 << 55) + 2 * msgs.size
    assert np.array_equal(host.encrypt(msgs, 77), gpu.encrypt(msgs, 77))
    assert np.array_equal(host.encrypt(msgs), gpu.encrypt(msgs))
    cts = gpu.encrypt(msgs, 5)
    assert np.array_equal(host.decrypt(cts), msgs) and np.array_equal(gpu.decrypt(host.encrypt(msgs, 6)), msgs)
    assert np.array_equal(host.expand_seeded(x, fx), gpu.expand_seeded(x, fx))
    host.close()
    gpu.close()


# ---- 8. the protocol end to end ----------------------------------------------------------------------------------------------------
def _members(obj):
    """a saved file as {member name: bytes}: np.savez stamps each zip member with the time of writing, the content is what travels"""
    buf = io.BytesIO()
    obj.save(buf)
    with zipfile.ZipFile(io.BytesIO(buf.getvalue())) as z:
        return {n: z.read(n) for n in z.namelist()}


def _same(got, clear, what):
    assert sorted(got) == sorted(clear), what
    for k in clear:
        assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (what, k)


@pytest.mark.parametrize("fixture", ["full_adder__search_p7", "adder8__search_p7"])
def test_host_client_and_gpu_server_speak_the_protocol(fixture):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    from tfhe_fbs_map_amd.split import CompactOutputs, EncryptedOutputs, PackedOutputs
    rec = load_fixture(fixture)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, _ = subsample(rec, T)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], ins)
    host = Client(env, ExecConfig(seed=5), packing=True, host=True)
    gpu = Client(env, ExecConfig(seed=5), packing=True, host=False)
    assert host.host is True and gpu.host is False and host.ctx.device_info == "host" and gpu.ctx.device_info.startswith("gfx950")
    assert host.params == gpu.params and host.fuse_tables == gpu.fuse_tables and host.packing == gpu.packing
    assert host.fingerprint == gpu.fingerprint
    assert _members(host.server_key()) == _members(gpu.server_key())
    enc_h, enc_g = host.encrypt(ins), gpu.encrypt(ins)
    assert _members(enc_h) == _members(enc_g) and enc_h.T == T

    server = Server(host.server_key())                                # keyed by the host client's file content alone
    runs = {"full": (server.run, EncryptedOutputs), "compact": (server.run_compact, CompactOutputs), "packed": (server.run_packed, PackedOutputs)}
    for what, (run, kind) in runs.items():
        out_h, out_g = run(env, enc_h), run(env, enc_g)
        assert isinstance(out_h, kind) and _members(out_h) == _members(out_g), what
        _same(host.decrypt(out_h), clear, what)                       # the host client reads the result
        _same(gpu.decrypt(out_h), clear, what + ", GPU client")       # ... and each client the other's
        _same(host.decrypt(out_g), clear, what + ", crossed")


# ---- 9. a chain ----------------------------------------------------------------------------------------------------------------------
def test_adder8_accumulator_keyed_and_fed_by_the_host_client():
    """acc <- acc + b over three hops with the state resident on the GPU; every input is encrypted by the host client, hop by hop,
    and the compact fetch at the end decrypts to the integer sums mod 256"""
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    from tfhe_fbs_map_amd.split import CompactOutputs
    rec = load_fixture("adder8__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=7), programs=[env], host=True)
    assert client.host is True
    server = Server(client.server_key())
    rng = np.random.default_rng(3)
    bits = lambda v, names: {n: (v >> i) & 1 for i, n in enumerate(names)}      # noqa: E731
    a, b = rng.integers(0, 256, T), rng.integers(0, 256, T)
    acc = server.run(env, client.encrypt({**bits(a, [f"a{i}" for i in range(8)]), **bits(b, B_NAMES)}), resident=True)
    total = a + b
    for hop in range(3):
        b = rng.integers(0, 256, T)
        nxt = server.run_chain(env, [acc, client.encrypt(bits(b, B_NAMES), names=B_NAMES)], rename=A_FROM_S, resident=True)
        acc.close()
        acc = nxt
        total = (total & 0xFF) + b                                     # the carry out of bit 7 is an output, not fed back
    out = acc.fetch(compact=True)
    acc.close()
    assert isinstance(out, CompactOutputs)
    got = client.decrypt(out)
    low = sum(np.broadcast_to(got[f"s{i}"], (T,)).astype(np.int64) << i for i in range(8))
    assert np.array_equal(low, total & 0xFF)
    carry = [k for k in got if k not in A_FROM_S.values()]
    if len(carry) == 1:
        assert np.array_equal(np.broadcast_to(got[carry[0]], (T,)), total >> 8)
    assert server.ctx.stat("states_alive") == 0
