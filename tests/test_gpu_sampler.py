"""The rounded-Gaussian sampler (fbs_params.sampler = 1) on the GPU: the device computes the host's bits -- the sampler alone, both
encryption kernels, the whole client -- nothing downstream cares which sampler made the keys (the CPU oracle bootstraps to the same
words), the noise has the variance it is asked for, and a program at a default 128-bit set runs end to end under it."""
import numpy as np
import pytest

from oracle import lut_oracle
from oracle import tfhe_oracle as orc
from tests.helpers import load_fixture, subsample
from tests.test_gpu_host_client import _members
from tests.test_sampler import Q, planted_windows, random_windows

pytestmark = pytest.mark.gpu


def toy(**kw):
    from tfhe_fbs_map_amd import Params
    return Params(**dict(dict(n=8, log_n_poly=8, p_msg=7, sigma_lwe=1 << 6, sigma_glwe=1 << 10, sampler=1), **kw))


def toy_k2(**kw):
    return toy(k=2, l_bsk=1, beta_bsk=21, bsk_group=2, **kw)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def windows():
    """the planted windows and 2^16 random ones: a count that is no multiple of the 256 threads of a workgroup"""
    w = np.concatenate([planted_windows(), random_windows(1 << 16, 31)])
    assert w.shape[0] % 256 != 0 and w.shape[0] % 64 != 0
    return w


@pytest.mark.parametrize("ctx_sampler", [0, 1])
def test_device_sampler_is_the_host_sampler_word_for_word(windows, ctx_sampler):
    from tfhe_fbs_map_amd import Context, _native
    ctx = Context(toy(sampler=ctx_sampler), seed=1, keygen=False)       # (the hooks work whatever the context's own sampler)
    for sigma in (1, 1 << 10, 1 << 30, Q):
        host, device = _native.debug_gauss(windows, sigma), ctx.debug_gauss_dev(windows, sigma)
        bad = np.nonzero(host != device)[0]
        assert bad.size == 0, (sigma, bad[:8], windows[bad[:8]], host[bad[:8]], device[bad[:8]])
    assert (ctx.debug_gauss_dev(windows[:300], 0) == 0).all()
    assert ctx.debug_gauss_dev(windows[:0], 5).shape == (0,)
    with pytest.raises(_native.FbsError):
        ctx.debug_gauss_dev(windows[:4], Q + 1)
    ctx.close()


@pytest.mark.parametrize("make", [toy, toy_k2], ids=["k1", "k2"])
def test_device_encryption_is_host_encryption_under_the_gaussian(make):
    import torch
    from tfhe_fbs_map_amd import Context
    prm = make()
    ctx = Context(prm, seed=21, keygen=False)
    ctx.keygen_seeded()
    msgs = np.random.default_rng(4).integers(0, 2 * prm.p_msg, 1000, dtype=np.int64)    # 1000: a partial workgroup of four waves
    d_m = dev(msgs)
    d_c = torch.empty((1000, prm.ct_words), dtype=torch.int64, device="cuda")
    ctx.encrypt_dev(d_m.data_ptr(), 1000, d_c.data_ptr(), nonce0=500)
    ctx.sync()
    full = ctx.encrypt(msgs, 500)
    assert np.array_equal(d_c.cpu().numpy().view(np.uint64), full)
    on_dev, _ = ctx.encrypt_seeded(msgs, nonce0=9000, device=True)
    on_host, _ = ctx.encrypt_seeded(msgs, nonce0=9000, device=False)
    assert np.array_equal(on_dev, on_host)
    assert np.array_equal(ctx.decrypt(full), msgs) and np.array_equal(ctx.decrypt(ctx.expand_seeded(on_dev, 9000)), msgs)
    # ... and they are not the Irwin-Hall words: the same seed under sampler 0 has the same masks and other bodies
    twin = Context(prm.replace(sampler=0), seed=21, keygen=False)
    twin.keygen_seeded()
    other = twin.encrypt(msgs, 500)
    assert np.array_equal(other[:, :-1], full[:, :-1]) and (other[:, -1] != full[:, -1]).mean() > 0.9
    ctx.close()
    twin.close()


def test_host_client_and_gpu_client_write_the_same_files_under_the_gaussian():
    from tfhe_fbs_map_amd import Client, ExecConfig, parse_fbs
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, _ = subsample(rec, 16)
    cfg = dict(seed=bytes(range(3, 35)), sampler="gaussian", params=toy(n=12, sigma_glwe=4, l_bsk=2, beta_bsk=10, sampler=0))
    host = Client(env, ExecConfig(**cfg), packing=True, host=True)
    gpu = Client(env, ExecConfig(**cfg), packing=True, host=False)
    assert host.params == gpu.params and host.params.sampler == 1 and host.packing == gpu.packing and host.packing
    a, b = _members(host.server_key()), _members(gpu.server_key())
    assert a == b and "sampler.npy" in a and "packing_bodies.npy" in a
    enc_h, enc_g = host.encrypt(ins, nonce0=77), gpu.encrypt(ins, nonce0=77)      # the host loop and the device kernel
    assert _members(enc_h) == _members(enc_g)
    # the sampler-0 twin of the same seed is another key altogether
    plain = Client(env, ExecConfig(**dict(cfg, sampler="irwin_hall")), packing=True, host=True)
    c = _members(plain.server_key())
    assert "sampler.npy" not in c and c["mask_key.npy"] != a["mask_key.npy"] and c["bsk_bodies.npy"] != a["bsk_bodies.npy"]


def test_oracle_bootstraps_gaussian_keys_to_the_same_words():
    from tfhe_fbs_map_amd import Context
    prm = toy(n=16)
    ctx = Context(prm, seed=33)
    o = orc.Oracle(prm, seed=33, keygen=False)
    o.set_keys(**ctx.export_keys())
    table = [0, 1, 2, 3, 4, 5, 6]
    msgs = np.arange(32) % prm.p_msg
    cts = ctx.encrypt(msgs, nonce0=10)
    tv = ctx.tvset([table])
    mine = ctx.bootstrap_batch(tv, cts)
    theirs, _ = o.bootstrap_batch(cts, [table])
    assert np.array_equal(mine, theirs)
    assert np.array_equal(ctx.decrypt(mine), [table[m] for m in msgs]) and np.array_equal(o.decrypt(theirs), ctx.decrypt(mine))
    assert not np.array_equal(cts, orc.Oracle(prm, seed=33).encrypt(msgs, 10))     # (the oracle's own draws are Irwin-Hall)
    ctx.close()


def test_measured_noise_of_fresh_encryptions():
    import torch
    from tfhe_fbs_map_amd import Context
    prm = toy(sigma_glwe=1 << 20)
    ctx = Context(prm, seed=8)
    n = 4096
    msgs = np.arange(n, dtype=np.int64) % (2 * prm.p_msg)
    d_m = dev(msgs)
    d_c = torch.empty((n, prm.ct_words), dtype=torch.int64, device="cuda")
    ctx.encrypt_dev(d_m.data_ptr(), n, d_c.data_ptr(), nonce0=1)
    ctx.sync()
    cts = d_c.cpu().numpy().astype(np.int64)
    sk = ctx.export_keys()["sk_glwe"].astype(np.int64)
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    e = (cts[:, -1] - (cts[:, :-1] * sk[None, :]).sum(axis=1) - msgs * delta) % Q
    e = np.where(e > Q // 2, e - Q, e).astype(np.float64)
    ratio = (e ** 2).mean() / float(prm.sigma_glwe) ** 2
    print("variance of phase - Delta m over sigma^2:", ratio)
    assert abs(ratio - 1) <= 5 * np.sqrt(2 / n), ratio
    ctx.close()


def test_one_real_program_under_the_gaussian():
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    from tfhe_fbs_map_amd.split import client_choice
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, _ = subsample(rec, 16)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], ins)
    client = Client(env, ExecConfig(seed=5, sampler="gaussian"))
    assert client.params.sampler == 1 and client.params.replace(sampler=0) == client_choice(env, ExecConfig(seed=5))[0]   # a default 128-bit set
    server = Server(client.server_key())
    assert server.ctx.params.sampler == 1 and server.ctx.stat("has_secret") == 0
    got = client.decrypt(server.run(env, client.encrypt(ins)))
    assert sorted(got) == sorted(clear)
    for k in clear:
        assert np.array_equal(np.broadcast_to(got[k], (16,)), np.broadcast_to(clear[k], (16,))), k
