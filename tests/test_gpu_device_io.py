"""Encryption and decryption on the device (include/fbs_exec.h: fbs_encrypt_dev, fbs_encrypt_fresh_dev, fbs_decrypt_dev,
fbs_eval_messages): word for word what the host entries and the CPU oracle compute, the same refusals and nonce rules, ordered
on the caller's stream, and the facade's device path equal to its host path."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import assert_outputs_equal, load_fixture, subsample, toy_k2, toy_k3

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
NONCE_LIMIT = 1 << 55


def _toy(**kw):
    from tfhe_fbs_map_amd import Params
    return Params(**{**dict(n=12, log_n_poly=10, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=1 << 8), **kw})


def _default128():
    from tfhe_fbs_map_amd.params import choose_params
    return choose_params(15, 1)


SETS = {
    "k1_n1024": lambda: _toy(),
    "k1_n2048": lambda: _toy(log_n_poly=11),
    "k2": lambda: toy_k2(),
    "k3": lambda: toy_k3(),
    "sigma0": lambda: _toy(sigma_glwe=0),
    "default128": _default128,
}
_CTX = {}


def keyed(name):
    """(context, oracle keyed identically) of a set, made once per module"""
    if name not in _CTX:
        from tfhe_fbs_map_amd import Context
        prm = SETS[name]()
        ctx = Context(prm, seed=11)
        o = orc.Oracle(prm, seed=11, keygen=False)
        o.set_keys(**ctx.export_keys())
        _CTX[name] = (ctx, o)
    return _CTX[name]


def messages(count, p, seed=0):
    """negative values, values >= 2p and the int64 extremes among ordinary ones"""
    m = np.random.default_rng(seed).integers(-8 * p, 8 * p, count, dtype=np.int64)
    special = np.array([INT64_MIN, INT64_MAX, -1, 2 * p, 2 * p - 1, -2 * p - 1, 0, 4 * p + 3], np.int64)
    m[:min(count, special.size)] = special[:count]
    return m


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


def encrypt_on_device(ctx, m, nonce0=None, stream=0):
    import torch
    d_m = dev(m)
    d_c = torch.empty((m.size, ctx.params.ct_words), dtype=torch.int64, device="cuda")
    first = ctx.encrypt_dev(d_m.data_ptr(), m.size, d_c.data_ptr(), nonce0=nonce0, stream=stream)
    ctx.sync(stream)
    return first, host(d_c)


def decrypt_on_device(ctx, cts):
    import torch
    cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, ctx.params.ct_words)
    d_m = torch.full((cts.shape[0],), -7, dtype=torch.int64, device="cuda")
    ctx.decrypt_dev(dev(cts).data_ptr(), cts.shape[0], d_m.data_ptr())
    ctx.sync()
    return host(d_m, np.int64)


@pytest.mark.parametrize("name", list(SETS))
def test_encrypt_dev_is_word_identical_to_host_and_oracle(name):
    ctx, o = keyed(name)
    p = ctx.params.p_msg
    for count in (1, 7, 1000, 4099):
        m = messages(count, p, seed=count)
        for nonce0 in (0, NONCE_LIMIT - count):
            first, got = encrypt_on_device(ctx, m, nonce0=nonce0)
            assert first == nonce0
            assert np.array_equal(got, ctx.encrypt(m, nonce0=nonce0)), (name, count, nonce0)
            assert np.array_equal(got, o.encrypt(m, nonce0=nonce0)), (name, count, nonce0)
    assert np.array_equal(decrypt_on_device(ctx, got), ctx.decrypt(got))


def test_refusals_touch_nothing():
    import torch
    from tfhe_fbs_map_amd import Context, FbsError
    ctx, _ = keyed("k1_n1024")
    ctw = ctx.params.ct_words
    d_m = dev(np.arange(4, dtype=np.int64))
    d_c = torch.full((4, ctw), 123, dtype=torch.int64, device="cuda")
    d_out = torch.full((4,), 55, dtype=torch.int64, device="cuda")
    before = ctx.stat("next_nonce")
    for nonce0, count in ((NONCE_LIMIT - 3, 4), (NONCE_LIMIT, 1), (2**64 - 1, 4)):
        with pytest.raises(FbsError) as e:
            ctx.encrypt_dev(d_m.data_ptr(), count, d_c.data_ptr(), nonce0=nonce0)
        assert e.value.code == -1
    for args in ((0, 4, d_c.data_ptr()), (d_m.data_ptr(), 4, 0)):
        for nonce0 in (0, None):
            with pytest.raises(FbsError) as e:
                ctx.encrypt_dev(*args, nonce0=nonce0)
            assert e.value.code == -1
    with pytest.raises(FbsError) as e:
        ctx.decrypt_dev(0, 4, d_out.data_ptr())
    assert e.value.code == -1
    with pytest.raises(FbsError) as e:
        ctx.decrypt_dev(d_c.data_ptr(), 4, 0)
    assert e.value.code == -1
    assert ctx.encrypt_dev(0, 0, 0, nonce0=5) == 5                 # count = 0: OK, no work
    ctx.decrypt_dev(0, 0, 0)
    assert ctx.encrypt_dev(d_m.data_ptr(), 0, d_c.data_ptr()) == before   # fresh, count = 0: nothing reserved
    bare = Context(ctx.params, seed=11, keygen=False)
    for call in (lambda: bare.encrypt_dev(d_m.data_ptr(), 4, d_c.data_ptr(), nonce0=0),
                 lambda: bare.encrypt_dev(d_m.data_ptr(), 4, d_c.data_ptr()),
                 lambda: bare.decrypt_dev(d_c.data_ptr(), 4, d_out.data_ptr())):
        with pytest.raises(FbsError) as e:
            call()
        assert e.value.code == -3
    ctx.sync()
    assert bool((d_c == 123).all()) and bool((d_out == 55).all())
    assert ctx.stat("next_nonce") == before and bare.stat("next_nonce") == NONCE_LIMIT


def test_fresh_streams_interleave_with_the_host_counter():
    ctx, o = keyed("k2")
    m = messages(9, 7)
    f1, c1 = encrypt_on_device(ctx, m)
    mid = ctx.stat("next_nonce")
    ctx.encrypt(m[:5])                                            # host, fresh: takes [mid, mid + 5)
    f3, c3 = encrypt_on_device(ctx, m[:3])
    assert mid == f1 + 9 and f3 == mid + 5 and ctx.stat("next_nonce") == f3 + 3
    assert f1 >= NONCE_LIMIT
    assert np.array_equal(c1, o.encrypt(m, nonce0=f1)) and np.array_equal(c3, o.encrypt(m[:3], nonce0=f3))


def test_decrypt_dev_equals_decrypt():
    from tfhe_fbs_map_amd import Context
    q = (1 << 46) - 62 * (1 << 13) + 1
    rng = np.random.default_rng(3)
    for p in (7, 15, 4096):
        ctx = Context(_toy(p_msg=p), seed=4)
        ctw = ctx.params.ct_words
        fresh = ctx.encrypt(messages(300, p), nonce0=1)
        assert np.array_equal(decrypt_on_device(ctx, fresh), ctx.decrypt(fresh))
        # trivial ciphertexts on every rounding boundary (phase 2p / q = k + 1/2) and one either side
        ks = np.arange(2 * p) if p < 100 else rng.choice(2 * p, 256, replace=False)
        edges = [((2 * int(k) + 1) * q) // (4 * p) + d for k in ks for d in (-1, 0, 1, 2)] + [0, 1, q - 1]
        triv = np.zeros((len(edges), ctw), np.uint64)
        triv[:, -1] = np.array(edges, np.uint64) % q
        assert np.array_equal(decrypt_on_device(ctx, triv), ctx.decrypt(triv)), p
        rnd = rng.integers(0, q, (500, ctw), dtype=np.uint64)
        assert np.array_equal(decrypt_on_device(ctx, rnd), ctx.decrypt(rnd)), p
        ctx.close()


def _program(nat, ctx, name, fuse=False):
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    tv = ctx.tvset(low["tables"])
    prog = nat.Program(ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"],
                       low["term_coef"], low["term_src"], low["out_wire"], fuse_tables=fuse)
    prog._tv = tv
    return rec, low, prog


def _bits(rec, low, T):
    ins, expect = subsample(rec, T)
    return np.stack([np.asarray(ins[n], np.int64) for n in low["input_names"]]).reshape(len(low["input_names"]), T), expect


@pytest.mark.parametrize("name,fuse", [("edge_outputs", False), ("edge_outputs", True), ("adder8__search_p7", False)])
def test_eval_messages_equals_host_encrypt_eval_decrypt(name, fuse):
    from tfhe_fbs_map_amd import Context, _native as nat
    ctx = Context(_toy(), seed=6)
    rec, low, prog = _program(nat, ctx, name, fuse)
    assert prog.fused == fuse
    for T in (0, 1, 37):
        bits, expect = _bits(rec, low, T)
        want = ctx.decrypt(prog.eval(ctx.encrypt(bits, nonce0=21), T))
        got = prog.eval_messages(bits, nonce0=21)
        assert got.shape == (len(low["out_names"]), T) and np.array_equal(got, want), (name, T)
        for k, n in enumerate(low["out_names"]):
            e = expect[n]
            assert np.array_equal(got[k], np.full(T, e) if isinstance(e, int) else e), (name, T, n)
    if name == "edge_outputs":
        assert any(w < 0 for w in low["out_wire"]) and any(0 <= w < len(low["input_names"]) for w in low["out_wire"])


def test_eval_messages_in_chunks(monkeypatch):
    from tfhe_fbs_map_amd import Context, _native as nat
    T = 37
    ctx = Context(_toy(), seed=6)
    rec, low, prog = _program(nat, ctx, "adder8__search_p7")
    bits, _ = _bits(rec, low, T)
    want = ctx.decrypt(prog.eval(ctx.encrypt(bits, nonce0=2), T))
    monkeypatch.setenv("FBS_WIRE_BUDGET_MB", "2")               # a handful of samples per chunk (test_gpu_levels.py)
    assert 2 * 2**20 * 0.6 / (prog.n_slots * ctx.params.ct_words * 8) < T / 3
    ctx2 = Context(_toy(), seed=6)                              # a fresh context: its wire buffer has not grown yet
    _, _, prog2 = _program(nat, ctx2, "adder8__search_p7")
    assert np.array_equal(prog2.eval_messages(bits, nonce0=2), want)


def test_eval_messages_fresh_streams():
    from tfhe_fbs_map_amd import Context, _native as nat
    ctx = Context(_toy(), seed=6)
    o = orc.Oracle(ctx.params, seed=6, keygen=False)
    o.set_keys(**ctx.export_keys())
    rec, low, prog = _program(nat, ctx, "adder8__search_p7")
    T = 5
    bits, _ = _bits(rec, low, T)
    first = ctx.stat("next_nonce")
    got = prog.eval_messages(bits)
    assert ctx.stat("next_nonce") == first + bits.size
    assert np.array_equal(got, ctx.decrypt(prog.eval(o.encrypt(bits, nonce0=first), T)))
    prog.eval_messages(bits[:, :0])
    assert ctx.stat("next_nonce") == first + bits.size             # T = 0: no streams


def test_encrypt_dev_is_ordered_on_the_callers_stream():
    import torch
    ctx, _ = keyed("k1_n1024")
    count = 4096
    m = messages(count, 7) % 7
    tv = ctx.tvset([[0, 1, 1, 0, 1, 0, 0]])
    want = ctx.bootstrap_batch(tv, ctx.encrypt(m, nonce0=5))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_m = dev(m)
        d_c = torch.empty((count, ctx.params.ct_words), dtype=torch.int64, device="cuda")
        d_out = torch.empty_like(d_c)
    side.synchronize()
    ctx.encrypt_dev(d_m.data_ptr(), count, d_c.data_ptr(), nonce0=5, stream=side.cuda_stream)
    ctx.bootstrap_batch_dev(tv, d_c.data_ptr(), 0, count, d_out.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(host(d_out), want)


def test_facade_device_io_equals_host_io():
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    for name in ("full_adder__search_p7", "edge_outputs"):
        rec = load_fixture(name)
        ins, expect = subsample(rec, 16)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        on = env.eval(ins, config=ExecConfig(seed=1, reduced_noise=True, nonce0=77))
        off = env.eval(ins, config=ExecConfig(seed=1, reduced_noise=True, nonce0=77, device_io=False))
        assert on.keys() == off.keys()
        for k in on:
            assert np.array_equal(on[k], off[k]), (name, k)
        assert_outputs_equal(on, expect)


@pytest.mark.parametrize("name", ["full_adder__search_p7", "edge_outputs"])
def test_facade_default_config_gives_the_goldens(name):
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    rec = load_fixture(name)
    ins, expect = subsample(rec, 24)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = ExecConfig(seed=2)
    assert cfg.device_io
    assert_outputs_equal(env.eval(ins, config=cfg), expect)
