"""Keys on the device (knob "keys_on_device", `Context(device_keys=True)`): the evaluation keys made and expanded by the kernels of
csrc/fbs_keygen.hip are, word for word, those of the host path -- the client library's `HostContext` with the same parameters and
seed is the reference --, everything derived from them on the device bootstraps to the same words, and a `Server` keyed that way
returns the same files."""
import io
import zipfile

import numpy as np
import pytest

from oracle import lut_oracle
from tests.helpers import assert_outputs_equal, load_fixture, subsample

pytestmark = pytest.mark.gpu

Q = 0x3FFFFFF84001
T = 16
SEED32 = bytes(range(7, 39))
E_INVALID = -1


def _sets():
    """the smallest sets that reach every branch: k = 1 .. 4, every N, one and two key bits per step, one and two gadget levels,
    an odd n (a partial ChaCha block in every key-switching row), no noise, the rounded Gaussian"""
    from tfhe_fbs_map_amd import Params
    common = dict(n=12, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=4)
    sets = {
        "k1_N256_l2": Params(log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, **common),
        "k2_N256_g2": Params(log_n_poly=8, k=2, l_bsk=1, beta_bsk=21, bsk_group=2, **common),
        "k4_N256_g2_l2": Params(log_n_poly=8, k=4, l_bsk=2, beta_bsk=9, bsk_group=2, **common),
        "k3_N512_g2": Params(log_n_poly=9, k=3, l_bsk=1, beta_bsk=18, bsk_group=2, **common),
        "k2_N1024_g2_n64": Params(n=64, log_n_poly=10, k=2, l_bsk=1, beta_bsk=21, bsk_group=2, t_ksk=7, gamma_ksk=2, p_msg=15,
                                  sigma_lwe=1 << 30, sigma_glwe=4),
        "k1_N2048_n13_l2": Params(log_n_poly=11, k=1, l_bsk=2, beta_bsk=14, **dict(common, n=13)),
        "k1_N4096_n5": Params(log_n_poly=12, k=1, l_bsk=1, beta_bsk=21, **dict(common, n=5)),
    }
    sets["noiseless"] = sets["k2_N256_g2"].replace(sigma_lwe=0, sigma_glwe=0)
    sets["gauss"] = sets["k3_N512_g2"].replace(sampler=1, sigma_lwe=1 << 30)
    return sets


NAMES = ["k1_N256_l2", "k2_N256_g2", "k4_N256_g2_l2", "k3_N512_g2", "k2_N1024_g2_n64", "k1_N2048_n13_l2", "k1_N4096_n5", "noiseless",
         "gauss"]
CASES = [(n, 23) for n in NAMES] + [("k2_N256_g2", SEED32), ("k3_N512_g2", SEED32)]

_host = {}


def _host_keys(name, seed, seeded):
    """the reference, computed once: `HostContext` keys of a (set, seed, keygen | keygen_seeded)"""
    key = (name, seed, seeded)
    if key not in _host:
        from tfhe_fbs_map_amd import HostContext
        ctx = HostContext(_sets()[name], seed=seed, keygen=False)
        if seeded:
            ctx.keygen_seeded()
        else:
            ctx.keygen()
        rec = dict(keys=ctx.export_keys(), seeded=ctx.export_seeded_keys() if seeded else None)
        if seeded and name in ("k3_N512_g2", "k2_N1024_g2_n64") and seed == 23:
            ctx.packing_keygen(2, 7)
            rec["packing"] = ctx.export_packing_key(full=True)
        ctx.close()
        for group in (rec["keys"], rec["seeded"] or {}):
            for v in group.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _host[key] = rec
    return _host[key]


def _bsk_bytes(prm):
    G = prm.n // 2 * 3 if prm.bsk_group == 2 else prm.n
    return G * (prm.k + 1) * prm.l_bsk * (prm.k + 1) * (1 << prm.log_n_poly) * 8


# ---- 1. word identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seeded", [False, True], ids=["keygen", "keygen_seeded"])
@pytest.mark.parametrize("name,seed", CASES, ids=["%s-%s" % (n, "seed64" if s == 23 else "seed32bytes") for n, s in CASES])
def test_device_keys_are_the_host_keys_word_for_word(name, seed, seeded):
    from tfhe_fbs_map_amd import Context
    prm = _sets()[name]
    want = _host_keys(name, seed, seeded)
    ctx = Context(prm, seed=seed, keygen=False, device_keys=True)
    make = ctx.keygen_seeded if seeded else ctx.keygen
    make()
    assert ctx.stat("keys_made_on_device") == 1 and ctx.stat("bsk_upload_bytes") == 0
    got = ctx.export_keys()
    assert set(got) == set(want["keys"]) == {"sk_lwe", "sk_glwe", "bsk", "ksk"}
    for k, ref in want["keys"].items():
        assert ref.size and got[k].size == ref.size, k
        diff = np.flatnonzero(got[k] != ref)
        assert diff.size == 0, "%s: %d of %d words differ, the first at %d" % (k, diff.size, ref.size, diff[0])
    if seeded:
        bodies = ctx.export_seeded_keys()
        assert bodies["mask_key"] == want["seeded"]["mask_key"]
        for k in ("bsk_bodies", "ksk_bodies"):
            assert np.array_equal(bodies[k], want["seeded"][k]), k
    # the same context with the knob at 0: the host path, the same words again
    ctx.tune(keys_on_device=0)
    make()
    assert ctx.stat("keys_made_on_device") == 0 and ctx.stat("bsk_upload_bytes") == _bsk_bytes(prm)
    again = ctx.export_keys()
    for k, ref in want["keys"].items():
        assert np.array_equal(again[k], ref), k
    ctx.close()


# ---- 2. what the device derives from them ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks_mfma", [1, 0])
@pytest.mark.parametrize("name", ["k2_N1024_g2_n64", "k1_N256_l2"])
def test_device_keyed_and_host_keyed_contexts_bootstrap_to_the_same_words(name, ks_mfma):
    """the transform straight from the device rows (d_bsk_hat) and the key-switching tables made from the copied-back rows"""
    from tfhe_fbs_map_amd import Context
    prm = _sets()[name]
    p = prm.p_msg
    msgs = np.arange(64) % (2 * p)
    outs = []
    for device_keys in (True, False):
        ctx = Context(prm, seed=23, device_keys=device_keys)
        assert ctx.stat("keys_made_on_device") == int(device_keys)
        ctx.tune(ks_mfma=ks_mfma)
        tv = ctx.tvset([[(3 * x + 1) % p for x in range(p)]])
        outs.append(ctx.bootstrap_batch(tv, ctx.encrypt(msgs, nonce0=100)))
        ctx.close()
    assert outs[0].shape == (64, prm.ct_words) and np.array_equal(outs[0], outs[1])


# ---- 3. a server keyed on the device ---------------------------------------------------------------------------------------------
def _members(obj):
    """a saved file as {member name: bytes}: np.savez stamps each zip member with the time of writing, the content is what travels"""
    buf = io.BytesIO()
    obj.save(buf)
    with zipfile.ZipFile(io.BytesIO(buf.getvalue())) as z:
        return {n: z.read(n) for n in z.namelist()}


def test_server_keyed_on_the_device_returns_the_same_files():
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, _ = subsample(rec, T)
    clear = lut_oracle.eval_fbs_text(rec["fbs"], ins)
    client = Client(env, ExecConfig(seed=5), packing=True, host=True)
    key = client.server_key()
    dev, host = Server(key, device_keys=True), Server(key)
    assert dev.ctx.stat("keys_made_on_device") == 1 and host.ctx.stat("keys_made_on_device") == 0
    assert dev.ctx.stat("bsk_upload_bytes") == np.asarray(key.bsk_bodies).size * 8
    assert host.ctx.stat("bsk_upload_bytes") == _bsk_bytes(key.params)
    enc = client.encrypt(ins)
    for what in ("run", "run_compact", "run_packed"):
        out_d, out_h = getattr(dev, what)(env, enc), getattr(host, what)(env, enc)
        assert _members(out_d) == _members(out_h), what
        got = client.decrypt(out_d)
        assert sorted(got) == sorted(clear), what
        for k in clear:
            assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (what, k)


# ---- 4. the packing key ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k3_N512_g2", "k2_N1024_g2_n64"])
def test_packing_key_made_on_the_device_is_the_host_key(name):
    from tfhe_fbs_map_amd import Context
    want = _host_keys(name, 23, True)["packing"]
    ctx = Context(_sets()[name], seed=23, keygen=False, device_keys=True)
    ctx.keygen_seeded()
    ctx.packing_keygen(2, 7)
    got = ctx.export_packing_key(full=True)
    assert (got["packing_levels"], got["packing_base_bits"]) == (want["packing_levels"], want["packing_base_bits"]) == (2, 7)
    assert want["packing_bodies"].size and np.array_equal(got["packing_bodies"], want["packing_bodies"])
    assert np.array_equal(got["full"], want["full"])
    ctx.close()


# ---- 5. one context through every way of being keyed -------------------------------------------------------------------------------
def test_lifecycle_on_one_context_and_the_facade():
    from tfhe_fbs_map_amd import Context, ExecConfig, parse_fbs
    prm = _sets()["k2_N256_g2"]
    full = _bsk_bytes(prm)
    ctx = Context(prm, seed=23, keygen=False, device_keys=True)
    assert ctx.stat("keys_made_on_device") == 0 and ctx.stat("bsk_upload_bytes") == 0     # no keys yet
    ctx.keygen()
    assert (ctx.stat("keys_made_on_device"), ctx.stat("bsk_upload_bytes"), ctx.stat("seeded_keys")) == (1, 0, 0)
    ctx.tune(keys_on_device=0)
    ctx.keygen()
    assert (ctx.stat("keys_made_on_device"), ctx.stat("bsk_upload_bytes"), ctx.stat("seeded_keys")) == (0, full, 0)
    assert np.array_equal(ctx.export_keys()["bsk"], _host_keys("k2_N256_g2", 23, False)["keys"]["bsk"])
    ctx.tune(keys_on_device=1)
    ctx.keygen_seeded()
    assert (ctx.stat("keys_made_on_device"), ctx.stat("bsk_upload_bytes"), ctx.stat("seeded_keys")) == (1, 0, 1)
    server_key, keys = ctx.export_seeded_keys(), ctx.export_keys()
    ctx.import_seeded_keys(**server_key)
    assert (ctx.stat("keys_made_on_device"), ctx.stat("bsk_upload_bytes")) == (1, server_key["bsk_bodies"].size * 8)
    assert (ctx.stat("has_secret"), ctx.stat("seeded_keys")) == (0, 1)
    # the expansion is the key it came from (an evaluation-only context exports its evaluation keys, not the secrets)
    from tfhe_fbs_map_amd import _native
    bsk, ksk = np.empty(keys["bsk"].size, np.uint64), np.empty(keys["ksk"].size, np.uint64)
    ctx._check(_native.lib.fbs_export_keys(ctx._h, None, None, _native._ptr(bsk), _native._ptr(ksk)))
    assert np.array_equal(bsk, keys["bsk"]) and np.array_equal(ksk, keys["ksk"])
    ctx.close()

    rec = load_fixture("adder8__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, outs = subsample(rec, T)
    cfg = ExecConfig(seed=5, device_keys=True)
    assert_outputs_equal(env.eval(ins, config=cfg), outs)
    made = list(cfg._contexts.values())
    assert len(made) == 1 and made[0].stat("keys_made_on_device") == 1 and made[0].stat("bsk_upload_bytes") == 0


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_import_under_the_knob_leaves_the_previous_keys_usable():
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd._native import FbsError
    prm = _sets()["k2_N256_g2"]
    p = prm.p_msg
    ctx = Context(prm, seed=23, keygen=False, device_keys=True)
    ctx.keygen_seeded()
    tv = ctx.tvset([[(x + 2) % p for x in range(p)]])
    cts = ctx.encrypt(np.arange(32) % (2 * p), nonce0=7)
    before = ctx.bootstrap_batch(tv, cts)
    key = ctx.export_seeded_keys()
    for which, text in (("bsk_bodies", "bootstrapping-key body word is not a canonical residue"),
                        ("ksk_bodies", "key-switching-key body word is not a canonical residue")):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in key.items()}
        bad[which][bad[which].size // 2] = Q
        with pytest.raises(FbsError) as err:
            ctx.import_seeded_keys(**bad)
        assert err.value.code == E_INVALID and text in str(err.value)
    assert (ctx.stat("has_secret"), ctx.stat("keys_made_on_device"), ctx.stat("bsk_upload_bytes")) == (1, 1, 0)
    assert np.array_equal(ctx.bootstrap_batch(tv, cts), before)
    ctx.close()
