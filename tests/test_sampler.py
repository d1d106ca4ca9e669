"""The opt-in rounded-Gaussian noise sampler (fbs_params.sampler = 1, csrc/fbs_sampler.hpp) without a GPU: its formula against
numpy on random and planted windows, its distribution, and the plumbing -- selection and refusal, key derivation, every kind of
draw of a context, the saved server key.

The host sampler is reached through `fbs_debug_gauss` (libfbsexec.so, which loads without a GPU; the entry needs no context).  The
client library's export list is pinned by tests/test_client_lib.py and carries no debug entry for the sampler; libfbsclient.so
(`HostContext`) is what the context-level tests here key and encrypt with, and `test_context_draws_are_the_sampler_on_the_stream_words`
ties its draws to that entry word for word.
"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_client_lib import chacha_rows, fold, negacyclic_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
Q = (1 << 46) - 62 * (1 << 13) + 1
M64 = (1 << 64) - 1
DOM_KSK_NOISE, DOM_ENC_MASK, DOM_ENC_NOISE, DOM_SENC_NOISE = 6, 7, 8, 15


@pytest.fixture(scope="module", autouse=True)
def client_library():
    subprocess.check_call(["make", "-s", "-C", CSRC, "client"], timeout=600)


def gauss(words, sigma):
    from tfhe_fbs_map_amd import _native
    return _native.debug_gauss(words, sigma)


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------------
def window(U, t, rest=(0, 0, 0), low=0):
    """six words with U = w0 2^64 + w1 and t = w2 >> 11 (`low`: the eleven bits of w2 below t, which the sampler must not read)"""
    return [(U >> 64) & M64, U & M64, ((t << 11) | low) & M64, *rest]


def z_reference(words):
    """z of each window [count][6] by the definition of include/fbs_exec.h / csrc/fbs_sampler.hpp, in float64 with np.log and np.cos.
    -2 ln u1 is taken as -2 np.log(u1) on u1 = f 2^(-e-1) itself, which a double holds exactly: the same closed formula as
    -2 (ln f - (e + 1) ln 2) without that form's cancellation in float64 at u1 near 1 (U = 2^128 - 1 would otherwise come out of numpy
    as r = 0 or r = 2^-26 by the rounding of ln 2, sixteen units apart at sigma = 2^30)."""
    words = np.asarray(words, np.uint64).reshape(-1, 6)
    f = np.empty(len(words))
    e = np.empty(len(words), np.int64)
    for i, (w0, w1) in enumerate(zip(words[:, 0].tolist(), words[:, 1].tolist())):
        U = (w0 << 64) | w1
        if U == 0:
            U = 1
        e[i] = 128 - U.bit_length()
        f[i] = float((U << int(e[i])) >> 75) / float(1 << 52)          # the leading one and the 52 bits after it, truncated
    assert ((f >= 1.0) & (f < 2.0)).all() and ((e >= 0) & (e <= 127)).all()
    u1 = np.ldexp(f, -(e + 1).astype(np.int64))
    r = np.sqrt(-2.0 * np.log(u1))
    t = (words[:, 2] >> np.uint64(11)).astype(np.float64)               # 53 bits: exact
    return r * np.cos(2.0 * np.pi * t / float(1 << 53))


def planted_windows():
    """the edge inputs no ChaCha20 stream would hit: U = 0, 2^128 - 1, 2^j and 2^j - 1 for every j at several angles, and t at 0,
    2^53 - 1 and every octant boundary +- 1 at several radii"""
    Us = [0, (1 << 128) - 1] + [1 << j for j in range(128)] + [(1 << j) - 1 for j in range(128)]
    ts = [0, (1 << 53) - 1] + [(o << 50) + d for o in range(1, 8) for d in (-1, 0, 1)] + [1, (1 << 50) - 1]
    out = []
    for U in Us:
        for t in (0, (1 << 52) + 12345, (3 << 50) - 1, 0x0123456789ABCD):
            out.append(window(U, t, rest=(M64, 0, M64), low=0x7FF))
    for t in ts:
        for U in (0, 1 << 127, (1 << 128) - 1, 0x9E3779B97F4A7C15F39CC0605CEDC834, (1 << 64) - 1, 1 << 64, 0xB504F333F9DE6484 << 64,
                  (0xB504F333F9DE6484 << 64) + (1 << 75)):
            out.append(window(U, t, rest=(0, M64, 0)))
    return np.array(out, np.uint64)


def random_windows(count, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (count, 6), dtype=np.uint64)


def check_against_reference(words, sigma):
    got = gauss(words, sigma)
    want = np.rint(float(sigma) * z_reference(words))
    worst = np.abs(got - want).max()
    assert worst <= 1 + sigma * 2.0 ** -44, (sigma, worst)
    return got


# ---- formula -----------------------------------------------------------------------------------------------------------------------
def test_formula_on_random_windows():
    check_against_reference(random_windows(1 << 16, 2024), 1 << 30)


def test_formula_on_planted_windows():
    words = planted_windows()
    for sigma in (1 << 30, 1 << 10, Q):
        got = check_against_reference(words, sigma)
        assert np.abs(got).max() <= 13.4 * sigma
    # the tail is reached: U = 0 at angle 0 is sqrt(2 128 ln 2) sigma, and u1 next to 1 is next to nothing
    top = gauss(np.array([window(0, 0)], np.uint64), 1 << 30)[0]
    assert abs(top - math.sqrt(256 * math.log(2)) * (1 << 30)) <= 1 + 2.0 ** -14
    assert gauss(np.array([window((1 << 128) - 1, 0)], np.uint64), 1 << 30)[0] == 16
    # words 3 .. 5 and the low eleven bits of word 2 are not read
    base = random_windows(64, 7)
    other = base.copy()
    other[:, 3:] = random_windows(64, 8)[:, 3:]
    other[:, 2] ^= np.uint64(0x7FF)
    assert np.array_equal(gauss(base, 1 << 30), gauss(other, 1 << 30))


def test_relative_accuracy_of_z():
    """z to 2^-46 relative against the closed formula in extended precision (np.longdouble: 64 mantissa bits on x86-64), read off
    at sigma = q, where one unit of the result is 2^-46 of sigma (so the rounding to an integer costs half a unit on top)."""
    assert np.finfo(np.longdouble).nmant >= 63
    words = np.concatenate([random_windows(1 << 14, 99), planted_windows()])
    ld = np.longdouble
    f = np.empty(len(words), ld)
    e = np.empty(len(words), np.int64)
    for i, (w0, w1) in enumerate(zip(words[:, 0].tolist(), words[:, 1].tolist())):
        U = ((w0 << 64) | w1) or 1
        e[i] = 128 - U.bit_length()
        f[i] = ld((U << int(e[i])) >> 75) / ld(1 << 52)
    ln2 = np.log(ld(2))
    r = np.sqrt(-2 * (np.log1p(f / 2 - 1) - e.astype(ld) * ln2))        # ln f - (e + 1) ln 2 = ln(f / 2) - e ln 2, f / 2 - 1 exact
    t = (words[:, 2] >> np.uint64(11)).astype(ld)
    pi = ld("3.14159265358979323846264338327950288")
    z = r * np.cos(2 * pi * t / ld(1 << 53))
    got = gauss(words, Q).astype(ld)
    err = np.abs(got - Q * z)
    print("largest error beyond the rounding, in units of 2^-46 |z|:", float(((err - 0.5) / np.maximum(np.abs(z) * Q * 2.0 ** -46, 1e-300)).max()))
    assert (err <= 0.5 + 2.0 ** -46 * np.abs(Q * z)).all()


# ---- distribution ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_draw():
    n, sigma = 1 << 20, 1 << 20
    return n, sigma, gauss(random_windows(n, 20261018), sigma).astype(np.float64)


def test_moments(big_draw):
    n, sigma, x = big_draw
    assert abs(x.mean()) <= 5 * sigma / math.sqrt(n)
    c = x - x.mean()
    var = (c ** 2).mean()
    assert abs(var / sigma ** 2 - 1) <= 5 * math.sqrt(2 / n), var / sigma ** 2
    kurt = (c ** 4).mean() / var ** 2 - 3
    assert abs(kurt) <= 5 * math.sqrt(24 / n), kurt          # (Irwin-Hall(12): -0.1, about twenty standard errors out)


def test_chi_square_over_equiprobable_bins(big_draw):
    from scipy import stats
    n, sigma, x = big_draw
    edges = stats.norm.ppf(np.arange(1, 64) / 64.0)
    counts = np.bincount(np.searchsorted(edges, x / sigma), minlength=64)
    chi2 = ((counts - n / 64.0) ** 2 / (n / 64.0)).sum()
    assert counts.sum() == n and chi2 < stats.chi2.isf(1e-6, 63), chi2


def test_tail_beyond_four_sigma(big_draw):
    n, sigma, x = big_draw
    want = n * math.erfc(4 / math.sqrt(2))
    got = int((np.abs(x) > 4 * sigma).sum())
    assert abs(got - want) <= 5 * math.sqrt(want), (got, want)


@pytest.mark.parametrize("sigma", [1, 2, 3])
def test_small_sigma_follows_the_rounded_gaussian_pmf(sigma):
    """chi-square against P(k) = Phi((k + 1/2) / sigma) - Phi((k - 1/2) / sigma) on the integers of +- 4 sigma, the two tails beyond
    them pooled into the outermost integers (their own expected counts are too small for the statistic)"""
    from scipy import stats
    n, lim = 1 << 18, 4 * sigma
    x = gauss(random_windows(n, 1000 + sigma), sigma)
    ks = np.arange(-lim, lim + 1)
    upper = stats.norm.cdf((ks + 0.5) / sigma)
    upper[-1] = 1.0
    pmf = np.diff(np.concatenate([[0.0], upper]))
    counts = np.bincount(np.clip(x, -lim, lim) + lim, minlength=2 * lim + 1)
    assert (pmf * n > 10).all()
    chi2 = ((counts - n * pmf) ** 2 / (n * pmf)).sum()
    assert chi2 < stats.chi2.isf(1e-6, 2 * lim), (sigma, chi2)
    assert np.abs(x).max() <= 13.4 * sigma


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def toy(**kw):
    from tfhe_fbs_map_amd import Params
    return Params(**dict(dict(n=8, log_n_poly=8, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=1 << 10), **kw))


def test_unknown_sampler_is_refused_by_both_libraries_with_one_text():
    import ctypes as C
    from tfhe_fbs_map_amd import Context, FbsError, HostContext, _client_native, _native
    texts = []
    for make in (lambda p: HostContext(p, seed=1), lambda p: HostContext(p, seed=bytes(32)), lambda p: Context(p, seed=1)):
        for bad in (2, 3, 0xFFFFFFFF):
            with pytest.raises(FbsError) as e:
                make(toy(sampler=bad))
            assert e.value.code == -1
            texts.append(str(e.value))
    assert len(set(texts)) == 1 and "sampler is 0 (Irwin-Hall) or 1 (rounded Gaussian)" in texts[0]
    # the field sits where `reserved` sat: the layout did not move
    assert C.sizeof(_client_native._Params) == 56 and _client_native._Params.sampler.offset == 52 and _native._Params is _client_native._Params
    assert toy().sampler == 0 and toy().to_c().sampler == 0 and toy(sampler=1).to_c().sampler == 1
    HostContext(toy(sampler=1), seed=1).close()
    with pytest.raises(FbsError) as e:                                   # sigma up to q under the Gaussian
        HostContext(toy(sampler=1, sigma_glwe=Q + 1), seed=1)
    assert e.value.code == -1


def test_sampler_one_shares_no_key_material_with_its_twin():
    from tfhe_fbs_map_amd import HostContext
    raw = bytes(range(32))
    keys = {}
    for s in (0, 1):
        ctx = HostContext(toy(sampler=s), seed=raw)
        ctx.keygen_seeded()
        keys[s] = dict(ctx.export_keys(), **ctx.export_seeded_keys())
    for name in ("sk_lwe", "sk_glwe", "bsk_bodies", "ksk_bodies"):
        assert not np.array_equal(keys[0][name], keys[1][name]), name
    assert keys[0]["mask_key"] != keys[1]["mask_key"]
    # the reproducible form keeps its secrets (the oracle is keyed identically) and changes every noisy word
    rep = {s: HostContext(toy(sampler=s), seed=9, keygen=True).export_keys() for s in (0, 1)}
    assert np.array_equal(rep[0]["sk_lwe"], rep[1]["sk_lwe"]) and np.array_equal(rep[0]["sk_glwe"], rep[1]["sk_glwe"])
    assert not np.array_equal(rep[0]["ksk"], rep[1]["ksk"]) and not np.array_equal(rep[0]["bsk"], rep[1]["bsk"])


def test_sampler_zero_did_not_move():
    """a context that names sampler 0 is the context of before: the oracle's keys and ciphertexts, word for word"""
    from oracle import tfhe_oracle as orc
    from tfhe_fbs_map_amd import HostContext
    prm = toy()
    mine, theirs = HostContext(prm, seed=9, keygen=True), orc.Oracle(prm, seed=9)
    for k, v in mine.export_keys().items():
        assert np.array_equal(v, theirs.keys()[k]), k
    msgs = np.arange(20) % 14
    assert np.array_equal(mine.encrypt(msgs, 77), theirs.encrypt(msgs, 77))


def seed_key(seed):
    """the ChaCha20 key of the reproducible form (fbs_ctx_create): the seed, then the fixed tail"""
    return struct.pack("<II", seed & 0xFFFFFFFF, seed >> 32) + b"fbs-exec-amd-gfx950-key1"


def centred(v):
    v = np.asarray(v, np.int64) % Q
    return np.where(v > Q // 2, v - Q, v)


@pytest.mark.parametrize("k", [1, 2])
def test_context_draws_are_the_sampler_on_the_stream_words(k):
    """Under sampler 1 the noise of a key-switching row, of a full encryption and of a seeded encryption is gauss_sample of words
    0 .. 5 of its stream -- the window Irwin-Hall read -- and under sigma 0 nothing is drawn."""
    from tfhe_fbs_map_amd import HostContext
    glwe = dict(k=2, l_bsk=1, beta_bsk=21, bsk_group=2, sigma_glwe=1 << 12) if k == 2 else {}
    prm = toy(sampler=1, **glwe)
    ctx = HostContext(prm, seed=5)
    ctx.keygen_seeded()
    keys, key = ctx.export_keys(), seed_key(5)
    s_big, s_small = keys["sk_glwe"].astype(np.int64), keys["sk_lwe"].astype(np.int64)
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    msgs = np.arange(40) % (2 * prm.p_msg)

    def noise(domain, first, count, sigma):
        streams = (domain << 56) + first + np.arange(count, dtype=np.uint64)
        return gauss(chacha_rows(key, streams, 6), sigma)

    cts = ctx.encrypt(msgs, 300).astype(np.int64)
    masks = fold(chacha_rows(key, (DOM_ENC_MASK << 56) + 300 + np.arange(40, dtype=np.uint64), prm.big_dim)).astype(np.int64)
    assert np.array_equal(cts[:, :-1], masks)
    phase = centred(cts[:, -1] - (masks * s_big[None, :] % Q).sum(axis=1) - msgs * delta)
    want = noise(DOM_ENC_NOISE, 300, 40, prm.sigma_glwe)
    assert np.array_equal(phase, want) and np.abs(want).max() > 0
    bodies, _ = ctx.encrypt_seeded(msgs, nonce0=900)
    full = ctx.expand_seeded(bodies, 900).astype(np.int64)
    sphase = centred(full[:, -1] - (full[:, :-1] * s_big[None, :] % Q).sum(axis=1) - msgs * delta)
    assert np.array_equal(sphase, noise(DOM_SENC_NOISE, 900, 40, prm.sigma_glwe))
    # the key-switching key of fbs_keygen: row (j, v) = mask, mask . sk_lwe + sk_glwe[j] h_v + e
    full_ctx = HostContext(prm, seed=5, keygen=True)
    ksk = full_ctx.export_keys()["ksk"].astype(np.int64).reshape(-1, prm.n + 1)
    h = np.array([(Q + (1 << (prm.gamma_ksk * (v + 1) - 1))) >> (prm.gamma_ksk * (v + 1)) for v in range(prm.t_ksk)], np.int64)
    kphase = centred(ksk[:, -1] - (ksk[:, :-1] * s_small[None, :]).sum(axis=1) - (s_big[:, None] * h[None, :]).reshape(-1))
    assert np.array_equal(kphase, noise(DOM_KSK_NOISE, 0, len(ksk), prm.sigma_lwe))
    # sigma 0: no draw
    assert (gauss(random_windows(100, 3), 0) == 0).all()
    quiet = HostContext(prm.replace(sigma_glwe=0, sigma_lwe=0), seed=5, keygen=True)
    qc = quiet.encrypt(msgs, 300).astype(np.int64)
    sq = quiet.export_keys()["sk_glwe"].astype(np.int64)
    assert (centred(qc[:, -1] - (qc[:, :-1] * sq[None, :] % Q).sum(axis=1) - msgs * delta) == 0).all()


def test_bootstrapping_key_noise_has_unit_variance_ratio():
    """the bodies of a sampler-1 bootstrapping key at sigma_glwe = 2^20: phase minus message over sigma, 2 l N n draws"""
    from tfhe_fbs_map_amd import HostContext
    prm = toy(sampler=1, n=16, sigma_glwe=1 << 20)
    ctx = HostContext(prm, seed=11)
    ctx.keygen_seeded()
    keys = ctx.export_keys()
    N, rows = prm.N, 2 * prm.l_bsk
    bsk = keys["bsk"].astype(np.int64).reshape(prm.n * rows, 2, N)
    S = negacyclic_matrix(keys["sk_glwe"].astype(np.int64))
    phase = (bsk[:, 1] - (bsk[:, 0] @ S) % Q) % Q
    sk, sg = keys["sk_lwe"].astype(np.int64), keys["sk_glwe"].astype(np.int64)
    for r in range(prm.n * rows):
        g, comp, lv = r // rows, (r % rows) // prm.l_bsk, r % prm.l_bsk
        g_lv = (Q + (1 << (prm.beta_bsk * (lv + 1) - 1))) >> (prm.beta_bsk * (lv + 1))
        if sk[g]:
            phase[r] = (phase[r] - (g_lv * (np.arange(N) == 0) if comp == 1 else -g_lv * sg)) % Q
    e = centred(phase).astype(np.float64).reshape(-1)
    n = e.size
    assert abs((e ** 2).mean() / float(prm.sigma_glwe) ** 2 - 1) <= 5 * math.sqrt(2 / n)
    assert abs(e.mean()) <= 5 * prm.sigma_glwe / math.sqrt(n)


def test_config_and_selector_carry_the_sampler():
    from tfhe_fbs_map_amd import ExecConfig, choose_params, params_for
    assert ExecConfig().sampler == "irwin_hall" and ExecConfig().params_choice(7, 4).sampler == 0
    a, b = ExecConfig().params_choice(7, 4), ExecConfig(sampler="gaussian").params_choice(7, 4)
    assert b.sampler == 1 and b.replace(sampler=0) == a
    assert choose_params(7, 4, glwe_dims=(1, 2, 3), sampler=1) == b and choose_params(7, 4, glwe_dims=(1, 2, 3)) == a
    assert ExecConfig(sampler=1, reduced_noise=True).params_choice(7).sampler == 1
    assert ExecConfig(reduced_noise=True).params_choice(7) == params_for(7)
    assert ExecConfig(sampler="gaussian", params=toy()).params_choice(7).sampler == 1
    assert ExecConfig(params=toy(sampler=1)).params_choice(7).sampler == 1          # explicit params keep their own
    with pytest.raises(ValueError):
        ExecConfig(sampler="normal").params_choice(7)


def test_server_key_file_stores_the_sampler(tmp_path):
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, ServerKey, parse_fbs
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    files = {}
    for name in ("irwin_hall", "gaussian"):
        cfg = ExecConfig(seed=5, sampler=name, params=toy(n=8))
        client = Client(env, cfg, host=True)
        path = str(tmp_path / (name + ".npz"))
        client.server_key().save(path)
        back = ServerKey.load(path)
        assert back.params == client.params and back.params.sampler == client.params.sampler == (name == "gaussian")
        assert np.array_equal(back.bsk_bodies, client.server_key().bsk_bodies)
        with np.load(path) as z:
            files[name] = {k: z[k] for k in z.files}
    assert "sampler" not in files["irwin_hall"] and int(files["gaussian"]["sampler"]) == 1
    assert len(files["gaussian"]["params"]) == len(files["irwin_hall"]["params"]) == 11
    # a file without the field -- every file written before it existed -- is a sampler-0 key
    stripped = {k: v for k, v in files["gaussian"].items() if k != "sampler"}
    old = str(tmp_path / "old.npz")
    np.savez(old, **stripped)
    assert ServerKey.load(old).params.sampler == 0


def test_client_build_needs_no_gpu_toolchain_and_exports_no_debug_entry():
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "client"], capture_output=True, text=True, check=True).stdout
    assert "hipcc" not in out and "rocm" not in out.lower()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("fbs_sampler.hpp") == 2                              # a dependency of both libraries
    from tfhe_fbs_map_amd import _client_native, _native
    assert "fbs_debug_gauss" in _native.EXPORTED_SYMBOLS and "fbs_debug_gauss_dev" in _native.EXPORTED_SYMBOLS
    assert not [s for s in _client_native.EXPORTED_SYMBOLS if "gauss" in s]


def test_debug_entry_refusals():
    from tfhe_fbs_map_amd import FbsError, _native
    lib = _native.lib
    w = random_windows(4, 1)
    out = np.zeros(4, np.int64)
    assert lib.fbs_debug_gauss(None, w.ctypes.data, 4, Q + 1, out.ctypes.data) == -1 and "sigma above q" in lib.fbs_last_error(None).decode()
    assert lib.fbs_debug_gauss(None, None, 4, 1, out.ctypes.data) == -1 and lib.fbs_debug_gauss(None, w.ctypes.data, 4, 1, None) == -1
    assert lib.fbs_debug_gauss(None, None, 0, 1, None) == 0
    assert lib.fbs_debug_gauss(None, w.ctypes.data, (1 << 26) + 1, 1, out.ctypes.data) == -1
    assert lib.fbs_debug_gauss_dev(None, None, 0, 1, None, None) == -1
    with pytest.raises(FbsError):
        _native.debug_gauss(w, Q + 1)
    assert gauss(w, Q).shape == (4,)
