"""The client library without a GPU: libfbsclient.so is host code built with the C++ compiler alone, exports exactly the client's
subset of include/fbs_exec.h, makes the keys and ciphertexts the CPU oracle makes, closes the seeded path on the host, decodes compact
and packed outputs, refuses what libfbsexec.so refuses -- and the package imports and keys a `split.Client` where libfbsexec.so does
not exist at all."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import load_fixture, subsample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tfhe_fbs_map_amd")
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libfbsclient.so")
Q = (1 << 46) - 62 * (1 << 13) + 1
E_INVALID, E_DEVICE, E_STATE, E_POLY_SIZE, E_NOMEM = -1, -2, -3, -5, -6

# the client's subset of include/fbs_exec.h ("client library")
CLIENT_ENTRIES = """
    fbs_poly_size_check fbs_ctx_create fbs_ctx_create_seeded fbs_ctx_destroy fbs_ctx_stat fbs_last_error fbs_device_info
    fbs_keygen fbs_key_sizes fbs_export_keys
    fbs_keygen_seeded fbs_seeded_key_sizes fbs_export_seeded_keys
    fbs_encrypt fbs_encrypt_fresh fbs_decrypt
    fbs_encrypt_seeded fbs_encrypt_seeded_fresh fbs_expand_seeded
    fbs_compact_words fbs_decrypt_compact
    fbs_packing_keygen fbs_packing_key_sizes fbs_export_packing_key fbs_packed_words fbs_decrypt_packed
    fbs_debug_raise
""".split()


@pytest.fixture(scope="module", autouse=True)
def client_library():
    subprocess.check_call(["make", "-s", "-C", CSRC, "client"], timeout=600)
    return LIB


def toy_sets():
    """the toy sets the parity tests key: k = 1 at N = 256 and N = 1024, k = 2 and k = 3 with two key bits per step at their
    smallest N"""
    from tfhe_fbs_map_amd import Params
    k1 = Params(n=12, log_n_poly=10, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=1 << 8)
    glwe = dict(n=12, log_n_poly=8, l_bsk=1, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=4, bsk_group=2)
    return {"k1_N256": k1.replace(log_n_poly=8), "k1_N1024": k1, "k2_N256_g2": Params(k=2, beta_bsk=21, **glwe),
            "k3_N256_g2": Params(k=3, beta_bsk=18, **glwe)}


SETS = ["k1_N256", "k1_N1024", "k2_N256_g2", "k3_N256_g2"]


# ---- 1. build hygiene ----------------------------------------------------------------------------------------------------------
def test_client_target_uses_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "client"], capture_output=True, text=True, check=True).stdout
    assert "fbs_client_entries.cpp" in out and "fbs_client_capi.cpp" in out and "libfbsclient.so" in out
    assert "hipcc" not in out and "rocm" not in out.lower(), out
    assert "__HIP_PLATFORM_AMD__" not in out
    for flag in ("-std=c++17", "-O3", "-fPIC", "-pthread", "-ffp-contract=off"):
        assert flag in out, flag
    for src in ("fbs_plan.cpp", "fbs_select.cpp", "fbs_capi.cpp", "fbs_eval.cpp", ".hip"):
        assert src not in out, src


def test_client_library_needs_no_gpu_runtime():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert needed, dyn
    for lib in needed:
        assert not re.search(r"hip|hsa|roc|amd", lib, re.I), lib
    undefined = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for line in undefined.splitlines():
        name = line.split()[-1]
        assert not name.startswith(("hip", "__hip", "hsa")), name


def test_client_library_exports_exactly_the_client_entries():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _client_native
    defined = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in defined.splitlines() if ln.split()[-1].startswith("fbs_"))
    assert exported == sorted(CLIENT_ENTRIES)
    assert sorted(_client_native.EXPORTED_SYMBOLS) == sorted(CLIENT_ENTRIES)
    assert set(CLIENT_ENTRIES) <= set(declared_symbols())            # a subset of the header, nothing of its own
    text = open(os.path.join(ROOT, "include", "fbs_exec.h")).read()
    assert "#define FBS_DEVICE_NONE (-1)" in text and "client library" in text


def test_every_client_entry_is_an_exception_barrier():
    body = ""   # the entries both libraries are built from, then the client library's own
    for name in ("fbs_client_entries.cpp", "fbs_client_capi.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        body += text[text.index('extern "C" {'):]
    seen = []
    for m in re.finditer(r"^(?:int|void|double|const char \*) ?(fbs_\w+)\(([^{};]*?)\) (try )?\{", body, flags=re.M):
        seen.append(m.group(1))
        if m.group(1) in ("fbs_last_error", "fbs_device_info"):      # accessors of an existing string: nothing can throw
            continue
        assert m.group(3), "%s has no function-try-block" % m.group(1)
    assert sorted(seen) == sorted(CLIENT_ENTRIES)


def test_client_module_imports_neither_torch_nor_the_gpu_binding():
    """(what the process loads where the GPU library is absent is checked below, in a child of its own)"""
    src = open(os.path.join(PKG, "_client_native.py")).read()
    imports = re.findall(r"^\s*(?:from\s+(\S+)\s+import|import\s+(\S+))", src, flags=re.M)
    names = {a or b for a, b in imports}
    assert names == {"__future__", "ctypes", "os", "sys", "types", "dataclasses", "numpy", ".security"}, names
    assert "libfbsexec.so" in src and "CDLL(LIB_PATH)" in src and "libfbsclient.so" in src


# ---- 2. against the oracle, without a GPU --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keyed():
    """name -> (parameter set, HostContext after keygen(), its exported keys), made once"""
    from tfhe_fbs_map_amd import HostContext
    out = {}
    for name, prm in toy_sets().items():
        ctx = HostContext(prm, seed=9, keygen=True)
        out[name] = (prm, ctx, ctx.export_keys())
    return out


@pytest.mark.parametrize("name", SETS)
def test_keys_and_encryption_identical_to_oracle(keyed, name):
    prm, ctx, mine = keyed[name]
    o = orc.Oracle(prm, seed=9)
    theirs = o.keys()
    assert set(mine) == {"sk_lwe", "sk_glwe", "bsk", "ksk"}
    for k in mine:
        assert np.array_equal(mine[k], theirs[k]), k
    msgs = np.arange(20) % (2 * prm.p_msg)
    assert np.array_equal(ctx.encrypt(msgs, 77), o.encrypt(msgs, 77))
    assert np.array_equal(ctx.decrypt(o.encrypt(msgs, 5)), msgs)
    assert ctx.stat("has_secret") == 1 and ctx.stat("seeded_keys") == 0


def test_byte_seed_keys_depend_on_the_parameter_set():
    from tfhe_fbs_map_amd import HostContext
    sets = toy_sets()
    raw = bytes(range(32))
    a, b = HostContext(sets["k1_N256"], seed=raw, keygen=True), HostContext(sets["k1_N256"], seed=raw, keygen=True)
    c = HostContext(sets["k1_N256"].replace(p_msg=15), seed=raw, keygen=True)
    ka, kb, kc = a.export_keys(), b.export_keys(), c.export_keys()
    assert all(np.array_equal(ka[k], kb[k]) for k in ka)
    assert not np.array_equal(ka["sk_glwe"], kc["sk_glwe"])
    with pytest.raises(ValueError):
        HostContext(sets["k1_N256"], seed=b"short")


# ---- 3. the seeded path closed on the host -------------------------------------------------------------------------------------
def _rol(v, s):
    return (v << np.uint32(s)) | (v >> np.uint32(32 - s))


def chacha_rows(key_bytes, streams, count):
    """words 0 .. count-1 of each ChaCha20 stream of `streams` under the 32-byte key -> [len(streams)][count]: the original
    64-bit-counter layout, words 12-13 the block counter, words 14-15 the stream id; each block 8 little-endian 64-bit words
    ("Randomness")"""
    key = np.frombuffer(bytes(key_bytes), "<u4")
    streams = np.asarray(streams, np.uint64)
    blocks = (count + 7) // 8
    ctr, sid = [a.reshape(-1) for a in np.meshgrid(np.arange(blocks, dtype=np.uint64), streams)]      # stream-major
    x0 = np.empty((16, ctr.size), np.uint32)
    x0[0:4] = np.array([0x61707865, 0x3320646e, 0x79622d32, 0x6b206574], np.uint32)[:, None]
    x0[4:12] = key[:, None]
    x0[12], x0[13] = ctr.astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32)
    x0[14], x0[15] = sid.astype(np.uint32), (sid >> np.uint64(32)).astype(np.uint32)
    x = x0.copy()

    def quarter(a, b, c, d):
        x[a] += x[b]; x[d] = _rol(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rol(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rol(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rol(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
            quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
        x += x0
    words = x[0::2].astype(np.uint64) | (x[1::2].astype(np.uint64) << np.uint64(32))      # [8][streams * blocks]
    return words.T.reshape(len(streams), blocks * 8)[:, :count]


def fold(words):
    """a uniform residue from a random word: its top 46 bits, folded once"""
    r = words >> np.uint64(18)
    return np.where(r >= Q, r - np.uint64(Q), r)


def negacyclic_matrix(s):
    """M with (a @ M)[j] = (a * S)_j in Z[X]/(X^N + 1) for the binary polynomial S: entries in {-1, 0, 1}"""
    N = len(s)
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return np.where(j >= i, 1, -1) * np.asarray(s, np.int64)[(j - i) % N]


def centred(v):
    v = np.asarray(v, np.int64) % Q
    return np.where(v > Q // 2, v - Q, v)


DOM_SBSK_MASK, DOM_SKSK_MASK = 10, 12


@pytest.fixture(scope="module")
def seeded():
    """name -> (parameter set, HostContext after keygen_seeded(), the server key it exports, its secrets)"""
    from tfhe_fbs_map_amd import HostContext
    out = {}
    for name, prm in toy_sets().items():
        ctx = HostContext(prm, seed=9)
        ctx.keygen_seeded()
        full = ctx.export_keys()
        out[name] = (prm, ctx, ctx.export_seeded_keys(), full)
    return out


@pytest.mark.parametrize("name", SETS)
def test_seeded_inputs_round_trip_on_the_host(seeded, name):
    prm, ctx, _, _ = seeded[name]
    msgs = np.arange(3 * 2 * prm.p_msg).reshape(3, -1) % (2 * prm.p_msg)              # every message of [0, 2p)
    bodies, first = ctx.encrypt_seeded(msgs, nonce0=41)
    assert first == 41 and bodies.shape == msgs.shape and bodies.dtype == np.uint64 and (bodies < Q).all()
    cts = ctx.expand_seeded(bodies, 41)
    assert cts.shape == msgs.shape + (prm.ct_words,) and np.array_equal(cts[..., -1], bodies)
    assert np.array_equal(ctx.decrypt(cts), msgs)
    fresh, at = ctx.encrypt_seeded(msgs)
    assert at >= 1 << 55 and np.array_equal(ctx.decrypt(ctx.expand_seeded(fresh, at)), msgs)


@pytest.mark.parametrize("name", SETS)
def test_seeded_key_rows_decrypt_under_the_exported_mask_key(seeded, name):
    """The server's view restated in numpy: masks regenerated from the exported mask key and the bodies alone give rows whose
    phases under the secrets are the GGSW and key-switching messages of the fbs_key_sizes layout, within the sampler's 6 sigma."""
    prm, ctx, key, full = seeded[name]
    n, N, k, l, t = prm.n, prm.N, prm.k, prm.l_bsk, prm.t_ksk
    sk_lwe, sk_glwe = full["sk_lwe"].astype(np.int64), full["sk_glwe"].astype(np.int64).reshape(k, N)
    G = n // 2 * 3 if prm.bsk_group == 2 else n
    rows = (k + 1) * l
    assert ctx.seeded_key_sizes() == (G * rows * N, k * N * t) == (key["bsk_bodies"].size, key["ksk_bodies"].size)
    assert len(key["mask_key"]) == 32 and ctx.stat("seeded_keys") == 1
    # the full keys the context holds are the expansion of what it exports
    bodies = key["bsk_bodies"].reshape(G * rows, N)
    masks = fold(chacha_rows(key["mask_key"], (DOM_SBSK_MASK << 56) + np.arange(G * rows, dtype=np.uint64), k * N))
    bsk = full["bsk"].reshape(G * rows, k + 1, N)
    assert np.array_equal(bsk[:, :k].reshape(G * rows, k * N), masks) and np.array_equal(bsk[:, k], bodies)
    # phases of the bootstrapping key: bit g_lv at X^0 on the body row, -bit g_lv S_comp on a mask row
    phase = bodies.astype(np.int64)
    for c in range(k):
        phase = (phase - (masks[:, c * N:(c + 1) * N].astype(np.int64) @ negacyclic_matrix(sk_glwe[c])) % Q) % Q
    tol = 6 * prm.sigma_glwe + 1
    for r in range(G * rows):
        g, comp, lv = r // rows, (r % rows) // l, r % l
        if prm.bsk_group == 2:
            s0, s1 = sk_lwe[2 * (g // 3)], sk_lwe[2 * (g // 3) + 1]
            bit = (s0 & (1 - s1), (1 - s0) & s1, s0 & s1)[g % 3]
        else:
            bit = sk_lwe[g]
        g_lv = (Q + (1 << (prm.beta_bsk * (lv + 1) - 1))) >> (prm.beta_bsk * (lv + 1))
        want = np.zeros(N, np.int64)
        if bit and comp == k:
            want[0] = g_lv
        elif bit:
            want = -g_lv * sk_glwe[comp]
        assert np.abs(centred(phase[r] - want)).max() <= tol, (r, g, comp, lv)
    # ... and of the key-switching key: row (j, v) encrypts sk_glwe[j] h_v under sk_lwe
    kb = key["ksk_bodies"].astype(np.int64)
    kmask = fold(chacha_rows(key["mask_key"], (DOM_SKSK_MASK << 56) + np.arange(k * N * t, dtype=np.uint64), n)).astype(np.int64)
    assert np.array_equal(full["ksk"].reshape(-1, n + 1)[:, :n], kmask.astype(np.uint64))
    h = np.array([(Q + (1 << (prm.gamma_ksk * (v + 1) - 1))) >> (prm.gamma_ksk * (v + 1)) for v in range(t)], np.int64)
    want = sk_glwe.reshape(-1)[:, None] * h[None, :]
    kphase = (kb - (kmask * sk_lwe[None, :]).sum(axis=1) % Q) % Q
    assert np.abs(centred(kphase.reshape(k * N, t) - want)).max() <= 6 * prm.sigma_lwe + 1


def test_fresh_nonces_follow_the_header_rule():
    from tfhe_fbs_map_amd import FbsError, HostContext
    ctx = HostContext(toy_sets()["k1_N256"], seed=3)
    ctx.keygen_seeded()
    assert ctx.stat("next_nonce") == 1 << 55
    msgs = np.arange(5) % 2
    _, a = ctx.encrypt_seeded(msgs)
    assert a == 1 << 55 and ctx.stat("next_nonce") == (1 << 55) + 5
    ctx.encrypt(np.arange(7) % 2)                                                    # the full entry draws from the same counter
    assert ctx.stat("next_nonce") == (1 << 55) + 12
    _, b = ctx.encrypt_seeded(msgs)
    assert b == (1 << 55) + 12 and b >= a + 5                                          # two fresh calls never overlap
    for call in (lambda: ctx.encrypt_seeded(msgs, nonce0=1 << 55), lambda: ctx.encrypt(msgs, nonce0=1 << 55),
                 lambda: ctx.encrypt_seeded(msgs, nonce0=(1 << 55) - 2), lambda: ctx.encrypt(msgs, nonce0=(1 << 60))):
        with pytest.raises(FbsError) as e:
            call()
        assert e.value.code == E_INVALID and "2^55" in str(e.value)
    assert ctx.stat("next_nonce") == (1 << 55) + 17                                  # a refused call moves no counter
    # explicit nonces just below the bound are served, and expansion reads fresh streams too
    bodies, _ = ctx.encrypt_seeded(msgs, nonce0=(1 << 55) - 5)
    assert np.array_equal(ctx.decrypt(ctx.expand_seeded(bodies, (1 << 55) - 5)), msgs)


# ---- 4. compact and packed decoders ----------------------------------------------------------------------------------------------
def pack_fields(fields, bits):
    """fields [..][F] below 2^bits -> words [..][ceil(F bits / 64)]: field j at bits [j bits, j bits + bits) of the bit stream,
    stream bit b = bit b mod 64 of word b / 64, zero padding"""
    fields = np.asarray(fields, np.uint64)
    F = fields.shape[-1]
    W = (F * bits + 63) // 64
    flat = fields.reshape(-1, F)
    out = [[0] * W for _ in range(flat.shape[0])]
    for r, row in enumerate(flat):
        stream = 0
        for j, f in enumerate(row):
            stream |= int(f) << (j * bits)
        for w in range(W):
            out[r][w] = (stream >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return np.array(out, np.uint64).reshape(fields.shape[:-1] + (W,))


def compact_from_small_key_cts(x, bits):
    """the header's rounding of small-key ciphertexts x [count][n + 1] over Z_q to width `bits`, q treated as 2^46"""
    sh = 46 - bits
    x = np.asarray(x, np.int64)
    m = ((x[:, :-1] >> (sh - 1)) + 1) >> 1
    eps = (x[:, :-1] - (m << sh)).sum(axis=1)
    body = (x[:, -1] - (eps >> 1)) % Q                                                # (>> floors)
    m_n = ((body >> (sh - 1)) + 1) >> 1
    return np.concatenate([m, m_n[:, None]], axis=1) & ((1 << bits) - 1)


@pytest.mark.parametrize("name", ["k1_N256", "k3_N256_g2"])
def test_decrypt_compact_reads_words_built_from_the_header_formulas(keyed, name):
    prm, ctx, keys = keyed[name]
    rng = np.random.default_rng(5)
    n, two_p = prm.n, 2 * prm.p_msg
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    msgs = np.arange(3 * two_p).reshape(3, two_p) % two_p
    s = keys["sk_lwe"].astype(np.int64)
    a = rng.integers(0, Q, (msgs.size, n), dtype=np.int64)
    e = rng.integers(-prm.sigma_lwe, prm.sigma_lwe + 1, msgs.size)
    body = ((a * s).sum(axis=1) + msgs.reshape(-1) * delta + e) % Q
    x = np.concatenate([a, body[:, None]], axis=1)
    for bits in (prm.log_n_poly + 1, 31):
        words = pack_fields(compact_from_small_key_cts(x, bits), bits).reshape(msgs.shape + (-1,))
        assert words.shape[-1] == ctx.compact_words(bits) == ((n + 1) * bits + 63) // 64
        assert np.array_equal(ctx.decrypt_compact(words, bits), msgs), bits
    assert np.array_equal(ctx.decrypt_compact(words[:0], 31), np.zeros((0, two_p), np.int64))


@pytest.mark.parametrize("name", ["k1_N256", "k2_N256_g2"])
def test_decrypt_packed_reads_words_built_from_the_header_formulas(keyed, name):
    """GLWE samples under the exported big key, rounded and bit-packed as the header's TRANSPORT says: one full sample and a partly
    filled one.  Widths 16 and 31: at w bits the k N / 2 roundings of a phase add about sqrt(k N / 24) units of 2^-w, far below
    Delta / 2 = 2^w / 4p there (at the narrowest width, log2(2N), that sum is what `params.packed_output_variance` budgets)."""
    prm, ctx, keys = keyed[name]
    rng = np.random.default_rng(6)
    N, k, two_p = prm.N, prm.k, 2 * prm.p_msg
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    count = N + 37
    msgs = rng.integers(0, two_p, count)
    S = keys["sk_glwe"].astype(np.int64).reshape(k, N)
    for bits in (16, 31):
        parts = []
        for g0 in range(0, count, N):
            fill = min(N, count - g0)
            A = rng.integers(0, Q, (k, N), dtype=np.int64)
            B = np.zeros(N, np.int64)
            B[:fill] = msgs[g0:g0 + fill] * delta % Q
            B = (B + rng.integers(-prm.sigma_glwe, prm.sigma_glwe + 1, N)) % Q
            for c in range(k):
                B = (B + (A[c] @ negacyclic_matrix(S[c])) % Q) % Q
            rnd = lambda v: (((v >> (45 - bits)) + 1) >> 1) & ((1 << bits) - 1)      # noqa: E731  (no mean compensation)
            parts.append(pack_fields(np.concatenate([rnd(A).reshape(-1), rnd(B[:fill])]), bits))  # every sample starts on a word boundary
        words = np.concatenate(parts)
        assert words.size == ctx.packed_words(count, bits)
        assert np.array_equal(ctx.decrypt_packed(words, count, bits), msgs), bits
    with pytest.raises(ValueError):
        ctx.decrypt_packed(words[:-1], count, 31)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _raw():
    from tfhe_fbs_map_amd import _client_native
    return _client_native._lib()


def _create(prm, device=-1, seed=1):
    lib, h = _raw(), C.c_void_p()
    cp = prm.to_c()
    rc = lib.fbs_ctx_create(C.byref(cp), seed, device, C.byref(h))
    return rc, h, lib.fbs_last_error(None).decode()


def test_refusals_carry_the_gpu_librarys_codes():
    from tfhe_fbs_map_amd import FbsError, HostContext, Params
    lib = _raw()
    prm = toy_sets()["k1_N256"]
    for device in (0, 1, -2):
        rc, h, text = _create(prm, device=device)
        assert rc == E_DEVICE and not h.value and "libfbsexec" in text, (device, text)
    cp, h = prm.to_c(), C.c_void_p()
    assert lib.fbs_ctx_create_seeded(C.byref(cp), bytes(32), 0, C.byref(h)) == E_DEVICE and not h.value
    assert lib.fbs_ctx_create_seeded(C.byref(cp), None, -1, C.byref(h)) == E_INVALID
    # polynomial sizes: a non-power-of-two has its own code
    for n_poly in (1536, 768, 1000):
        assert lib.fbs_poly_size_check(n_poly) == E_POLY_SIZE and "not a power of two" in lib.fbs_last_error(None).decode()
        with pytest.raises(FbsError) as e:
            Params.for_poly_size(n_poly)
        assert e.value.code == E_POLY_SIZE
    assert lib.fbs_poly_size_check(8192) == E_INVALID and lib.fbs_poly_size_check(0) == E_INVALID and lib.fbs_poly_size_check(2048) == 0
    # parameter sets libfbsexec.so refuses, the shift-overflowing beta among them, before anything is computed from them
    for bad in (prm.replace(beta_bsk=200), prm.replace(l_bsk=5, beta_bsk=7), prm.replace(p_msg=0), prm.replace(log_n_poly=13),
                prm.replace(k=2, log_n_poly=11), prm.replace(k=5), prm.replace(bsk_group=2), prm.replace(bsk_group=2, n=13, log_n_poly=10),
                prm.replace(t_ksk=16, gamma_ksk=2), prm.replace(n=0), prm.replace(gamma_ksk=200)):
        rc, h, text = _create(bad)
        assert rc == E_INVALID and not h.value and text, bad
        with pytest.raises(FbsError) as e:
            HostContext(bad, seed=1)
        assert e.value.code == E_INVALID


def test_calls_out_of_order_and_bad_arguments():
    from tfhe_fbs_map_amd import FbsError, HostContext
    lib = _raw()
    prm = toy_sets()["k1_N256"]
    ctx = HostContext(prm, seed=2)
    msgs = np.arange(4) % 2
    for call in (lambda: ctx.export_seeded_keys(), lambda: ctx.export_keys(), lambda: ctx.encrypt(msgs, 1), lambda: ctx.packing_keygen(2, 7),
                 lambda: ctx.decrypt(np.zeros((1, prm.ct_words), np.uint64)), lambda: ctx.packing_key_sizes()):
        with pytest.raises(FbsError) as e:                                             # no keys yet
            call()
        assert e.value.code == E_STATE
    ctx.keygen()
    for call in (lambda: ctx.export_seeded_keys(), lambda: ctx.packing_keygen(2, 7)):   # full keys are not seeded keys
        with pytest.raises(FbsError) as e:
            call()
        assert e.value.code == E_STATE
    ctx.keygen_seeded()
    ctx.export_seeded_keys()
    for t_p, gamma_p in ((4, 8), (32, 1), (1, 32), (0, 7), (2, 0)):
        with pytest.raises(FbsError) as e:
            ctx.packing_keygen(t_p, gamma_p)
        assert e.value.code == E_INVALID, (t_p, gamma_p)
    assert ctx.stat("packing_key") == 0
    ctx.packing_keygen(2, 7)
    pk = ctx.export_packing_key(full=True)
    assert (ctx.stat("packing_key"), pk["packing_levels"], pk["packing_base_bits"]) == (1, 2, 7)
    assert pk["packing_bodies"].size == prm.n * 2 * prm.N and np.array_equal(pk["full"][:, :, prm.k].reshape(-1), pk["packing_bodies"])
    ctx.keygen_seeded()                                                                # new keys drop the packing key
    assert ctx.stat("packing_key") == 0 and ctx.stat("packing_levels") == 0
    for name in ("cu_count", "scratch_growths", "states_alive", "nonsense"):
        with pytest.raises(FbsError) as e:
            ctx.stat(name)
        assert e.value.code == E_INVALID
    for bits in (prm.log_n_poly, 32, 0):
        with pytest.raises(FbsError) as e:
            ctx.compact_words(bits)
        assert e.value.code == E_INVALID
        with pytest.raises(FbsError) as e:
            ctx.packed_words(10, bits)
        assert e.value.code == E_INVALID
    # the exception barrier: what the header lists for kinds 0 .. 4
    want = {0: (E_NOMEM, "out of host memory"), 1: (E_NOMEM, "out of host memory"), 2: (E_INVALID, "internal error: raised on request"),
            3: (E_INVALID, "unknown internal error"), 4: (0, None)}
    for kind, (code, text) in want.items():
        assert lib.fbs_debug_raise(None, kind) == code, kind
        if text:
            assert text in lib.fbs_last_error(None).decode(), kind
        assert lib.fbs_debug_raise(ctx._h, kind) == code, kind
        if text:
            assert text in lib.fbs_last_error(ctx._h).decode(), kind
    assert np.array_equal(ctx.decrypt(ctx.encrypt(msgs, 3)), msgs)                     # the context is as usable as before
    ctx.close()
    ctx.close()


def test_packing_key_refusals_word_for_word():
    """(call, code, text) of every refusal of the packing-key entries, as the library said them before the packing and fold keys
    were given one code path (tests/test_gpu_fold.py pins the fold key's and the imports' on the GPU library)"""
    from tfhe_fbs_map_amd import FbsError, HostContext
    prm = toy_sets()["k1_N256"]
    ctx = HostContext(prm, seed=2)

    def refused(call, code, text):
        with pytest.raises(FbsError) as e:
            call()
        assert (e.value.code, str(e.value)) == (code, f"libfbsexec error {code}: {text}"), (code, text, str(e.value))

    no_key = "the context has no packing key"
    refused(lambda: ctx.packing_keygen(2, 7), E_STATE, "fbs_keygen has not run")                       # no keys
    refused(lambda: ctx.packing_key_sizes(0), E_STATE, no_key)
    refused(lambda: ctx.export_packing_key(), E_STATE, no_key)
    refused(lambda: ctx.packing_key_sizes(32), E_INVALID, "packing key needs 1 <= t_p <= 31")
    ctx.keygen()                                                                                       # plain keys, not seeded ones
    refused(lambda: ctx.packing_keygen(2, 7), E_STATE, "a packing key goes with seeded keys (fbs_keygen_seeded)")
    ctx.keygen_seeded()
    refused(lambda: ctx.packing_keygen(0, 1), E_INVALID, "packing key needs t_p >= 1 and gamma_p >= 1")
    refused(lambda: ctx.packing_keygen(1, 0), E_INVALID, "packing key needs t_p >= 1 and gamma_p >= 1")
    refused(lambda: ctx.packing_keygen(32, 1), E_INVALID, "packing key needs t_p * gamma_p <= 31")
    refused(lambda: ctx.packing_keygen(4, 8), E_INVALID, "packing key needs t_p * gamma_p <= 31")
    refused(lambda: ctx.packing_key_sizes(0), E_STATE, no_key)                                         # keys, and still no packing key
    refused(lambda: ctx.packing_key_sizes(32), E_INVALID, "packing key needs 1 <= t_p <= 31")
    lib, buf = _raw(), np.zeros(1, np.uint64)
    assert lib.fbs_export_packing_key(ctx._h, buf.ctypes.data, None) == E_STATE
    assert lib.fbs_last_error(ctx._h).decode() == no_key
    assert ctx.packing_key_sizes(31) == (prm.n * 31 * prm.N, prm.n * 31 * prm.N * (prm.k + 1)) and ctx.stat("packing_key") == 0
    ctx.close()


# ---- 6. no GPU library at all -----------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(REPO)]
sys.path.insert(0, HERE)
os.chdir(HERE)
import numpy as np
import tfhe_fbs_map_amd as pkg
from tfhe_fbs_map_amd import Client, ExecConfig, Params, ServerKey, EncryptedInputs, parse_fbs, params_for
assert os.path.dirname(os.path.abspath(pkg.__file__)) == os.path.join(HERE, "tfhe_fbs_map_amd")
assert not os.path.exists(os.path.join(HERE, "tfhe_fbs_map_amd", "libfbsexec.so"))
job = json.load(open(os.path.join(HERE, "job.json")))
env = parse_fbs(job["fbs"], inputs=job["program_inputs"])
assert env.lower()["input_names"] and env.stats()["norm2_linprod"] >= 1 and params_for(7).p_msg == 7
client = Client(env, ExecConfig(seed=5), packing=True)
assert client.host is True and type(client.ctx).__name__ == "HostContext" and client.ctx.device_info == "host"
ins = {k: np.asarray(v) for k, v in job["inputs"].items()}
client.server_key().save(os.path.join(HERE, "server_key.npz"))
enc = client.encrypt(ins)
enc.save(os.path.join(HERE, "inputs.npz"))
key, back = ServerKey.load(os.path.join(HERE, "server_key.npz")), EncryptedInputs.load(os.path.join(HERE, "inputs.npz"))
assert key.params == client.params and key.mask_key == client.server_key().mask_key and key.fingerprint == client.fingerprint
assert np.array_equal(key.bsk_bodies, client.server_key().bsk_bodies) and np.array_equal(key.ksk_bodies, client.server_key().ksk_bodies)
assert key.packing_bodies is not None and np.array_equal(key.packing_bodies, client.server_key().packing_bodies)
assert (key.packing_levels, key.packing_base_bits) == tuple(client.packing[:2])
assert back.T == 8 and back.nonce0 == enc.nonce0 and np.array_equal(back.bodies, enc.bodies) and back.fingerprint == client.fingerprint
bits = np.stack([np.broadcast_to(ins[n], (8,)) for n in back.input_names])
assert np.array_equal(client.ctx.decrypt(client.ctx.expand_seeded(back.bodies, back.nonce0)), bits)
assert "torch" not in sys.modules, "torch was imported"
from tfhe_fbs_map_amd import _native
for touch in (lambda: _native.Context, lambda: pkg.Context, lambda: pkg.Server(key), lambda: env.eval(ins, config=ExecConfig(seed=5))):
    try:
        touch()
    except ImportError as e:
        assert "libfbsexec.so is missing" in str(e) and "no CPU fallback" in str(e), str(e)
    else:
        raise AssertionError("the GPU library was not asked for")
assert _native.Params is Params
print("client ok")
"""


def test_package_imports_and_keys_a_client_without_the_gpu_library(tmp_path):
    dst = tmp_path / "tfhe_fbs_map_amd"
    shutil.copytree(PKG, dst, ignore=shutil.ignore_patterns("libfbsexec.so", "csrc", "__pycache__"))
    assert (dst / "libfbsclient.so").exists() and not (dst / "libfbsexec.so").exists()
    rec = load_fixture("full_adder__search_p7")
    ins, _ = subsample(rec, 8)
    json.dump(dict(fbs=rec["fbs"], program_inputs=rec["program_inputs"], inputs={k: np.asarray(v).tolist() for k, v in ins.items()}),
              open(tmp_path / "job.json", "w"))
    code = "HERE, REPO = %r, %r\n" % (str(tmp_path), ROOT) + CHILD
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "FBS_LIB", "FBS_CLIENT_LIB")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0 and "client ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_neither_library_fails_as_before(tmp_path):
    dst = tmp_path / "tfhe_fbs_map_amd"
    shutil.copytree(PKG, dst, ignore=shutil.ignore_patterns("*.so", "csrc", "__pycache__"))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "try:\n    import tfhe_fbs_map_amd\nexcept ImportError as e:\n    assert 'libfbsexec.so is missing' in str(e) and 'no CPU fallback' in str(e), str(e)\n"
            "else:\n    raise AssertionError('imported')\n" % str(tmp_path))
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "FBS_LIB", "FBS_CLIENT_LIB")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stdout + r.stderr


def test_client_defaults_to_the_gpu_context_where_its_library_is_built():
    from tfhe_fbs_map_amd import _client_native
    from tfhe_fbs_map_amd.split import _host_client
    assert os.path.exists(_client_native.gpu_library_path())          # (this tree is built with both)
    assert _host_client(None) is False and _host_client(True) is True and _host_client(False) is False
