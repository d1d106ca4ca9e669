"""Public-key inputs against an independent restatement (include/fbs_exec.h, "public-key inputs"; DESIGN.md section 2,
"Randomness", for the streams and the derivation of the encryptor's key), in Python integers: the public key's bodies, encrypted
samples, the expansion and the decryption of what it gives, word for word against libfbspublic.so at the toy sets; sampler 1 in
doubles with the formulas of tests/test_sampler.py; and the phase noise against params.public_input_variance."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_client_lib import SETS, negacyclic_matrix, toy_sets
from tests.test_device_io_abi import chacha_block, irwin_hall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
Q = (1 << 46) - 62 * (1 << 13) + 1
M64 = (1 << 64) - 1
DOM_PUB_MASK, DOM_PUB_NOISE, DOM_PUB_ENC_U, DOM_PUB_ENC_NOISE = 18, 19, 20, 21
NOISE_SEED, ENC_SEED = bytes(range(100, 132)), bytes(range(7, 39))


@pytest.fixture(scope="module", autouse=True)
def libraries():
    subprocess.check_call(["make", "-s", "-C", CSRC, "client", "public"], timeout=900)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def key_words(b32):
    return [int.from_bytes(bytes(b32)[4 * i:4 * i + 4], "little") for i in range(8)]


def stream_words(key, domain, sub, first, count):
    """words first .. first + count - 1 of stream (domain, sub): block b holds words 8 b .. 8 b + 7"""
    sid = (domain << 56) | sub
    blocks = {b: chacha_block(key, sid, b) for b in range(first // 8, (first + count + 7) // 8)}
    return [blocks[i // 8][i % 8] for i in range(first, first + count)]


def fold(w):
    r = w >> 18
    return r - Q if r >= Q else r


def derived_key(seed32, prm):
    """fbs_ctx_create_seeded's derivation: FNV-1a (64 bits) over the parameter fields, eight little-endian bytes each; the key is
    the first 32 bytes of block 0 of stream (0xFF << 56 | hash mod 2^56) under the caller's bytes"""
    h = 0xCBF29CE484222325
    fields = [prm.n, prm.log_n_poly, prm.k, prm.l_bsk, prm.beta_bsk, prm.t_ksk, prm.gamma_ksk, prm.p_msg, prm.sigma_lwe, prm.sigma_glwe,
              2 if prm.bsk_group == 2 else 1] + ([prm.sampler] if prm.sampler else [])
    for f in fields:
        for b in range(8):
            h = ((h ^ ((f >> (8 * b)) & 0xFF)) * 0x100000001B3) & M64
    blk = chacha_block(key_words(seed32), (0xFF << 56) | (h & ((1 << 56) - 1)), 0)
    return [w for v in blk[:4] for w in (v & 0xFFFFFFFF, v >> 32)]


def noise_windows(key, domain, sub, first, count):
    """the six-word windows of samples first .. first + count - 1 of a stream"""
    w = stream_words(key, domain, sub, 6 * first, 6 * count)
    return [w[6 * i:6 * i + 6] for i in range(count)]


def times_bits(a, bits):
    """a * u in Z[X]/(X^N + 1) for the binary polynomial u, in Python integers (not reduced)"""
    N = len(a)
    a, out = np.array(a, dtype=object), np.zeros(N, dtype=object)
    for sh in range(N):
        if bits[sh]:
            out[sh:] += a[:N - sh]
            if sh:
                out[:sh] -= a[N - sh:]
    return out.tolist()


def ref_masks(prm, mask_key):
    """A[r][c] as lists of N integers"""
    k, N = prm.k, prm.N
    return [[[fold(w) for w in stream_words(key_words(mask_key), DOM_PUB_MASK, r, c * N, N)] for c in range(k)] for r in range(k)]


def ref_public_key(prm, mask_key, sk, noise_of):
    """bodies [k][N]: P_r = sum_c A[r][c] S_c + E_r.  noise_of(windows) -> the sampler's integers"""
    k, N = prm.k, prm.N
    A = ref_masks(prm, mask_key)
    out = []
    for r in range(k):
        body = noise_of(noise_windows(key_words(NOISE_SEED), DOM_PUB_NOISE, r, 0, N))
        for c in range(k):
            body = [x + y for x, y in zip(body, times_bits(A[r][c], sk[c * N:(c + 1) * N]))]
        out.append([x % Q for x in body])
    return out


def ref_sample_bits(prm, key, nu):
    k, N = prm.k, prm.N
    w = stream_words(key, DOM_PUB_ENC_U, nu, 0, (k * N + 63) // 64)
    return [[(w[(r * N + j) // 64] >> ((r * N + j) % 64)) & 1 for j in range(N)] for r in range(k)]


def ref_sample(prm, A, P, key, nu, msgs, noise_of):
    """one GLWE sample [k+1][N] of stream nu for the messages msgs (at most N; the rest carry message 0)"""
    k, N = prm.k, prm.N
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    u = ref_sample_bits(prm, key, nu)
    e = noise_of(noise_windows(key, DOM_PUB_ENC_NOISE, nu, 0, (k + 1) * N))
    out = []
    for c in range(k + 1):
        acc = e[c * N:(c + 1) * N]
        for r in range(k):
            acc = [x + y for x, y in zip(acc, times_bits(A[r][c] if c < k else P[r], u[r]))]
        if c == k:
            acc = [x + delta * int(m) for x, m in zip(acc, list(msgs) + [0] * (N - len(msgs)))]
        out.append([x % Q for x in acc])
    return out


def irwin_hall_of(sigma):
    return lambda windows: [irwin_hall(w, sigma) for w in windows]


# ---- the library, keyed once per set -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
    from tfhe_fbs_map_amd import HostContext, _public_native as pub
    out = {}
    for name, prm in toy_sets().items():
        ctx = HostContext(prm, seed=9)
        ctx.keygen_seeded()
        sk = ctx.export_keys()["sk_glwe"]
        mask_key = ctx.export_seeded_keys()["mask_key"]
        bodies = pub.keygen(prm, mask_key, sk, NOISE_SEED)
        out[name] = dict(prm=prm, ctx=ctx, sk=sk, mask_key=mask_key, bodies=bodies, enc=pub.Encryptor(prm, mask_key, bodies, ENC_SEED))
    return out


@pytest.mark.parametrize("name", SETS)
def test_public_key_bodies_word_for_word(worlds, name):
    w = worlds[name]
    prm = w["prm"]
    want = ref_public_key(prm, w["mask_key"], [int(b) for b in w["sk"]], irwin_hall_of(prm.sigma_glwe))
    assert w["bodies"].shape == (prm.k, prm.N) and w["bodies"].tolist() == want
    assert int(w["bodies"].max()) < Q


@pytest.mark.parametrize("name", SETS)
def test_encrypted_samples_word_for_word(worlds, name):
    """count in {1, N - 1, N, N + 1}: one sample each, the last count two, the second filled with one message"""
    w = worlds[name]
    prm, N = w["prm"], w["prm"].N
    A, P, key = ref_masks(prm, w["mask_key"]), w["bodies"].tolist(), derived_key(ENC_SEED, prm)
    rng = np.random.default_rng(5)
    for count, nonce0 in ((1, 0), (N - 1, 40), (N, (1 << 55) - 1), (N + 1, 1 << 20)):
        msgs = rng.integers(0, 2 * prm.p_msg, count)
        got, first = w["enc"].encrypt(msgs, nonce0=nonce0)
        assert first == nonce0 and got.shape == (-(-count // N), prm.k + 1, N)
        for g in range(got.shape[0]):
            assert got[g].tolist() == ref_sample(prm, A, P, key, nonce0 + g, msgs[g * N:(g + 1) * N], irwin_hall_of(prm.sigma_glwe)), (count, g)


def extraction(prm, glwe, j):
    """the header's formula for message j, in Python integers"""
    N, k = prm.N, prm.k
    sample, t = glwe[j // N], j % N
    ct = []
    for c in range(k):
        a = [int(x) for x in sample[c]]
        ct += [a[t - i] if i <= t else (Q - a[N + t - i]) % Q for i in range(N)]
    return ct + [int(sample[k][t])]


@pytest.mark.parametrize("name", SETS)
def test_host_expansion_is_the_extraction_formula(name):
    from tfhe_fbs_map_amd import _public_native as pub
    prm = toy_sets()[name]
    N, count = prm.N, 2 * prm.N + 3
    rng = np.random.default_rng(11)
    glwe = rng.integers(0, Q, (3, prm.k + 1, N), dtype=np.uint64)
    glwe[0, 0, :4] = [0, Q - 1, 1, 0]
    glwe[1] = 0
    glwe[2, :, 0] = 0
    cts = pub.expand(prm, glwe, count)
    assert cts.shape == (count, prm.ct_words)
    for j in (0, 1, 2, 3, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 2, int(rng.integers(4, N - 1))):
        assert cts[j].tolist() == extraction(prm, glwe, j), j
    # every word of every ciphertext, by index arithmetic on the whole batch
    j = np.arange(count)
    i = np.arange(N)
    src = (j[:, None] % N - i[None, :]) % N
    neg = i[None, :] > (j[:, None] % N)
    for c in range(prm.k):
        a = glwe[j // N, c][np.arange(count)[:, None], src]
        want = np.where(neg & (a != 0), np.uint64(Q) - a, a)
        assert np.array_equal(cts[:, c * N:(c + 1) * N], want), c
    assert np.array_equal(cts[:, -1], glwe[j // N, prm.k, j % N])


@pytest.mark.parametrize("name", SETS)
def test_every_message_decrypts_at_the_edge_coefficients(worlds, name):
    w = worlds[name]
    prm, N = w["prm"], w["prm"].N
    from tfhe_fbs_map_amd import _public_native as pub
    for m in range(2 * prm.p_msg):
        msgs = (np.arange(N) + m) % (2 * prm.p_msg)
        msgs[[0, 1, N - 1]] = m
        glwe, _ = w["enc"].encrypt(msgs, nonce0=500 + m)
        got = w["ctx"].decrypt(pub.expand(prm, glwe, N))
        assert got[0] == m and got[1] == m and got[N - 1] == m
        assert np.array_equal(got, msgs)


def test_sampler_one_in_doubles():
    """Sampler 1 at k = 1, N = 256: what is left of the bodies and of a sample after the deterministic part of the restatement is
    taken off is rint(sigma z) of the stream windows, z by the closed formula of tests/test_sampler.py in float64, to its tolerance
    there (1 + sigma 2^-44)."""
    from tests.test_sampler import z_reference
    from tfhe_fbs_map_amd import HostContext, _public_native as pub
    prm = toy_sets()["k1_N256"].replace(sampler=1)
    N, sigma = prm.N, prm.sigma_glwe
    ctx = HostContext(prm, seed=9)
    ctx.keygen_seeded()
    sk = [int(b) for b in ctx.export_keys()["sk_glwe"]]
    mask_key = ctx.export_seeded_keys()["mask_key"]
    bodies = pub.keygen(prm, mask_key, sk, NOISE_SEED)
    zero = lambda windows: [0] * len(windows)      # noqa: E731

    def centred(v):
        v = np.array([int(x) % Q for x in v], dtype=object)
        return np.array([int(x) - Q if x > Q // 2 else int(x) for x in v], np.float64)

    def gauss_of(windows):
        return np.rint(float(sigma) * z_reference(np.array(windows, np.uint64)))

    quiet = ref_public_key(prm, mask_key, sk, zero)
    E = centred([int(a) - b for a, b in zip(bodies[0].tolist(), quiet[0])])
    want = gauss_of(noise_windows(key_words(NOISE_SEED), DOM_PUB_NOISE, 0, 0, N))
    assert np.abs(E - want).max() <= 1 + sigma * 2.0 ** -44 and np.abs(want).max() > sigma

    enc = pub.Encryptor(prm, mask_key, bodies, ENC_SEED)
    msgs = np.arange(N - 3) % (2 * prm.p_msg)
    got, _ = enc.encrypt(msgs, nonce0=77)
    key = derived_key(ENC_SEED, prm)
    quiet = ref_sample(prm, ref_masks(prm, mask_key), bodies.tolist(), key, 77, msgs, zero)
    e = centred([int(a) - b for c in range(2) for a, b in zip(got[0, c].tolist(), quiet[c])])
    want = gauss_of(noise_windows(key, DOM_PUB_ENC_NOISE, 77, 0, 2 * N))
    assert np.abs(e - want).max() <= 1 + sigma * 2.0 ** -44 and np.abs(want).max() > sigma
    assert np.array_equal(ctx.decrypt(pub.expand(prm, got, msgs.size)), msgs)


# ---- the phase noise ---------------------------------------------------------------------------------------------------------------
KEYS, SAMPLES_PER_KEY = 8, 8          # one measurement: 8 keys x 8 samples x N = 256 coefficients = 16 384 phases


def numpy_measurement(prm, seed):
    """The restatement's encryption with numpy randomness: mean square of KEYS * SAMPLES_PER_KEY * N phases over
    params.public_input_variance q^2.  Noise: the sum of twelve uniform 32-bit terms, centred, times sigma / 2^32, rounded -- the
    distribution of sampler 0."""
    from tfhe_fbs_map_amd.params import public_input_variance
    rng = np.random.default_rng(seed)
    N, k, sigma = prm.N, prm.k, prm.sigma_glwe
    assert k == 1
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))

    def noise(count):
        s = rng.integers(0, 1 << 32, (count, 12)).sum(axis=1) - 6 * ((1 << 32) - 1)
        return (s * sigma + (1 << 31)) >> 32

    total = 0.0
    for _ in range(KEYS):
        S = rng.integers(0, 2, N)
        A = rng.integers(0, Q, N)
        P = (A @ negacyclic_matrix(S) + noise(N)) % Q
        for _ in range(SAMPLES_PER_KEY):
            u, m = rng.integers(0, 2, N), rng.integers(0, 2 * prm.p_msg, N)
            Mu = negacyclic_matrix(u)
            a1 = (A @ Mu + noise(N)) % Q
            b1 = (P @ Mu + noise(N) + delta * m) % Q
            ph = (b1 - a1 @ negacyclic_matrix(S) - delta * m) % Q
            ph = np.where(ph > Q // 2, ph - Q, ph).astype(np.float64)
            total += float((ph ** 2).sum())
    return total / (KEYS * SAMPLES_PER_KEY * N) / (public_input_variance(prm) * float(Q) ** 2)


def test_phase_noise_is_the_models():
    """k = 1, N = 256, sigma_glwe = 2^8: the mean square of 16 384 phases (8 keys, 8 samples each, all 256 coefficients; the public
    key's E and the secret S are fixed per key, so the second moment about zero is what (1 + kN) sigma^2 predicts) over
    params.public_input_variance.  The accepted band is the restatement's own: its encryption with numpy randomness over 20
    seeds, the observed range widened by the standard deviation of those 20 values.
    Recorded (this restatement, seeds 0 .. 19): min 0.8606, max 1.1055, standard deviation 0.0712 -> band [0.7895, 1.1766]; the
    test prints both figures before it compares."""
    from tfhe_fbs_map_amd import HostContext, _public_native as pub
    from tfhe_fbs_map_amd.params import public_input_variance
    prm = toy_sets()["k1_N256"]
    N = prm.N
    ref = np.array([numpy_measurement(prm, seed) for seed in range(20)])
    lo, hi = ref.min() - ref.std(), ref.max() + ref.std()
    print("restatement: min %.4f max %.4f sd %.4f -> band [%.4f, %.4f]" % (ref.min(), ref.max(), ref.std(), lo, hi))
    assert abs(ref.mean() - 1.0) <= 3.0 * ref.std() / np.sqrt(len(ref))      # the model itself: the restatement sits on (1 + kN) sigma^2
    delta = 2 * ((Q + 2 * prm.p_msg) // (4 * prm.p_msg))
    total = 0.0
    for key in range(KEYS):
        ctx = HostContext(prm, seed=1000 + key)
        ctx.keygen_seeded()
        S = ctx.export_keys()["sk_glwe"].astype(np.int64)
        mask_key = ctx.export_seeded_keys()["mask_key"]
        enc = pub.Encryptor(prm, mask_key, pub.keygen(prm, mask_key, S, bytes([key]) * 32), bytes([200 + key]) * 32)
        msgs = np.random.default_rng(key).integers(0, 2 * prm.p_msg, SAMPLES_PER_KEY * N)
        glwe, _ = enc.encrypt(msgs)
        M = negacyclic_matrix(S)
        for g in range(SAMPLES_PER_KEY):
            a1, b1 = glwe[g, 0].astype(np.int64), glwe[g, 1].astype(np.int64)
            ph = (b1 - a1 @ M - delta * msgs[g * N:(g + 1) * N]) % Q
            ph = np.where(ph > Q // 2, ph - Q, ph).astype(np.float64)
            total += float((ph ** 2).sum())
    got = total / (KEYS * SAMPLES_PER_KEY * N) / (public_input_variance(prm) * float(Q) ** 2)
    print("library: %.4f" % got)
    assert lo <= got <= hi, (got, lo, hi)
