"""Folded state (include/fbs_exec.h, "folded state") restated in numpy: the rounding of the mask words, the balanced digits, the
sum of negacyclic products against the fold key, the body words added as they are.  Two forms of the product sum: the schoolbook
one (`slow=True`: one oracle product per key polynomial) and a fast one that every GPU comparison uses -- the digits and the key
words cut into limbs small enough that a float64 matrix product of limb matrices is exact, the limbs put back together with Python
integers.  tests/test_fold_reference.py holds the fast form to the schoolbook one and the definition to decryption; tests/
test_gpu_fold.py holds the kernels of csrc/fbs_fold.hip to the fast form, word for word."""
import numpy as np

from tests import helpers as H

Q = H.Q
QBITS = 46
FOLD_KEYS = ((3, 10),)                                  # D t_f rows: far past PACK_CENTRE_EVERY
FOLD_EDGE_KEYS = ((1, 31), (31, 1), (2, 15))            # the widest digit; the most levels; r = 16
# (log N, k) once per transform class: N = 256 at k = 1, 2, 4; 512 at k = 3; 1024 at k = 1, 2; 2048 at k = 1 (held at one level)
FOLD_SHAPES = [(8, 1), (8, 2), (8, 4), (9, 3), (10, 1), (10, 2), (11, 1)]


def fold_toy(log_n, k, n=12, p=3):
    """the toy set of a shape (tests/helpers.py: pack_toy), n = 12 as the parity tests use"""
    return H.pack_toy(log_n, k, n, p)


def round_mask(a, t, gamma):
    """mask words in [0, q) -> a' at t gamma bits, q treated as 2^46 (step 1)"""
    a = np.asarray(a, np.uint64).astype(np.int64)
    r = QBITS - t * gamma
    return (((a >> (r - 1)) + 1) >> 1) % (1 << (t * gamma))


def digit_rows(masks, t, gamma, N):
    """masks [fill][D] -> the digit polynomials D_(i,v), [D t][N] int64 in key-row order r = i t + v, zero past the fill"""
    fill, D = masks.shape
    digits = H.balanced_digits(round_mask(masks, t, gamma), t, gamma)          # [t][fill][D]
    rows = np.zeros((D, t, N), np.int64)
    rows[:, :, :fill] = digits.transpose(2, 0, 1)
    return rows.reshape(D * t, N)


def _balanced_limbs(d, bits=16):
    """signed integers -> [(limb, shift)] with limb in [-2^(bits-1), 2^(bits-1)] and sum limb << shift = d"""
    out, shift = [], 0
    d = d.copy()
    while True:
        if int(np.abs(d).max(initial=0)) < 1 << (bits - 1):
            out.append((d, shift))
            return out
        lo = ((d + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))
        out.append((lo, shift))
        d = (d - lo) >> bits
        shift += bits


def product_sum(rows, key):
    """sum over r of rows[r] (small signed integers) times key[r] (canonical residues), negacyclic mod q, [N] uint64.  Exact:
    M = rows^T key per pair of limbs is a float64 matrix product whose every entry stays below 2^53, M[j][m] is the weight of
    X^(j + m), and the sums over its anti-diagonals are taken on integers."""
    R, N = rows.shape
    key = np.asarray(key, np.uint64).astype(np.int64)
    kbits = 23
    total = np.zeros(N, object)
    used = np.flatnonzero(rows.any(axis=0))                                    # (a partly filled sample: only its coefficients)
    for dl, ds in _balanced_limbs(rows[:, used]):
        for ks in (0, kbits):
            kl = (key >> ks) & ((1 << kbits) - 1)
            assert R * int(np.abs(dl).max(initial=0)) * (1 << kbits) < 1 << 53
            M = np.mod((dl.T.astype(np.float64) @ kl.astype(np.float64)).astype(np.int64), Q)
            full = np.zeros(2 * N, np.int64)
            for row, j in enumerate(used):
                full[j:j + N] += M[row]                                        # (N terms below q: far inside 64 bits)
            total += (full[:N] - full[N:]).astype(object) * (1 << (ds + ks))
    return np.array([int(x) % Q for x in total], np.uint64)


def product_sum_schoolbook(rows, key):
    """the same, one schoolbook product (tests/helpers.py: negacyclic) per row"""
    acc = np.zeros(rows.shape[1], np.uint64)
    for r in range(rows.shape[0]):
        if rows[r].any():
            acc = (acc + H.negacyclic(rows[r], key[r])) % np.uint64(Q)
    return acc


def fold_sample(cts, key, t, gamma, slow=False, j0=0):
    """cts [fill][D+1] and the whole fold key [D][t][k+1][N] -> the sample [k+1][N] (steps 1 - 4) whose coefficients j0 .. j0 + fill - 1
    hold them (j0 = 0: the definition; the fold is linear in its ciphertexts, so a sample is the sum mod q of the samples of its parts
    at their own coefficients -- `fold_prefixes`)"""
    D, _, k1, N = key.shape
    fill = cts.shape[0]
    assert cts.shape[1] == D + 1 and 1 <= fill and j0 + fill <= N
    rows = np.roll(digit_rows(cts[:, :D], t, gamma, N), j0, axis=1)              # (zero past the fill: nothing wraps)
    res = np.zeros((k1, N), np.uint64)
    for c in range(k1):
        kc = key[:, :, c, :].reshape(D * t, N)
        s = product_sum_schoolbook(rows, kc) if slow else product_sum(rows, kc)
        res[c] = (np.uint64(Q) - s) % np.uint64(Q)
    res[k1 - 1, j0:j0 + fill] = (res[k1 - 1, j0:j0 + fill] + cts[:, D]) % np.uint64(Q)
    return res


def fold_prefixes(cts, key, t, gamma):
    """cts [N + 1][D+1] -> {count: words of the batch cts[:count]} for count = 1, N - 1, N, N + 1, from ONE product sum over most of a
    sample: the parts [0, 1), [1, N - 1), [N - 1, N) of the first sample are folded at their own coefficients and added mod q"""
    N = key.shape[3]
    assert cts.shape[0] == N + 1
    q = np.uint64(Q)
    first = fold_sample(cts[:1], key, t, gamma)
    most = (first + fold_sample(cts[1:N - 1], key, t, gamma, j0=1)) % q
    whole = (most + fold_sample(cts[N - 1:N], key, t, gamma, j0=N - 1)) % q
    second = fold_sample(cts[N:], key, t, gamma)
    return {1: first.reshape(-1), N - 1: most.reshape(-1), N: whole.reshape(-1), N + 1: np.concatenate([whole.reshape(-1), second.reshape(-1)])}


def fold_reference(cts, key, t, gamma, slow=False):
    """cts [count][D+1] -> the words of the batch: the samples back to back, [ceil(count / N)][k+1][N] flattened"""
    N = key.shape[3]
    return np.concatenate([fold_sample(cts[g0:g0 + N], key, t, gamma, slow).reshape(-1) for g0 in range(0, cts.shape[0], N)])


def planted_mask_words(t, gamma):
    """{name: a mask word in [0, q)} for a fold key (t, gamma), r = 46 - t gamma >= 15: the edges of the rounding and of the
    balanced digits (tests/helpers.py: planted_mask_fields, at 46 bits).  A word a' << r rounds to a'.
      zero, qm1         0, and q - 1: the largest word there is; where r >= 20 it rounds up to 2^(t gamma) and wraps to 0
      tie, below_tie    2^(r-1) -> 1 and 2^(r-1) - 1 -> 0
      wraps             the smallest word that rounds up to 2^(t gamma) and wraps: 2^46 - 2^(r-1), which is a residue when
                        2^(r-1) > 2^46 - q = 507903, r >= 20; with wider keys no residue comes that close to 2^46
      all_low           every digit -B/2: the carry that starts at the bottom, runs through every level and is dropped at the top
      all_high          every digit B/2 - 1
      top_half          a' = 2^(t gamma - 1): the top digit alone is -B/2 (and the carry dropped)"""
    tg, r, B = t * gamma, QBITS - t * gamma, 1 << gamma
    offs = sum((B // 2) << (gamma * v) for v in range(t))
    out = {"zero": 0, "qm1": Q - 1, "tie": 1 << (r - 1), "below_tie": (1 << (r - 1)) - 1,
           "all_low": ((-offs) % (1 << tg)) << r, "all_high": ((1 << tg) - 1 - offs) << r, "top_half": (1 << (tg - 1)) << r}
    if (1 << QBITS) - (1 << (r - 1)) < Q:
        out["wraps"] = (1 << QBITS) - (1 << (r - 1))
    assert all(0 <= w < Q for w in out.values())
    return out


def planted_rows(count, N):
    """the ciphertexts that carry planted words: the first two, and N - 2, N - 1, N where the batch has them -- fixed positions, so
    that every prefix cts[:count] with count = 1, N - 1, N, N + 1 of a planted batch of N + 1 ends on one"""
    return sorted({j for j in (0, 1, N - 2, N - 1, N, count - 1) if 0 <= j < count})


def planted_cts(D, count, t, gamma, seed, N=256):
    """[count][D+1] canonical residues: random words; in the first 32 and the last 32 mask columns the values of `planted_mask_words`
    in turn over `planted_rows`; body words 0 and q - 1 alternating over those rows"""
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, Q, (count, D + 1), dtype=np.uint64)
    values = list(planted_mask_words(t, gamma).values())
    turn = 0
    for i in list(range(32)) + list(range(D - 32, D)):
        for j in planted_rows(count, N):
            cts[j, i] = values[turn % len(values)]
            turn += 1
    for s, j in enumerate(planted_rows(count, N)):
        cts[j, D] = (0, Q - 1)[s % 2]
    return cts


def phase_errors(glwe, prm, count, sk_glwe, expected):
    """the samples [G][k+1][N] under the GLWE key S: phase_j = B[j] - sum_c (A_c S_c)[j] mod q for the `count` coefficients in use,
    minus `expected` [count] (residues), centred: int64 errors [count].  Exact (Python integers behind numpy convolutions of
    23-bit limbs)."""
    N, k = prm.N, prm.k
    S = np.asarray(sk_glwe, np.int64).reshape(k, N)
    glwe = np.asarray(glwe, np.uint64).astype(np.int64).reshape(-1, k + 1, N)
    out = []
    for g in range(glwe.shape[0]):
        phase = glwe[g, k].astype(object)
        for c in range(k):
            for ks in (0, 23):
                limb = (glwe[g, c] >> ks) & ((1 << 23) - 1)
                conv = np.convolve(limb, S[c])                                  # below 2^23 N
                prod = conv[:N].copy()
                prod[:N - 1] -= conv[N:]
                phase = phase - prod.astype(object) * (1 << ks)
        out.append(phase)
    phase = np.concatenate(out)[:count]
    err = np.array([(int(x) - int(e) + Q // 2) % Q - Q // 2 for x, e in zip(phase, expected)], np.int64)
    return err


def negacyclic_by_bits(a, s):
    """rows a [R][N] (canonical residues) times the binary polynomial s [N], negacyclic mod q, [R][N] uint64: the matrix of s has
    entries 0 and +-1, so a float64 product of 23-bit limbs is exact"""
    N = len(s)
    T = np.zeros((N, N), np.float64)                                          # row j: X^j s
    for j in range(N):
        T[j, j:] = s[:N - j]
        T[j, :j] = -np.asarray(s[N - j:], np.float64)
    a = np.asarray(a, np.uint64).astype(np.int64)
    lo = (a & ((1 << 23) - 1)).astype(np.float64) @ T
    hi = (a >> 23).astype(np.float64) @ T
    out = (np.mod(hi.astype(np.int64), Q).astype(object) * (1 << 23) + lo.astype(np.int64).astype(object)) % Q
    return out.astype(np.uint64)


def python_fold_key(prm, sk_glwe, t, gamma, seed=1):
    """a fold key made here, [D][t][k+1][N]: row (i, v) a GLWE encryption of s_i h_v under S with numpy's masks and noise of
    standard deviation sigma_glwe (rounded normal) -- a valid key of the definition, not the library's streams"""
    N, k, D = prm.N, prm.k, prm.k * prm.N
    rng = np.random.default_rng(seed)
    S = np.asarray(sk_glwe, np.int64).reshape(k, N)
    key = np.zeros((D * t, k + 1, N), np.uint64)
    key[:, :k] = rng.integers(0, Q, (D * t, k, N), dtype=np.uint64)
    body = np.rint(rng.normal(0.0, float(prm.sigma_glwe), (D * t, N))).astype(np.int64) % Q
    for c in range(k):
        body = (body + negacyclic_by_bits(key[:, c], S[c]).astype(np.int64)) % Q
    h = [(Q + (1 << (gamma * (v + 1))) // 2) >> (gamma * (v + 1)) for v in range(t)]
    for i in range(D):
        if S.reshape(-1)[i]:
            for v in range(t):
                body[i * t + v, 0] = (int(body[i * t + v, 0]) + h[v]) % Q
    key[:, k] = body.astype(np.uint64)
    return key.reshape(D, t, k + 1, N)
