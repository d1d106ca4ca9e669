"""Encrypted-index reads (include/fbs_exec.h, "encrypted-index reads") restated in numpy: the box map, the map of a mapped fold and
its materialised array, and the blind rotation started from a whole GLWE sample instead of the trivial one.

`blind_rotate_from` restates both step forms of oracle/tfhe_oracle.c on the oracle's exported keys (`Oracle.keys()`: the
bootstrapping key in the coefficient domain) with one exact negacyclic product, `oracle.tfhe_oracle.polymul_ntt`: one key bit per
step (rotate and subtract on centred representatives, `decompose_poly`'s rounding) and two (the three-monomial bundle, ACC itself
decomposed), skipped steps included.  Every value is an exact residue, so working in the coefficient domain where the oracle works
in the transform domain changes no word.  tests/test_lookup_reference.py ties it to the frozen oracle on the trivial sample."""
import numpy as np

from oracle import tfhe_oracle as orc
from tests import fold_reference as F

Q = orc.Q
QBITS = 46
MAP_NONE, MAP_NEG = 0xFFFFFFFF, 0x80000000


def slot(j, p, N):
    """the box coefficient j < N lies in: < p an entry, == p the half box below X^N (minus entry 0)"""
    return (2 * p * j + N) // (2 * N)


def lookup_map(p, N, length, base=0, stride=1):
    """fbs_lookup_map restated: uint32 [N]"""
    if not (p >= 2 and 1 <= length <= p and base + (length - 1) * stride < MAP_NEG):
        raise ValueError("refused")
    out = np.empty(N, np.uint32)
    for j in range(N):
        x = slot(j, p, N)
        out[j] = base + x * stride if x < length else MAP_NONE if x < p else base | MAP_NEG
    return out


def negated(cts):
    """every word x -> (q - x) mod q"""
    cts = np.asarray(cts, np.uint64)
    return (np.uint64(Q) - cts) % np.uint64(Q)


def materialise(cts, fmap):
    """the array a mapped fold folds: row j = ciphertext fmap[j] & 0x7FFFFFFF (negated where bit 31 is set; ciphertext 0 where the
    index is past the array), or zero words for MAP_NONE"""
    cts = np.asarray(cts, np.uint64)
    out = np.zeros((len(fmap), cts.shape[1]), np.uint64)
    for j, m in enumerate(int(x) for x in fmap):
        if m == MAP_NONE:
            continue
        src = m & 0x7FFFFFFF
        row = cts[src if src < len(cts) else 0]
        out[j] = negated(row) if m & MAP_NEG else row
    return out


# ---- the blind rotation from a whole sample -----------------------------------------------------------------------------------------
def _centred(a):
    a = np.asarray(a, np.uint64).astype(np.int64)
    return np.where(a > Q // 2, a - Q, a)


def _rotate(poly, r, N):
    """X^r poly, r in [0, 2N) (poly_rotate)"""
    idx = (np.arange(N) - int(r)) % (2 * N)
    v = np.asarray(poly, np.uint64)[idx % N]
    return np.where(idx >= N, (np.uint64(Q) - v) % np.uint64(Q), v)


def _decompose(poly, l, beta):
    """decompose_poly: signed representatives in (-q, q) -> balanced digits of the closest multiple of q / B^l, q treated as 2^46,
    as residues, [l][N] uint64"""
    s = QBITS - l * beta
    B, half = 1 << beta, 1 << (beta - 1)
    abar = ((np.asarray(poly, np.int64) + (1 << (s - 1))) >> s) & ((1 << (l * beta)) - 1)
    out = np.empty((l, len(poly)), np.uint64)
    for lv in range(l - 1, -1, -1):
        dg = abar & (B - 1)
        abar = abar >> beta
        up = dg >= half
        dg = np.where(up, dg - B, dg)
        abar = abar + up
        out[lv] = (dg % Q).astype(np.uint64)
    return out


def _keys_of(o):
    if not hasattr(o, "_lookup_bsk"):
        k1, l = o.p["k"] + 1, o.p["l_bsk"]
        o._lookup_bsk = o.keys()["bsk"].reshape(-1, k1 * l, k1, o.N)
    return o._lookup_bsk


def blind_rotate_from(o, ms, acc0):
    """orc_blind_rotate with the accumulator started from X^-ms[n] acc0, acc0 [k+1][N] canonical residues -> [(k+1) N] uint64.
    On acc0 = (0, .., 0, tv) it is Oracle.blind_rotate(ms, tv), word for word."""
    N, k1, n, l, beta = o.N, o.p["k"] + 1, o.p["n"], o.p["l_bsk"], o.p["beta_bsk"]
    bsk = _keys_of(o)
    q = np.uint64(Q)
    ms = [int(x) for x in ms]
    acc = np.stack([_rotate(c, (2 * N - ms[n]) % (2 * N), N) for c in np.asarray(acc0, np.uint64).reshape(k1, N)])
    steps = n // o.group
    for i in range(steps):
        if o.group == 1:
            r = ms[i]
            if r == 0:
                continue
            inputs = [_centred(_rotate(acc[cc], r, N)) - _centred(acc[cc]) for cc in range(k1)]
            key = lambda row, oc: bsk[i, row, oc]                                       # noqa: E731
        else:
            e = (ms[2 * i], ms[2 * i + 1], (ms[2 * i] + ms[2 * i + 1]) % (2 * N))
            if e[0] == 0 and e[1] == 0:
                continue
            inputs = [_centred(acc[cc]) for cc in range(k1)]

            def key(row, oc):                                                           # sum_jj (X^e_jj - 1) E_jj
                tot = np.zeros(N, np.uint64)
                for jj in range(3):
                    if e[jj]:
                        E = bsk[3 * i + jj, row, oc]
                        tot = (tot + _rotate(E, e[jj], N) + (q - E)) % q
                return tot
        total = np.zeros((k1, N), np.uint64)
        for cc in range(k1):
            dig = _decompose(inputs[cc], l, beta)
            for lv in range(l):
                for oc in range(k1):
                    total[oc] = (total[oc] + orc.polymul_ntt(dig[lv], key(cc * l + lv, oc))) % q
        acc = (acc + total) % q
    return acc.reshape(-1)


def lookup_reference(o, ms, table):
    """a whole lookup after the modulus switch: the rotation from `table`, then sample extraction of coefficient 0, nothing added"""
    return o.sample_extract(blind_rotate_from(o, ms, table), 0)


# ---- encrypted tables for the tests: genuine folds, made cheaply --------------------------------------------------------------------
def sparse_fold_key(prm, sk_glwe, t, gamma, cols, seed=1):
    """the rows (i, v), i in `cols`, of a fold key as tests/fold_reference.py:python_fold_key makes them, [len(cols)][t][k+1][N]: all a
    fold needs when every other mask word of its ciphertexts is zero (a zero word has zero digits and meets no key row)"""
    N, k = prm.N, prm.k
    rng = np.random.default_rng([seed, N, k, t, gamma])
    S = np.asarray(sk_glwe, np.int64).reshape(k, N)
    R = len(cols) * t
    key = np.zeros((R, k + 1, N), np.uint64)
    key[:, :k] = rng.integers(0, Q, (R, k, N), dtype=np.uint64)
    body = np.rint(rng.normal(0.0, float(prm.sigma_glwe), (R, N))).astype(np.int64) % Q
    for c in range(k):
        body = (body + F.negacyclic_by_bits(key[:, c], S[c]).astype(np.int64)) % Q
    h = [(Q + (1 << (gamma * (v + 1))) // 2) >> (gamma * (v + 1)) for v in range(t)]
    for at, i in enumerate(cols):
        if S.reshape(-1)[i]:
            for v in range(t):
                body[at * t + v, 0] = (int(body[at * t + v, 0]) + h[v]) % Q
    key[:, k] = body.astype(np.uint64)
    return key.reshape(len(cols), t, k + 1, N)


def sparse_encryptions(prm, sk_glwe, cols, bodies_phase, rng):
    """big-key ciphertexts [len(bodies_phase)][D+1] whose mask is random in the columns `cols` and zero elsewhere, of the given
    phases (residues; the caller adds its noise): body = sum a_i s_i + phase"""
    D = prm.k * prm.N
    sk = np.asarray(sk_glwe, np.int64)
    cts = np.zeros((len(bodies_phase), D + 1), np.uint64)
    cts[:, cols] = rng.integers(0, Q, (len(bodies_phase), len(cols)), dtype=np.uint64)
    for r, ph in enumerate(bodies_phase):
        cts[r, D] = (sum(int(cts[r, i]) for i in cols if sk[i]) + int(ph)) % Q
    return cts


def fold_by_boxes(cts, fmap, key, t, gamma, cols=None):
    """the mapped fold of `cts` under `fmap` (one sample, len(fmap) <= N), from the fold's linearity in its ciphertexts (tests/
    fold_reference.py, fold_prefixes): for every distinct map value, the fold of that one materialised ciphertext at coefficient 0
    (fold_sample) times the 0/1 polynomial of the positions that name it, summed mod q.  Word for word
    fold_reference(materialise(cts, fmap)).  cols: the key holds only these mask columns (sparse_fold_key) and every other mask
    word of cts is zero."""
    _, _, k1, N = key.shape
    D = cts.shape[1] - 1
    q = np.uint64(Q)
    out = np.zeros((k1, N), np.uint64)
    fmap = np.asarray(fmap, np.uint32)
    for m in sorted(set(int(x) for x in fmap)):
        if m == MAP_NONE:
            continue
        one = materialise(cts, [m])
        if cols is not None:
            assert not np.delete(one[0, :D], cols).any()
            one = one[:, list(cols) + [D]]
        s = F.fold_sample(one, key, t, gamma)
        box = (fmap == m).astype(np.uint64)
        box = np.concatenate([box, np.zeros(N - len(box), np.uint64)])
        for c in range(k1):
            out[c] = (out[c] + orc.polymul_ntt(box, s[c])) % q
    return out


TABLE_FOLD_KEY = (2, 10)                                                 # (t_f, gamma_f) of the tables below
TABLE_COLS = 16                                                          # mask columns in use (sparse_fold_key)


def encrypted_tables(o, prm, n_tables, seed, p=7):
    """-> (tables [n_tables][k+1][N], entries [n_tables][p]): mapped folds (box map, len = p) of sparse-mask encryptions of a
    permutation of 0 .. p - 1 each, noise sigma_glwe, under the oracle's GLWE key"""
    from tfhe_fbs_map_amd import Params
    P = Params(**prm)
    rng = np.random.default_rng([seed, P.N, P.k])
    sk = o.keys()["sk_glwe"]
    D = P.k * P.N
    cols = sorted(rng.choice(D, TABLE_COLS, replace=False).tolist())
    key = sparse_fold_key(P, sk, *TABLE_FOLD_KEY, cols)
    delta = 2 * o.delta_half
    tables, entries = [], []
    for _ in range(n_tables):
        msgs = rng.permutation(p)
        noise = np.rint(rng.normal(0.0, float(P.sigma_glwe), p)).astype(np.int64)
        cts = sparse_encryptions(P, sk, cols, [(int(m) * delta + int(e)) % Q for m, e in zip(msgs, noise)], rng)
        tables.append(fold_by_boxes(cts, lookup_map(p, P.N, p), key, *TABLE_FOLD_KEY, cols=cols))
        entries.append(msgs)
    return np.stack(tables), np.stack(entries)
