"""Encrypted tables (include/fbs_exec.h, "encrypted tables") restated in numpy: the wide-box map, the wide-box property on cleartext
polynomials, and a whole write -- the value folded into a unit box, turned by the NEGATED amounts of the index and added to the
table -- on the references of tests/lookup_reference.py and tests/fold_reference.py."""
import numpy as np

from oracle import tfhe_oracle as orc
from tests import lookup_reference as L

Q = orc.Q
MAP_NONE, MAP_NEG = L.MAP_NONE, L.MAP_NEG


def wide_slot(c, p, N, s):
    """W(c) for signed c in (-N, N), floor division towards minus infinity"""
    return (2 * p * c + s * N) // (2 * s * N)


def table_map(p, N, spread, length, base=0, stride=1):
    """fbs_table_map restated: uint32 [N]"""
    if not (p >= 2 and spread >= 1 and 1 <= length <= p // spread and base + (length - 1) * stride < MAP_NEG):
        raise ValueError("refused")
    out = np.empty(N, np.uint32)
    for j in range(N):
        w = wide_slot(j, p, N, spread)
        out[j] = base + w * stride if w < length else base | MAP_NEG if wide_slot(j - N, p, N, spread) == 0 else MAP_NONE
    return out


def negated_amounts(ms, N):
    """every amount a -> (2N - a) mod 2N"""
    return ((2 * N - np.asarray(ms, np.int64)) % (2 * N)).astype(np.uint32)


def box_slot(r, p, N):
    """the message in [0, 2p) the box rule decodes the amount r to"""
    return (2 * p * (r % (2 * N)) + N) // (2 * N) % (2 * p)


def amounts_of(msg, p, N):
    """every amount in (-N, N) that decodes to `msg`"""
    return [r for r in range(-N + 1, N) if box_slot(r, p, N) == msg]


def unit_box(p, N, s):
    """U of a write as a cleartext polynomial: +1 where the map of a one-entry table names the entry, -1 where it names it negated"""
    m = table_map(p, N, s, 1)
    return np.where(m == 0, 1, np.where(m == MAP_NEG, -1, 0)).astype(np.int64)


def rotated(poly, r):
    """X^r poly in Z[X]/(X^N + 1), any integer r"""
    N = len(poly)
    idx = (np.arange(N) - r) % (2 * N)
    return np.where(idx >= N, -poly[idx % N], poly[idx % N])


def read_at(poly, r):
    """what a read by the amount r in (-N, N) returns: coefficient r, or minus coefficient r + N below zero"""
    return int(poly[r]) if r >= 0 else -int(poly[r + len(poly)])


def wide_box_failures(N, p, s):
    """-> (failing, pairs): over all entries i, i' < floor(p / s) and all amounts r_w, r_r in (-N, N) that decode to s i and s i',
    the pairs where reading X^{r_w} U at r_r is not [i == i']"""
    U = unit_box(p, N, s)
    amounts = [(i, r) for i in range(p // s) for r in amounts_of(s * i, p, N)]
    failing = pairs = 0
    for i, r_w in amounts:
        written = rotated(U, r_w)
        for i2, r_r in amounts:
            pairs += 1
            failing += read_at(written, r_r) != (1 if i == i2 else 0)
    return failing, pairs


# ---- a whole write on the references --------------------------------------------------------------------------------------------------
def amount_row(mask, sk_lwe, r, N):
    """the modulus-switched row [n + 1] whose rotation amount b~ - <a~, s> is r mod 2N"""
    mask = [int(m) for m in mask]
    return np.array(mask + [(sum(m for m, s in zip(mask, sk_lwe) if int(s)) + r) % (2 * N)], np.uint32)


class CheapFolds:
    """what tests/lookup_reference.py:encrypted_tables is made of, kept: sparse-mask encryptions and the 16 rows of a fold key they
    meet, under the oracle's GLWE key"""

    def __init__(self, o, prm, seed):
        from tfhe_fbs_map_amd import Params
        self.o, self.P = o, Params(**prm)
        self.rng = np.random.default_rng([seed, self.P.N, self.P.k])
        self.sk = o.keys()["sk_glwe"]
        D = self.P.k * self.P.N
        self.cols = sorted(self.rng.choice(D, L.TABLE_COLS, replace=False).tolist())
        self.key = L.sparse_fold_key(self.P, self.sk, *L.TABLE_FOLD_KEY, self.cols)
        self.delta = 2 * o.delta_half

    def encrypt(self, msgs):
        noise = np.rint(self.rng.normal(0.0, float(self.P.sigma_glwe), len(msgs))).astype(np.int64)
        return L.sparse_encryptions(self.P, self.sk, self.cols, [(int(m) * self.delta + int(e)) % Q for m, e in zip(msgs, noise)], self.rng)

    def fold(self, cts, fmap):
        return L.fold_by_boxes(cts, fmap, self.key, *L.TABLE_FOLD_KEY, cols=self.cols)


def write_add(o, table, unit, ms):
    """table + X^{+r} unit, r the amount of the row `ms`: the rotation of `unit` by the negated amounts, whole, added word by word"""
    N = o.N
    turned = L.blind_rotate_from(o, negated_amounts(ms, N), unit).reshape(-1, N)
    return (np.asarray(table, np.uint64) + turned) % np.uint64(Q)
