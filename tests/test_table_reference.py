"""Encrypted tables without a GPU: the wide-box map restated (tests/table_reference.py), fbs_table_map against it, the wide-box
property that makes a write by a noisy index safe, and a whole write on the CPU references.

(a) `table_map` at spread 1 is tests/lookup_reference.py's `lookup_map` for every (p, N) its tests use, and fbs_table_map is
    `table_map` at every spread, and refuses what the header says it refuses.
(b) THE PROPERTY, exhaustively: at spread s >= 2, for all entries i, i' < floor(p / s) and ALL amounts r_w, r_r in (-N, N) that the
    box rule decodes to s i and s i', reading X^{r_w} U at r_r gives [i == i'].  The negative control: at spread 1 it fails.
(c) A whole write on cheap folds (tests/lookup_reference.py, encrypted_tables' construction): the value folded into a unit box,
    turned by the negated amounts of the index (`blind_rotate_from`), added to the table; `lookup_reference` of the result decrypts
    to entry + value at the written entry and to the old entry elsewhere -- written at one edge of the index's box, read at the
    other."""
import ctypes

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests import lookup_reference as L
from tests import table_reference as R
from tests.helpers import PLANTED_FAMILIES, planted_mask_lists, planted_set

Q = orc.Q
WIDE_CASES = [(64, 7, 2), (64, 4, 2), (64, 5, 2), (128, 15, 2), (256, 15, 2), (128, 7, 3)]


def test_at_spread_one_it_is_the_box_map():
    for p in (2, 7, 15, 31):
        for N in (256, 1024):
            for length in sorted({1, p - 1, p}):
                for base, stride in ((0, 1), (5, 3), ((1 << 31) - 1 - (length - 1) * 1000, 1000)):
                    assert np.array_equal(R.table_map(p, N, 1, length, base, stride), L.lookup_map(p, N, length, base, stride)), (p, N, length)


def test_the_map_has_the_shape_the_header_gives_it():
    m = R.table_map(7, 64, 2, 3, base=10, stride=4)
    # a wide box is 2 N / 7 = 18.3 coefficients: entry 0 opens the polynomial with half of one (14 j + 128 < 256: j <= 9), entries 1
    # and 2 take a whole one each, and the half box below X^N (14 (64 - j) <= 128: j >= 55) is minus entry 0
    assert m.tolist() == [10] * 10 + [14] * 18 + [18] * 18 + [R.MAP_NONE] * 9 + [10 | R.MAP_NEG] * 9
    # the unit box of a write: +1 on [0, sN/2p), -1 on [N - sN/2p, N), 0 between
    U = R.unit_box(7, 64, 2)
    assert U[:10].tolist() == [1] * 10 and U[10:55].tolist() == [0] * 45 and U[55:].tolist() == [-1] * 9
    for bad in ((7, 64, 0, 1), (7, 64, 2, 0), (7, 64, 2, 4), (7, 64, 8, 1)):
        with pytest.raises(ValueError):
            R.table_map(*bad)


@pytest.mark.parametrize("N,p,s", WIDE_CASES)
def test_a_wide_box_written_anywhere_is_read_anywhere(N, p, s):
    failing, pairs = R.wide_box_failures(N, p, s)
    per_entry = [len(R.amounts_of(s * i, p, N)) for i in range(p // s)]
    assert pairs == sum(per_entry) ** 2 and min(per_entry) >= N // p          # every amount of every box, both ways
    assert any(r < 0 for r in R.amounts_of(0, p, N))                          # ... the ones below zero among them
    assert failing == 0, (N, p, s, failing, pairs)


def test_an_ordinary_box_is_not_enough():
    """the negative control: with one box an entry a read can fall outside what a write covered"""
    failing, pairs = R.wide_box_failures(64, 7, 1)
    assert pairs == 4096 and failing == 290


def test_fbs_table_map_is_the_restatement_and_refuses_what_it_says():
    from tfhe_fbs_map_amd import FbsError, _native as nat
    for p, N in ((2, 256), (7, 256), (7, 1024), (15, 1024), (31, 1024), (4, 64), (5, 64), (15, 128)):
        for s in (1, 2, 3):
            for length in sorted({1, max(1, p // s - 1), p // s} - {0}):
                if p // s == 0:
                    continue
                for base, stride in ((0, 1), (5, 3), ((1 << 31) - 1 - (length - 1) * 1000, 1000)):
                    got = nat.table_map(p, N, s, length, base, stride)
                    assert got.dtype == np.uint32 and np.array_equal(got, R.table_map(p, N, s, length, base, stride)), (p, N, s, length, base)
            if p // s:
                assert np.array_equal(nat.table_map(p, N, 1, p // s), nat.lookup_map(p, N, p // s))
    for bad, text in (((7, 256, 0, 1, 0, 1), "at least one box"), ((7, 256, 2, 0, 0, 1), "at least one entry"),
                      ((7, 256, 2, 4, 0, 1), "floor(p / spread)"), ((7, 256, 8, 1, 0, 1), "floor(p / spread)"), ((1, 256, 1, 1, 0, 1), "p >= 2"),
                      ((7, 300, 2, 3, 0, 1), "power of two"), ((7, 256, 2, 3, 1 << 31, 1), "below 2^31"), ((7, 256, 2, 3, 0, 1 << 30), "below 2^31")):
        with pytest.raises(FbsError) as e:
            nat.table_map(*bad)
        assert e.value.code == -1 and text in str(e.value), bad
    assert nat.lib.fbs_table_map(7, 256, 2, 3, 0, 1, None) == -1                 # null output
    out = np.full(257, 0x5A5A5A5A, np.uint32)                                    # writes N words and no more; nothing when refused
    assert nat.lib.fbs_table_map(7, 256, 2, 3, 0, 1, out.ctypes.data) == 0 and out[256] == 0x5A5A5A5A and (out[:256] != 0x5A5A5A5A).all()
    out[:] = 0x5A5A5A5A
    assert nat.lib.fbs_table_map(7, 256, 2, 4, 0, 1, out.ctypes.data) == -1 and (out == 0x5A5A5A5A).all()


def test_entries_are_declared_exported_and_bound_in_the_gpu_library_only():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _client_native, _native, _public_native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("fbs_table_map", "fbs_rotate_dev", "fbs_rotate_compact_dev", "fbs_glwe_add_dev"):
        assert name in declared_symbols() and hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
        assert name not in _client_native.EXPORTED_SYMBOLS and name not in _public_native.EXPORTED_SYMBOLS, name
    for meth in ("rotate_dev", "rotate_compact_dev", "glwe_add_dev"):
        assert callable(getattr(_native.Context, meth)), meth
    assert len([k for k in _native.kernel_catalog() if k.startswith("k_blind_rotate")]) >= 155   # no new name, none taken out


@pytest.mark.parametrize("family", ["k2_n1024_g2", "k4_n256_g2", "k1_n1024_g1"])
def test_a_whole_write_on_cheap_folds(family):
    prm = planted_set(**PLANTED_FAMILIES[family])
    o = orc.Oracle(prm, seed=33)
    N, n, p, s = o.N, prm["n"], prm["p_msg"], 2
    length = p // s
    folds = R.CheapFolds(o, prm, seed=5)
    entries = np.array([2, 0, 1])
    assert len(entries) == length == 3
    table = folds.fold(folds.encrypt(entries), R.table_map(p, N, s, length))
    sk = [int(b) for b in o.keys()["sk_lwe"]]
    masks = planted_mask_lists(N, n, prm["bsk_group"])                           # skipped steps, every edge amount
    want = entries.copy()
    # entry 0 written from BELOW zero (the half box under X^N), entry 2 at the top edge of its index's box, entry 1 at the bottom
    for turn, (i, value, pick_w) in enumerate(((0, 3, 0), (2, 4, -1), (1, 2, 0), (2, 1, 0))):
        at = R.amounts_of(s * i, p, N)
        r_w = at[pick_w]
        unit = folds.fold(folds.encrypt([value]), R.table_map(p, N, s, 1))
        table = R.write_add(o, table, unit, R.amount_row(masks[turn % 5], sk, r_w, N))
        assert int(table.max()) < Q
        want[i] += value
        assert want.max() < p
        for i2 in range(length):                                                 # read at the OTHER edge of the box, and at its centre
            at2 = R.amounts_of(s * i2, p, N)
            for r_r in (at2[-1 - pick_w if pick_w else -1], at2[len(at2) // 2]):
                out = L.lookup_reference(o, R.amount_row(masks[(turn + 3) % 5], sk, r_r, N), table)
                assert int(o.decrypt(out)) == int(want[i2]), (family, turn, i2, r_r)
    assert R.amounts_of(0, p, N)[0] < 0
