"""The inputs of tests/test_gpu_keyswitch.py, checked without a GPU: planted key-switching keys (tests/helpers.py: mask columns that
hold the worst case of each key-switch kernel's accumulators, bodies recomputed so that the key is a valid one) and planted
ciphertext rows (every digit at either end of its range, the rounding carry, random, honest).

* the definition restated on Python integers (helpers.ks_switch) is the C oracle's key switch on every planted key and row, and
  the rounding restated in numpy (round_fields of tests/test_gpu_compact.py) is the oracle's modulus switch: the reference of the
  GPU tests is anchored before a GPU is involved;
* every row of every planted key decrypts to sk_glwe[j] h_v within fbs_import_keys's tolerance, and every tuned word sits on the
  rounding boundary it was aimed at, so that an error of one unit in a tuned sum flips a 31-bit field;
* the stress stresses: from the patterns alone, the largest value each kernel family holds is at least half of the bound its code
  states for that family at that set (KS_REACHED below: the figures DESIGN.md quotes).

Fractions of the stated bounds the planted inputs reach (both keys, stress rows 0..2), as ks_reached computes them:

    set      gemm_int32  fp64   u64_sum  lanes_hi  lanes_hi_wave
    g9       -           -      0.998    0.998     0.998
    g8_t1    1.000       1.000  0.996    0.996     0.996
    g8_t2    1.000       -      0.996    0.996     0.996
    n4096    1.000       0.999  0.875    0.875     0.875
    k3       1.000       0.995  0.969    0.969     0.969
    shipped  1.000       0.996  0.750    0.750     0.750

(-: the family never runs at the set.  The integer sums reach (B - 1) / B of their bound: the largest field is B - 1.)"""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (KS_SETS, KS_SIGMA, Q, centred, ks_gadget, ks_reached, ks_set, ks_shape, ks_stated_bounds, ks_switch,
                           planted_keys, planted_rows)
from tests.test_gpu_compact import round_fields

# at least this fraction of each stated bound, per set; None where the family never runs at the set (select_keyswitch).  One half
# is what the issue asks; the figures reached are in the module docstring.
MIN_FRACTION = 0.5
_MADE = {}


def made(name):
    """(parameter dict, keyed oracle, {mirrored: (planted key dict, tuned)}, rows) of a set, made once"""
    if name not in _MADE:
        prm = ks_set(name)
        o = orc.Oracle(prm, seed=11)
        keys = o.keys()
        honest = o.encrypt(np.arange(4) % prm["p_msg"], nonce0=40)
        _MADE[name] = (prm, o, {m: planted_keys(keys, prm, mirrored=m) for m in (False, True)}, planted_rows(prm, 12, honest))
    return _MADE[name]


@pytest.mark.parametrize("name", list(KS_SETS))
def test_the_restatement_is_the_oracle_on_every_planted_key_and_row(name):
    prm, o, planted, rows = made(name)
    n, D, t, gamma = ks_shape(prm)
    w0 = prm["log_n_poly"] + 1
    for mirrored, (keys, _) in planted.items():
        o.set_keys(**keys)
        ksk = np.array([int(x) for x in keys["ksk"]], dtype=object).reshape(D * t, n + 1)
        want = np.stack([o.keyswitch(r) for r in rows])
        got = ks_switch(rows, ksk, prm)
        assert got.shape == want.shape and all(int(g) == int(w) for g, w in zip(got.ravel(), want.ravel())), (name, mirrored)
        assert np.array_equal(round_fields(want, w0), np.stack([o.modswitch(r) for r in want]).astype(np.uint64)), (name, mirrored)


@pytest.mark.parametrize("name", list(KS_SETS))
def test_planted_keys_decrypt_and_tuned_words_sit_on_the_boundary(name):
    prm, _, planted, rows = made(name)
    n, D, t, gamma = ks_shape(prm)
    h = ks_gadget(prm)
    for mirrored, (keys, tuned) in planted.items():
        ksk = np.array([int(x) for x in keys["ksk"]], dtype=object).reshape(D * t, n + 1)
        assert all(0 <= int(x) < Q for x in ksk.ravel())
        s = np.array([int(x) for x in keys["sk_lwe"]], dtype=object)
        phase = (ksk[:, n] - ksk[:, :n].dot(s)) % Q
        for r, ph in enumerate(phase):
            want = h[r % t] if keys["sk_glwe"][r // t] else 0
            assert abs(centred(int(ph) - want)) <= KS_SIGMA < 1024 + 16 * KS_SIGMA, (name, mirrored, r)
        out = ks_switch(rows[:2], ksk, prm)                            # stress rows 0 and 1
        assert len(tuned) >= 16 and {c for _, c, _, _ in tuned} >= {0, n - 1, 8, 16} | ({63, 64} if n > 64 else set())
        for which in (0, 1):
            mine = [(c, low) for w, c, _, low in tuned if w == which]
            assert len(mine) >= 8 and sorted(low for _, low in mine) == [0x3FFF] * (len(mine) // 2) + [0x4000] * (len(mine) // 2)
            for col, low in mine:
                assert int(out[which, col]) & 0x7FFF == low, (name, mirrored, which, col)
        fields = round_fields(np.array(out, dtype=np.uint64), 31)       # ... where one unit either way changes the 31-bit field
        for which, col, _, low in tuned:
            r = int(out[which, col])
            up, down = ((r >> 14) + 1) >> 1, ((r - 1 >> 14) + 1) >> 1
            assert int(fields[which, col]) == up & 0x7FFFFFFF
            assert (up != down) if low == 0x4000 else (((r + 1 >> 14) + 1) >> 1 != up), (name, which, col)


@pytest.mark.parametrize("name", list(KS_SETS))
def test_the_planted_inputs_reach_half_of_every_stated_bound(name):
    prm, _, planted, rows = made(name)
    n, D, t, gamma = ks_shape(prm)
    bounds = ks_stated_bounds(prm)
    assert bounds["u64_sum"] < 2 ** 63.9 and bounds["lanes_hi"] < 2 ** 31.9      # params_out_of_range admits the set
    assert bounds["gemm_int32"] is None or bounds["gemm_int32"] < 1 << 31
    assert bounds["fp64"] is None or bounds["fp64"] <= 1 << 53
    assert (bounds["gemm_int32"] is None) == (name == "g9") and (bounds["fp64"] is None) == (name in ("g9", "g8_t2"))
    reached = {}
    for keys, _ in planted.values():
        ksk = np.array([int(x) for x in keys["ksk"]], dtype=object).reshape(D * t, n + 1)
        for fam, v in ks_reached(prm, ksk, rows[:3]).items():
            reached[fam] = max(reached.get(fam, 0), v)
    frac = {fam: None if bounds[fam.replace("_wave", "")] is None else reached[fam] / bounds[fam.replace("_wave", "")] for fam in reached}
    print(name, " ".join("%s=%s" % (f, "-" if v is None else "%.3f" % v) for f, v in frac.items()))
    for fam, v in frac.items():
        assert v is None or MIN_FRACTION <= v <= 1.0, (name, fam, v)
