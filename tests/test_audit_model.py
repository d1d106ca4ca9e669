"""The host side of the audit (tfhe_fbs_map_amd/audit.py) without a GPU: the cleartext value of every wire against the recorded
outputs of small goldens, the model's variance per wire against numbers worked out by hand, and the report's arithmetic on
synthetic fbs_audit_row values in Python ints and fractions."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import fixture_names, load_fixture

GOLDENS = (fixture_names("full_adder__*")[:3] + fixture_names("half_adder__*")[:2] + fixture_names("aoi21__*")[:2] +
           ["adder8__basic_p2", "adder8__search_p7", "adder8__search_p15", "2_input_gates__basic_p2", "2_input_gates__search_p7",
            "edge_outputs", "edge_nomerge"])


def lowered(name):
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"], merge_linear_prods="nomerge" not in name)
    return rec, env, env.lower()


@pytest.mark.parametrize("name", GOLDENS)
def test_cleartext_wires_give_the_recorded_outputs(name):
    """at the smallest p that fits the tables (where the longest table is longer than p: the negacyclic extension carries its tail),
    one more, and the p the mappers target"""
    from tfhe_fbs_map_amd import min_fbs_size, table_is_valid
    from tfhe_fbs_map_amd.audit import cleartext_wires
    rec, env, low = lowered(name)
    p_min = min_fbs_size(low["tables"])
    checked = 0
    for p in (p_min, p_min + 1, 7, 15, 31):
        if p < p_min or not all(table_is_valid(t, p) for t in low["tables"]):
            continue
        wires = cleartext_wires(low, rec["inputs"], p)
        assert wires.shape == (len(low["input_names"]) + len(low["kind"]), rec["T"]) and wires.dtype == np.int64
        for k, out in enumerate(low["out_names"]):
            w = low["out_wire"][k]
            if w < 0:
                assert -1 - w == rec["outputs"][out]
            else:
                assert np.array_equal(wires[w], rec["outputs"][out]), (name, p, out)
        checked += 1
    assert checked >= 2


def test_the_goldens_cover_multi_valued_and_long_tables():
    from tfhe_fbs_map_amd import min_fbs_size
    from tfhe_fbs_map_amd.audit import cleartext_wires
    rec, _, low = lowered("edge_outputs")
    assert [0, 1, 2, 3, 2] in low["tables"]                                   # multi-valued
    assert min_fbs_size(low["tables"]) == 3 < 5                               # ... and longer than p there
    t = low["tables"].index([0, 1, 2, 3, 2])
    gate = next(i for i, k in enumerate(low["kind"]) if k == 1 and low["arg1"][i] == t)
    n_in = len(low["input_names"])
    wires = cleartext_wires(low, rec["inputs"], 3)
    src = wires[low["arg0"][gate]]
    assert src.max() >= 3                                                     # the tail past p is reached: c - f(x - p)
    assert np.array_equal(wires[n_in + gate], np.array([0, 1, 2, 3, 2])[src])
    _, _, low = lowered("adder8__search_p15")
    assert max(len(t) for t in low["tables"]) > min_fbs_size(low["tables"])   # len > p


def test_table_lookup_restates_the_test_vector_contract():
    from tfhe_fbs_map_amd.audit import table_lookup
    # len <= p: the table, zero on the unreachable slots, the negative of both on the second half turn
    assert table_lookup([0, 1, 1], 5, np.arange(-2, 12)).tolist() == [0, 0, 0, 1, 1, 0, 0, 0, -1, -1, 0, 0, 0, 1]
    # len > p: table[x] + table[x + p] = c = 3, slots past the end read c - f
    t = [0, 1, 2, 3, 2]
    assert table_lookup(t, 3, np.arange(6)).tolist() == [0, 1, 2, 3, 2, 1]
    assert table_lookup(t, 3, [6, 7, -1, -6]).tolist() == [0, 1, 1, 0]
    with pytest.raises(ValueError):
        table_lookup([0, 1, 1, 1, 1], 3, [0])                                 # c = 0 + 1, but table[1] + table[4] = 2
    with pytest.raises(ValueError):
        table_lookup([0] * 7, 3, [0])                                         # longer than 2p


def hand_program(merge):
    """three levels: t = B(a + b), u = B(b + c); m = 2 t + u, then w = m + 3 t (a LinearProd of a LinearProd unless merged);
    v = B(w); z = v - 2 a (bootstrap output and fresh input in one sum); out = B(z)"""
    from tfhe_fbs_map_amd import LutExecEnv
    env = LutExecEnv(merge_linear_prods=merge)
    a, b, c = env.input("a"), env.input("b"), env.input("c")
    t = env.bootstrap(env.linear([1, 1], [a, b]), [0, 1, 1])
    u = env.bootstrap(env.linear([1, 1], [b, c]), [0, 1, 0])
    m = env.linear([2, 1], [t, u])
    w = env.linear([1, 3], [m, t])
    v = env.bootstrap(w, [0, 1, 0, 1, 1, 0, 1])
    z = env.linear([1, 2], [v, a])
    env.output("out", env.bootstrap(z, [0, 1, 1, 0]))
    return env


@pytest.mark.parametrize("merge", [True, False])
def test_predicted_variance_by_hand(merge):
    from tfhe_fbs_map_amd import MODULUS, Params
    from tfhe_fbs_map_amd.audit import predicted_variance
    from tfhe_fbs_map_amd.params import variances
    prm = Params(n=630, log_n_poly=10, l_bsk=3, beta_bsk=7, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1 << 20, sigma_glwe=1 << 10)
    v_br, v_ks, v_ms = variances(prm)
    v_in = (float(1 << 10) / MODULUS) ** 2
    env = hand_program(merge)
    low = env.lower()
    names = low["input_names"] + [i.name for i in env.instructions if not isinstance(i, type(env).Input)]
    wire, rot = predicted_variance(low, prm, fused=False)
    assert len(wire) == len(rot) == len(names)
    kinds = [None] * 3 + list(low["kind"])
    lin = [i for i, k in enumerate(kinds) if k == 0]
    boot = [i for i, k in enumerate(kinds) if k == 1]
    # merged: w = 2 t + u + 3 t as three terms (4 + 1 + 9 = 14 v_br: what independence makes of a wire met twice);
    # unmerged: m = 2 t + u (5 v_br) feeds w = m + 3 t (5 + 9 = 14 v_br): the same number by another road
    want_lin = [2 * v_in, 2 * v_in, 5 * v_br, 14 * v_br, v_br + 4 * v_in]
    assert len(lin) == 5 and len(boot) == 4
    for i, want in zip(lin, want_lin):
        assert wire[i] == pytest.approx(want, rel=1e-12), names[i]
        assert rot[i] == pytest.approx(want + v_ks + v_ms, rel=1e-12)
    for i in boot:
        assert wire[i] == pytest.approx(v_br, rel=1e-12)
    assert np.allclose(wire[:3], v_in, rtol=1e-12)
    if not merge:
        m, w = lin[2], lin[3]
        assert low["term_src"][low["arg0"][w - 3]] == m          # a LinearProd feeds a LinearProd


def test_predicted_variance_of_a_fused_program_by_hand():
    """three tables on one source: fused, each output carries its table's fusion factor -- here |D_F|^2 of [0,1,1] is 1 + 1 = 2
    (one step up, the flip back), of [0,0,1] the same, of [0,1,0] 1 + 1 + 0 = 2 -- and the LinearProd over them sums c^2 times those"""
    from tfhe_fbs_map_amd import LutExecEnv, Params
    from tfhe_fbs_map_amd.audit import predicted_variance
    from tfhe_fbs_map_amd.fbs_exec_env import table_fusion_factor
    from tfhe_fbs_map_amd.params import variances
    env = LutExecEnv()
    a, b = env.input("a"), env.input("b")
    s = env.linear([1, 1], [a, b])
    tables = [[0, 1, 1], [0, 0, 1], [0, 1, 0]]
    x, y, z = (env.bootstrap(s, t) for t in tables)
    only = env.bootstrap(env.linear([1, 2], [a, b]), [0, 1, 0, 1])      # the only reader of its source: never shared
    env.output("o", env.bootstrap(env.linear([1, 2, 3, 1], [x, y, z, only]), [0, 1, 0, 1, 1, 0, 1, 1]))
    low = env.lower()
    prm = Params(n=630, log_n_poly=10, l_bsk=3, beta_bsk=7, t_ksk=8, gamma_ksk=2, p_msg=11, sigma_lwe=1 << 20, sigma_glwe=1 << 10)
    v_br, v_ks, v_ms = variances(prm)
    f = [table_fusion_factor(t, 11) for t in tables]
    assert all(v >= 2.0 for v in f)
    n_in = 2
    boots = [n_in + i for i, k in enumerate(low["kind"]) if k == 1]
    lins = [n_in + i for i, k in enumerate(low["kind"]) if k == 0]
    plain, _ = predicted_variance(low, prm, fused=False)
    fused, rot = predicted_variance(low, prm, fused=True)
    assert [plain[w] for w in boots] == pytest.approx([v_br] * 5)
    assert [fused[w] for w in boots] == pytest.approx([f[0] * v_br, f[1] * v_br, f[2] * v_br, v_br, v_br])
    last = lins[-1]
    assert plain[last] == pytest.approx((1 + 4 + 9 + 1) * v_br)
    assert fused[last] == pytest.approx((f[0] + 4 * f[1] + 9 * f[2] + 1) * v_br)
    assert rot[last] == pytest.approx(fused[last] + v_ks + v_ms)


def synthetic_row(errors, unit, p, point="bootstrap", predicted_var=1e-12):
    """an AuditRow fed what the device would report for `errors` (Python ints), in two chunks"""
    from tfhe_fbs_map_amd.audit import AuditRow
    row = AuditRow(point, 0, 5, "m3", p, unit, predicted_var, norm2=1.0)
    half = len(errors) // 2
    for part in (errors[:half], errors[half:]):
        sq = sum(e * e for e in part)
        lo, hi = sq & ((1 << 64) - 1), sq >> 64
        over = sum(1 for e in part if 4 * p * abs(e) >= unit)
        row.add(dict(count=len(part), over=over, max_abs=max(map(abs, part)), sum=sum(part), sumsq=(hi << 64) | lo))
    return row


def test_report_arithmetic_in_ints_and_fractions():
    from tfhe_fbs_map_amd import MODULUS
    from tfhe_fbs_map_amd.audit import AuditReport
    q, p = MODULUS, 7
    big = (q - 1) // 2
    errors = [big, -big + 3, big - 1, 12345678901, -7, 0, 1 << 44, -(1 << 44)]
    row = synthetic_row(errors, q, p)
    assert row.sumsq >> 64 != 0                                         # the high word of the 128-bit sum is in play
    assert row.count == 8 and row.sum == sum(errors) and row.max_abs == big
    mean = Fraction(sum(errors), 8 * q)
    var = Fraction(sum(e * e for e in errors), 8 * q * q) - mean ** 2
    assert row.mean_exact == mean and row.var_exact == var
    assert row.mean == pytest.approx(float(mean)) and row.std == pytest.approx(math.sqrt(float(var)), rel=1e-12)
    assert row.margin == pytest.approx(float(Fraction(1, 4 * p) - abs(mean)) / math.sqrt(float(var)), rel=1e-12)
    assert row.worst == pytest.approx(float(Fraction(big, q) * 4 * p))
    assert row.over == sum(1 for e in errors if 4 * p * abs(e) >= q) == 5
    assert row.model_margin == pytest.approx((1 / 28) / 1e-6)
    # field units: 4pN a turn, the half box is N
    N = 1024
    ferr = [3, -5, 1023, -1024, 100, -100]
    frow = synthetic_row(ferr, 4 * p * N, p, point="rotation_input", predicted_var=(50.0 / (4 * p * N)) ** 2)
    assert frow.over == 1 and frow.worst == pytest.approx(1.0)          # 4p |e| >= 4pN  <=>  |e| >= N: only -1024
    fmean = Fraction(sum(ferr), 6 * 4 * p * N)
    fvar = Fraction(sum(e * e for e in ferr), 6 * (4 * p * N) ** 2) - fmean ** 2
    assert frow.var_exact == fvar and frow.margin == pytest.approx(float(Fraction(1, 4 * p) - abs(fmean)) / math.sqrt(float(fvar)))
    assert frow.model_margin == pytest.approx(N / 50.0)

    quiet = synthetic_row([10, -10, 20, -20], q, p)
    quiet.level, quiet.point, quiet.name = 1, "lincomb", "m9"
    frow.level = 1
    row.level = 2
    report = AuditReport([quiet, frow, row], outputs={"o": np.arange(3)}, asked_margin=6.0)
    assert report.failures == 6 and report.first_failure is frow         # level 1 before level 2, whatever the list order
    assert report.min_margin == min(quiet.margin, frow.margin, row.margin)
    assert report.worst(2) == sorted([quiet, frow, row], key=lambda r: r.margin)[:2]
    back = json.loads(report.to_json())
    assert back["failures"] == 6 and back["first_failure"]["name"] == "m3" and back["first_failure"]["point"] == "rotation_input"
    assert [r["over"] for r in back["rows"]] == [0, 1, 5] and back["rows"][0]["count"] == 4
    assert "first at level 1, rotation_input of m3" in report.summary()
    clean = AuditReport([quiet])
    assert clean.failures == 0 and clean.first_failure is None and "min margin" in clean.summary()


def test_a_row_without_spread_has_an_infinite_margin():
    row = synthetic_row([0, 0, 0, 0], 1 << 20, 7)
    assert row.std == 0 and row.margin == math.inf and row.worst == 0
