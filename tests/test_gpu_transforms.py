"""Every transform variant the blind-rotation kernels instantiate, alone on the device, at the edge of its stated range.

`fbs_debug_transform_list` names the variants (made from the lists the kernels are instantiated from), `fbs_debug_transform` runs one
in a workgroup the way the kernels call it, `fbs_debug_field` the field primitives element by element (csrc/fbs_debug_transform.hip).
References are big-integer transforms (tests/helpers.py, checked in tests/test_transform_reference.py); inputs sit AT the entry promise
a header states for the variant, in sign patterns that make every stage's sums (or differences) add up; every comparison is exact.
Layouts are never assumed: transforming the monomial X shows which evaluation point each output word holds."""
import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import Q

pytestmark = pytest.mark.gpu


# ---- entry promises and exit bounds, each where a header states it: (file, line at the time of writing, words of that line) ------------
# (tests/test_transform_reference.py holds the words against the headers, so a figure cannot change under this table unnoticed)
LANE_ENTRY = 64 + 32 * (Q - 1) + (4 * Q) // 5
BOUND_SOURCES = {
    "fwd first=0/1": ("fbs_ntt.hpp", 12, "every stage adds a product below 0.75 q"),
    "fwd first=1 entry": ("fbs_ntt.hpp", 44, "|b| <= 2^8"),
    "fwd first=2": ("fbs_ntt.hpp", 47, "64 + 32 (q - 1) + 11 * 0.8 q < 40.9 q"),
    "fwd first=3": ("fbs_ntt_split.hpp", 177, "ends below 105.5 q"),
    "fwd lane 256": ("fbs_ntt_lane.hpp", 122, "the eight stages end below 39.3 q"),
    "fwd lane 512": ("fbs_ntt_lane.hpp", 335, "|x| <= 64 + 32 (q - 1) + 0.8 q; the nine stages end below 40.1 q"),
    "inv PolyNtt": ("fbs_ntt.hpp", 242, "|x| < 2^52) -> N * coefficients (group-0 layout, |x| <= 8 q)"),
    "inv PolyNtt bounded": ("fbs_ntt.hpp", 243, "of |x| <= 8 q) is accepted"),
    "inv SplitNtt": ("fbs_ntt_split.hpp", 235, "(|x| < 2^52; BOUNDED: |x| < 16 q, which spares the first centring pass) -> N * coefficients (|x| <= 8 q)"),
    "inv WavesNtt": ("fbs_ntt_split.hpp", 418, "(|x| < 2^52; BOUNDED: |x| <= 8 q) -> N * coefficients, |x| <= 8 W q"),
    "inv LaneNtt256": ("fbs_ntt_lane.hpp", 185, "|x| < 2^52) -> 256 * coefficients of the part (layout A, |x| <= 8 q)"),
    "inv LaneNtt512": ("fbs_ntt_lane.hpp", 409, "|x| < 2^52) -> 512 * coefficients of the part (layout A, |x| <= 4 q)"),
}


def variant_bounds(v):
    """-> (entry promise, exit bound, scale of the inverse or None, keys of BOUND_SOURCES): |in| <= entry, |out| <= exit"""
    if v["dir"] == "forward":
        if v["cls"].startswith("LaneNtt"):   # FIRST = 0 behind the callers' cross stages
            stages = v["size"].bit_length() - 1
            return LANE_ENTRY, LANE_ENTRY + stages * ((4 * Q) // 5), None, ("fwd lane 256" if v["size"] == 256 else "fwd lane 512",)
        if v["first"] == 0:                  # what the callers supply: canonical residues, balanced digits
            return Q - 1, Q - 1 + v["logn"] * ((3 * Q) // 4), None, ("fwd first=0/1",)
        if v["first"] == 1:
            return 1 << 8, (1 << 8) + v["logn"] * ((3 * Q) // 4), None, ("fwd first=1 entry", "fwd first=0/1")
        if v["first"] == 2:
            return 64, 64 + 32 * (Q - 1) + (v["logn"] - 1) * ((4 * Q) // 5), None, ("fwd first=2",)
        return 64, (1055 * Q) // 10, None, ("fwd first=3",)
    wide = (1 << 52) - 1
    if v["cls"] == "PolyNtt":
        return (8 * Q if v["bounded"] else wide), 8 * Q, 1 << v["logn"], ("inv PolyNtt", "inv PolyNtt bounded")
    if v["cls"] == "SplitNtt":
        return (16 * Q - 1 if v["bounded"] else wide), 8 * Q, 1 << v["logn"], ("inv SplitNtt",)
    if v["cls"] == "WavesNtt":
        return (8 * Q if v["bounded"] else wide), 8 * (v["lanes"] // 64) * Q, 1 << v["logn"], ("inv WavesNtt",)
    return wide, (8 if v["size"] == 256 else 4) * Q, v["size"], ("inv " + v["cls"],)


def _variants():
    from tfhe_fbs_map_amd import _native
    return _native.debug_transform_list()


VARIANTS = _variants()
_ctx, _probe = {}, {}


def context(logn, k=1):
    """one context per (N, k); a variant for which none can be built fails here"""
    if (logn, k) not in _ctx:
        from tfhe_fbs_map_amd import Params, _native
        _ctx[logn, k] = _native.Context(Params(n=2, log_n_poly=logn, k=k, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=1 << 8), seed=3)
    return _ctx[logn, k]


def run(v, polys):
    """[polys][N] Python integers -> [polys][N] Python integers (a variant with np > 1 takes np polynomials side by side)"""
    pad = (-len(polys)) % v["np"]
    out = context(v["logn"]).debug_transform(v["line"], np.array(list(polys) + [polys[0]] * pad, dtype=np.int64))
    return [[int(x) for x in row] for row in out[:len(polys)]]


def forward_of(v):
    """the forward variant whose register order an inverse variant reads: same class, N and lanes"""
    return next(w for w in map(H.parse_variant, VARIANTS)
                if w["dir"] == "forward" and (w["cls"], w["logn"], w["lanes"]) == (v["cls"], v["logn"], v["lanes"]))


def probe(v):
    """position (of the whole polynomial's evaluation array) held by every word of the evaluation side, found by transforming the monomial X
    (of every part): word j then holds its evaluation point.  Asserts the points are the N distinct odd powers of psi."""
    f = v if v["dir"] == "forward" else forward_of(v)
    if f["line"] not in _probe:
        n, size = 1 << f["logn"], f["size"]
        mono = [1 if j % size == 1 else 0 for j in range(n)]
        points = [x % Q for x in run(f, [mono])[0]]
        where = H.point_positions(f["logn"])
        assert len(where) == n and sorted(points) == sorted(where), "the outputs for X are not the N distinct odd powers of psi"
        _probe[f["line"]] = [where[p] for p in points]
    return _probe[f["line"]]


def reference_by_position(v, values, fn):
    """fn = reference_ntt / reference_intt applied per part, parts back to back"""
    size, parts = v["size"], v["parts"]
    out = []
    for w in range(parts):
        out += fn(values[w * size:(w + 1) * size], v["logn"], parts + w if parts > 1 else 1)
    return out


# ---- primitives ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(H.FIELD_MODELS))
def test_field_primitive_equals_its_host_model(op):
    """~10^5 operands, edges included: the device's raw result (not its residue) is the value the literal host model gives -- what pins
    the instruction sequence (-ffp-contract=off, no reassociation) that tests/test_fused_opening.py replays."""
    x, w = H.field_operands()
    model = H.FIELD_MODELS[op]
    ctx = context(8)
    if op == "fp_u64_round_trip":
        x = [abs(a) & ((1 << 52) - 1) for a in x]
        want = [model(a) for a in x]
        got = ctx.debug_field(op, x)
    elif op.startswith("fp_mulmod"):
        want = [int(model(float(a), float(b))) for a, b in zip(x, w)]
        got = ctx.debug_field(op, x, w)
    else:
        want = [int(model(float(a))) for a in x]
        got = ctx.debug_field(op, x)
    bad = [i for i, (g, e) in enumerate(zip(got.tolist(), want)) if g != e]
    assert not bad, "%s: %d of %d differ, first x=%d w=%d: device %d, model %d" % (op, len(bad), len(x), x[bad[0]], w[bad[0]], got[bad[0]], want[bad[0]])
    if op == "fp_mulmod":   # and the model's value is the residue, inside the range fbs_field.hpp states for |x| < 2^53
        assert all((g - a * b) % Q == 0 and abs(g) * 1000 < 1236 * Q for g, a, b in zip(got.tolist(), x, w))


# ---- layout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", [l for l in VARIANTS if "dir=forward" in l])
def test_layout_probe(line):
    v = H.parse_variant(line)
    pos = probe(v)
    assert sorted(pos) == list(range(1 << v["logn"]))
    if v["parts"] > 1:   # wave w holds part w: positions w M .. (w + 1) M - 1
        e = (1 << v["logn"]) // v["lanes"]
        assert all(pos[j] // v["size"] == (j // e) // 64 for j in range(len(pos)))


# ---- forward and inverse, every variant --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", VARIANTS)
def test_variant_at_the_edge_of_its_promise(line):
    v = H.parse_variant(line)
    entry, exit_bound, scale, _ = variant_bounds(v)
    pos = probe(v)
    n = 1 << v["logn"]
    cases = list(H.variant_cases(v, entry))
    if v["dir"] == "forward":
        got = run(v, [c for _, c in cases])
        for (name, c), out in zip(cases, got):
            want = reference_by_position(v, c, H.reference_ntt)
            bad = [j for j in range(n) if out[j] % Q != want[pos[j]]]
            assert not bad, "%s, %s: %d residues differ, first at word %d" % (line, name, len(bad), bad[0])
            peak = max(abs(x) for x in out)
            print("%s | %s | max |out| = %.3f q (bound %.3f q)" % (line, name, peak / Q, exit_bound / Q))
            assert peak <= exit_bound, "%s, %s: max |out| = %d = %.3f q above the stated %.3f q" % (line, name, peak, peak / Q, exit_bound / Q)
    else:
        # cases are by position; word j of the input holds position pos[j]
        got = run(v, [[c[pos[j]] for j in range(n)] for _, c in cases])
        for (name, c), out in zip(cases, got):
            want = reference_by_position(v, c, H.reference_intt)     # scale * coefficients: the network's own 2^stages
            assert scale == v["size"]
            bad = [j for j in range(n) if out[j] % Q != want[j]]
            assert not bad, "%s, %s: %d residues differ, first at coefficient %d" % (line, name, len(bad), bad[0])
            peak = max(abs(x) for x in out)
            print("%s | %s | max |out| = %.3f q (bound %.3f q)" % (line, name, peak / Q, exit_bound / Q))
            assert peak <= exit_bound, "%s, %s: max |out| = %d = %.3f q above the stated %.3f q" % (line, name, peak, peak / Q, exit_bound / Q)


# ---- tie to the host replay ----------------------------------------------------------------------------------------------------
def test_device_equals_the_host_replay_of_the_fused_opening():
    """SplitNtt<10,6>, FIRST = 3 and inverse<true>: the device's raw values are those of forward_fused / inverse_bounded
    (tests/helpers.py, what tests/test_fused_opening.py proves the ranges on), value for value, on digit_cases()."""
    fwd = H.parse_variant("class=SplitNtt logn=10 lanes=64 dir=forward first=3")
    inv = H.parse_variant("class=SplitNtt logn=10 lanes=64 dir=inverse bounded=1")
    assert fwd["line"] in VARIANTS and inv["line"] in VARIANTS
    pos = probe(fwd)
    cases = list(H.digit_cases())
    replay = [H.forward_fused(d) for _, d in cases]
    got = run(fwd, [d for _, d in cases])
    for (name, _), out, x in zip(cases, got, replay):
        assert out == [int(x[pos[j]]) for j in range(H.N)], name
    sums = [H.key_product_sums(name, x) for (name, _), x in zip(cases, replay)]
    back = run(inv, [[int(s[pos[j]]) for j in range(H.N)] for s in sums])
    for (name, _), out, s in zip(cases, back, sums):
        assert out == [int(x) for x in H.inverse_bounded(s)], name


# ---- the hook refuses what it cannot run -----------------------------------------------------------------------------------------
def test_hook_refuses_a_context_of_another_size_and_unknown_variants():
    from tfhe_fbs_map_amd import FbsError
    zeros = np.zeros((1, 256), np.int64)
    for line in ("class=SplitNtt logn=10 lanes=64 dir=forward first=3", "class=SplitNtt logn=8 lanes=64 dir=forward first=0"):
        with pytest.raises(FbsError) as e:
            context(8).debug_transform(line, zeros)
        assert e.value.code == -1
