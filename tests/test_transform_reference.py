"""What tests/test_gpu_transforms.py stands on, checked without a GPU: the big-integer reference transforms (against Horner evaluation and,
through a product, against the oracle's two multiplications), the case generators (no input past an entry promise), the bounds table
(every figure where the header states it) and the coverage of fbs_debug_transform_list (every blind-rotation kernel of fbs_kernel_catalog
maps to a forward and an inverse line; every FIRST / BOUNDED a kernel template derives from its DIG is listed)."""
import os
import random
import re

import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import Q
from tests.test_gpu_transforms import BOUND_SOURCES, LANE_ENTRY, variant_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")


def variants():
    from tfhe_fbs_map_amd import _native
    return [H.parse_variant(l) for l in _native.debug_transform_list()]


@pytest.mark.parametrize("logn", [8, 9, 10, 11, 12])
def test_reference_ntt_is_evaluation_at_the_odd_powers_of_psi(logn):
    n = 1 << logn
    psi = H.twiddle_tables(logn)[0]
    assert pow(psi, n, Q) == Q - 1
    rng = random.Random(logn)
    coefs = [rng.randrange(-Q, Q) for _ in range(n)]
    out = H.reference_ntt(coefs, logn)
    where = H.point_positions(logn)
    assert len(where) == n
    for point in rng.sample(sorted(where), 16):
        acc = 0
        for c in reversed(coefs):
            acc = (acc * point + c) % Q
        assert out[where[point]] == acc
    assert H.reference_intt(out, logn) == [c * n % Q for c in coefs]
    # a part of a polynomial dealt over four waves: the sub-network at node 4 + w evaluates the part at positions w N/4 ..
    for w in range(4):
        part = coefs[:n // 4]
        sub = H.reference_ntt(part, logn, 4 + w)
        for point in rng.sample(sorted(where), 64):
            P = where[point]
            if P // (n // 4) != w:
                continue
            acc = 0
            for c in reversed(part):
                acc = (acc * point + c) % Q
            assert sub[P - w * (n // 4)] == acc
        assert H.reference_intt(sub, logn, 4 + w) == [c * (n // 4) % Q for c in part]


@pytest.mark.parametrize("logn", [8, 9, 10, 11, 12])
def test_reference_product_agrees_with_the_oracle(logn):
    from oracle import tfhe_oracle as orc
    n = 1 << logn
    rng = np.random.default_rng(logn)
    a, b = rng.integers(0, Q, n, dtype=np.uint64), rng.integers(0, Q, n, dtype=np.uint64)
    fa, fb = H.reference_ntt([int(x) for x in a], logn), H.reference_ntt([int(x) for x in b], logn)
    n_inv = pow(n, Q - 2, Q)
    c = [x * n_inv % Q for x in H.reference_intt([x * y % Q for x, y in zip(fa, fb)], logn)]
    assert c == [int(x) for x in orc.polymul_ntt(a, b)]
    assert c == [int(x) for x in orc.polymul_schoolbook(a, b)]


def test_every_generated_case_obeys_its_entry_promise():
    vs = variants()
    assert vs
    for v in vs:
        entry, exit_bound, scale, sources = variant_bounds(v)
        assert 0 < entry < 1 << 53 and 0 < exit_bound < 1 << 53 and sources
        if v["dir"] == "forward":
            # what the first stage is told about its inputs (first_butterfly, csrc/fbs_ntt.hpp)
            assert entry <= {0: LANE_OR_Q(v), 1: 1 << 8, 2: 1 << 6, 3: 1 << 6}[v["first"]]
        else:
            assert entry <= ((16 * Q - 1 if v["cls"] == "SplitNtt" else 8 * Q) if v["bounded"] else (1 << 52) - 1)
            assert scale == v["size"]
        names = set()
        for name, case in H.variant_cases(v, variant_bounds(v)[0]):
            assert len(case) == 1 << v["logn"] and max(abs(x) for x in case) <= entry, (v["line"], name)
            names.add(name)
        assert {"random", "all +", "all -"} <= names and all("alternating, stride 2^%d" % s in names for s in range(v["logn"]))
        assert all("extreme class %d" % c in names for c in range(4))
    # the extreme classes of N = 1024 are those of digit_cases
    v = H.parse_variant("class=SplitNtt logn=10 lanes=64 dir=forward first=3")
    mine = {name: case for name, case in H.variant_cases(v, variant_bounds(v)[0])}
    for name, digits in H.digit_cases():
        if name.startswith("extreme"):
            assert mine[name] == digits


def LANE_OR_Q(v):
    return LANE_ENTRY if v["cls"].startswith("LaneNtt") else Q


def test_bounds_are_where_the_headers_state_them():
    for key, (name, line, words) in BOUND_SOURCES.items():
        text = open(os.path.join(CSRC, name)).read()
        assert text.count(words) == 1, "%s: %s (near line %d) no longer says %r" % (key, name, line, words)
    used = set()
    for v in variants():
        used.update(variant_bounds(v)[3])
    assert used == set(BOUND_SOURCES)
    # the figures: everything a transform holds stays where fp_mulmod is exact
    for v in variants():
        entry, exit_bound, _, _ = variant_bounds(v)
        if v["dir"] == "forward":
            assert exit_bound < (1 << 53 if v["first"] == 3 else 1 << 52)
    assert LANE_ENTRY * 10 < 329 * Q and 64 + 32 * (Q - 1) + 11 * ((4 * Q) // 5) < 409 * Q // 10 < 2 ** 51.4
    assert LANE_ENTRY + 8 * ((4 * Q) // 5) < 393 * Q // 10 and LANE_ENTRY + 9 * ((4 * Q) // 5) < 401 * Q // 10


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def br_first(dig, fused):
    return (3 if fused else 2) if dig in (3, 7) else 1 if dig in (2, 6) else 0


def lines_of_kernel(name):
    """the (forward, inverse) lines of fbs_debug_transform_list a kernel of fbs_kernel_catalog runs, by the rules of its template"""
    def shape(logn, ll):
        cls = "PolyNtt" if logn <= 9 else "SplitNtt" if (logn, ll) == (10, 6) else "WavesNtt"
        return "class=%s logn=%d lanes=%d" % (cls, logn, 1 << ll)

    def lane(logn, nl):
        head = "class=%s logn=%d lanes=256" % ("LaneNtt256" if logn == 10 else "LaneNtt512", logn)
        return head + " dir=forward first=0 np=%d" % nl, head + " dir=inverse bounded=0"

    m = re.fullmatch(r"k_blind_rotate<(\d+),(\d+),(\d+),(\d+)(,false)?>", name)
    if m:
        logn, ll, dig = (int(m.group(i)) for i in (1, 2, 3))
        return (shape(logn, ll) + " dir=forward first=%d" % br_first(dig, (logn, ll) == (10, 6)),
                shape(logn, ll) + " dir=inverse bounded=%d" % (dig >= 1))
    m = re.fullmatch(r"k_blind_rotate_pairs<(\d+),(\d+),(\d+)>", name)
    if m:
        logn, ll, dig = (int(m.group(i)) for i in (1, 2, 3))
        return shape(logn, ll) + " dir=forward first=%d" % (2 if dig == 3 else 0), shape(logn, ll) + " dir=inverse bounded=1"
    m = re.fullmatch(r"k_blind_rotate_pairs_k2<(\d+),(\d+)>", name)
    if m:
        return shape(int(m.group(1)), 6) + " dir=forward first=0", shape(int(m.group(1)), 6) + " dir=inverse bounded=1"
    m = re.fullmatch(r"k_blind_rotate_glwe<(\d+),(\d),(\d),(\d+)>", name)
    if m:
        return shape(int(m.group(1)), 6) + " dir=forward first=0", shape(int(m.group(1)), 6) + " dir=inverse bounded=0"
    m = re.fullmatch(r"k_blind_rotate_cu<(\d+),(\d+),(\d+)(,lean)?>", name) or re.fullmatch(r"k_blind_rotate_cu_pairs<(\d+),(\d+)>", name)
    if m:
        return lane(int(m.group(1)), int(m.group(2)))
    if name == "k_blind_rotate_cu_k2":
        return lane(10, 1)
    return None


def test_every_blind_rotation_kernel_maps_to_listed_variants():
    from tfhe_fbs_map_amd import _native
    listed = set(_native.debug_transform_list())
    assert len(listed) == len(_native.debug_transform_list())
    reached = set()
    kernels = [k for k in _native.kernel_catalog() if k.startswith("k_blind_rotate")]
    assert len(kernels) > 100
    for k in kernels:
        lines = lines_of_kernel(k)
        assert lines is not None, "no rule for " + k
        for line in lines:
            assert line in listed, "%s runs %r, which fbs_debug_transform_list does not name" % (k, line)
        reached.update(lines)
    assert reached == listed, "listed but run by no kernel of the catalog: %s" % sorted(listed - reached)


def test_the_rules_are_the_kernel_templates():
    """the FIRST / BOUNDED a k_blind_rotate* template derives from its DIG, as the source states it, is what the rules above and
    csrc/fbs_debug_transform.hip restate -- and every value they can take is in the list"""
    br = open(os.path.join(CSRC, "fbs_blind_rotate.hip")).read()
    dbg = open(os.path.join(CSRC, "fbs_debug_transform.hip")).read()
    first = "(DIG == 3 || DIG == 7) ? (has_fused_opening<W>::value ? 3 : 2) : (DIG == 2 || DIG == 6) ? 1 : 0;"
    assert "constexpr int FIRST = " + first in br and "return " + first.replace("DIG", "dig") in dbg
    assert "constexpr bool BOUNDED = DIG >= 1;" in br and "constexpr bool br_bounded(int dig) { return dig >= 1; }" in dbg
    assert "constexpr int FIRST = DIG == 3 ? 2 : 0;" in br and "constexpr int pairs_first(int dig) { return dig == 3 ? 2 : 0; }" in dbg
    assert br.count("constexpr int FIRST =") == 2 and br.count("constexpr bool BOUNDED =") == 1
    assert "W::template inverse<true>(own, xc, t, twi, inv_uni);" in br
    k2 = open(os.path.join(CSRC, "fbs_blind_rotate_k2.hip")).read()
    assert "W::template forward<0>(x, xc, t, twf, typename W::NoHook{});" in k2 and "W::template inverse<true>(own, xc, t, twi" in k2
    assert "LaneNtt256::forward_multi<1, 0>(x, bufs, ln, tw.f," in k2
    glwe = open(os.path.join(CSRC, "fbs_blind_rotate_glwe.hip")).read()
    assert "W::template forward<0>(x, xc, t, twf, typename W::NoHook{});" in glwe and "W::template inverse<false>(own, xc, t, twi" in glwe
    cu = open(os.path.join(CSRC, "fbs_blind_rotate_cu.hpp")).read()
    assert "LaneNtt256::forward_multi<NL, 0>(" in cu and "LaneNtt512::forward_multi<NL, 0>(" in cu
    lines = [v["line"] for v in variants()]
    for dig in range(8):
        for fused in (False, True):
            assert any(l.endswith("dir=forward first=%d" % br_first(dig, fused)) for l in lines)
        assert any(l.endswith("dir=inverse bounded=%d" % (dig >= 1)) for l in lines)


def test_the_list_needs_no_gpu_and_the_hooks_need_a_context():
    from tfhe_fbs_map_amd import _native
    assert _native.lib.fbs_debug_transform(None, b"x", None, None, 1) == -1
    assert _native.lib.fbs_debug_field(None, 0, None, None, 0, None) == -1
