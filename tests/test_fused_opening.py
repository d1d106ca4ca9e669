"""The fused opening of the digit transforms (csrc/fbs_ntt_split.hpp `first_two_stages`, FIRST = 3) and the lazy ranges that
follow it, replayed on the host.

Every value on that path is an integer-valued double, so each device instruction is restated here as the exact integer
operation followed by IEEE round-to-nearest-even (Python's int -> float conversion), which is what the FP64 unit does:
v_mul_f64 / v_fma_f64 / v_add_f64 on integers, and x * (1/q) and rint on the one non-integer product.  The transforms run
in the device's order of butterflies (which pair, which twiddle, which operand is reduced); the split schedule only moves
values between lanes and LDS, which changes no value.  Results are compared with an integer negacyclic NTT mod q, every
sum and FMA is asserted to be exact, and every stage is checked against the worst-case bounds derived in the comments
of fbs_field.hpp (fp_mulmod) and fbs_ntt_split.hpp (first_two_stages, inv_group)."""
import math
import os
import random
import re
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")

# the device's FP64 instructions on integer-valued doubles, the twiddles, the worst-case bounds and the replayed transforms:
# tests/helpers.py (shared with tests/test_gpu_transforms.py, which holds them against the device)
from tests.helpers import (Q, QINV, LOGN, N, TWO53, HALF, rnd, exact, fma, fp_mulmod, fp_center, centred, bitrev, PSI, TW, TWI, W12, W13, EPS1, half_ulp, rho,
                           OPENING, FWD_BOUNDS, PRODUCT, first_two_stages, ct_stage, forward_fused, forward_int, inverse_bounded, inverse_int,
                           digit_cases)  # noqa: E402,F401


# ---- the tests -----------------------------------------------------------------------------------------------------
def test_header_layout_and_bounds_as_stated():
    field = open(os.path.join(CSRC, "fbs_field.hpp")).read()
    assert "constexpr uint32_t tw_fused_word(uint32_t n) { return 3 * n; }" in field
    assert "constexpr uint32_t tw_table_words(uint32_t n) { return 3 * n + 2; }" in field
    host = open(os.path.join(CSRC, "fbs_host.cpp")).read()
    assert re.search(r"fwd\[tw_fused_word\(N\)\] = fq_mul\(fwd\[1\], fwd\[2\]\);", host)
    assert re.search(r"fwd\[tw_fused_word\(N\) \+ 1\] = fq_mul\(fwd\[1\], fwd\[3\]\);", host)
    # the figures the comments quote
    assert float(EPS1) < 2.0 ** -54.09
    assert rho(TWO53 - 1) < Fraction(1236, 1000) * Q
    assert OPENING < 96 * Q < Fraction(3, 2) * 2 ** 52
    assert FWD_BOUNDS[-1] < Fraction(1055, 10) * Q and FWD_BOUNDS[-1] < 2 ** 52.73
    assert PRODUCT < Fraction(12, 10) * Q
    assert 10 * PRODUCT < 16 * Q and 8 * 16 * Q < TWO53   # l <= 5: 2l products enter the uncentred inverse group


@pytest.mark.parametrize("w", [TW[1], TW[2], TW[3], W12, W13, HALF, -HALF, 1, -1, 12345678901])
def test_fp_mulmod_exact_up_to_2_53(w):
    rng = random.Random(w & 0xFFFF)
    xs = [TWO53 - 1, -(TWO53 - 1), 2 ** 52 + 1, 3 * 2 ** 51 - 7] + [rng.randrange(-(TWO53 - 1), TWO53) for _ in range(2000)]
    for x in xs:
        r = fp_mulmod(float(x), float(w))
        assert (int(r) - x * w) % Q == 0
        assert abs(r) <= rho(abs(x)) < Fraction(1236, 1000) * Q


@pytest.mark.parametrize("name,digits", list(digit_cases()))
def test_fused_opening_matches_two_stages(name, digits):
    y = first_two_stages([float(d) for d in digits])
    assert max(abs(v) for v in y) <= OPENING
    # the first two Cooley-Tukey stages, in integers mod q
    x = [d % Q for d in digits]
    for s in range(2):
        half = N >> (s + 1)
        for blk in range(1 << s):
            w = TW[(1 << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half] * w
                x[i], x[i + half] = (u + v) % Q, (u - v) % Q
    assert [int(v) % Q for v in y] == x


@pytest.mark.parametrize("name,digits", list(digit_cases()))
def test_transform_products_and_inverse(name, digits):
    x = forward_fused(digits, FWD_BOUNDS)
    assert [int(v) % Q for v in x] == forward_int(digits)
    # one step at l = 5 (the most DIG = 3 allows): ten key products per evaluation, own and partner's sums added
    rng = random.Random(len(name))
    own = [0.0] * N
    for _ in range(10):
        key = [rng.choice((HALF, -HALF, rng.randrange(-HALF, HALF + 1))) for _ in range(N)]
        prod = [fp_mulmod(v, float(k)) for v, k in zip(x, key)]
        assert max(abs(p) for p in prod) <= PRODUCT
        own = [exact(int(o) + int(p)) for o, p in zip(own, prod)]
    assert max(abs(v) for v in own) < 10 * PRODUCT < 16 * Q
    got = inverse_bounded(own)
    assert [int(v) % Q for v in got] == inverse_int([int(v) for v in own])
