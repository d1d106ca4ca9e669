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

Q = 0x3FFFFFF84001
QINV = 1.0 / Q
LOGN, N = 10, 1024
TWO53 = 1 << 53
HALF = (Q - 1) // 2


# ---- the device's FP64 instructions on integer-valued doubles --------------------------------------------------------
def rnd(v):
    """round an exact integer to the nearest double (ties to even), as the FP64 unit does"""
    return float(v)


def exact(v):
    f = float(v)
    assert int(f) == v, "inexact: %d" % v
    return f


def fma(a, b, c):
    return rnd(int(a) * int(b) + int(c))


def fp_mulmod(x, w):
    h = rnd(int(x) * int(w))
    l = exact(int(x) * int(w) - int(h))              # fma(x, w, -h): the exact remainder
    qh = round(h * QINV)                              # rint(h * QINV), ties to even
    r0 = exact(int(h) - qh * Q)                       # fma(-qh, q, h)
    return exact(int(r0) + int(l))                    # r0 + l


def fp_center(x):
    return exact(int(x) - round(x * QINV) * Q)


def centred(v):
    v %= Q
    return v - Q if v > Q // 2 else v


# ---- twiddles as host_twiddles makes them (fbs_host.cpp), centred as uploaded ----------------------------------------
def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


PSI = pow(7, (Q - 1) // (2 * N), Q)
TW = [centred(pow(PSI, bitrev(i, LOGN), Q)) for i in range(N)]
TWI = [centred(pow(pow(PSI, Q - 2, Q), bitrev(i, LOGN), Q)) for i in range(N)]
W12, W13 = centred(TW[1] * TW[2]), centred(TW[1] * TW[3])   # tw_fused_word(N), tw_fused_word(N) + 1


# ---- worst-case bounds (the proofs in the headers, evaluated exactly) ------------------------------------------------
EPS1 = abs(Fraction(QINV) * Q - 1)


def half_ulp(x):
    """half an ulp of a double of magnitude at most x"""
    e = math.floor(math.log2(x))
    if Fraction(2) ** (e + 1) <= x:
        e += 1
    return Fraction(2) ** (e - 53)


def rho(x_max):
    """bound on |fp_mulmod(x, w)| for |x| <= x_max < 2^53 and |w| <= (q-1)/2"""
    assert x_max < TWO53
    h = Fraction(x_max) * HALF
    h += half_ulp(h)
    z = h / Q * (1 + EPS1)
    z += half_ulp(z)
    return Q * (Fraction(1, 2) + h / Q * EPS1 + half_ulp(z)) + half_ulp(h)


OPENING = 64 + 96 * (Q - 1)          # |a + al c + be b + ga d|, |digit| <= 64, |coefficient| <= (q-1)/2
FWD_BOUNDS = [Fraction(OPENING)]      # after the opening and after each of the 8 remaining stages
for _ in range(8):
    FWD_BOUNDS.append(FWD_BOUNDS[-1] + rho(FWD_BOUNDS[-1]))
PRODUCT = rho(FWD_BOUNDS[-1])         # one key product


# ---- the transforms ------------------------------------------------------------------------------------------------
def first_two_stages(x):
    """SplitNtt::first_two_stages: registers (r, r+4, r+8, r+12) of a lane are coefficients j, j+256, j+512, j+768"""
    y = list(x)
    w1, w2, w3 = TW[1], TW[2], TW[3]
    for j in range(N // 4):
        a, b, c, d = x[j], x[j + 256], x[j + 512], x[j + 768]
        s, u = fma(c, w1, a), fma(-c, w1, a)
        y[j] = fma(d, W12, fma(b, w2, s))
        y[j + 256] = fma(-d, W12, fma(-b, w2, s))
        y[j + 512] = fma(-d, W13, fma(b, w3, u))
        y[j + 768] = fma(d, W13, fma(-b, w3, u))
    return y


def ct_stage(x, s):
    """Cooley-Tukey stage s: blocks of N >> s, twiddle tw[2^s + block]; only the multiplied operand is reduced"""
    half = N >> (s + 1)
    for blk in range(1 << s):
        w = TW[(1 << s) + blk]
        for i in range(blk * 2 * half, blk * 2 * half + half):
            u, v = x[i], fp_mulmod(x[i + half], w)
            x[i], x[i + half] = exact(int(u) + int(v)), exact(int(u) - int(v))


def forward_fused(digits, bounds=None):
    x = first_two_stages([float(d) for d in digits])
    seen = [max(abs(v) for v in x)]
    for s in range(2, LOGN):
        ct_stage(x, s)
        seen.append(max(abs(v) for v in x))
    if bounds is not None:
        for got, lim in zip(seen, bounds):
            assert got <= lim < TWO53
    return x


def forward_int(coefs):
    x = [c % Q for c in coefs]
    for s in range(LOGN):
        half = N >> (s + 1)
        for blk in range(1 << s):
            w = TW[(1 << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half] * w
                x[i], x[i + half] = (u + v) % Q, (u - v) % Q
    return x


def inverse_bounded(x):
    """SplitNtt::inverse<true>: GS stages 9..7 uncentred (entry promise |x| < 16 q), centring before 6..4 and 3..1, then the
    joining stage 0; returns N * coefficients"""
    x = list(x)
    assert max(abs(v) for v in x) < 16 * Q
    for stages, centre in (((9, 8, 7), False), ((6, 5, 4), True), ((3, 2, 1), True), ((0,), False)):
        if centre:
            x = [fp_center(v) for v in x]
        for s in stages:
            half = N >> (s + 1)
            for blk in range(1 << s):
                w = TWI[(1 << s) + blk]
                for i in range(blk * 2 * half, blk * 2 * half + half):
                    u, v = x[i], x[i + half]
                    x[i] = exact(int(u) + int(v))
                    x[i + half] = fp_mulmod(exact(int(u) - int(v)), w)
            assert max(abs(v) for v in x) < 128 * Q < TWO53
    return x


def inverse_int(x):
    x = [v % Q for v in x]
    for s in range(LOGN - 1, -1, -1):
        half = N >> (s + 1)
        for blk in range(1 << s):
            w = TWI[(1 << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half]
                x[i], x[i + half] = (u + v) % Q, (u - v) * w % Q
    return x


def digit_cases():
    rng = random.Random(7)
    yield "random", [rng.randrange(-64, 64) for _ in range(N)]
    yield "all -64", [-64] * N
    yield "alternating +-64", [64 if i % 2 else -64 for i in range(N)]
    # the largest opening each output class can reach: every digit at 64 with the sign of its coefficient
    for cls, coef in enumerate(((1, TW[1], TW[2], W12), (1, TW[1], -TW[2], -W12), (1, -TW[1], TW[3], -W13), (1, -TW[1], -TW[3], W13))):
        sgn = [64 if c >= 0 else -64 for c in coef]   # (a, c, b, d) of the class
        yield "extreme class %d" % cls, [sgn[0]] * 256 + [sgn[2]] * 256 + [sgn[1]] * 256 + [sgn[3]] * 256


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
