"""Shared by the test modules: fixture loading and an oracle-backed program evaluator."""
import glob
import gzip
import json
import math
import os
import random
import re
import struct
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_names(pattern="*"):
    names = (os.path.basename(p)[:-len(".json.gz")] for p in glob.glob(os.path.join(GOLDEN, pattern + ".json.gz")))
    return sorted(n for n in names if not n.startswith("_"))        # _*.json.gz: collections, not one program each


def _decode(v):
    if "const" in v:
        return int(v["const"])
    if "bits" in v:
        raw = np.frombuffer(bytes.fromhex(v["bits"]), np.uint8)
        return np.unpackbits(raw)[:v["n"]].astype(np.int64)
    return np.asarray(v["ints"], np.int64)


_cache = {}


def load_fixture(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rb") as f:
            rec = json.loads(f.read().decode())
        rec["inputs"] = {k: _decode(v) for k, v in rec["inputs"].items()}
        rec["outputs"] = {k: _decode(v) for k, v in rec["outputs"].items()}
        if rec.get("outputs_bitenv"):
            rec["outputs_bitenv"] = {k: _decode(v) for k, v in rec["outputs_bitenv"].items()}
        _cache[name] = rec
    return _cache[name]


def toy_k2(p_msg=7, n=12, beta=21):
    """A toy set of the k = 2 shape (GLWE dimension 2 at N = 1024, one gadget level, two key bits per step): n small enough for
    the CPU oracle to bootstrap in milliseconds, real N so that the kernels are the shipped ones (k_blind_rotate_pairs_k2 and
    the whole-CU k = 2 shape, ct_words = 2049 through k_lincomb and the level calls)."""
    from tfhe_fbs_map_amd import Params
    return Params(n=n, log_n_poly=10, k=2, l_bsk=1, beta_bsk=beta, t_ksk=8, gamma_ksk=2, p_msg=p_msg, sigma_lwe=1 << 8, sigma_glwe=4,
                  bsk_group=2)


def toy_k3(p_msg=7, n=12, beta=18):
    """A toy set of the k = 3 shape the default 128-bit sets for p <= 8 run on (GLWE dimension 3 at N = 512, one gadget level, two key
    bits per step: k_blind_rotate_glwe, ciphertexts of 3 N + 1 = 1537 words, accumulator rows of 4 N)."""
    from tfhe_fbs_map_amd import Params
    return Params(n=n, log_n_poly=9, k=3, l_bsk=1, beta_bsk=beta, t_ksk=8, gamma_ksk=2, p_msg=p_msg, sigma_lwe=1 << 8, sigma_glwe=4,
                  bsk_group=2)


def toy_glwe(k, p_msg=7, n=12):
    """toy_k2 / toy_k3 by GLWE dimension"""
    return toy_k2(p_msg, n) if k == 2 else toy_k3(p_msg, n)


def subsample(rec, T):
    """First T samples of the harness inputs and of the expected outputs."""
    ins = {k: v[:T] for k, v in rec["inputs"].items()}
    outs = {k: (v if isinstance(v, int) else v[:T]) for k, v in rec["outputs"].items()}
    return ins, outs


def assert_outputs_equal(got, expected):
    assert set(got.keys()) == set(expected.keys())
    for k, e in expected.items():
        g = got[k]
        if isinstance(e, int):
            assert isinstance(g, (int, np.integer)) or np.ndim(g) == 0, k
            assert int(g) == e, k
        else:
            assert np.array_equal(np.asarray(g).reshape(-1), e), "output %s differs" % k


def oracle_eval_program(orc, ops, outputs, in_cts, fuse=False):
    """Run a program (oracle.lut_oracle.read_fbs form) on ciphertexts with the C oracle.
    in_cts: {input name: [T][ct_words]}.  Returns {wire name: [T][ct_words]} for all wires.
    fuse: a wire that two or more bootstraps read is rotated once and every table cut out of that accumulator
    (oracle bootstrap_multi) -- what a program loaded with FBS_LOAD_FUSE_TABLES computes."""
    wires = dict(in_cts)
    T = len(next(iter(in_cts.values()))) if in_cts else 1
    readers = {}
    for op in ops:
        if op[0] == "boot":
            readers.setdefault(op[2], []).append(op)
    for op in ops:
        if op[0] == "lin":
            _, name, terms, const = op
            out = np.empty((T, orc.ctw), np.uint64)
            for s in range(T):
                out[s] = orc.lincomb([wires[src][s] for _, src in terms], [c for c, _ in terms], const)
            wires[name] = out
        elif fuse and len(readers[op[2]]) >= 2:
            if op[1] in wires:
                continue                                        # computed with the first gate of its source
            group = readers[op[2]]
            res = orc.bootstrap_multi(wires[op[2]], [g[3] for g in group])
            for g, r in zip(group, res):
                wires[g[1]] = r
        else:
            _, name, src, table = op
            res, _ = orc.bootstrap_batch(wires[src], [table], None)
            wires[name] = res
    return wires


# ---- kernel selection: which parameter set, batch size and knobs reach each instantiation of fbs_kernel_catalog ----
CUS = 256

# what the selection derives DIG from (csrc/fbs_select.cpp): l > 5 -> 0; l = 1 -> 4; l = 2 -> 4 + by_beta; else by_beta,
# by_beta = 3 for beta <= 7, 2 for beta <= 9, 1 otherwise
GADGET_OF_DIG = {0: (6, 4), 1: (3, 10), 2: (3, 8), 3: (3, 7), 4: (1, 20), 5: (2, 10), 6: (2, 8), 7: (2, 7)}


def recipe(name):
    """-> dict(log_n, l, beta, group, count, knobs) that makes the launcher pick `name`"""
    m = re.fullmatch(r"k_blind_rotate<(\d+),(\d+),(\d+),(\d+)(,false)?>", name)
    if m:
        L, LL, dig, fpw = (int(m.group(i)) for i in range(1, 5))
        l, beta = GADGET_OF_DIG[dig]
        main_ll = 6 if L <= 10 else L - 4
        knobs = {}
        if m.group(5):                                    # no priority hand-over: two-level N = 1024 sets beyond two rounds
            count = 8 * CUS + 60
        elif fpw == 4:                                    # whole rounds of the benchmark shape
            count = 4 * CUS
        elif fpw == 2:                                    # between one and two bootstraps per CU, two per workgroup
            count, knobs = CUS + 44, dict(br_cu_kernel=0)
        elif LL != main_ll:                               # N = 1024 / 2048 on four waves per polynomial, generic kernel
            count, knobs = 40, dict(br_cu_kernel=0)
        elif L in (10, 11):                               # main shape: more than two bootstraps per CU (below, the one-per-CU shapes)
            count = 2 * CUS + 88
        else:
            count = 40
        return dict(log_n=L, l=l, beta=beta, group=1, count=count, knobs=knobs)
    m = re.fullmatch(r"k_blind_rotate_pairs<(\d+),(\d+),(\d+)>", name)
    if m:
        L, dig = int(m.group(1)), int(m.group(3))
        l, beta = {4: (1, 20), 3: (2, 7), 0: (2, 10)}[dig]
        # (N = 2048 with two levels goes to the whole-CU kernel whatever the size: the A/B switch brings the generic one back)
        return dict(log_n=L, l=l, beta=beta, group=2, count=CUS + 40 if (L, l) == (11, 1) else 40,
                    knobs=dict(br_cu_kernel=0) if (L, l) == (11, 2) else {})
    if name == "k_blind_rotate_cu_pairs<11,1>":           # two key bits per step on a whole CU: up to one bootstrap per CU
        return dict(log_n=11, l=1, beta=20, group=2, count=CUS - 9, knobs={})
    if name == "k_blind_rotate_cu_pairs<11,2>":           # ... with two gadget levels: every launch, round after round
        return dict(log_n=11, l=2, beta=10, group=2, count=CUS + 21, knobs={})
    m = re.fullmatch(r"k_blind_rotate_pairs_k2<10,(\d)>", name)
    if m:                                                 # GLWE dimension k = 2 on three waves per bootstrap: one, two or four bootstraps per
        fpw = int(m.group(1))                             # workgroup, a ragged last one (up to three per CU the launcher prefers the shape below)
        return dict(log_n=10, l=1, beta=20, group=2, k=2, count={1: 41, 2: CUS + 41, 4: 3 * CUS + 41}[fpw],
                    knobs={} if fpw == 4 else dict(br_k2_shape=3))
    if name == "k_blind_rotate_cu_k2":                    # ... one bootstrap on the twelve waves of a workgroup: two rounds, the second partial
        return dict(log_n=10, l=1, beta=20, group=2, k=2, count=CUS + 41, knobs={})
    m = re.fullmatch(r"k_blind_rotate_glwe<(\d+),(\d),(\d),(\d)>", name)
    if m:                                                 # every other GLWE dimension / size / depth: k + 1 waves per bootstrap, two gadget levels
        L, k1, group, fpw = (int(m.group(i)) for i in (1, 2, 3, 4))   # (k = 2 at N = 1024 with one level and two key bits per step has its own kernels);
        # one bootstrap per workgroup up to one per CU, two up to two, the throughput shape beyond: a ragged last workgroup each time
        return dict(log_n=L, l=2, beta=8, group=group, k=k1 - 1, count={1: 41, 2: CUS + 41}.get(fpw, 2 * CUS + 41), knobs={})
    m = re.fullmatch(r"k_blind_rotate_cu<(\d+),(\d+),(\d+)(,lean)?>", name)
    if m:
        L, nl, first = int(m.group(1)), int(m.group(2)), int(m.group(3))
        beta = {2: 7, 1: 9, 0: 10}[first]
        if nl * beta > 30:
            beta = 30 // nl
        if m.group(4):                                    # two workgroups per CU: between one and two bootstraps per CU
            return dict(log_n=L, l=nl, beta=beta, group=1, count=CUS + 70, knobs=dict(br_cu_lean=1))
        return dict(log_n=L, l=nl, beta=beta, group=1, count=CUS + 3 if nl == 3 or (L, nl) == (11, 2) else 40, knobs=dict(br_cu_lean=0))
    ks = {"k_ks_gemm<2,2> (int8 MFMA)": (40, {}), "k_keyswitch_fp<8,2,8>": (70, dict(ks_mfma=0)),
          "k_keyswitch_lanes<8,2,8>": (70, dict(ks_mfma=0, ks_fp=0)), "k_keyswitch_lanes<8,1,4>": (40, dict(ks_mfma=0)),
          "k_keyswitch<8>": (9, dict(ks_mfma=0))}
    if name in ks:
        count, knobs = ks[name]
        return dict(log_n=9, l=2, beta=8, group=1, count=count, knobs=knobs)
    return None


# ==== the device's exact FP64 arithmetic, replayed on the host (tests/test_fused_opening.py, tests/test_gpu_transforms.py) ====
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


# ---- the other field primitives of csrc/fbs_field.hpp, as literally as fp_mulmod and fp_center above -------------------------------
def fp_mulmod_exact(x, w):
    h = rnd(int(x) * int(w))                          # x * w (exact where the contract holds, rounded where it does not)
    return rnd(int(h) - round(h * QINV) * Q)          # fma(-rint(h * QINV), q, h)


def fp_canon(x):
    c = fp_center(x)
    return c + Q if c < 0.0 else c


def fp_canon_near(x):
    return rnd(int(x) - math.floor(x * QINV) * Q)     # fma(-floor(x * QINV), q, x)


def fp_u64_round_trip(v):
    """fp_to_u64(fp_from_u64(v)), 0 <= v < 2^52, through the bit patterns the device builds"""
    d = struct.unpack("<d", struct.pack("<Q", v | 0x4330000000000000))[0] - 4503599627370496.0
    return struct.unpack("<Q", struct.pack("<d", d + 4503599627370496.0))[0] & 0x000FFFFFFFFFFFFF


FIELD_MODELS = {"fp_mulmod": fp_mulmod, "fp_mulmod_exact": fp_mulmod_exact, "fp_center": fp_center, "fp_canon": fp_canon,
                "fp_canon_near": fp_canon_near, "fp_u64_round_trip": fp_u64_round_trip}


def field_operands(count=100000, seed=11):
    """-> (x, w): `count` operand pairs, |x| < 2^53 and |w| <= (q-1)/2: every edge x against every edge w, then random ones"""
    xs = [s * v for s in (1, -1) for v in ((1 << 50) - 1, (1 << 52) - 1, (1 << 53) - 1, HALF)]
    xs += [s * k * Q + d for s in (1, -1) for k in range(13) for d in (0, 1, -1)]
    ws = [HALF, -HALF, 1, -1, W12, W13] + TW[1:8] + TWI[1:8]
    pairs = [(x, w) for x in xs for w in ws]
    rng = random.Random(seed)
    while len(pairs) < count:
        span = rng.choice((1 << 53, 1 << 52, 1 << 50, 16 * Q, Q))
        pairs.append((rng.randrange(-span + 1, span), rng.choice((rng.randrange(-HALF, HALF + 1), rng.choice(ws), rng.choice(TW)))))
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ==== big-integer reference transforms and the cases of tests/test_gpu_transforms.py ================================================
# The negacyclic NTT as the textbook in-place Cooley-Tukey network on Python integers: stage s pairs positions N >> (s + 1) apart in
# blocks of N >> s, block b under tw[2^s + b], tw[i] = psi^bitrev(i) (host_twiddles, csrc/fbs_host.cpp); position P then holds the
# value at psi^(2 bitrev(P) + 1).  `root`: the node of the twiddle tree the network hangs from -- 1 for a whole polynomial; W + w for
# part w of a polynomial dealt over W waves, a transform of N / W points whose positions are positions w N / W .. of the whole.
_tables = {}


def twiddle_tables(logn):
    """-> (psi, tw, tw_inv) of N = 2^logn as canonical residues"""
    if logn not in _tables:
        psi = pow(7, (Q - 1) >> (logn + 1), Q)
        ipsi = pow(psi, Q - 2, Q)
        _tables[logn] = (psi, [pow(psi, bitrev(i, logn), Q) for i in range(1 << logn)], [pow(ipsi, bitrev(i, logn), Q) for i in range(1 << logn)])
    return _tables[logn]


def reference_ntt(coefs, logn, root=1):
    """coefficients (natural order) of a (part of a) polynomial of N = 2^logn -> residues by position"""
    tw = twiddle_tables(logn)[1]
    x = [c % Q for c in coefs]
    size, s = len(x), 0
    while (size >> s) > 1:
        half = size >> (s + 1)
        for blk in range(1 << s):
            w = tw[(root << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half] * w % Q
                x[i], x[i + half] = (u + v) % Q, (u - v) % Q
        s += 1
    return x


def reference_intt(values, logn, root=1):
    """residues by position -> len(values) * coefficients (natural order) mod q: the Gentleman-Sande mirror image, unscaled as on the device"""
    twi = twiddle_tables(logn)[2]
    x = [v % Q for v in values]
    size = len(x)
    stages = size.bit_length() - 1
    for s in range(stages - 1, -1, -1):
        half = size >> (s + 1)
        for blk in range(1 << s):
            w = twi[(root << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half]
                x[i], x[i + half] = (u + v) % Q, (u - v) * w % Q
    return x


def point_positions(logn):
    """{evaluation point: position}: position P of the whole polynomial holds the value at psi^(2 bitrev(P) + 1)"""
    psi = twiddle_tables(logn)[0]
    return {pow(psi, 2 * bitrev(P, logn) + 1, Q): P for P in range(1 << logn)}


def parse_variant(line):
    """a line of fbs_debug_transform_list -> dict(cls, logn, lanes, dir, first | bounded[, np], parts, size, line)"""
    v = dict(f.split("=") for f in line.split())
    out = dict(cls=v["class"], logn=int(v["logn"]), lanes=int(v["lanes"]), dir=v["dir"], np=int(v.get("np", 1)), line=line)
    out["first" if out["dir"] == "forward" else "bounded"] = int(v["first" if out["dir"] == "forward" else "bounded"])
    out["parts"] = 4 if out["cls"].startswith("LaneNtt") else 1          # a lane transform: the four parts of a polynomial, one per wave
    out["size"] = (1 << out["logn"]) // out["parts"]
    return out


def sign_families(v):
    """(name, [sign per index]) over the N words of a polynomial -- natural index for forward, position for inverse: all equal, alternating
    with the stride of every stage, and per part the four 'extreme classes' of the first two stages (digit_cases, for this N and root):
    signs aligned with the centred twiddles so that every term of one output class of the opening adds up"""
    n, size, parts = 1 << v["logn"], v["size"], v["parts"]
    yield "all +", [1] * n
    yield "all -", [-1] * n
    for s in range(v["logn"]):
        yield "alternating, stride 2^%d" % s, [1 if (j >> s) & 1 == 0 else -1 for j in range(n)]
    tw = [centred(w) for w in twiddle_tables(v["logn"])[1 if v["dir"] == "forward" else 2]]
    for cls in range(4):
        signs = []
        for part in range(parts):
            root = part + parts if parts > 1 else 1
            w1, w2, w3 = tw[root], tw[2 * root], tw[2 * root + 1]
            w12, w13 = centred(w1 * w2), centred(w1 * w3)
            coef = ((1, w1, w2, w12), (1, w1, -w2, -w12), (1, -w1, w3, -w13), (1, -w1, -w3, w13))[cls]   # of (a, c, b, d)
            sg = [1 if c >= 0 else -1 for c in coef]
            signs += [sg[0]] * (size // 4) + [sg[2]] * (size // 4) + [sg[1]] * (size // 4) + [sg[3]] * (size // 4)
        yield "extreme class %d" % cls, signs


def variant_cases(v, entry):
    """(name, [N values]) for a variant with entry promise |x| <= entry: random within the promise, then every sign family at the promise itself and just inside
    it.  At the promise itself every value is +-entry, so sums of 2^k of them are exact in a double however far they run past 2^53 (few
    significant bits): only the magnitude shows a missing range fix-up.  'just inside' subtracts a random amount below 2^16 from each
    magnitude, so that every mantissa bit is in use and a sum past 2^53 is rounded -- then the residues show it."""
    rng = random.Random(v["line"])
    yield "random", [rng.randrange(-entry, entry + 1) for _ in range(1 << v["logn"])]
    jitter = min(1 << 16, entry // 2)
    for name, signs in sign_families(v):
        yield name, [s * entry for s in signs]
        yield name + ", just inside", [s * (entry - rng.randrange(jitter)) for s in signs]


def key_product_sums(name, x):
    """the ten lazy key products per evaluation of tests/test_fused_opening.py::test_transform_products_and_inverse (l = 5), summed"""
    rng = random.Random(len(name))
    own = [0.0] * N
    for _ in range(10):
        key = [rng.choice((HALF, -HALF, rng.randrange(-HALF, HALF + 1))) for _ in range(N)]
        own = [exact(int(o) + int(fp_mulmod(v, float(k)))) for o, v, k in zip(own, x, key)]
    return own
