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
        if nl == 1 and first == 0:                        # any beta > 9 reaches FIRST = 0: one level of 20 bits is a usable gadget,
            beta = 20                                     # one of 10 is not (tests/test_gpu_rotation_amounts.py decrypts its outputs)
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


# ==== the key switch on worst-case keys and digits (tests/test_keyswitch_reference.py, tests/test_gpu_keyswitch.py) =====================
# A key-switching-key row is (mask[0..n), body) with body = sum_i s_i mask_i + sk_glwe[j] h_v + e: the MASK can be anything, so a key
# whose mask columns hold the words that drive each kernel's accumulators to their stated bounds is a valid key for fbs_import_keys.
# Everything below is Python integers (numpy arrays of dtype object where an array is handy): no fixed-width word anywhere.
QBITS = 46
# name -> the parameter set: the smallest at which each bound of the key-switch kernels is tight (l, beta, p only make it a set a
# blind-rotation kernel is built for)
KS_SETS = {
    "g9": dict(n=20, log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, t_ksk=1, gamma_ksk=9),       # 9-bit digits: no int8 GEMM
    "g8_t1": dict(n=20, log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, t_ksk=1, gamma_ksk=8),    # digit -128 in the GEMM; FP64 folds every word
    "g8_t2": dict(n=20, log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, t_ksk=2, gamma_ksk=8),    # 63.0 bits; no room for FP64
    "n4096": dict(n=20, log_n_poly=12, k=1, l_bsk=2, beta_bsk=10, t_ksk=7, gamma_ksk=3),   # 63.8 of 63.9 bits; FP64 folds every 9 words
    "k3": dict(n=77, log_n_poly=9, k=3, l_bsk=2, beta_bsk=8, t_ksk=4, gamma_ksk=5),        # D = 1536, a second 64-column block
    "shipped": dict(n=130, log_n_poly=10, k=1, l_bsk=3, beta_bsk=7, t_ksk=8, gamma_ksk=2), # the everyday gadget, three 64-column blocks
}
KS_SIGMA = 1 << 8


def ks_set(name):
    """the full parameter dict of a KS_SETS entry (what Oracle and Params take)"""
    return dict(KS_SETS[name], p_msg=7, sigma_lwe=KS_SIGMA, sigma_glwe=4, bsk_group=1)


def ks_shape(prm):
    """-> (n, D, t, gamma) of a parameter dict"""
    return prm["n"], prm["k"] << prm["log_n_poly"], prm["t_ksk"], prm["gamma_ksk"]


def _limb_word(low_limb):
    """the word whose balanced base-256 limbs are `low_limb` in planes 0..4 and, in plane 5, the limb of the OTHER sign that is
    largest in magnitude while |x| < q/2 (so that the word is the centred value the limb kernel decomposes back to these limbs)"""
    low = sum(low_limb << (8 * b) for b in range(5))
    top = next(m for m in range(127, 0, -1) if abs(low + (-m if low_limb > 0 else m) * 256 ** 5) <= HALF)
    return (low + (-top if low_limb > 0 else top) * 256 ** 5) % Q


def balanced_limbs(word):
    """the six balanced base-256 limbs of the centred value of a canonical word (k_ks_limbs)"""
    x, out = centred(word), []
    for _ in range(6):
        limb = ((x + 128) & 255) - 128
        out.append(limb)
        x = (x - limb) >> 8
    assert x == 0
    return out


KS_WORDS = {"qm1": Q - 1, "half+": (Q - 1) // 2, "half-": (Q + 1) // 2, "limb-": _limb_word(-128), "limb+": _limb_word(127)}
KS_MIRROR = {"qm1": "qm1", "half+": "half-", "half-": "half+", "limb-": "limb+", "limb+": "limb-", "alt": "alt'", "rand": "rand'"}


def ks_column_plan(n, mirrored=False):
    """pattern name per mask column.  Every pattern within the first 8-column block; columns 8 and 16 (the second and third 8-column
    blocks: grid indices 8 and 1 of the XCD-paired column order of k_keyswitch_lanes / _fp) on the FP64 worst cases; column n - 1 and,
    where the key has them, columns 63 and 64 (the last of a 64-column block of the GEMM and the first of the next) on stress patterns
    too.  mirrored: the second key -- every pattern swapped for the one of the other sign."""
    cycle = ("qm1", "half+", "half-", "limb-", "limb+", "alt", "rand")
    plan = [cycle[i % 7] for i in range(n)]
    plan[n - 1] = "half+"
    if n > 64:
        plan[63], plan[64] = "limb-", "half-"
    assert plan[0] == "qm1" and plan[8] == "half+" and plan[16] == "half-"
    return [KS_MIRROR[p] for p in plan] if mirrored else plan


def ks_listed_columns(n):
    """the columns the issue names: 0, n - 1, one in each of the next two 8-column blocks, 63 and 64 where they exist"""
    return [0, n - 1, 8, 16] + ([63, 64] if n > 64 else [])


def ks_gadget(prm):
    """h_v = round(q / 2^(gamma (v + 1)))"""
    _, _, t, gamma = ks_shape(prm)
    return [(Q + (1 << (gamma * (v + 1) - 1))) >> (gamma * (v + 1)) for v in range(t)]


def ks_digits(word, t, gamma):
    """balanced digits (most significant first) in [-B/2, B/2), carries propagated, of abar = round(w 2^(t gamma) / 2^46) mod 2^(t gamma)"""
    tg, B = t * gamma, 1 << gamma
    abar = (((word << tg) + (1 << (QBITS - 1))) >> QBITS) % (1 << tg)
    digs = [0] * t
    for v in range(t - 1, -1, -1):
        d = abar % B
        abar //= B
        if d >= B // 2:
            d -= B
            abar += 1
        digs[v] = d
    return digs


def ks_word_for_digits(digs, gamma):
    """a canonical word that ks_digits maps to `digs` (most significant first): w = abar << (46 - t gamma).  Where that is not
    below q (only patterns whose top bits are all ones, from t gamma = 28 on) the nearest pattern below that has a preimage is taken;
    none of the rows below needs it, the assertion in planted_rows says so."""
    t = len(digs)
    tg = t * gamma
    abar = sum(d << (gamma * (t - 1 - v)) for v, d in enumerate(digs)) % (1 << tg)
    while (abar << (QBITS - tg)) >= Q:
        abar -= 1
    return abar << (QBITS - tg)


def ks_body(mask_row, j, v, r, sk_lwe, sk_glwe, h):
    """body of key row r = (j, v): sum_i s_i mask_i + sk_glwe[j] h_v + e, e deterministic with |e| <= sigma_lwe"""
    e = (r * 2654435761 + 12345) % (2 * KS_SIGMA + 1) - KS_SIGMA
    return (sum(int(m) for m, s in zip(mask_row, sk_lwe) if s) + (h[v] if sk_glwe[j] else 0) + e) % Q


def ks_switch(rows, ksk, prm):
    """THE DEFINITION on Python integers: rows [R][D + 1], ksk [D t][n + 1] (object) -> [R][n + 1] (object),
    out = (0, .., 0, body) - sum_(j, v) digit_v(a_j) K[(j, v)] mod q"""
    n, D, t, gamma = ks_shape(prm)
    digs = np.array([[d for w in row[:D] for d in ks_digits(int(w), t, gamma)] for row in rows], dtype=object)
    out = -digs.dot(ksk)
    out[:, n] += np.array([int(row[D]) for row in rows], dtype=object)
    return out % Q


def planted_keys(keys, prm, mirrored=False):
    """keys: dict(sk_lwe, sk_glwe, bsk, ksk) of a normally keyed context or oracle (export_keys / keys).  -> (the same dict with the
    key-switching key's masks planted by ks_column_plan and every body recomputed, tuned), tuned = [(row pattern 0 | 1, column, key
    row, target low bits)]: in each of eight-plus columns per stress row one key word is moved so that the switched word of that
    row in that column ends in 0x4000 (rounds up at 31 bits, one less rounds down) or 0x3FFF (rounds down, one more rounds up).
    Stress rows 0 and 1 both have uniform digits, so one column cannot be tuned for both (the two conditions on it are
    proportional): the listed columns are dealt to the two rows alternately, and the mirrored key deals them the other way round."""
    n, D, t, gamma = ks_shape(prm)
    rows = D * t
    sk_lwe, sk_glwe = [int(x) for x in keys["sk_lwe"]], [int(x) for x in keys["sk_glwe"]]
    h = ks_gadget(prm)
    rng = random.Random("planted key %d %d %d %d %d" % (n, D, t, gamma, mirrored))
    ksk = np.empty((rows, n + 1), dtype=object)
    for i, pat in enumerate(ks_column_plan(n, mirrored)):
        if pat in KS_WORDS:
            ksk[:, i] = KS_WORDS[pat]
        elif pat.startswith("alt"):                                   # the FP64 worst case with the sign alternating by row parity
            a, b = ("half+", "half-") if pat == "alt" else ("half-", "half+")
            ksk[0::2, i], ksk[1::2, i] = KS_WORDS[a], KS_WORDS[b]
        else:
            ksk[:, i] = [rng.randrange(Q) for _ in range(rows)]
    # the tuned words
    B = 1 << gamma
    listed = ks_listed_columns(n)
    others = [i for i in range(n) if i not in listed]
    cols = listed + others[:max(0, 16 - len(listed))]                 # sixteen columns (all of the listed ones), eight per stress row
    if mirrored:
        cols = cols[1:] + cols[:1]
    tuned = []
    for idx, col in enumerate(cols):
        which = idx & 1                                               # stress row 0: every digit -B/2; 1: every digit B/2 - 1
        d0 = -(B // 2) if which == 0 else B // 2 - 1
        r = (-d0 * sum(int(x) for x in ksk[:, col])) % Q              # the switched word of that row in a mask column
        low = 0x4000 if (idx >> 1) & 1 == 0 else 0x3FFF
        target = (r & ~0x7FFF) | low
        kr = ((idx % 8) * (D // 8) + 5 * idx + 1) % D * t + idx % t   # one key row in every eighth of the mask words, every level
        ksk[kr, col] = (int(ksk[kr, col]) + (r - target) * pow(d0, Q - 2, Q)) % Q
        tuned.append((which, col, kr, low))
    for r in range(rows):
        ksk[r, n] = ks_body(ksk[r, :n], r // t, r % t, r, sk_lwe, sk_glwe, h)
    out = dict(keys)
    out["ksk"] = np.array(ksk.reshape(-1), dtype=np.uint64)           # (the transport format of import_keys / set_keys)
    return out, tuned


def planted_rows(prm, count, honest, seed=1):
    """[count][D + 1] canonical words, the six row patterns in turn (row i has pattern i % 6) with bodies 0, q - 1 and random in turn
    ((i + i // 6) % 3: every pattern meets every body within eighteen rows): 0 every balanced digit -B/2; 1 every digit B/2 - 1; 2 those two alternating by word; 3 words 0 and q - 1
    alternating (q - 1 rounds up past the top digit: the carry is dropped); 4 uniform random; 5 the next row of `honest` (encryptions
    under the context's key, body and all)"""
    n, D, t, gamma = ks_shape(prm)
    B = 1 << gamma
    lo, hi = ks_word_for_digits([-(B // 2)] * t, gamma), ks_word_for_digits([B // 2 - 1] * t, gamma)
    assert ks_digits(lo, t, gamma) == [-(B // 2)] * t and ks_digits(hi, t, gamma) == [B // 2 - 1] * t   # both have a preimage
    assert ks_digits(Q - 1, t, gamma) == [0] * t and ((Q - 1) >> (QBITS - 1 - t * gamma)) + 1 == 2 << (t * gamma)   # the carry
    rng = random.Random("planted rows %d %d" % (D, seed))
    out = np.zeros((count, D + 1), dtype=np.uint64)
    for i in range(count):
        pat = i % 6
        if pat == 5:
            out[i] = honest[(i // 6) % len(honest)]
            continue
        mask = {0: [lo] * D, 1: [hi] * D, 2: [lo, hi] * (D // 2), 3: [0, Q - 1] * (D // 2)}.get(pat) or [rng.randrange(Q) for _ in range(D)]
        out[i, :D] = mask
        out[i, D] = (0, Q - 1, rng.randrange(Q))[(i + i // 6) % 3]
    return out


# ---- what the planted inputs make each kernel family hold, against the bound its code states ----------------------------------
def ks_fp_words_per_fold(prm):
    """launch_keyswitch's formula; 0: the FP64 kernel is refused (select_keyswitch)"""
    _, _, t, gamma = ks_shape(prm)
    return min(1024, ((1 << 53) - (1 << 45)) // (t << (44 + gamma)))


def ks_gemm_admitted(prm):
    """ks_gemm_exact: int8 digits and int32 sums"""
    _, D, t, gamma = ks_shape(prm)
    return gamma <= 8 and (D * t) << (gamma + 6) < 1 << 31


def ks_stated_bounds(prm):
    """family -> the bound its code states, evaluated at the set (None: the family never runs there)"""
    _, D, t, gamma = ks_shape(prm)
    wpf = ks_fp_words_per_fold(prm)
    return {"gemm_int32": (D * t) << (gamma - 1 + 7) if ks_gemm_admitted(prm) else None,      # 2^(gamma-1) 2^7 kN t  (< 2^31)
            "fp64": (1 << 45) + wpf * (t << (44 + gamma)) if wpf else None,                    # 2^45 + words t 2^(44+gamma)  (<= 2^53)
            "u64_sum": (D * t) << (46 + gamma),                                                # 2^(46+gamma) t D  (<= 2^63.9)
            "lanes_hi": (D * t) << (14 + gamma)}                                               # its high part  (<= 2^31.9)


def ks_reached(prm, ksk, rows):
    """family -> the largest magnitude that family's accumulators hold on these inputs.  ksk [D t][n + 1], rows [R][D + 1].
    gemm_int32: running sums over kappa = v D + j of digit x limb per plane; fp64: per wave of k_keyswitch_fp<8,2,8> (an eighth of the
    mask words each), the running sum of digit x centred word from a centred start, folded every words_per_fold words; u64_sum: the whole
    sum of field x word (k_keyswitch; the lanes kernels after their waves met); lanes_hi: the whole sum of field x (word >> 32), and
    lanes_hi_wave: the fullest 32-bit register of one wave, which sums 1 / WAVES of the mask words (an eighth in <8,2,8>, a quarter in
    <8,1,4>), times WAVES -- its fill against its equal share of the stated bound."""
    n, D, t, gamma = ks_shape(prm)
    B = 1 << gamma
    K = np.array(ksk, dtype=object).reshape(D, t, n + 1)
    Kc = np.vectorize(centred, otypes=[object])(K)
    digs = [np.array([ks_digits(int(w), t, gamma) for w in row[:D]], dtype=object) for row in rows]      # [D][t] each
    reached = dict.fromkeys(("gemm_int32", "fp64", "u64_sum", "lanes_hi", "lanes_hi_wave"), 0)
    x, planes = Kc.astype(np.int64), []                               # (what k_ks_limbs does, on machine words as it does)
    for _ in range(6):
        planes.append(((x + 128) & 255) - 128)
        x = (x - planes[-1]) >> 8
    limbs = np.stack(planes, axis=-1)                                                                      # [D][t][n + 1][6]
    wpf = ks_fp_words_per_fold(prm)
    for d in digs:
        if ks_gemm_admitted(prm):
            terms = d.astype(np.int64).T[:, :, None, None] * limbs.transpose(1, 0, 2, 3)                  # [t][D][n + 1][6], kappa order
            run = np.cumsum(terms.reshape(D * t, n + 1, 6), axis=0)
            reached["gemm_int32"] = max(reached["gemm_int32"], int(np.abs(run).max()))
        if wpf:
            slice_len = -(-D // 8)
            for wave in range(8):
                acc = np.zeros(n + 1, dtype=object)
                for at, j in enumerate(range(wave * slice_len, min(D, (wave + 1) * slice_len))):
                    for v in range(t):
                        acc = acc + d[j, v] * Kc[j, v]
                        reached["fp64"] = max(reached["fp64"], max(abs(x) for x in acc))
                    if (at + 1) % wpf == 0:
                        acc = np.array([centred(x) for x in acc], dtype=object)
        u = d + B // 2                                                                                     # the fields the integer kernels see
        reached["u64_sum"] = max(reached["u64_sum"], max((u[:, :, None] * K).sum(axis=(0, 1))))
        hi = u[:, :, None] * (K >> 32)
        reached["lanes_hi"] = max(reached["lanes_hi"], max(hi.sum(axis=(0, 1))))
        for waves in (4, 8):
            slice_len = -(-D // waves)
            share = max(max(hi[w * slice_len:(w + 1) * slice_len].sum(axis=(0, 1))) for w in range(waves))
            reached["lanes_hi_wave"] = max(reached["lanes_hi_wave"], share * waves)                        # as a fraction of the whole bound
    return reached


# ==== linear combinations and shared-rotation extraction at their bounds (tests/test_level_arithmetic_reference.py, ===============
# ==== tests/test_gpu_level_arithmetic.py) ==========================================================================================
# k_lincomb keeps a lazy FP64 sum of products below 0.75 q each, centred after every 16th term; k_multi_extract sums value x word in
# an int64 on the loader's promise sum |d| < 2^16.  The inputs below drive both to those bounds; everything is Python integers.
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
LC_SHAPES = [(1, 8), (2, 8), (4, 8), (3, 9), (2, 10), (1, 12)]          # (k, log N): ct_words 257, 513, 1025, 1537, 2049, 4097
LC_TARGET = 49 * Q // 100                                               # |product| of a planted term: floor(0.49 q) - term index
LC_NONZERO = [1, -1, 3, -3, HALF, -HALF, (Q + 1) // 2, Q - 1, 1 << 40, -(1 << 45), INT64_MAX, INT64_MIN]   # (none is 0 mod q)
LC_ZERO = [Q, -Q, -2 * Q]                                               # 0 mod q: the product is 0 whatever the word
LC_CONSTS = [0, 1, -1, 2 * 7 - 1, Q, -Q, INT64_MAX, INT64_MIN]          # (2p - 1 at p = 7)
LC_SLOTS = 48                                                           # source slots of a launch; an output of more terms repeats them
# (first slot, terms, constant) per output of a launch: term t reads slot (first + t) % LC_SLOTS.  Slots 0 .. 31 have coefficients
# that are not 0 mod q, so every output of 16 terms or more opens with 16 planted products of one sign; the outputs of 15 terms and
# of 48 and 100 run over slots 32 .. 47, where q, -q and -2q sit.  The constants of the outputs of 16 terms or more leave the body
# column its peak (see lc_replay) at either sign.
LC_OUTPUTS = [(0, 0, 2 * 7 - 1), (11, 1, -1), (33, 15, INT64_MAX), (0, 16, 1), (0, 17, Q), (0, 31, -Q), (0, 32, 0), (0, 33, -1),
              (0, 48, INT64_MAX), (0, 100, INT64_MIN), (0, 400, 1)]
# (400 terms: what shows a centring that is never done -- 196 q of one sign, past the 2^53 = 128 q to which a double holds every
# integer.  Between 16 and 100 terms the sum stays exact with or without centring, and so does a cadence of 32.)


def lc_delta(p=7):
    """Delta = 2 round(q / 4p): what one unit of a LinearProd's constant adds to the body"""
    return 2 * ((Q + 2 * p) // (4 * p))


def lc_columns(ct_words):
    """the planted columns: first word, either side of the 256-thread pass, the last mask word, the body"""
    return [0, 255, 256, ct_words - 2, ct_words - 1]


def lc_coefs(n_terms):
    """coefficient of term (slot) i: twelve fixed ones that are not 0 mod q and four random int64 in every sixteen, the order turned
    by five from one sixteen to the next; from term 32 on every fifth is q, -q or -2q in turn"""
    rng = random.Random("lincomb coefficients")
    out = []
    for i in range(n_terms):
        r = rng.randrange(INT64_MIN, INT64_MAX + 1)
        while r % Q == 0:
            r = rng.randrange(INT64_MIN, INT64_MAX + 1)
        pool = LC_NONZERO + [r] * 4
        c = pool[(i + 5 * (i // 16)) % 16]
        if i >= 32 and i % 5 == 3:
            c = LC_ZERO[(i // 5) % 3]
        out.append(c)
    return out


def planted_lincomb(ct_words, n_terms, sign, seed):
    """-> (words uint64 [n_terms][ct_words], coefs [n_terms] Python integers).  In the planted columns word j of term i is such that
    coef_i * word = sign * (LC_TARGET - i) mod q (a coefficient that is 0 mod q keeps its random word); every other word is random
    canonical, one in eight of them 0, q - 1, (q - 1) / 2 or (q + 1) / 2."""
    coefs = lc_coefs(n_terms)
    rng = np.random.default_rng([ct_words, n_terms, sign + 1, seed])
    words = rng.integers(0, Q, (n_terms, ct_words), dtype=np.uint64)
    edge = np.array([0, Q - 1, HALF, HALF + 1], np.uint64)[rng.integers(0, 4, words.shape)]
    words = np.where(rng.integers(0, 8, words.shape) == 0, edge, words)
    for i, c in enumerate(coefs):
        if c % Q:
            words[i, lc_columns(ct_words)] = sign * (LC_TARGET - i) * pow(c % Q, Q - 2, Q) % Q
    return words, coefs


def lc_terms(first, n_terms):
    """the source slots of an output of LC_OUTPUTS, term by term"""
    return [(first + t) % LC_SLOTS for t in range(n_terms)]


def lc_definition(words, coefs, terms, const, p=7):
    """THE DEFINITION on Python integers: sum of coef x word over the terms, const x Delta more on the body -> [ct_words] (object)"""
    w = np.array(words, dtype=object)
    out = np.zeros(w.shape[1], dtype=object)
    if terms:
        out = np.array([coefs[t] for t in terms], dtype=object).dot(w[terms])
    out[-1] += const * lc_delta(p)
    return out % Q


def lc_replay(words, coefs, terms, const, column, p=7, every=16):
    """k_lincomb's accumulation of one output word on the exact-integer model of the FP64 unit (fp_mulmod, fp_center above) ->
    (canonical result, peak |accumulator|).  Asserts what the kernel relies on: every product below 0.75 q, every intermediate an
    integer below 2^52 (exactly representable, and what fp_to_u64 takes).  every: the centring cadence (the kernel's 16; 0: never)."""
    acc = exact(const % Q * lc_delta(p) % Q) if column == len(words[0]) - 1 else 0.0      # (the last column is the body)
    peak = abs(acc)
    for n, t in enumerate(terms):
        c = centred(coefs[t])
        assert abs(c) <= HALF
        prod = fp_mulmod(exact(int(words[t][column])), exact(c))
        assert abs(prod) < 0.75 * Q
        acc = exact(int(acc) + int(prod))
        peak = max(peak, abs(acc))
        assert peak < 1 << 52
        if every and n % every == every - 1:
            acc = fp_center(acc)
    return int(fp_canon(acc)), peak


# ---- tables cut out of a shared rotation ------------------------------------------------------------------------------------------
EX_P = 7
# sum |d| of the difference polynomial: 65534 is the most an evaluable table can have below the loader's limit of 2^16 (the total
# variation from f(0) round to -f(0) is even), 65536 the least above it
EX_TABLES = {
    "at_limit_a": [0, 32767, 0],
    "at_limit_b": [1, 32767, 1, 1, 1, 1, 1],
    "over_limit_a": [0, 32767, 0, 1, 0],
    "over_limit_b": [0, 32768, 0],
    "negative": [-3, -20000, 5, -1, 0, -7, 2],
    "c1_long": [0, 9000, -7000, 3, 0, 1, 0, 1, -8999, 7001, -2, 1, 0, 1],       # f(x + p) = 1 - f(x)
    "small": [0, 1, 2, 3, 2, 1, 0],
}
EX_ABS_SUM = {"at_limit_a": 65534, "at_limit_b": 65534, "over_limit_a": 65536, "over_limit_b": 65536, "negative": 40026,
              "c1_long": 32009, "small": 6}


def table_diff(table, N, p=EX_P):
    """-> (D_F as N Python integers, c): G_j = +-(2 f(round(j p / N)) - c), the sign turning where the index reaches p, and
    D_F = G (1 - X) / 2 mod X^N + 1"""
    c = table[0] + table[p] if len(table) > p else 0
    assert 0 < len(table) <= 2 * p and all(table[i] + table[i + p] == c for i in range(len(table) - p))
    G = []
    for j in range(N):
        x = (2 * j * p + N) // (2 * N)
        f = (table[x] if x < len(table) else 0) if x < p else table[0]
        G.append(2 * f - c if x < p else -(2 * f - c))
    d = [G[j] - G[j - 1] if j else G[0] + G[N - 1] for j in range(N)]
    assert all(v % 2 == 0 for v in d)
    return [v // 2 for v in d], c


def planted_accumulators(k, N, seed=1):
    """{name: (k + 1) N canonical words}: all q - 1, all 0, 0 and q - 1 in turn, q - 1 on one polynomial only (the body's when
    seed is even, the first mask polynomial's when odd), random"""
    rng = np.random.default_rng([k, N, seed])
    one = np.zeros((k + 1, N), np.uint64)
    one[k if seed % 2 == 0 else 0] = Q - 1
    return {"all q-1": np.full((k + 1) * N, Q - 1, np.uint64), "all 0": np.zeros((k + 1) * N, np.uint64),
            "alternating": np.array([0, Q - 1] * ((k + 1) * N // 2), np.uint64), "one polynomial": one.reshape(-1),
            "random": rng.integers(0, Q, (k + 1) * N, dtype=np.uint64)}


def extract_definition(acc, diff, post, k, N):
    """THE DEFINITION on Python integers: every polynomial of the accumulator times D_F mod X^N + 1, then the sample extraction
    (mask polynomial c gives words P_0, -P_(N-1), .., -P_1; the body is B_0 + post) -> [k N + 1]"""
    out = []
    for c in range(k + 1):
        a = [int(x) for x in acc[c * N:(c + 1) * N]]
        prod = [0] * N
        for i, d in enumerate(diff):
            if d:
                for m in range(N):
                    prod[m] += d * a[m - i] if m >= i else -d * a[m + N - i]
        out += [prod[0]] + [-prod[N - j] for j in range(1, N)] if c < k else [prod[0] + post]
    return [v % Q for v in out]


def extract_kernel_sums(acc, pos, val, k, N):
    """k_multi_extract's signed 64-bit sum of every output word before its one reduction, statement by statement, from the
    (position, value) pairs the loader uploads -> [k N + 1] Python integers; asserts that each running sum fits an int64"""
    D, out = k * N, []
    for j in range(D + 1):
        c = j // N
        jj = j - c * N
        m = 0 if jj == 0 else N - jj
        total = 0
        for at, v in zip(pos, val):
            term = v * int(acc[c * N + m - at] if m >= at else acc[c * N + m + N - at])
            total += term if m >= at else -term
            assert -(1 << 63) <= total < 1 << 63
        out.append(-total if jj else total)
    return out


# ==== compact ciphertexts at real key sizes, on planted rounding boundaries (tests/test_compact_reference.py, =======================
# ==== tests/test_gpu_compact_wide.py) ==============================================================================================
# The format kernels (k_compact_pack, k_compact_unpack, k_decrypt_compact) loop over rounds of 256 words and over passes of 64 lanes,
# and their sums are exact through wrap-around and flooring shifts: none of it shows at n = 12 on random words.  The sets below reach
# n = 4096 on the cheapest polynomial size; the key-switching key is planted so that the switched ciphertexts are CHOSEN words.
# t = 1, so one digit is one key row; b = log2(2N) = 9 is the narrowest width the format has.
COMPACT_WIDE_SETS = {"n%d" % n: dict(n=n, log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, t_ksk=1, gamma_ksk=8, p_msg=7, sigma_lwe=1 << 8,
                                     sigma_glwe=4, bsk_group=1) for n in (64, 65, 734, 4096)}
COMPACT_PACK_WIDTHS = (9, 12, 23, 31)
PLANT_WORD = 1 << 38                                          # the word whose only digit (t = 1, gamma = 8) is 1


def planted_switch(keys, prm, targets, bodies=None, oracle=None):
    """keys: dict(sk_lwe, sk_glwe, bsk, ksk) (export_keys / Oracle.keys); targets: at most N rows of n canonical words;
    bodies[j]: the switched bodies wanted with row j (default: [0]).  -> (the same dict with key row (j, 0) planted, input ciphertexts
    [sum of len(bodies[j])][D + 1], row after row).  Key row (j, 0) gets the mask -targets[j] mod q and the body
    <mask, sk_lwe> + sk_glwe[j] h_0 without noise (a valid row for import_keys); a ciphertext of row j is zero but for mask word j,
    whose one digit is 1, and its body, so that its key switch is 0 - 1 x (key row j) + (0, .., 0, body): exactly (targets[j], the body
    wanted).  Asserted here through the oracle's key switch (`oracle`: one of this parameter set to use, its keys are replaced)."""
    from oracle import tfhe_oracle as orc
    n, D, t, gamma = ks_shape(prm)
    assert t == 1 and len(targets) <= D and ks_digits(PLANT_WORD, t, gamma) == [1]
    bodies = [[0]] * len(targets) if bodies is None else bodies
    sk_lwe, sk_glwe = [int(x) for x in keys["sk_lwe"]], [int(x) for x in keys["sk_glwe"]]
    h0 = ks_gadget(prm)[0]
    ksk = np.array(keys["ksk"], dtype=np.uint64).reshape(D, n + 1)
    cts, want = [], []
    for j, (row, wanted) in enumerate(zip(targets, bodies)):
        assert len(row) == n and all(0 <= int(x) < Q for x in row)
        mask = [(Q - int(x)) % Q for x in row]
        key_body = (sum(m for m, s in zip(mask, sk_lwe) if s) + (h0 if sk_glwe[j] else 0)) % Q
        ksk[j, :n], ksk[j, n] = mask, key_body
        for body in wanted:
            ct = np.zeros(D + 1, np.uint64)
            ct[j], ct[D] = PLANT_WORD, (int(body) + key_body) % Q
            cts.append(ct)
            want.append([int(x) for x in row] + [int(body)])
    out = dict(keys)
    out["ksk"] = ksk.reshape(-1)
    o = oracle if oracle is not None else orc.Oracle(prm, seed=1, keygen=False)
    o.set_keys(**out)
    for ct, w in zip(cts, want):
        assert [int(x) for x in o.keyswitch(ct)] == w
    return out, np.stack(cts) if cts else np.zeros((0, D + 1), np.uint64)


# ---- THE DEFINITIONS on Python integers (include/fbs_exec.h, "compact outputs" and "chained evaluation") ---------------------------
def _half_up(x, sh):
    """round-half-up(x / 2^sh), x >= 0"""
    return (x + (1 << sh >> 1)) >> sh


def _rounded_down(x, top, bits, modulus):
    """n mask words and a body below `modulus` (2^top or the q just below it) -> n + 1 fields below 2^bits: every mask word
    rounded half-up to a multiple of 2^(top - bits), the body taken down by floor(eps / 2) mod `modulus` first, eps the sum of the
    mask words' signed rounding errors"""
    sh = top - bits
    x = [int(v) for v in x]
    m = [_half_up(v, sh) for v in x[:-1]]
    eps = sum(v - (r << sh) for v, r in zip(x, m))
    body = (x[-1] - eps // 2) % modulus                                 # (// floors)
    return [r % (1 << bits) for r in m + [_half_up(body, sh)]]


def compact_definition(x, bits):
    """a small-key ciphertext (n mask words, body; canonical mod q) -> its n + 1 fields at width `bits`"""
    return _rounded_down(x, QBITS, bits, Q)


def reround_definition(fields, bits, b):
    """n + 1 fields at width `bits` -> the fields at width b <= bits the blind rotation reads"""
    return [int(f) for f in fields] if bits == b else _rounded_down(fields, bits, b, 1 << bits)


def decode_phase(body, mask_sum, bits, two_p):
    """round-half-up(phase 2p / 2^bits) mod 2p, phase = (body - mask_sum) mod 2^bits"""
    return _half_up((body - mask_sum) % (1 << bits) * two_p, bits) % two_p


def decode_definition(fields, sk, bits, two_p):
    """n + 1 fields and the small key's n bits -> the message"""
    return decode_phase(int(fields[-1]), sum(int(f) for f, s in zip(fields, sk) if s), bits, two_p)


def pack_definition(fields, bits):
    """fields of `bits` bits -> the words of the bit stream they make, field j at stream bits [j bits, j bits + bits): the stream
    written out as a string of binary digits, last field first, and cut into words of 64 from its low end"""
    digits = "".join(format(int(f), "0%db" % bits) for f in reversed(fields))
    W = -(-len(digits) // 64)
    digits = digits.zfill(64 * W)
    return [int(digits[64 * (W - 1 - w):64 * (W - w)], 2) for w in range(W)]


def unpack_definition(words, n1, bits):
    """the way back: n1 fields"""
    digits = "".join(format(int(w), "064b") for w in reversed(words))
    return [int(digits[len(digits) - (j + 1) * bits:len(digits) - j * bits], 2) for j in range(n1)]


# ---- planted rows: every mask word on a chosen side of its rounding boundary -------------------------------------------------------
def rounding_eps(x, top, bits):
    """eps of a row of mask words: the sum of their signed rounding errors from 2^top down to 2^bits"""
    sh = top - bits
    return sum(int(v) - (_half_up(int(v), sh) << sh) for v in x)


def boundary_rows(n, top, bits, modulus, seed):
    """{name: n mask words below `modulus`} for the rounding from 2^top down to 2^bits (sh = top - bits; m_i random below 2^bits,
    lowered where the word would reach `modulus`):
    half   (m_i << sh) + 2^(sh-1): every word rounds up, eps = -n 2^(sh-1), the negative extreme
    below  one less: every word rounds down, eps = +n (2^(sh-1) - 1), the positive extreme
    top    every word modulus - 1: rounds up to 2^bits (the field wraps to 0) where modulus - 1 is in the upper half of its step
    odd    every word one below a multiple of 2^sh, but the first on a multiple when n is even: eps is negative and odd
    alt    half and below in turn
    rand   uniform random words
    With sh = 0 nothing is rounded: top, rand and zero rows only."""
    rng = random.Random("boundary rows %d %d %d %d" % (n, top, bits, seed))
    sh = top - bits
    rand = [rng.randrange(modulus) for _ in range(n)]
    if sh == 0:
        return {"top": [modulus - 1] * n, "rand": rand, "zero": [0] * n}
    hb = 1 << (sh - 1)
    m = [min(rng.randrange(1 << bits), (modulus - 1 - hb) >> sh) for _ in range(n)]
    half = [(v << sh) + hb for v in m]
    below = [v - 1 for v in half]
    odd = [(max(v, 1) << sh) - 1 for v in m]
    if n % 2 == 0:
        odd[0] += 1
    alt = [h if i % 2 == 0 else b for i, (h, b) in enumerate(zip(half, below))]
    return {"half": half, "below": below, "top": [modulus - 1] * n, "odd": odd, "alt": alt, "rand": rand}


def boundary_bodies(row, top, bits, modulus, seed=0):
    """the bodies x_n paired with a row of mask words: those for which y = (x_n - floor(eps / 2)) mod `modulus` is the last value that
    rounds down, the first that rounds up and the one after it -- at a random step and at the highest step below `modulus` --, y = 0
    and y = modulus - 1, then x_n = 0 and x_n = modulus - 1 themselves.  Whatever eps is, the subtraction wraps through `modulus` in
    some of them: y = 0 and y = modulus - 1 lie either side of the wrap.  Computed from the definition of eps alone."""
    sh = top - bits
    rng = random.Random("boundary bodies %d %d %d %d" % (len(row), top, bits, seed))
    if sh == 0:
        return [0, modulus - 1, rng.randrange(modulus), rng.randrange(modulus)]
    half_eps = rounding_eps(row, top, bits) // 2
    hb = 1 << (sh - 1)
    ys = []
    for step in (rng.randrange(1 << bits), (modulus - 2 - hb) >> sh):
        ys += [(step << sh) + hb - 1, (step << sh) + hb, (step << sh) + hb + 1]
    ys += [0, modulus - 1]
    assert all(0 <= y < modulus for y in ys)
    return [(y + half_eps) % modulus for y in ys] + [0, modulus - 1]


def compact_target_rows(n, bits, seed=0):
    """{name: (n canonical words, [switched bodies])} for the pack at width `bits` (the row of q - 1 is called qm1 here)"""
    rows = boundary_rows(n, QBITS, bits, Q, seed)
    return {{"top": "qm1"}.get(name, name): (row, boundary_bodies(row, QBITS, bits, Q, seed)) for name, row in rows.items()}


def reround_field_rows(n, bits, b, seed=0):
    """{name: [rows of n + 1 fields below 2^bits]} for the unpack from width `bits` down to b"""
    rows = boundary_rows(n, bits, b, 1 << bits, seed)
    return {name: [row + [body] for body in boundary_bodies(row, bits, b, 1 << bits, seed)] for name, row in rows.items()}


# ---- decode cases: phases on every boundary between two messages --------------------------------------------------------------------
def decode_boundary_phases(bits, two_p):
    """the phases either side of every decode boundary (2j + 1) 2^bits / (2 two_p), j < two_p, and the boundary itself where it is an
    integer; in order, without repeats"""
    out = []
    for j in range(two_p):
        num, den = (2 * j + 1) << bits, 2 * two_p
        cands = (num // den - 1, num // den, num // den + 1) if num % den == 0 else (num // den, num // den + 1)
        out += [c % (1 << bits) for c in cands]
    return list(dict.fromkeys(out))


def decode_cases(n, sk, bits, two_p, seed=0, random_count=64):
    """-> {"ones": (mask fields [n], [body fields]), "zeros": (mask, bodies), "random": [rows of n + 1 fields]}: (a) every mask
    field 2^bits - 1, so that the sum over the key's set bits wraps 2^32 as often as it can, (b) zero masks -- both with the bodies
    that put the phase on every decode boundary and one either side -- and (c) `random_count` rows of random fields"""
    top = (1 << bits) - 1
    phases = decode_boundary_phases(bits, two_p)
    ones = sum(int(s) for s in sk) * top
    rng = random.Random("decode cases %d %d %d %d" % (n, bits, two_p, seed))
    return {"ones": ([top] * n, [(ph + ones) % (1 << bits) for ph in phases]), "zeros": ([0] * n, phases),
            "random": [[rng.randrange(1 << bits) for _ in range(n + 1)] for _ in range(random_count)]}


def decode_case_batches(cases, sk, bits, two_p, pack, chunk=8192):
    """the cases of decode_cases -> (name, packed words uint64 [<= chunk][W], the messages by the definition) per batch.  The mask
    fields that a set shares are packed once with `pack` (the restatement of tests/test_gpu_compact.py) and summed under the key
    once; the body field, the last of the stream, is set per row."""
    n = len(sk)
    at, o = n * bits // 64, n * bits % 64
    for name in ("ones", "zeros"):
        mask, bodies = cases[name]
        template = pack(np.array([mask + [0]], dtype=np.uint64), bits)
        mask_sum = sum(f for f, s in zip(mask, sk) if s)
        assert decode_phase(bodies[0], mask_sum, bits, two_p) == decode_definition(mask + bodies[:1], sk, bits, two_p)
        for c0 in range(0, len(bodies), chunk):
            part = bodies[c0:c0 + chunk]
            body = np.array(part, dtype=np.uint64)
            words = np.repeat(template, len(part), axis=0)
            words[:, at] |= body << np.uint64(o)
            if o + bits > 64:
                words[:, at + 1] |= body >> np.uint64(64 - o)
            assert unpack_definition(words[-1], n + 1, bits) == mask + part[-1:]
            yield name, words, [decode_phase(b, mask_sum, bits, two_p) for b in part]
    rows = cases["random"]
    yield "random", pack(np.array(rows, dtype=np.uint64), bits), [decode_definition(r, sk, bits, two_p) for r in rows]


# ==== planted rotation amounts for every blind-rotation kernel (tests/test_rotation_amounts_reference.py, ==========================
# ==== tests/test_gpu_rotation_amounts.py) ==========================================================================================
# At bits = log2(2N) fbs_refresh_compact_dev unpacks its fields, unrounded, into the rows the blind rotation reads: the n + 1 fields of
# a row ARE the rotation amounts of its n steps and of the accumulator's start.  The rows below choose them: every step-skipping
# pattern (a step whose amounts are all zero is skipped) against every edge amount, on honest keys.
PLANTED_STEPS = 16
PLANTED_P = 7
PLANTED_ROWS = 60                                                       # 5 mask lists x 12 bodies: row j = (list j % 5, body j // 5)
PLANTED_DEFAULT_KNOBS = dict(br_cu_kernel=1, br_cu_lean=1, br_k2_shape=0, br_glwe_fpw=0)   # (Tune, csrc/fbs_internal.hpp)
# the families of the CPU test: name -> parameter set (the gadgets of the toy sets above and of `recipe`)
PLANTED_FAMILIES = {
    "k1_n1024_g1": dict(log_n_poly=10, k=1, l_bsk=3, beta_bsk=7, bsk_group=1),
    "k1_n2048_g2": dict(log_n_poly=11, k=1, l_bsk=1, beta_bsk=20, bsk_group=2),
    "k2_n1024_g2": dict(log_n_poly=10, k=2, l_bsk=1, beta_bsk=20, bsk_group=2),
    "k3_n512_g2": dict(log_n_poly=9, k=3, l_bsk=1, beta_bsk=18, bsk_group=2),
    "k4_n256_g2": dict(log_n_poly=8, k=4, l_bsk=2, beta_bsk=8, bsk_group=2),
}


def planted_set(log_n_poly, k, l_bsk, beta_bsk, bsk_group, n=PLANTED_STEPS):
    """the full parameter dict (what Oracle and Params take) of a planted-amounts case: the set tests/test_gpu_dispatch.py makes
    of a recipe, at n steps"""
    return dict(n=n, log_n_poly=log_n_poly, k=k, l_bsk=l_bsk, beta_bsk=beta_bsk, t_ksk=4, gamma_ksk=4 if log_n_poly < 12 else 3,
                p_msg=PLANTED_P, sigma_lwe=1 << 6, sigma_glwe=1 << 4, bsk_group=bsk_group)


def planted_edges(N, group):
    """the edge set: amounts E of a step of one key bit; pairs P (e0, e1) of a step of two, x = 5 and y = N + 7"""
    if group == 1:
        return [1, 2, 63, 64, 65, N // 2, N - 1, N, N + 1, 3 * N // 2, 2 * N - 2, 2 * N - 1]
    x, y, M = 5, N + 7, 2 * N
    return [(0, x), (x, 0), (x, M - x), (N, N), (N, 0), (0, N), (1, M - 1), (M - 1, M - 1), (N - 1, 1), (N, 1), (1, 1), (M - 2, 3),
            (y, M - y), (63, 65), (64, N - 64)]


def step_properties(amounts, N):
    """what the amounts of ONE step hit, as a set of names.  One key bit: 'odd', 'even', 'e == N'.  Two: the same of each of e0, e1
    and e2 = (e0 + e1) mod 2N that is not zero, and 'e2 == 0, parts non-zero', 'e2 == N', 'wrapped sum' (e0 + e1 > 2N),
    'one part zero'"""
    es = [int(a) for a in amounts]
    hits = set()
    if len(es) == 2:
        e0, e1 = es
        es = [e0, e1, (e0 + e1) % (2 * N)]
        if e0 and e1 and es[2] == 0:
            hits.add("e2 == 0, parts non-zero")
        if es[2] == N:
            hits.add("e2 == N")
        if e0 + e1 > 2 * N:
            hits.add("wrapped sum")
        if (e0 == 0) != (e1 == 0):
            hits.add("one part zero")
    for e in es:
        if e:
            hits.add("odd" if e & 1 else "even")
            if e == N:
                hits.add("e == N")
    return hits


def planted_mask_lists(N, n, group):
    """the five lists of n amounts: L0 skips its even steps (the first among them), L1 its odd steps (the last among them), L2 all but
    the middle one, L3 and L4 none.  A step is `group` amounts; the steps that run walk the edge set, each list from where the one
    before stopped (L3, L4, L0, L1, L2 in that order), so that n / group >= 6 steps cover it."""
    edges = planted_edges(N, group)
    steps = n // group
    assert n % group == 0 and steps % 2 == 0
    zero = 0 if group == 1 else (0, 0)
    at = [0]

    def walk():
        at[0] += 1
        return edges[(at[0] - 1) % len(edges)]
    L3 = [walk() for _ in range(steps)]
    L4 = [walk() for _ in range(steps)]
    L0 = [walk() if i % 2 else zero for i in range(steps)]
    L1 = [zero if i % 2 else walk() for i in range(steps)]
    L2 = [walk() if i == steps // 2 else zero for i in range(steps)]
    lists = [L0, L1, L2, L3, L4]
    return lists if group == 1 else [[e for pair in lst for e in pair] for lst in lists]


def planted_amount_rows(N, n, group, sk_lwe, p, turn=0):
    """-> (fields uint32 [60][n + 1], meta).  Row j: mask list j % 5 (planted_mask_lists), body j // 5.  Bodies 0 .. 6 are SEMANTIC:
    m_n = (<mask, sk_lwe> + round(msg N / p) + off) mod 2N for msg = body, so that the rotation through the identity table decrypts
    to msg; off is 0, +(N / 2p - 2), -(N / 2p - 2) in turn by row, from row `turn` on (either edge of the message's slot, two short of it:
    turn = 0, 1, 2 give every row every off).  Bodies 7 .. 11 are RAW: m_n = 0, 1, N - 1, N, 2N - 1.
    meta: dict(lists=[dict(amounts, skipped, hits)] per list -- skipped: its steps whose amounts are all zero; hits: the union of
    step_properties over its steps --, msg=[the message of a semantic row, -1 for a raw one] per row)"""
    lists = planted_mask_lists(N, n, group)
    sk = [int(s) for s in sk_lwe]
    assert len(sk) == n and len(lists) == 5
    edge = N // (2 * p) - 2
    raw = [0, 1, N - 1, N, 2 * N - 1]
    assert PLANTED_ROWS == 5 * (p + len(raw)) and edge > 0
    fields = np.zeros((PLANTED_ROWS, n + 1), np.uint32)
    msg = []
    for j in range(PLANTED_ROWS):
        mask, body = lists[j % 5], j // 5
        fields[j, :n] = mask
        if body < p:
            off = (0, edge, -edge)[(j + turn) % 3]
            fields[j, n] = (sum(m for m, s in zip(mask, sk) if s) + (2 * body * N + p) // (2 * p) + off) % (2 * N)
            msg.append(body)
        else:
            fields[j, n] = raw[body - p]
            msg.append(-1)
    meta_lists = []
    for lst in lists:
        steps = [lst[i:i + group] for i in range(0, n, group)]
        meta_lists.append(dict(amounts=list(lst), skipped=[i for i, s in enumerate(steps) if not any(s)],
                               hits=set().union(*(step_properties(s, N) for s in steps))))
    return fields, dict(lists=meta_lists, msg=msg)


def planted_output_margin(prm):
    """standard deviations between a bootstrap output's phase and the edge of its box, q / 4p over the blind rotation's own noise
    (params.variances: the planted fields carry no noise of their own, and neither key switch nor modulus switch runs).  Six
    instantiations, k_blind_rotate_cu<L,1,1> and <L,1,2>, are by their template arguments ONE gadget level of at most 9 and 7 bits: no
    gadget that reaches them is a usable parameter set (0.2 to 1 sigma at N >= 1024, the reference itself decrypts many rows wrongly
    there); they are compared word for word only."""
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.params import variances
    return (1.0 / (4.0 * prm["p_msg"])) / math.sqrt(variances(Params(**prm))[0])


PLANTED_MARGIN = 6.0                                                    # the margin the selector asks of a usable set (params.py)


# ---- packed outputs: the definition restated, its fast form, the shapes and the planted fields -------------------------------------
# (include/fbs_exec.h, "packed outputs", steps 2 - 5 and the transport; tests/test_packed_reference.py holds these helpers to their
# claims without a GPU, tests/test_gpu_pack_shapes.py and tests/test_gpu_packed.py hold the kernels of csrc/fbs_pack.hip to them)
PACK_SHAPES = [(8, 1), (9, 1), (10, 1), (11, 1), (12, 1),               # (log N, k): what FBS_PACK_SHAPES instantiates, restated
               (8, 2), (8, 3), (8, 4), (9, 2), (9, 3), (9, 4), (10, 2), (10, 3)]
PACK_BODY_FIELDS = (0, 1, 1 << 30, (1 << 31) - 1, 2114, 2115)           # 2114 < 2^30 / 507903 < 2115: pack_lift_body's floor term
PACK_KEYS = ((3, 10), (1, 27))                                          # n t_p = 18 > 16 centres the lazy sums, 6 does not; the shipped digit
PACK_EDGE_KEYS = ((1, 31), (31, 1), (2, 15))                            # r = 0 and the widest digit; r = 0 and the most levels; r = 1
_PACK_ACC = {}


def pack_toy(log_n, k, n, p=3):
    """the smallest parameter set of a packing shape: the toy recipes of the packed and GLWE tests, and at k = 1, N = 2048 / 4096 the
    gadgets of tests/test_gpu_device_keys.py"""
    from tfhe_fbs_map_amd import Params
    if k == 1:
        l, beta = {11: (2, 14), 12: (1, 21)}.get(log_n, (2, 10))
        return Params(n=n, log_n_poly=log_n, k=1, l_bsk=l, beta_bsk=beta, t_ksk=8, gamma_ksk=2, p_msg=p, sigma_lwe=1 << 8, sigma_glwe=4)
    return Params(n=n, log_n_poly=log_n, k=k, l_bsk=1, beta_bsk=21 if k == 2 else 18, t_ksk=8, gamma_ksk=2, p_msg=p,
                  sigma_lwe=1 << 8, sigma_glwe=4, bsk_group=2)


def balanced_digits(a, t, gamma):
    """a' [..] -> digits [t][..], v = 0 the most significant; carries upwards, the carry out of the top dropped"""
    a = np.asarray(a, np.int64)
    B = 1 << gamma
    out = np.zeros((t,) + a.shape, np.int64)
    carry = np.zeros(a.shape, np.int64)
    for v in range(t - 1, -1, -1):
        u = ((a >> (gamma * (t - 1 - v))) & (B - 1)) + carry
        carry = (u >= B // 2).astype(np.int64)
        out[v] = u - carry * B
    return out


def rounded_mask_fields(m, t, gamma):
    """mask fields at 31 bits -> a' at t gamma bits (step 2)"""
    m = np.asarray(m, np.int64)
    r = 31 - t * gamma
    return (((m >> (r - 1)) + 1) >> 1) % (1 << (t * gamma)) if r > 0 else m


def negacyclic(d, a):
    """d (small signed integers) times a (canonical residues): rotations when d is sparse, else the oracle's schoolbook product"""
    from oracle import tfhe_oracle as orc
    N = len(a)
    nz = np.flatnonzero(d)
    if nz.size <= 4:
        acc = [0] * N
        for j in nz:
            for i in range(N):
                s = int(d[j]) * int(a[i])
                if i + j < N:
                    acc[i + j] += s
                else:
                    acc[i + j - N] -= s
        return np.array([x % Q for x in acc], np.uint64)
    return orc.polymul_schoolbook(np.array([int(x) % Q for x in d], np.uint64), a)


def sample_residues(fields, key, t, gamma, tag, fast=False):
    """fields [fill][n+1] at 31 bits -> the k + 1 polynomials of the packed sample mod q (steps 2 - 5); `tag` names the key (the
    memo is per key, digits and fields).  fast: every product D_(i,v) times a key polynomial by the oracle's NTT, the digits taken
    mod q -- the same residues (tests/test_packed_reference.py), milliseconds where the schoolbook product takes seconds"""
    memo = (tag, t, gamma, fast, fields.tobytes())
    if memo in _PACK_ACC:
        return _PACK_ACC[memo]
    fill, n = fields.shape[0], fields.shape[1] - 1
    k1, N = key.shape[2], key.shape[3]
    digits = balanced_digits(rounded_mask_fields(fields[:, :n], t, gamma), t, gamma)                 # [t][fill][n]
    acc = np.zeros((k1, N), np.uint64)
    if fast:
        from oracle import tfhe_oracle as orc
        residues = np.mod(digits, Q).astype(np.uint64)
    for i in range(n):
        for v in range(t):
            if fast:
                d = np.zeros(N, np.uint64)
                d[:fill] = residues[v, :, i]
            else:
                d = np.zeros(N, np.int64)
                d[:fill] = digits[v, :, i]
            for c in range(k1):
                prod = orc.polymul_ntt(d, key[i, v, c]) if fast else negacyclic(d, key[i, v, c])
                acc[c] = (acc[c] + prod) % np.uint64(Q)
    res = (np.uint64(Q) - acc) % np.uint64(Q)
    for j in range(fill):
        res[k1 - 1, j] = (int(res[k1 - 1, j]) + ((int(fields[j, n]) * Q + (1 << 30)) >> 31)) % Q
    _PACK_ACC[memo] = res
    return res


def packed_sample_count(k, N, fill, bits):
    """words of a packed sample that holds `fill` outputs, restated"""
    return k * N * bits // 64 + -(-fill * bits // 64)


def packed_count(k, N, count, bits):
    """words of a batch of `count` outputs: full samples, then the rest"""
    return count // N * packed_sample_count(k, N, N, bits) + (packed_sample_count(k, N, count % N, bits) if count % N else 0)


def reference_pack(fields, key, t, gamma, bits, tag, fast=False):
    """fields [count][n+1] -> the packed words of the batch (transport rounding and format).  fast: `sample_residues`' fast form,
    and the bit stream made from its bits with numpy instead of one long integer"""
    k1, N = key.shape[2], key.shape[3]
    words = []
    for g0 in range(0, fields.shape[0], N):
        part = fields[g0:g0 + N]
        res = sample_residues(part, key, t, gamma, tag, fast)
        rounded = (((res >> np.uint64(45 - bits)) + np.uint64(1)) >> np.uint64(1)) & np.uint64((1 << bits) - 1)
        n_words = packed_sample_count(k1 - 1, N, part.shape[0], bits)
        if fast:
            flat = np.concatenate([rounded[:k1 - 1].reshape(-1), rounded[k1 - 1, :part.shape[0]]])
            stream = ((flat[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
            stream = np.concatenate([stream, np.zeros(64 * n_words - stream.size, np.uint8)])
            words += [int(w) for w in np.packbits(stream, bitorder="little").view("<u8")]
            continue
        flat = [int(x) for c in range(k1 - 1) for x in rounded[c]] + [int(x) for x in rounded[k1 - 1, :part.shape[0]]]
        stream = 0
        for idx, f in enumerate(flat):
            stream |= f << (idx * bits)
        words += [(stream >> (64 * j)) & (2 ** 64 - 1) for j in range(n_words)]
    return np.array(words, np.uint64)


def decode_phases(words, prm, count, bits, sk_glwe):
    """packed words -> phases [count] mod 2^bits (numpy restatement of the decode)"""
    N, k = prm.N, prm.k
    full = (k + 1) * N * bits // 64
    S = np.asarray(sk_glwe, np.int64).reshape(k, N)
    out = []
    for g in range(-(-count // N)):
        fill = min(N, count - g * N)
        sample = words[g * full:]
        stream = 0
        n_words = k * N * bits // 64 + -(-fill * bits // 64)
        for j in range(n_words):
            stream |= int(sample[j]) << (64 * j)
        f = np.array([(stream >> (i * bits)) & ((1 << bits) - 1) for i in range(k * N + fill)], np.int64)
        phase = np.zeros(N, np.int64)
        phase[:fill] = f[k * N:]
        for c in range(k):
            full_conv = np.convolve(f[c * N:(c + 1) * N], S[c])
            prod = full_conv[:N].copy()
            prod[:N - 1] -= full_conv[N:]
            phase -= prod
        out.append(phase[:fill] % (1 << bits))
    return np.concatenate(out)


def planted_mask_fields(t, gamma):
    """{name: a mask field at 31 bits} for a packing key (t, gamma), r = 31 - t gamma: the edges of pack_round_mask and of the
    balanced digits that random words do not reach.  A field a' << r rounds to a'.
      zero, ones        0, and 2^31 - 1: rounds up to 2^(t gamma) and wraps to 0 when r > 0 (at r = 0 it is a' itself)
      tie, below_tie    2^(r-1) -> 1 and 2^(r-1) - 1 -> 0, when r > 0
      all_low           a' = -offs mod 2^(t gamma), offs = B/2 at every position: every digit -B/2.  As an unsigned number that is
                        the lowest gamma bits B/2 and every higher group B/2 - 1: the carry that starts at the bottom, runs through
                        every level and is dropped at the top -- one value under both descriptions
      all_high          every digit B/2 - 1
      top_half          a' = 2^(t gamma - 1): the top digit alone is -B/2 (and the carry dropped); all_low itself at t = 1"""
    tg, r, B = t * gamma, 31 - t * gamma, 1 << gamma
    offs = sum((B // 2) << (gamma * v) for v in range(t))
    out = {"zero": 0, "ones": (1 << 31) - 1, "all_low": ((-offs) % (1 << tg)) << r, "all_high": ((1 << tg) - 1 - offs) << r,
           "top_half": (1 << (tg - 1)) << r}
    if r > 0:
        out.update(tie=1 << (r - 1), below_tie=(1 << (r - 1)) - 1)
    return out


def planted_positions(count):
    """the ciphertext positions the planted mask fields are spread over: the first two and the last two"""
    return sorted({j for j in (0, 1, count - 2, count - 1) if 0 <= j < count})


def planted_pack_fields(n, count, t_p, gamma_p, seed):
    """[count][n + 1] uint32 below 2^31, as the key switch of fbs_pack_dev leaves them: random fields; in every mask column the
    values of `planted_mask_fields` in turn over `planted_positions` (column i starts where column i - 1 stopped, so that n = 6
    columns of four positions hold every value); in the body column PACK_BODY_FIELDS over the first and the last three positions"""
    rng = np.random.default_rng(seed)
    fields = rng.integers(0, 1 << 31, (count, n + 1), dtype=np.uint32)
    values = list(planted_mask_fields(t_p, gamma_p).values())
    turn = 0
    for i in range(n):
        for j in planted_positions(count):
            fields[j, i] = values[turn % len(values)]
            turn += 1
    spots = sorted({j for j in (0, 1, 2, count - 3, count - 2, count - 1) if 0 <= j < count})
    for s, j in enumerate(spots):
        fields[j, n] = PACK_BODY_FIELDS[s % len(PACK_BODY_FIELDS)]
    return fields
