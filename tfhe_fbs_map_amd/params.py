"""Parameter sets, the security floor on the noise, a noise model and the parameter selector.

The reference never fixes cryptographic parameters: it hands (precision p = number of plaintext values, squared
2-norm of the linear combinations) -- `stats()["norm2_linprod"]`, fbs_mapper/fbs_exec_env.py:245-276 -- to a patched
concrete-optimizer (experiments/add_exec_estimates.py:9-16) that returns `k, N, n, br_l, br_b, ks_l, ks_b, cost`
(experiments/concrete.patch:163) at a fixed security level and error probability (`--security-level`, default 128;
`--p-error`, default "4 sigma", concrete.patch:56,139-140), under the contract that the noise entering a bootstrap
stays inside half a box, q/(4p), at that probability (concrete.patch:21-27: 2^(log q - 2) / precision).  That
optimizer is Rust, un-vendored and unbuildable here.  `choose_params` is its stand-in for THIS executor: same inputs,
same outputs, the same contract, this executor's own noise formulas and cost unit.

All variances are relative to q^2 (torus units).

Security.  `sigma_min(dim)` is the smallest noise standard deviation for which an LWE instance of dimension `dim`
with a binary secret is estimated to resist 2^128 operations.  It restates the 128-bit line of the security curves
that concrete-optimizer itself uses (concrete-security-curves, generated with the lattice estimator; the optimizer's
`minimal_variance_lwe` evaluates log2(sigma/q) = slope * dim + bias and floors it at 2^2/q):
        slope = -0.0265994623, bias = 2.9815431841   (security level 128, binary keys)
[NOT IN REFERENCE: restated from the public source of zama-ai/concrete at the release the reference pins
(README.md:17); neither that source nor the estimator is available offline, so the two constants are unverifiable
here.  Cross-check against published TFHE-rs 128-bit parameter sets: n = 742 -> 2^-16.8 here against 2^-17.1
published; N = 2048 -> 2^-51.5 against 2^-51.6: this line is the more conservative of the two.]
The line does not depend on q; the floor does: with the 46-bit modulus of this executor no noise is ever below
2^-44 q, which is why N = 2048 keys are noisier here than under a 64-bit modulus (and still far inside the budget).

`P1024` -- BASELINE.md's synthetic benchmark shape n=630 N=1024 k=1 l=3 beta=7 t=8 gamma=2 -- is kept for the
throughput benchmark with REDUCED NOISE (sigma = 2^-40 q): at 128-bit noise an N = 1024 accumulator cannot carry
p = 15 (see `margin_sigmas`), so that set is a kernel benchmark shape, not a secure configuration, and says so
(`Params.security_bits`).
"""
from __future__ import annotations

import math

from ._client_native import Params
from .security import MODULUS, MODULUS_BITS

# ---- security floor (constants and sigma_min live in security.py, which has no dependencies) --------------------
from .security import MIN_LOG2_SIGMA_ABS, SECURITY_CURVES, log2_sigma_min, sigma_min      # noqa: E402,F401


def security_bits(prm: Params) -> float:
    """Rough security estimate of a parameter set: 128 (or more) when both noises sit on or above the 128-bit
    line, otherwise 128 scaled by dimension over the dimension that noise would need (security is close to
    linear in the dimension at fixed log(q/sigma))."""
    slope, bias = SECURITY_CURVES[128]
    worst = float("inf")
    for dim, sigma in ((prm.n, prm.sigma_lwe), (prm.k * prm.N, prm.sigma_glwe)):
        rel = math.log2(max(sigma, 1) / MODULUS)
        need = (rel - bias) / slope                       # dimension at which this sigma is 128-bit secure
        worst = min(worst, 128.0 * dim / max(need, 1.0))
    return worst


def with_secure_noise(prm: Params, security: int = 128) -> Params:
    return prm.replace(sigma_lwe=sigma_min(prm.n, security), sigma_glwe=sigma_min(prm.k * prm.N, security))


REDUCED_SIGMA = 1 << 6                                                    # 2^-40 q

# BASELINE.md's benchmark shape, REDUCED NOISE (not secure; see the module docstring)
P1024 = Params(n=630, log_n_poly=10, l_bsk=3, beta_bsk=7, t_ksk=8, gamma_ksk=2).reduced_noise(REDUCED_SIGMA)
# its N = 2048 sibling for p = 31 (24 gadget bits as three levels of eight), REDUCED NOISE as well
P2048 = P1024.replace(log_n_poly=11, l_bsk=3, beta_bsk=8)


def params_for(p: int, norm2: int | None = None) -> Params:
    """The reduced-noise benchmark set for plaintext modulus p: the modulus switch alone (n = 630) leaves about
    N / (10.2 p) standard deviations between a value and the edge of its box, so p <= 16 fits N = 1024 and p <= 32
    wants N = 2048.  For a secure set use `choose_params`."""
    base = P1024 if p <= 16 else P2048
    return base.replace(p_msg=p)


# ---- noise model -------------------------------------------------------------------------------------------------
def variances(prm: Params):
    """(blind-rotate output, key switch, modulus switch) variances in torus units."""
    q = float(MODULUS)
    N, n, k, l, t = prm.N, prm.n, prm.k, prm.l_bsk, prm.t_ksk
    B, b2 = 2.0 ** prm.beta_bsk, 2.0 ** prm.gamma_ksk
    s_glwe, s_lwe = prm.sigma_glwe / q, prm.sigma_lwe / q
    # external product: (k+1) l N balanced digits of variance (B^2+2)/12 against key noise in every step, plus the
    # rounding of the decomposition (half an ulp of q/B^l) seen through a binary GLWE key -- the latter only in the
    # steps whose LWE key bit is 1 (the CMUX output is s_i times the rounded difference): half of them.
    # Measured on the GPU this lands 15-35 % above the observed noise (tests/test_gpu_parity.py).
    if prm.bsk_group == 2:
        # two key bits per step: n/2 external products by a bundle of three keys, each times a monomial difference
        # X^e - 1 (squared norm 2): 6 sigma^2 of key noise per product where two single steps carry 2; the rounding of
        # the decomposition of ACC is seen through X^(a0 s0 + a1 s1) - 1, non-zero for three of the four key-bit pairs
        v_br = n / 2.0 * ((k + 1) * l * N * (B * B + 2) / 12.0 * 6.0 * s_glwe ** 2
                          + 1.5 * (1 + k * N / 2.0) / (12.0 * B ** (2 * l)))
    else:
        v_br = n * ((k + 1) * l * N * (B * B + 2) / 12.0 * s_glwe ** 2 + 0.5 * (1 + k * N / 2.0) / (12.0 * B ** (2 * l)))
    # key switch: kN t balanced digits in [-2^g/2, 2^g/2) against key noise, plus the rounding to t*gamma bits
    # seen through a binary key
    v_ks = k * N * (t * (b2 * b2 + 2) / 12.0 * s_lwe ** 2 + 0.5 / (12.0 * b2 ** (2 * t)))
    # modulus switch, mean-compensated (k_ms_body, fbs_kernels.hip): the body's own rounding, and the n mask roundings seen through
    # s_i - 1/2 (variance 1/4) because the expected value sum eps_i / 2 is taken off the body before it is rounded
    v_ms = (1 + n / 4.0) / (12.0 * (2.0 * N) ** 2)
    return v_br, v_ks, v_ms


def margin_sigmas(prm: Params, norm2: float = 1.0) -> float:
    """Half box width q/(4p) divided by the standard deviation of the phase that enters the blind rotation, when
    the inputs of the linear combination are bootstrap outputs (the reference's contract, concrete.patch:21-27:
    norm2 * bootstrap noise + key switch + modulus switch against 2^(log q - 2)/p)."""
    v_br, v_ks, v_ms = variances(prm)
    sigma = math.sqrt(norm2 * v_br + v_ks + v_ms)
    return (1.0 / (4.0 * prm.p_msg)) / sigma


# ---- compact outputs (include/fbs_exec.h, "compact outputs") ----------------------------------------------------------------
def compact_output_variance(prm: Params, bits: int, out_norm2: float = 1.0) -> float:
    """Phase variance of a compact output at width `bits`: the output's own noise (out_norm2 times a blind rotation's: 1 for a
    bootstrap output, its coefficients' squared norm for a linear combination of bootstrap outputs, |D_F|^2 for a table cut from a
    shared rotation, about 0 for inputs and constants), the key switch to the small key, and the mean-compensated rounding of the
    n + 1 fields to Z_(2^bits) -- the modulus switch of `variances` at 2^bits in place of 2N."""
    v_br, v_ks, _ = variances(prm)
    return out_norm2 * v_br + v_ks + (1 + prm.n / 4.0) / (12.0 * 2.0 ** (2 * bits))


def compact_output_skew(prm: Params) -> float:
    """Bound on the deterministic shift of the phase (torus units) that rounding with q treated as 2^46 leaves: each of the
    n + 1 fields is off by at most (2^46 - q) / 2^46 of the torus, whatever the width."""
    return (prm.n + 1) * float((1 << MODULUS_BITS) - MODULUS) / float(1 << MODULUS_BITS)


def compact_output_margin(prm: Params, bits: int, out_norm2: float = 1.0) -> float:
    """Standard deviations between a compact output's phase and the edge of its box: (q/(4p) - skew) / sigma, the counterpart
    of `margin_sigmas` for what a client decodes."""
    return (1.0 / (4.0 * prm.p_msg) - compact_output_skew(prm)) / math.sqrt(compact_output_variance(prm, bits, out_norm2))


def compact_output_bits(prm: Params, norm2: float = 1.0, out_norm2: float = 1.0) -> int:
    """The narrowest width w >= log2(2N) at which a compact output decodes with at least the margin the parameter set was chosen
    for: `margin_sigmas(prm, norm2)` with the same skew counted on both sides (a deliberate departure from comparing against
    `margin_sigmas` as it stands, DESIGN.md section 4 "Compact outputs").  The modulus switch in front of every blind rotation
    rounds with q treated as 2^46 too, so the inputs the selector admitted carry that skew; `margin_sigmas` leaves it out, and
    comparing a skew-counted margin against it would ask for a wider field where nothing got worse (p = 31, N = 2048: 5.9986
    against 6.0017 at log2(2N)).  With out_norm2 <= norm2 -- every bootstrap output of a plain program -- the answer is log2(2N):
    such an output is no noisier than what the next bootstrap would have read.  31 when no width reaches the margin."""
    need = margin_sigmas(prm, norm2) * (1.0 - 4.0 * prm.p_msg * compact_output_skew(prm))
    for bits in range(prm.log_n_poly + 1, 32):
        if compact_output_margin(prm, bits, out_norm2) >= need * (1.0 - 1e-12):   # (equal variances: w = log2(2N))
            return bits
    return 31


# ---- packed outputs (include/fbs_exec.h, "packed outputs") -------------------------------------------------------------------
def packed_output_variance(prm: Params, t_p: int, gamma_p: int, bits: int, out_norm2: float = 1.0) -> float:
    """Phase variance of one output inside a packed GLWE sample at transport width `bits`, the sum of four terms: the compact
    output at 31 bits (what the packing key switch starts from); the packing key's noise, n t_p N balanced digits of variance
    (2^(2 gamma_p) + 2) / 12 against sigma_glwe; the rounding of the n mask fields to t_p gamma_p bits seen through a binary key;
    and the transport rounding of the body and of the k N mask coefficients (through a binary key) to 2^bits, without mean
    compensation."""
    s_glwe = prm.sigma_glwe / float(MODULUS)
    v_key = prm.n * t_p * prm.N * (2.0 ** (2 * gamma_p) + 2.0) / 12.0 * s_glwe ** 2
    v_digit = (prm.n / 2.0) * 2.0 ** (-2 * t_p * gamma_p) / 12.0
    v_transport = (1 + prm.k * prm.N / 2.0) / (12.0 * 2.0 ** (2 * bits))
    return compact_output_variance(prm, 31, out_norm2) + v_key + v_digit + v_transport


def packed_output_skew(prm: Params) -> float:
    """`compact_output_skew` for a packed output: the k N + 1 transport fields its phase is made of, plus the n + 1 fields of the
    31-bit stage, each off by at most (2^46 - q) / 2^46 of the torus."""
    return (prm.k * prm.N + 1 + prm.n + 1) * float((1 << MODULUS_BITS) - MODULUS) / float(1 << MODULUS_BITS)


def packed_output_margin(prm: Params, t_p: int, gamma_p: int, bits: int, out_norm2: float = 1.0) -> float:
    """Standard deviations between a packed output's phase and the edge of its box, skew counted as `compact_output_margin` does"""
    return (1.0 / (4.0 * prm.p_msg) - packed_output_skew(prm)) / math.sqrt(packed_output_variance(prm, t_p, gamma_p, bits, out_norm2))


def packed_margin_needed(prm: Params, norm2: float = 1.0) -> float:
    """`margin_sigmas(prm, norm2)` with the packed skew counted on its side too (as `compact_output_bits` does with its own)"""
    return margin_sigmas(prm, norm2) * (1.0 - 4.0 * prm.p_msg * packed_output_skew(prm))


def packing_choice(prm: Params, norm2: float = 1.0, out_norm2: float = 1.0):
    """(t_p, gamma_p, bits) of the packing key and the transport width for a program: among the choices whose
    `packed_output_margin` reaches `packed_margin_needed(prm, norm2)`, the smallest key -- the fewest levels t_p, then the widest
    digit gamma_p (t_p gamma_p <= 31) -- and then the narrowest width.  When nothing reaches it: (t_p, gamma_p) of the largest
    margin at 31 bits, the last resort `compact_output_bits` takes too."""
    need = packed_margin_needed(prm, norm2) * (1.0 - 1e-12)
    best = None
    for t_p in range(1, 32):
        for gamma_p in range(31 // t_p, 0, -1):
            if packed_output_margin(prm, t_p, gamma_p, 31, out_norm2) < need:
                if best is None or packed_output_margin(prm, t_p, gamma_p, 31, out_norm2) > 1.01 * packed_output_margin(prm, *best, out_norm2):
                    best = (t_p, gamma_p, 31)
                continue
            for bits in range(prm.log_n_poly + 1, 32):
                if packed_output_margin(prm, t_p, gamma_p, bits, out_norm2) >= need:
                    return t_p, gamma_p, bits
    return best


# ---- chained evaluation (include/fbs_exec.h, "chained evaluation") -------------------------------------------------------------
def refresh_input_variance(prm: Params, bits: int | None = None, out_norm2: float = 1.0) -> float:
    """Phase variance of what the refresh of a linked input rotates by.  A compact link (`bits` = its width w): the compact
    output's own variance (`compact_output_variance`), plus the modulus switch from 2^w down to 2N when w > log2(2N) (at w =
    log2(2N) the fields are already what the blind rotation reads).  A full link (bits=None): the ordinary bootstrap input at
    norm2 = out_norm2 -- its producer's noise, the key switch and the modulus switch."""
    v_br, v_ks, v_ms = variances(prm)
    if bits is None:
        return out_norm2 * v_br + v_ks + v_ms
    return compact_output_variance(prm, bits, out_norm2) + (v_ms if bits > prm.log_n_poly + 1 else 0.0)


def refresh_margin(prm: Params, bits: int | None = None, out_norm2: float = 1.0) -> float:
    """Standard deviations between the phase a refresh reads and the edge of its box, (q/(4p) - skew) / sigma with the 2^46 rounding
    skew (`compact_output_skew`) counted as `compact_output_bits` counts it.  A link is admitted when this is at least
    `refresh_margin_needed(prm, norm2)` of the consuming program: the refresh is then no likelier to fail than the program's own
    bootstraps.  At w = log2(2N) and out_norm2 = 1 it equals margin_sigmas(prm, 1) (1 - 4 p skew)."""
    return (1.0 / (4.0 * prm.p_msg) - compact_output_skew(prm)) / math.sqrt(refresh_input_variance(prm, bits, out_norm2))


def refresh_margin_needed(prm: Params, norm2: float = 1.0) -> float:
    """`margin_sigmas(prm, norm2)` of the consuming program with the same skew counted on its side (`compact_output_bits`)"""
    return margin_sigmas(prm, norm2) * (1.0 - 4.0 * prm.p_msg * compact_output_skew(prm))


# ---- public-key inputs (include/fbs_exec.h, "public-key inputs") ---------------------------------------------------------------
def public_input_variance(prm: Params) -> float:
    """Phase variance, in torus units, of a public-key encryption under the GLWE key: the phase is sum_r u_r E_r + e_k - sum_c e_c S_c
    + Delta M with u and S binary -- k N / 2 terms of variance sigma_glwe^2 from each sum on average, and e_k: (1 + k N) sigma_glwe^2."""
    return (1.0 + prm.k * prm.N) * (prm.sigma_glwe / float(MODULUS)) ** 2


def public_input_factor(prm: Params) -> float:
    """`public_input_variance` in units of one blind rotation's output variance: the unit `split.output_noise_factors` and
    `split.plan_chain` count in.  At most 1 means that a public-key input enters a program as a bootstrap output does."""
    return public_input_variance(prm) / variances(prm)[0]


# ---- folded state (include/fbs_exec.h, "folded state") ---------------------------------------------------------------------------
def folded_state_variance(prm: Params, t_f: int, gamma_f: int) -> float:
    """Phase variance, in torus units, that a fold adds to each ciphertext it holds (and an unfold gives back unchanged: sample
    extraction is exact).  Modelled as the packing key is in `packed_output_variance`, with the D = k N words of the big key in
    place of the n of the small one: D t_f N balanced digits of variance (2^(2 gamma_f) + 2) / 12 against sigma_glwe, and the
    rounding of the D mask words to t_f gamma_f bits seen through a binary key.  Neither sigma_lwe nor any transport rounding
    enters: the key switch is taken straight from the big key and the sample keeps every bit."""
    s_glwe = prm.sigma_glwe / float(MODULUS)
    D = prm.k * prm.N
    return D * t_f * prm.N * (2.0 ** (2 * gamma_f) + 2.0) / 12.0 * s_glwe ** 2 + (D / 2.0) * 2.0 ** (-2 * t_f * gamma_f) / 12.0


def folded_state_skew(prm: Params) -> float:
    """`packed_output_skew` for a fold: the D mask words are rounded with q treated as 2^46, each off by at most (2^46 - q) / 2^46
    of the torus; the body is not rounded at all."""
    return prm.k * prm.N * float((1 << MODULUS_BITS) - MODULUS) / float(1 << MODULUS_BITS)


def folded_state_factor(prm: Params, t_f: int, gamma_f: int) -> float:
    """`folded_state_variance` in units of one blind rotation's output variance, the unit `split.plan_chain` counts in"""
    return folded_state_variance(prm, t_f, gamma_f) / variances(prm)[0]


def folded_margin(prm: Params, norm2: float, t_f: int, gamma_f: int) -> float:
    """`margin_sigmas(prm, norm2)` recomputed with v_br (1 + folded_state_factor) in place of v_br: every input of the linear
    combination has been through one fold since its bootstrap"""
    v_br, v_ks, v_ms = variances(prm)
    v_br += folded_state_variance(prm, t_f, gamma_f)
    return (1.0 / (4.0 * prm.p_msg)) / math.sqrt(norm2 * v_br + v_ks + v_ms)


def fold_choice(prm: Params, norm2: float = 1.0, min_margin: float = 6.0):
    """(t_f, gamma_f) of the fold key for programs of that norm2: the fewest levels t_f at which some digit width keeps
    `folded_margin` at or above `min_margin`, and at that level count the gamma_f of least `folded_state_variance` (t_f gamma_f <=
    31).  The last resort, when no choice reaches the margin: the (t_f, gamma_f) of least variance over all of them -- the fold then
    costs as little margin as it can, and `split.plan_chain` refreshes the link if its own rule refuses it."""
    best = None
    for t_f in range(1, 32):
        gamma_f = min(range(1, 31 // t_f + 1), key=lambda g: folded_state_variance(prm, t_f, g))
        if folded_margin(prm, norm2, t_f, gamma_f) >= min_margin:
            return t_f, gamma_f
        if best is None or folded_state_variance(prm, t_f, gamma_f) < folded_state_variance(prm, *best):
            best = (t_f, gamma_f)
    return best


# ---- encrypted-index reads (include/fbs_exec.h, "encrypted-index reads") ------------------------------------------------------------
def lookup_output_norm2(table_out_norm2: float, fold_factor: float, digits: int = 1) -> float:
    """What a lookup's output carries, in units of one blind rotation's output variance: the table entry's own noise, and per digit
    the fold that laid the round's table out (`folded_state_factor`) and the rotation that read it.  Rotating by a monomial adds
    nothing, so the entry's noise goes through once however many digits there are."""
    return table_out_norm2 + digits * (fold_factor + 1.0)


# what `choose_params` and `fold_choice` ask of a set by default (their min_margin): the floor `split.plan_lookup` holds a lookup's
# refreshed output to when its caller names none
SET_MARGIN = 6.0


def lookup_index_margin(prm: Params, index_out_norm2: float = 1.0) -> float:
    """Standard deviations between the phase a lookup rotates by and the edge of its box: the index is read like any refreshed
    full link (`refresh_margin` at bits=None)"""
    return refresh_margin(prm, None, index_out_norm2)


# ---- encrypted tables (include/fbs_exec.h, "encrypted tables") ------------------------------------------------------------------------
TABLE_ADD, TABLE_SET = 0, 1


def table_write_norm2(table_norm2: float, value_norm2: float, fold_factor: float, mode: int = TABLE_ADD) -> float:
    """What a resident table carries after a write, in units of one blind rotation's output variance: what it carried, the value's own
    noise, the fold that laid the value out as a unit box and the rotation that turned it; a set adds the refreshed copy of the old
    entry that is taken off, a bootstrap output.  The fold is counted whole.  A unit box has only about spread N / p sources, but
    fold_factor x that share is NOT what its fold adds where the value lies: of `folded_state_variance`'s two terms only the key
    noise is a sum over the sources; the rounding of a ciphertext's own mask words stays whole at its own coefficient.  Measured on
    unit boxes alone, the filled coefficients carry 0.73 of the whole fold and 5.4 times the share (profiles/tables/README.md)."""
    return table_norm2 + value_norm2 + fold_factor + 1.0 + (1.0 if mode == TABLE_SET else 0.0)


def table_read_norm2(table_norm2: float) -> float:
    """What a read of a resident table returns: the table's noise and the rotation that read it"""
    return table_norm2 + 1.0


def p_error(margin: float) -> float:
    """Probability that a Gaussian leaves +-margin standard deviations (one bootstrap)."""
    return math.erfc(margin / math.sqrt(2.0))


def bootstrap_cost(prm: Params) -> float:
    """Relative cost of one functional bootstrap, in the unit the kernels are bound by (FP64 instruction issue), with
    the default P1024 shape = 1.  Per CMUX step and coefficient, from the instruction counts of k_blind_rotate (DESIGN.md
    section 5): (k+1)(l+1) transforms of log N / 2 butterflies of 8 instructions, (k+1)^2 l exact products of 7 (accumulate
    included), 2 l for the digits and 12 for rotation, rounding and re-centring; times n steps, times what the multi-wave
    transforms of N >= 2048 cost on top -- and what they do NOT gain from the whole-CU workgroups and the priority
    hand-over that sped the benchmark shape up at the end of round 2 (measured: 1.19 at N = 2048, 1.22 at N = 4096).
    Against measurements (profiles/r02/selector_bench.jsonl, blind rotation per 1024-batch over P1024's 9.33 ms): N = 1024
    l = 2 0.67-0.76 modelled / 0.69-0.82 measured; N = 2048 l = 1 1.41 / 1.41; N = 2048 l = 2 2.32 / 2.30; N = 4096 l = 2
    5.5 / 5.5.  The kN t (n+1) multiply-adds of the key switch are weighted by their measured share
    (1.2 % of the P1024 step since it runs as an int8 GEMM on the matrix cores; 5 % before).  The reference ranks parameter
    sets by the optimizer's `boot_cost` (experiments/analyse_results.py:10); this is the same ranking for this executor."""
    N, n, k, l, t = prm.N, prm.n, prm.k, prm.l_bsk, prm.t_ksk

    def blind(n_, l_, N_, log_n, k=k):
        per_coefficient = (k + 1) * ((l_ + 1) * 4.0 * log_n + 7.0 * (k + 1) * l_ + 2.0 * l_ + 12.0)
        return n_ * N_ * per_coefficient * (1.22 if log_n >= 12 else 1.19 if log_n == 11 else 1.0)

    # two key bits per step (bsk_group = 2), MEASURED against one bit per step at the same shape (profiles/r02): 0.74 with one
    # gadget level (9.8 against 13.2 ms per 1024 bootstraps at N = 2048, n = 714 / 710).  With l levels the bundle costs
    # 6 l exact products per coefficient and pair of key bits where it saves l + 1 transforms: it does not pay beyond
    # l = 1 in the two-waves-per-polynomial kernel (P1024, l = 3: 13.5 against 10.8 ms).  N = 2048 with TWO levels runs on the
    # whole-CU kernel, which has the registers for it: 17.1 ms per 1024 bootstraps at n = 758 against 21.9 ms at n = 766 with one
    # bit per step (round 3: what the 128-bit sets for p = 31 now take)
    pairs = 1.0 if prm.bsk_group != 2 else (0.74 if l == 1 else 0.79 if (l == 2 and prm.log_n_poly == 11) else 1.25)
    # GLWE dimension k = 2 at N = 1024 (k_blind_rotate_pairs_k2, round 3: three wave-private 1024-point transforms each way on three
    # waves per bootstrap, twelve waves per CU), MEASURED: 7.50 ms per 1024 bootstraps at n = 760 against P1024's 9.26
    if k == 2 and prm.log_n_poly == 10 and prm.bsk_group == 2 and l == 1:
        pairs = 0.867
    elif k >= 2:
        # every other k >= 2 (k_blind_rotate_glwe: k + 1 waves per bootstrap): modelled instructions times what the kernel was MEASURED
        # to take per modelled instruction, shape by shape (profiles/r04/glwe_calibration.txt), over P1024's 9.2 ms per 1 024
        # (a further level costs a step more than its instructions -- its transform hangs on the one before: at p = 2, 566 steps of
        # two levels at k = 2 take 1.93 ms per launch of 64 where 570 steps of one level at k = 3 take 1.44, at the same throughput)
        return (glwe_instructions(prm) / 1e6 * glwe_ms_per_minstr(prm.log_n_poly, k) / 9.2 * (1.0 + 0.04 * (l - 1))
                + 0.012 * (k * N * t * (n + 1)) / (1024 * 8 * 631.0))
    return 0.988 * pairs * blind(n, l, N, prm.log_n_poly) / blind(630, 3, 1024, 10, 1) + 0.012 * (k * N * t * (n + 1)) / (1024 * 8 * 631.0)


def glwe_shape_built(log_n: int, k: int) -> bool:
    """Is there a blind-rotation kernel for GLWE dimension k >= 2 at N = 2^log_n (csrc/fbs_select.hpp: FBS_GLWE_SHAPES)?"""
    return (k in (2, 3, 4) and log_n in (8, 9)) or (k in (2, 3) and log_n == 10)


def glwe_instructions(prm: Params) -> float:
    """FP64 wave-instructions per bootstrap of k_blind_rotate_glwe, modelled: per step and coefficient (k+1) [(l+1) transforms of log N / 2
    butterflies of 8 + (k+1) l products of 7 -- four times that with two key bits per step, the bundle's three products included -- + 2 l
    for the digits + 12 for rounding and re-centring], n (or n / 2) steps, 64 lanes."""
    k, l, group = prm.k, prm.l_bsk, prm.bsk_group if prm.bsk_group == 2 else 1
    per_coef = (k + 1) * ((l + 1) * 4.0 * prm.log_n_poly + 7.0 * (k + 1) * l * (4 if group == 2 else 1) + 2.0 * l + 12.0)
    return prm.n / group * prm.N * per_coef / 64.0


# ms per 1 024 bootstraps per million modelled instructions, in full rounds of workgroups (tools/glwe_calibrate.py on the 128-bit sets
# for p = 4 of every shape; k_blind_rotate_pairs_k2<10,4> on the same scale: 2.48): by (log2 N, k), the slower of one / two key bits per step
GLWE_MS_PER_MINSTR = {(8, 4): 3.04, (9, 2): 2.47, (9, 3): 2.70, (9, 4): 3.04, (10, 2): 3.37, (10, 3): 2.69}


def glwe_ms_per_minstr(log_n: int, k: int) -> float:
    return GLWE_MS_PER_MINSTR.get((log_n, k), 3.1)


# ---- selector ------------------------------------------------------------------------------------------------------
DEFAULT_GLWE_DIMS = (1, 2, 3)    # the GLWE dimensions ExecConfig admits (fbs_exec_env.ExecConfig.glwe_dims)
REFERENCE_MARGIN = 4.0          # the optimizer's default p_error is "4 sigma" (concrete.patch:56: default_value_t = _4_SIGMA)

_GADGETS = [(l, beta) for l in (1, 2, 3, 4, 5, 6) for beta in range(3, 24) if 10 <= l * beta <= 30]
_SWITCHES = [(t, g) for g in (1, 2, 3, 4, 5, 6) for t in range(1, 24) if 8 <= t * g <= 30]


def _switch_fits(t, g, N):
    bits = MODULUS_BITS + g + math.log2(t * N)
    return bits <= 63.9 and bits - 32.0 <= 31.9          # the key-switch kernels' 64-bit accumulators (dev_supported)


def choose_params(p: int, norm2: float = 1.0, min_margin: float = 6.0, security: int | None = 128,
                  sigma: int | None = None, poly_sizes=(9, 10, 11, 12), n_range=(450, 1200, 4),
                  floor_margin: float | None = None, groups=(1, 2), glwe_dims=(1,), sampler: int = 0) -> Params:
    """Cheapest parameter set (n, N, l, beta, t, gamma and both noises) for plaintext modulus p and squared 2-norm
    `norm2` whose modelled margin is at least `min_margin` standard deviations -- what the reference obtains from its
    patched optimizer for (precision, sq_norm2) (experiments/add_exec_estimates.py:9-16, concrete.patch:21-27,163).

    security = 128: each noise is the smallest the security line allows for its dimension (`sigma_min`); n runs over
    `n_range`, N over 2^poly_sizes (512 .. 4096; k = 1: the kernels' shape), the gadget over 1..6 levels of 3..23 bits, the key
    switch over 1..23 levels of 1..6 bits.  security = None with `sigma`: the same search at a fixed noise (the
    reduced-noise benchmark setting).  `groups`: key bits per blind-rotation step to consider (2 = the multi-bit form: half
    the steps on bundles of three GGSW samples, 1.5x the key, more noise per step; built for N >= 1024, l <= 5, even n).
    `glwe_dims`: GLWE dimensions to consider.  k = 2 at N = 1024 with two key bits per step and one gadget level has kernels of its
    own (k_blind_rotate_pairs_k2, k_blind_rotate_cu_k2): the noise floor of k N = 2048 on 1024-point transforms, what p = 15 takes at
    ordinary norms.  Every other k = 2, 3, 4 at N = 256 / 512 (k <= 3 at N = 1024), any depth, one or two key bits per step, runs on
    k_blind_rotate_glwe (k + 1 waves per bootstrap) and is priced by that kernel's measured cost: k = 3 at N = 512 -- k N = 1536, a
    noise floor between the two k = 1 offers, on 512-point transforms -- is what p <= 7 takes (183-208 k FBS/s in full rounds against
    151-164 k at k = 2, 1.6-1.9 ms per launch of up to one bootstrap per CU against 2.0-2.4).
    `sampler`: the noise sampler the set names (`Params.sampler`); it is carried through and moves nothing in the search -- both
    samplers have the standard deviation they are asked for.
    Cost = `bootstrap_cost`.  Raises ValueError when nothing reaches `min_margin`
    (p too large for N <= 4096 at this security level); with `floor_margin` the requirement is first relaxed in steps of
    half a sigma down to that floor."""
    import numpy as np
    if floor_margin is not None and floor_margin < min_margin:
        m = min_margin
        while True:
            try:
                return choose_params(p, norm2, m, security, sigma, poly_sizes, n_range, None, groups, glwe_dims, sampler)
            except ValueError:
                if m <= floor_margin:
                    raise
                m = max(floor_margin, m - 0.5)
    q = float(MODULUS)
    ns = np.arange(*n_range, dtype=np.float64)
    if security is not None:
        s_lwe = np.array([sigma_min(int(n), security) for n in ns]) / q
    else:
        s_lwe = np.full(ns.shape, float(sigma if sigma is not None else REDUCED_SIGMA) / q)
    need = (1.0 / (4.0 * p) / min_margin) ** 2              # largest admissible variance
    best = None
    for k, log_n in [(k_, ln) for k_ in glwe_dims for ln in poly_sizes]:
        if k >= 2 and not glwe_shape_built(log_n, k):
            continue                                        # no kernel for this (k, N)
        N = 1 << log_n
        s_glwe = (sigma_min(k * N, security) if security is not None else (sigma if sigma is not None else REDUCED_SIGMA)) / q
        v_ms = (1 + ns / 4.0) / (12.0 * (2.0 * N) ** 2)
        if (v_ms >= need).all():
            continue
        for (l, beta), group in [((l_, b_), g_) for (l_, b_) in _GADGETS for g_ in groups]:
            if group == 2 and k == 1 and (log_n < 10 or l > 5):
                continue
            if (k + 1) * l > 20:
                continue
            B = 2.0 ** beta
            key_term = (k + 1) * l * N * (B * B + 2) / 12.0 * s_glwe ** 2
            round_term = (1 + k * N / 2.0) / (12.0 * B ** (2 * l))
            v_br = ns * (key_term + 0.5 * round_term) if group == 1 else ns / 2.0 * (6.0 * key_term + 1.5 * round_term)
            room = need - v_ms - norm2 * v_br
            if (room <= 0).all():
                continue
            for t, g in _SWITCHES:
                if not _switch_fits(t, g, k * N):
                    continue
                b2 = 2.0 ** g
                v_ks = k * N * (t * (b2 * b2 + 2) / 12.0 * s_lwe ** 2 + 0.5 / (12.0 * b2 ** (2 * t)))
                ok = np.nonzero(v_ks <= room)[0]
                if ok.size == 0:
                    continue
                n = int(ns[ok[0]])                          # cost grows with n: the smallest feasible n is the cheapest
                cand = Params(n=n, log_n_poly=log_n, k=k, l_bsk=l, beta_bsk=beta, t_ksk=t, gamma_ksk=g, p_msg=p,
                              sigma_lwe=int(round(s_lwe[ok[0]] * q)), sigma_glwe=int(round(s_glwe * q)), bsk_group=group, sampler=int(sampler))
                key = (bootstrap_cost(cand), n, l, t)
                if best is None or key < best[0]:
                    best = (key, cand)
    if best is None:
        raise ValueError("no parameter set with N <= %d reaches %.1f sigma at p = %d, norm2 = %g"
                         % (1 << max(poly_sizes), min_margin, p, norm2))
    return best[1]


# ---- execution estimates: the reference's cost unit, in this executor's terms -------------------------------------------
# One MI355X at the benchmark shape P1024 (cost 1.0) in whole rounds of 1 024 bootstraps: profiles/r03/batch_sweep.txt,
# 106-110 k FBS/s by the box.  Everything `exec_estimate` says about time is this figure scaled by `bootstrap_cost`.
MI355X_FBS_PER_S_AT_COST_1 = 107e3


def exec_estimate(p: int, norm2: float, nb_bootstrap: int, samples: int = 1, **choose) -> dict:
    """What the reference's flow computes for a mapped circuit with its patched optimizer (experiments/add_exec_estimates.py:9-16:
    `boot_cost` of (precision = fbs_size, sq_norm2 = norm2_linprod); experiments/analyse_results.py: `total_cost = nb_bootstrap x
    boot_cost`), restated for THIS executor: the parameter set `choose_params(p, norm2)` picks, its `bootstrap_cost` (issue slots of
    these kernels, P1024 = 1) as `boot_cost`, `total_cost = nb_bootstrap x boot_cost`, and what that is in time on one MI355X when
    the levels are wide enough to fill whole rounds (`seconds`; narrow levels pay one bootstrap's latency per level instead:
    distributed.launch_ms prices those)."""
    prm = choose_params(p, norm2, **choose)
    cost = bootstrap_cost(prm)
    total = nb_bootstrap * cost
    return dict(params=prm, boot_cost=cost, total_cost=total, margin_sigmas=margin_sigmas(prm, norm2),
                seconds=total * samples / MI355X_FBS_PER_S_AT_COST_1, samples=samples)
