"""Security floor, noise model and parameter selector (tfhe_fbs_map_amd/params.py): the stand-in for the patched
concrete-optimizer the reference shells out to (experiments/add_exec_estimates.py:9-16, concrete.patch:21-27,163)."""
import math

import pytest

from tfhe_fbs_map_amd import MODULUS_BITS, P1024, P2048, Params, bootstrap_cost, choose_params, margin_sigmas, params_for
from tfhe_fbs_map_amd._native import MODULUS
from tfhe_fbs_map_amd.params import REFERENCE_MARGIN, p_error, security_bits, sigma_min, variances
from tfhe_fbs_map_amd.security import log2_sigma_min


def test_security_floor_table():
    assert MODULUS == (1 << 46) - 62 * (1 << 13) + 1 and MODULUS_BITS == 46
    # the 128-bit line, log2(sigma/q) per dimension (provenance in params.py) ...
    for dim, want in ((500, -10.3), (630, -13.8), (742, -16.8), (800, -18.3), (1024, -24.3)):
        assert abs(log2_sigma_min(dim) - want) < 0.06, dim
    # ... and its floor: nothing below 2^2 in absolute units of a 46-bit modulus
    assert log2_sigma_min(2048) == -44.0 and sigma_min(2048) == 4
    assert abs(math.log2(sigma_min(630)) - (46 - 13.78)) < 0.05
    # published TFHE-rs 128-bit sets sit just below this line (it is the more conservative): n = 742 -> 2^-17.1
    assert -17.1 < log2_sigma_min(742) < -16.5


def test_default_params_are_secure_and_the_benchmark_set_says_it_is_not():
    d = Params()
    assert d.sigma_lwe == sigma_min(630) and d.sigma_glwe == sigma_min(1024) and security_bits(d) >= 127.9
    assert P1024.sigma_lwe == 64 and (P1024.n, P1024.N, P1024.l_bsk, P1024.beta_bsk, P1024.t_ksk, P1024.gamma_ksk) == (630, 1024, 3, 7, 8, 2)
    assert security_bits(P1024) < 60                                         # reduced noise: a kernel benchmark shape
    # reduced noise: mul16@15 has norm2 84, aes_sbox@15 281 -- comfortably inside the box
    assert margin_sigmas(P1024.replace(p_msg=15), norm2=84) > 6
    assert margin_sigmas(P1024.replace(p_msg=15), norm2=281) > 5.5
    # the same shape at 128-bit noise cannot carry p = 15 (documented, not hidden); it carries p = 2
    assert margin_sigmas(d.replace(p_msg=15), norm2=1) < 2
    assert margin_sigmas(d.replace(p_msg=2), norm2=1) > 6
    # p = 31 does not fit N = 1024 (modulus switch alone) and is sent to N = 2048
    assert margin_sigmas(P1024.replace(p_msg=31), norm2=1) < 5.0           # (4.5 sigma even with the mean-compensated modulus switch)
    assert params_for(31).log_n_poly == 11 and params_for(15).log_n_poly == 10
    assert margin_sigmas(params_for(31), norm2=325) > 5


def test_bytes_per_fbs_is_baselines_figure():
    assert P1024.bytes_per_fbs() == 103_309_328


@pytest.mark.parametrize("p,norm2", [(15, 70), (15, 281), (4, 2), (2, 6), (9, 70)])
def test_selector_returns_secure_sets_with_the_asked_margin(p, norm2):
    """The reference's contract (concrete.patch:21-27,163): (precision, sq_norm2) -> n, N, gadget, key switch at a
    fixed security level and error probability."""
    c = choose_params(p, norm2)                         # 128 bits, 6 sigma
    assert c.p_msg == p and c.k == 1
    assert margin_sigmas(c, norm2) >= 6.0
    assert c.sigma_lwe >= sigma_min(c.n) and c.sigma_glwe >= sigma_min(c.N) and security_bits(c) >= 127.9
    # the kernels can run it (dev_supported in csrc/fbs_kernels.hip)
    assert 8 <= c.log_n_poly <= 12 and c.l_bsk * c.beta_bsk <= 30 and c.t_ksk * c.gamma_ksk <= 31
    assert MODULUS_BITS + c.gamma_ksk + math.log2(c.t_ksk * c.N) <= 63.9
    # a looser error probability is never dearer; a larger norm never cheaper
    assert bootstrap_cost(choose_params(p, norm2, min_margin=REFERENCE_MARGIN)) <= bootstrap_cost(c) + 1e-9
    assert bootstrap_cost(choose_params(p, norm2 * 4)) >= bootstrap_cost(c) - 1e-9


def test_selector_moves_n_and_N():
    small, big = choose_params(2, 1), choose_params(15, 281)
    assert small.N == 1024 and big.N == 2048 and big.n > small.n
    assert choose_params(15, 281).n != choose_params(15, 281, min_margin=4.0).n
    # p = 31 at norm2 = 325: with the mean-compensated modulus switch (variance (1 + n/4) roundings instead of (1 + n/2))
    # N = 2048 carries it at 6 sigma; without it the switch alone left 5.9 and the selector had to take N = 4096 at more than
    # twice the cost.  N = 1024 cannot.
    big = choose_params(31, 325)
    assert big.N == 2048 and margin_sigmas(big, 325) >= 6.0 and security_bits(big) >= 127.9
    with pytest.raises(ValueError):
        choose_params(31, 325, poly_sizes=(9, 10))
    # a margin relaxed towards the reference's own 4 sigma is never dearer
    c = choose_params(31, 325, floor_margin=REFERENCE_MARGIN, min_margin=REFERENCE_MARGIN)
    assert c.N == 2048 and margin_sigmas(c, 325) >= 4.0 and bootstrap_cost(c) <= bootstrap_cost(big)
    # p = 63 takes N = 4096; p = 127 is beyond it
    huge = choose_params(63, 100)
    assert huge.N == 4096 and margin_sigmas(huge, 100) >= 6.0 and bootstrap_cost(huge) > 2 * bootstrap_cost(big)
    with pytest.raises(ValueError):
        choose_params(127, 10)


def test_cost_ranking_against_the_references_points():
    """experiments/analyse_results.py:317,345-353 quotes the patched optimizer's cost per bootstrap: 40 at p = 4
    (Trivium/Kreyvium), 47 / 69 / 75 at precision 9 / 11 / 17 with sq_norm2 > 2.  Units differ (theirs counts FFT
    flops of a CPU library, ours FP64 issue slots of these kernels); the ORDER must agree."""
    ours = [bootstrap_cost(choose_params(p, n2, min_margin=REFERENCE_MARGIN)) for p, n2 in ((4, 3), (9, 3), (11, 3), (17, 3))]
    theirs = [40, 47, 69, 75]
    assert all(a <= b for a, b in zip(ours, ours[1:])), ours
    assert sorted(range(4), key=lambda i: ours[i]) == sorted(range(4), key=lambda i: theirs[i])
    assert 1.0 < ours[3] / ours[0] < theirs[3] / theirs[0] * 1.5
    assert abs(bootstrap_cost(P1024) - 1.0) < 1e-9 and bootstrap_cost(P2048) > 1.5


def test_two_key_bits_per_step_is_chosen_where_it_pays():
    """bsk_group = 2 halves the blind-rotation steps at 3x the key-noise term: the selector takes it for one-level gadgets at
    N = 2048 (measured 0.81 of the one-bit cost) and keeps one bit per step where more levels are needed."""
    a, b = choose_params(15, 70), choose_params(15, 70, groups=(1,))
    assert a.bsk_group == 2 and a.l_bsk == 1 and a.n % 2 == 0 and b.bsk_group == 1
    assert bootstrap_cost(a) < bootstrap_cost(b) and margin_sigmas(a, 70) >= 6.0
    va, vb = variances(a)[0], variances(a.replace(bsk_group=1))[0]
    assert 1.4 < va / vb < 3.1                                  # between the rounding term's 1.5x and the key term's 3x
    assert choose_params(2, 1).bsk_group == 1 and choose_params(4, 2).bsk_group == 1
    assert a.bytes_per_fbs() > b.replace(n=a.n).bytes_per_fbs()  # 1.5x the bootstrapping key


def test_reduced_noise_search_and_error_probability():
    """security=None: the same search at a fixed (benchmark) noise."""
    c = choose_params(15, 84, security=None)
    assert c.sigma_lwe == 64 and margin_sigmas(c, 84) >= 6.0 and bootstrap_cost(c) <= bootstrap_cost(P1024)
    noisy = choose_params(3, 20, security=None, sigma=1 << 21)
    assert margin_sigmas(noisy, 20) >= 6.0 and bootstrap_cost(noisy) > bootstrap_cost(choose_params(3, 20, security=None))
    assert 5e-5 < p_error(4.0) < 7e-5 and p_error(6.0) < 3e-9              # "4 sigma" = 6.3e-5 (concrete.patch:56)
    v_br, v_ks, v_ms = variances(P1024)
    assert v_ms > v_ks > 0 and v_br > 0


def test_exec_estimate_is_the_references_total_cost_in_this_executors_unit():
    """experiments/add_exec_estimates.py + analyse_results.py: boot_cost(precision, sq_norm2) x nb_bootstrap.  Here boot_cost is
    `bootstrap_cost` of the set the selector picks (P1024 = 1) and the time is that over the measured rate at cost 1."""
    from tfhe_fbs_map_amd.params import MI355X_FBS_PER_S_AT_COST_1, bootstrap_cost, choose_params, exec_estimate
    e = exec_estimate(15, 70, 482, samples=1000)
    assert e["params"] == choose_params(15, 70) and e["boot_cost"] == bootstrap_cost(e["params"])
    assert abs(e["total_cost"] - 482 * e["boot_cost"]) < 1e-9 and e["margin_sigmas"] >= 6.0
    assert abs(e["seconds"] - e["total_cost"] * 1000 / MI355X_FBS_PER_S_AT_COST_1) < 1e-12
    assert 3.0 < e["seconds"] < 7.0                              # the 16x16 multiplier on 1000 samples: 4.5 s measured at P1024
    # more plaintext bits per bootstrap cost more per bootstrap (the reference's 40 / 47 / 69 / 75 points have the same order)
    costs = [exec_estimate(p, 59, 1)["boot_cost"] for p in (4, 9, 17, 31)]
    assert costs == sorted(costs)


def test_glwe_dimension_three_at_n512_for_small_plaintext_moduli():
    """k N = 1536 is a noise floor between the two k = 1 offers: with k = 3 admitted (ExecConfig's default since the end of round 4) p <= 8
    at ordinary norms takes N = 512 with two key bits per step and one level (k_blind_rotate_glwe), at the margin and the security
    asked, cheaper by the kernel's MEASURED cost; p = 15 and heavy norms keep what they had; shapes without a kernel are never returned."""
    from tfhe_fbs_map_amd import ExecConfig
    from tfhe_fbs_map_amd.params import (DEFAULT_GLWE_DIMS, bootstrap_cost, choose_params, glwe_instructions, glwe_shape_built, margin_sigmas,
                                        security_bits)
    assert DEFAULT_GLWE_DIMS == (1, 2, 3) == ExecConfig(seed=1).glwe_dims
    for p, norm2 in ((2, 1), (3, 2), (4, 2), (4, 8), (7, 10), (8, 10)):
        a, b = choose_params(p, norm2, glwe_dims=(1, 2)), choose_params(p, norm2, glwe_dims=DEFAULT_GLWE_DIMS)
        assert (b.k, b.N, b.l_bsk, b.bsk_group) == (3, 512, 1, 2), (p, norm2, b)
        assert margin_sigmas(b, norm2) >= 6.0 and security_bits(b) >= 127.9 and bootstrap_cost(b) < (0.93 if a.N == 1024 else 1.0) * bootstrap_cost(a)
    assert choose_params(15, 70, glwe_dims=DEFAULT_GLWE_DIMS) == choose_params(15, 70, glwe_dims=(1, 2))
    assert choose_params(7, 59, glwe_dims=DEFAULT_GLWE_DIMS).k == 2 and choose_params(15, 281, glwe_dims=DEFAULT_GLWE_DIMS).k == 1
    assert choose_params(31, 325, glwe_dims=DEFAULT_GLWE_DIMS) == choose_params(31, 325)
    for k in (2, 3, 4, 5):
        for log_n in (8, 9, 10, 11):
            assert glwe_shape_built(log_n, k) == ((k <= 4 and log_n <= 9) or (k <= 3 and log_n == 10))
    for dims in ((1, 2, 3, 4, 5), (4, 5)):
        for p, norm2 in ((2, 1), (4, 2)):
            s = choose_params(p, norm2, glwe_dims=dims, poly_sizes=(8, 9, 10, 11, 12))
            assert s.k == 1 or glwe_shape_built(s.log_n_poly, s.k)
    prm = choose_params(4, 2, glwe_dims=DEFAULT_GLWE_DIMS)
    assert abs(glwe_instructions(prm) - 307 * 512 * 4 * (2 * 4.0 * 9 + 7.0 * 4 * 4 + 2 + 12) / 64.0) < 1e-6


def test_glwe_dimension_two_is_an_option_not_the_default():
    """k = 2 (N = 1024, two key bits per step, one level: what k_blind_rotate_pairs_k2 is built for) is returned only when asked
    for, where it is cheaper and reaches the margin; ExecConfig asks for it for every program (since the twelve-wave latency
    shape it is ahead at every launch size), unless told to stay on k = 1."""
    from tfhe_fbs_map_amd import ExecConfig
    from tfhe_fbs_map_amd.params import bootstrap_cost, choose_params, margin_sigmas, security_bits
    a, b = choose_params(15, 70), choose_params(15, 70, glwe_dims=(1, 2))
    assert a.k == 1 and b.k == 2 and (b.N, b.l_bsk, b.bsk_group) == (1024, 1, 2)
    assert bootstrap_cost(b) < 0.85 * bootstrap_cost(a) and margin_sigmas(b, 70) >= 6.0 and security_bits(b) >= 127.9
    assert choose_params(31, 325, glwe_dims=(1, 2)).k == 1          # p = 31 does not fit 2N = 2048 slots at 6 sigma
    assert choose_params(15, 70, glwe_dims=(1, 2), groups=(1,)).k == 1
    cfg = ExecConfig(seed=1)
    assert cfg.params_choice(15, 70).k == 2 and cfg.params_choice(15, 70, glwe_dims=(1,)).k == 1
    assert ExecConfig(seed=1, glwe_dims=(1,)).params_choice(15, 70).k == 1
