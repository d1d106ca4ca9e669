"""The inputs of tests/test_gpu_level_arithmetic.py, checked without a GPU: the kernels that run between bootstraps (k_lincomb,
k_multi_extract, csrc/fbs_kernels.hip) are exact on the strength of a bound each, and the inputs planted in tests/helpers.py are
meant to sit at those bounds.  Here

* the C oracle's linear combination is the definition on Python integers for every planted case -- coefficients and constants at
  the ends of int64, multiples of q, both halves of the field -- and so is its cut of a table out of a shared rotation: the
  reference of the GPU tests is anchored before a GPU is involved;
* a replay of k_lincomb's lazy FP64 accumulation on the exact-integer model of the FP64 unit (helpers.fp_mulmod, fp_center) gives
  the definition, every intermediate an integer below 2^52, AND the planted columns of every output of 16 terms or more drive the
  accumulator to 7.5 q or beyond at either sign (16 products of one sign just inside q/2 between two centrings; 12.5 q is what
  the kernel's own bound of 0.75 q a product would allow);
* a statement-by-statement replay of k_multi_extract's int64 sum gives the definition too, and on an accumulator of q - 1 throughout
  the tables whose difference polynomial has sum |d| = 65534 -- the most a table the loader fuses can have -- take that sum to
  exactly +-65534 (q - 1), 2^61.99 of the 2^63 it has.

What the replay says about the centring cadence (the figures are asserted below): between 16 and 100 terms the accumulator peaks
at 7.77 q to 8.84 q; 15 terms stay below 7.5 q.  Sums of integers are exact in a double up to 2^53 = 128 q, so a cadence of 32 gives
the same words as the kernel's 16 on every input (32 products below 1.24 q each and a centred start: under 41 q), and so does no
centring at all up to 100 such terms; the output of 400 terms is there for that: without centring it runs to 196 q."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (EX_ABS_SUM, EX_P, EX_TABLES, HALF, INT64_MAX, INT64_MIN, LC_CONSTS, LC_NONZERO, LC_OUTPUTS, LC_SHAPES,
                           LC_SLOTS, LC_TARGET, LC_ZERO, Q, extract_definition, extract_kernel_sums, lc_coefs, lc_columns,
                           lc_definition, lc_delta, lc_replay, lc_terms, planted_accumulators, planted_lincomb, table_diff)

SIGNS = (1, -1)


def oracle_of(k, log_n):
    """an oracle of the shape, without keys: the linear combination and the extraction take none"""
    return orc.Oracle(dict(n=8, log_n_poly=log_n, k=k, l_bsk=3, beta_bsk=10, t_ksk=8, gamma_ksk=2, p_msg=EX_P, sigma_lwe=1 << 8,
                           sigma_glwe=4, bsk_group=1), keygen=False)


def test_the_planted_cases_are_the_ones_the_kernel_is_to_meet():
    coefs = lc_coefs(LC_SLOTS)
    assert set(LC_NONZERO + LC_ZERO) <= set(coefs) and len(set(coefs)) > len(LC_NONZERO + LC_ZERO)        # ... and random int64
    assert {1, -1, 3, -3, HALF, -HALF, HALF + 1, Q - 1, Q, -Q, -2 * Q, 1 << 40, -(1 << 45), INT64_MAX, INT64_MIN} <= set(coefs)
    assert all(c % Q for c in coefs[:32]) and all(INT64_MIN <= c <= INT64_MAX for c in coefs)
    assert any(abs(c) >= Q // 2 for c in coefs)                              # (needs the loader's reduction)
    assert [n for _, n, _ in LC_OUTPUTS] == [0, 1, 15, 16, 17, 31, 32, 33, 48, 100, 400]
    assert {c for _, _, c in LC_OUTPUTS} == set(LC_CONSTS) == {0, 1, -1, 2 * EX_P - 1, Q, -Q, INT64_MAX, INT64_MIN}
    assert all(first == 0 for first, n, _ in LC_OUTPUTS if n >= 16)          # they open with sixteen products that are not 0
    zero_slots = {i for i, c in enumerate(coefs) if c % Q == 0}
    assert zero_slots and any(zero_slots & set(lc_terms(first, n)) for first, n, _ in LC_OUTPUTS if n < 16)
    assert lc_delta(EX_P) == 2 * oracle_of(1, 8).delta_half
    assert [k * (1 << ln) + 1 for k, ln in LC_SHAPES] == [257, 513, 1025, 1537, 2049, 4097]
    words, _ = planted_lincomb(257, LC_SLOTS, 1, 0)
    assert words.max() < Q and {0, Q - 1, HALF, HALF + 1} <= set(words[:, 1:255].ravel().tolist())
    for sign in SIGNS:
        words, _ = planted_lincomb(257, LC_SLOTS, sign, 3)
        for i, c in enumerate(coefs):
            for j in lc_columns(257):
                assert c % Q == 0 or c * int(words[i, j]) % Q == sign * (LC_TARGET - i) % Q


@pytest.mark.parametrize("k,log_n", LC_SHAPES)
def test_the_oracle_lincomb_is_the_definition_on_every_planted_case(k, log_n):
    o = oracle_of(k, log_n)
    ctw = o.ctw
    ones = np.ones(ctw, np.uint64)
    for c in lc_coefs(LC_SLOTS) + LC_CONSTS:                                 # one term, one constant: canonical whatever the int64
        got = o.lincomb([ones], [c], c)
        assert int(got[0]) == c % Q and int(got[-1]) == (c + c * lc_delta()) % Q
    assert not o.lincomb([], [], 0).any()
    for sign in SIGNS:
        words, coefs = planted_lincomb(ctw, LC_SLOTS, sign, seed=k)
        for first, n, const in LC_OUTPUTS:
            terms = lc_terms(first, n)
            got = o.lincomb([words[t] for t in terms], [coefs[t] for t in terms], const)
            want = lc_definition(words, coefs, terms, const)
            assert got.max() < Q and np.array_equal(got, np.array(want, dtype=np.uint64)), (sign, n)


@pytest.mark.parametrize("k,log_n", LC_SHAPES)
def test_the_replay_of_k_lincomb_is_the_definition_and_peaks_at_7_5_q(k, log_n):
    ctw = k * (1 << log_n) + 1
    peaks = {}
    for sign in SIGNS:
        words, coefs = planted_lincomb(ctw, LC_SLOTS, sign, seed=k)
        for first, n, const in LC_OUTPUTS:
            terms = lc_terms(first, n)
            want = lc_definition(words, coefs, terms, const)
            for j in lc_columns(ctw) + [1, 254, 257 % ctw, ctw - 3]:         # the planted columns, then ordinary ones
                got, peak = lc_replay(words, coefs, terms, const, j)
                assert got == want[j], (sign, n, j)
                if j in lc_columns(ctw):
                    peaks.setdefault(n, []).append(peak / Q)
                    if n >= 16:                                              # THE CONDITION ON THE INPUTS (not a measurement)
                        assert peak >= 7.5 * Q, (sign, n, j, peak / Q)
                    if 16 <= n <= 100:                                       # a cadence of 32, or none, gives the same word here
                        assert lc_replay(words, coefs, terms, const, j, every=32)[0] == got
                        assert lc_replay(words, coefs, terms, const, j, every=0)[0] == got
    print({n: "%.2f..%.2f" % (min(v), max(v)) for n, v in peaks.items()})
    assert max(peaks[15]) < 7.5 and max(max(v) for v in peaks.values()) < 12.5
    # ... and 400 terms do not survive a centring that is never done: the sum leaves the integers a double holds
    words, coefs = planted_lincomb(ctw, LC_SLOTS, 1, seed=k)
    with pytest.raises(AssertionError):
        lc_replay(words, coefs, lc_terms(0, 400), 1, 0, every=0)


# ---- tables cut out of a shared rotation --------------------------------------------------------------------------------------
def sparse(diff):
    """the (positions, values) the loader uploads"""
    pos = [i for i, d in enumerate(diff) if d]
    return pos, [diff[i] for i in pos]


@pytest.mark.parametrize("N", [256, 512, 1024])
def test_difference_polynomials_have_the_sums_stated(N):
    o = oracle_of(1, N.bit_length() - 1)
    for name, table in EX_TABLES.items():
        diff, post = o.build_tv_diff(table)
        mine, c = table_diff(table, N)
        assert [int(d) for d in diff] == mine and post == c * o.delta_half % Q, name
        assert sum(abs(d) for d in mine) == EX_ABS_SUM[name], name
        assert len(sparse(mine)[0]) <= EX_P + 1 and mine[0] == 0             # (no table puts a value at position 0)
    assert EX_ABS_SUM["at_limit_a"] == EX_ABS_SUM["at_limit_b"] == (1 << 16) - 2
    assert EX_ABS_SUM["over_limit_a"] == EX_ABS_SUM["over_limit_b"] == 1 << 16
    # the total variation round the negacyclic circle is even: no evaluable table sits at 65535
    for table in ([0, 32767, 1], [5, -32760, 3, 1], [0, 1, 0, 1, 0, 1, 32764]):
        assert sum(abs(d) for d in table_diff(table, N)[0]) % 2 == 0


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_oracle_extraction_and_the_replay_of_k_multi_extract_are_the_definition(k):
    N = 256
    o = oracle_of(k, 8)
    rows = planted_accumulators(k, N, seed=k)
    rows.update({"one polynomial'": planted_accumulators(k, N, seed=k + 1)["one polynomial"]})
    diffs = {name: table_diff(t, N) for name, t in EX_TABLES.items()}
    # by hand: values at position 0 and at the largest one (no table has them; the kernel's index arithmetic does not know that)
    edge = [0] * N
    edge[0], edge[1], edge[N - 1] = 32767, -3, -32764
    diffs["positions 0 and N-1"] = (edge, 0)
    branches = set()
    for tname, (diff, c) in diffs.items():
        post = c * o.delta_half % Q
        pos, val = sparse(diff)
        for rname, acc in rows.items():
            want = extract_definition(acc, diff, post, k, N)
            got = o.multi_extract(acc, np.array(diff, np.int32), post)
            assert got.max() < Q and [int(x) for x in got] == want, (tname, rname)
            sums = extract_kernel_sums(acc, pos, val, k, N)
            sums[-1] += post
            assert [s % Q for s in sums] == want, (tname, rname)
        for j in (0, 1, N - 1, k * N - 1, k * N):                            # the paths the restatement took
            jj = j % N
            m = 0 if jj == 0 else N - jj
            branches |= {("m >= pos" if m >= at else "m < pos", "pos 0" if at == 0 else "pos N-1" if at == N - 1 else "pos",
                          "jj 0" if jj == 0 else "jj", "body" if j == k * N else "mask") for at in pos}
    assert {b[0] for b in branches} == {"m >= pos", "m < pos"} and {b[1] for b in branches} == {"pos", "pos 0", "pos N-1"}
    assert {b[2:] for b in branches} == {("jj 0", "mask"), ("jj", "mask"), ("jj 0", "body")}
    assert ("m >= pos", "pos 0", "jj 0", "body") in branches and ("m < pos", "pos N-1", "jj 0", "mask") in branches


@pytest.mark.parametrize("k", [1, 2, 3])
def test_tables_at_the_limit_take_the_int64_sum_to_65534_q_minus_1(k):
    N = 256
    full = planted_accumulators(k, N)["all q-1"]
    for name in ("at_limit_a", "at_limit_b"):
        pos, val = sparse(table_diff(EX_TABLES[name], N)[0])
        sums = extract_kernel_sums(full, pos, val, k, N)
        assert max(sums) == 65534 * (Q - 1) or min(sums) == -65534 * (Q - 1), name
        assert max(abs(s) for s in sums) == 65534 * (Q - 1) < 1 << 62
        assert sum(abs(s) == 65534 * (Q - 1) for s in sums[:k * N]) >= k * (N // EX_P - 1)        # (every word under the large entry)
    # ... and one step over the limit is still inside an int64 -- the limit is the loader's round figure, not the edge of the type
    pos, val = sparse(table_diff(EX_TABLES["over_limit_b"], N)[0])
    assert max(abs(s) for s in extract_kernel_sums(full, pos, val, k, N)) == 65536 * (Q - 1)
