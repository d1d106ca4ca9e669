"""The inputs and references of tests/test_gpu_compact_wide.py, checked without a GPU: compact ciphertexts at n = 64, 65, 734 and 4096
(helpers.COMPACT_WIDE_SETS), with the key-switching key planted so that the switched ciphertexts are chosen words.

* planted_switch through the C oracle's key switch gives exactly the target words, at every set and width;
* the target rows reach the extremes they are named for, evaluated on Python integers: eps / n = -2^(sh-1) for `half` and
  2^(sh-1) - 1 for `below`, an odd negative eps for `odd`, |eps >> 1| >= q at n = 4096 and 9 bits, and more than 256 packed words
  (a second round of k_compact_pack) at n = 734 from 23 bits on and at n = 4096 at every width; the bodies put
  x_n - floor(eps / 2) on a rounding boundary, one either side, on 0 and on q - 1;
* the numpy restatements the GPU tests compare with (round_fields, pack, unpack of tests/test_gpu_compact.py, reround of
  tests/test_gpu_chain.py) equal the definitions on Python integers (tests/helpers.py) on all of these inputs;
* the decode cases wrap the 32-bit sum of the set mask fields 178 times at n = 734 and 1022 times at n = 4096 (31 bits, every mask
  field 2^31 - 1), put the phase on every boundary between two messages for p = 7 and p = 4096, and the client library's host decode
  equals decode_definition on every one of them."""
import os
import subprocess

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (COMPACT_PACK_WIDTHS, COMPACT_WIDE_SETS, Q, compact_definition, compact_target_rows, decode_boundary_phases,
                           decode_case_batches, decode_cases, decode_phase, pack_definition, planted_switch,
                           reround_definition, reround_field_rows, rounding_eps, unpack_definition)
from tests.test_gpu_chain import reround
from tests.test_gpu_compact import pack, round_fields, unpack
from tests.test_gpu_compact_wide import decode_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
B = 9                                                # log2(2N) of every set
UNPACK_WIDTHS = (10, 23, 31)
DECODE_WIDTHS = (9, 23, 31)
DECODE_P = (7, 4096)
SEED = 11
_MADE = {}


def made(name):
    """(parameter dict, keyed oracle, its keys) of a set, made once"""
    if name not in _MADE:
        prm = COMPACT_WIDE_SETS[name]
        o = orc.Oracle(prm, seed=SEED)
        _MADE[name] = (prm, o, o.keys())
    return _MADE[name]


def as_u64(rows):
    return np.array([[int(v) for v in r] for r in rows], dtype=np.uint64)


def switched_rows(n, bits):
    """the planted small-key ciphertexts of a width: every target row with every one of its bodies"""
    return [row + [body] for row, bodies in compact_target_rows(n, bits).values() for body in bodies]


@pytest.fixture(scope="module")
def client_library():
    subprocess.check_call(["make", "-s", "-C", CSRC, "client"], timeout=600)


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_planted_switch_gives_the_targets_through_the_oracle(name):
    prm, o, keys = made(name)
    n = prm["n"]
    try:
        for bits in COMPACT_PACK_WIDTHS:
            rows = compact_target_rows(n, bits)
            planted, cts = planted_switch(keys, prm, [r for r, _ in rows.values()], [b for _, b in rows.values()], oracle=o)
            want = switched_rows(n, bits)                  # (planted_switch has asserted it; once more, from outside)
            assert cts.shape == (len(want), (prm["k"] << prm["log_n_poly"]) + 1) and 32 <= len(want) <= 64
            assert np.array_equal(np.stack([o.keyswitch(c) for c in cts]), as_u64(want)), (name, bits)
            # every planted key row decrypts to sk_glwe[j] h_0 exactly, and the rest of the key is untouched
            ksk = planted["ksk"].reshape(-1, n + 1)
            assert np.array_equal(ksk[len(rows):], keys["ksk"].reshape(-1, n + 1)[len(rows):])
            h0 = (Q + 128) >> 8
            for j in range(len(rows)):
                phase = (int(ksk[j, n]) - sum(int(m) for m, s in zip(ksk[j, :n], keys["sk_lwe"]) if s)) % Q
                assert phase == (h0 if keys["sk_glwe"][j] else 0)
    finally:
        o.set_keys(**keys)


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_the_target_rows_reach_their_extremes(name):
    n = COMPACT_WIDE_SETS[name]["n"]
    for bits in COMPACT_PACK_WIDTHS:
        sh = 46 - bits
        rows = compact_target_rows(n, bits)
        assert list(rows) == ["half", "below", "qm1", "odd", "alt", "rand"]
        eps = {k: rounding_eps(r, 46, bits) for k, (r, _) in rows.items()}
        assert all(0 <= x < Q for r, _ in rows.values() for x in r)
        assert eps["half"] == -n << (sh - 1) and eps["below"] == n * ((1 << (sh - 1)) - 1)
        assert abs(eps["half"] / n + (1 << (sh - 1))) <= 1 and abs(eps["below"] / n - (1 << (sh - 1))) <= 1
        assert eps["odd"] < 0 and eps["odd"] % 2 == 1 and eps["odd"] // 2 != int(eps["odd"] / 2)   # floor and truncation differ
        assert eps["alt"] == -((n + 1) // 2 << (sh - 1)) + n // 2 * ((1 << (sh - 1)) - 1)
        fields = compact_definition(rows["qm1"][0] + [0], bits)[:n]
        assert len(set(fields)) == 1 and (fields[0] == 0 if bits <= 27 else fields[0] >= (1 << bits) - 16)   # q - 1 rounds up to 2^bits
        up, down = (compact_definition(rows[k][0] + [0], bits)[:n] for k in ("half", "below"))
        assert all(u == (d + 1) % (1 << bits) for u, d in zip(up, down))      # one rounds up where the other rounds down
        if (n, bits) == (4096, 9):
            assert abs(eps["half"] >> 1) >= Q
        for kind, (row, bodies) in rows.items():
            ys = [(body - eps[kind] // 2) % Q for body in bodies]
            assert len(bodies) == 10 and bodies[8:] == [0, Q - 1] and ys[6:8] == [0, Q - 1]
            hb = 1 << (sh - 1)
            for down, up, after in (ys[0:3], ys[3:6]):                        # either side of a boundary, and the boundary
                assert down + 1 == up == after - 1 and up % (1 << sh) == hb
                got = [compact_definition(row + [(y + eps[kind] // 2) % Q], bits)[n] for y in (down, up, after)]
                assert got[1] == got[2] == (got[0] + 1) % (1 << bits)
            assert ys[5] + (1 << sh) >= Q                                      # the highest step q has
        W = len(pack_definition([0] * (n + 1), bits))
        assert (W > 256) == ((n == 734 and bits >= 23) or n == 4096), (n, bits, W)   # two rounds of k_compact_pack or more


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_the_restatements_are_the_definitions(name):
    n = COMPACT_WIDE_SETS[name]["n"]
    for bits in COMPACT_PACK_WIDTHS:
        x = switched_rows(n, bits)
        want = [compact_definition(r, bits) for r in x]
        got = round_fields(as_u64(x), bits)
        assert np.array_equal(got, as_u64(want)), (name, bits)
        words = pack(got, bits)
        assert np.array_equal(words, as_u64([pack_definition(f, bits) for f in want])), (name, bits)
        assert np.array_equal(unpack(words, n, bits), as_u64([unpack_definition(w, n + 1, bits) for w in words])), (name, bits)
        assert np.array_equal(unpack(words, n, bits), got)
    for bits in (B,) + UNPACK_WIDTHS:
        kinds = reround_field_rows(n, bits, B)
        assert list(kinds) == (["top", "rand", "zero"] if bits == B else ["half", "below", "top", "odd", "alt", "rand"])
        rows = [r for group in kinds.values() for r in group]
        assert all(0 <= f < 1 << bits for r in rows for f in r)
        want = [reround_definition(r, bits, B) for r in rows]
        assert np.array_equal(reround(as_u64(rows), n, bits, B), as_u64(want)), (name, bits)
        assert np.array_equal(unpack(pack(as_u64(rows), bits), n, bits), as_u64(rows)), (name, bits)
        if bits == B:
            assert want == rows
            continue
        sh = bits - B
        eps = {k: rounding_eps(group[0][:n], bits, B) for k, group in kinds.items()}
        assert eps["half"] == -n << (sh - 1) and eps["below"] == n * ((1 << (sh - 1)) - 1)
        assert eps["odd"] < 0 and eps["odd"] % 2 == 1
        assert kinds["top"][0][:n] == [(1 << bits) - 1] * n and {r[n] for r in kinds["top"]} >= {0, (1 << bits) - 1}
        for kind, group in kinds.items():                                     # the bodies: a boundary, one either side, 0 and 2^bits - 1
            ys = [(r[n] - eps[kind] // 2) % (1 << bits) for r in group]
            assert ys[1] % (1 << sh) == ys[4] % (1 << sh) == 1 << (sh - 1) and ys[0] + 1 == ys[1] == ys[2] - 1
            assert ys[6:8] == [0, (1 << bits) - 1] and [r[n] for r in group[8:]] == [0, (1 << bits) - 1]
            out = [reround_definition(r, bits, B)[n] for r in group[:3]]
            assert out[1] == out[2] == (out[0] + 1) % (1 << B)


def test_decode_boundaries_are_boundaries():
    for bits in DECODE_WIDTHS:
        for p in DECODE_P:
            phases = decode_boundary_phases(bits, 2 * p)
            have = set(phases)
            assert len(phases) == len(have) and all(0 <= ph < 1 << bits for ph in phases)
            if (1 << bits) < 2 * p:                                          # more messages than phases: every phase is a case
                assert sorted(phases) == list(range(1 << bits))
                continue
            for j in range(2 * p):                                           # the last phase of message j and the first of j + 1
                num, den = (2 * j + 1) << bits, 4 * p
                last, first = (num - 1) // den, -(-num // den)
                assert {last, first, first + 1 if num % den == 0 else last} <= have or first == 1 << bits
                assert decode_phase(last, 0, bits, 2 * p) == j and decode_phase(first, 0, bits, 2 * p) == (j + 1) % (2 * p)


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_host_decode_is_the_definition(name, client_library):
    from tfhe_fbs_map_amd import HostContext, Params
    prm = COMPACT_WIDE_SETS[name]
    n = prm["n"]
    for p in DECODE_P:
        ctx = HostContext(Params(**{**prm, "p_msg": p}), seed=SEED, keygen=True)
        sk = [int(s) for s in ctx.export_keys()["sk_lwe"]]
        assert sk == [int(s) for s in made(name)[2]["sk_lwe"]]              # (the oracle's key of this seed)
        for bits in DECODE_WIDTHS:
            cases = decode_cases(n, sk, bits, 2 * p)
            if bits == 31:                                                   # set (a): the 32-bit sum wraps, many times
                wraps = sum(f for f, s in zip(cases["ones"][0], sk) if s) >> 32
                assert wraps == {64: 15, 65: 15, 734: 178, 4096: 1022}[n]
            total = 0
            for kind, words, want in decode_case_batches(cases, sk, bits, 2 * p, pack):
                got = ctx.decrypt_compact(words, bits)
                if kind == "random":                                         # the numpy decode the GPU test uses for 262 149 rows
                    assert np.array_equal(decode_fields(unpack(words, n, bits), sk, bits, 2 * p), want)
                assert np.array_equal(got, want), (name, p, bits, kind)
                total += len(want)
            assert total == 2 * len(decode_boundary_phases(bits, 2 * p)) + 64
        ctx.close()
