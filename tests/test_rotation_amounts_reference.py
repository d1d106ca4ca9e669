"""The planted rotation amounts of tests/test_gpu_rotation_amounts.py, checked without a GPU: the lists are what their description
says (tests/helpers.py, planted_amount_rows), and the REFERENCE is right on them -- every semantic row, rotated through the identity
table by the CPU oracle and extracted, decrypts to its message.  One parameter set per family of kernels: one key bit per step
(k = 1, N = 1024) and two (k = 1 at N = 2048; k = 2, 3 and 4 at N = 1024, 512 and 256)."""
import re

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (PLANTED_FAMILIES, PLANTED_MARGIN, PLANTED_P, PLANTED_ROWS, PLANTED_STEPS, pack_definition, planted_amount_rows,
                           planted_edges, planted_mask_lists, planted_output_margin, planted_set, recipe, reround_definition, step_properties,
                           unpack_definition)

PAIR_PROPERTIES = {"e2 == 0, parts non-zero", "e2 == N", "wrapped sum", "one part zero", "odd", "even", "e == N"}


def steps_of(row, n, group):
    return [tuple(int(a) for a in row[i:i + group]) for i in range(0, n, group)]


def properties_of(steps, N):
    """the properties a list hits, written out here a second time (not through tests/helpers.py:step_properties, which made `meta`)"""
    M, out = 2 * N, set()
    exponents = [s[0] for s in steps] if len(steps[0]) == 1 else [e for a, b in steps for e in (a, b, (a + b) % M)]
    out |= {"odd" for e in exponents if e % 2 == 1} | {"even" for e in exponents if e and e % 2 == 0} | {"e == N" for e in exponents if e == N}
    if len(steps[0]) == 2:
        out |= {"e2 == 0, parts non-zero" for a, b in steps if a > 0 and b > 0 and (a + b) % M == 0}
        out |= {"e2 == N" for a, b in steps if (a + b) % M == N}
        out |= {"wrapped sum" for a, b in steps if a + b > M}
        out |= {"one part zero" for a, b in steps if (a == 0) + (b == 0) == 1}
    return out


@pytest.mark.parametrize("family", sorted(PLANTED_FAMILIES))
def test_the_lists_are_what_their_description_says(family):
    shape = PLANTED_FAMILIES[family]
    N, group, n = 1 << shape["log_n_poly"], shape["bsk_group"], PLANTED_STEPS
    sk = np.arange(n) % 2
    fields, meta = planted_amount_rows(N, n, group, sk, PLANTED_P)
    assert fields.shape == (PLANTED_ROWS, n + 1) and fields.dtype == np.uint32 and int(fields.max()) < 2 * N   # legal fields, all
    n_steps = n // group
    want_skipped = [list(range(0, n_steps, 2)), list(range(1, n_steps, 2)), [i for i in range(n_steps) if i != n_steps // 2], [], []]
    seen, hits = set(), set()
    for j in range(PLANTED_ROWS):
        steps = steps_of(fields[j], n, group)
        skipped = [i for i, s in enumerate(steps) if not any(s)]                # (recomputed from the fields, not from meta)
        assert skipped == want_skipped[j % 5] == meta["lists"][j % 5]["skipped"], j
        assert list(fields[j, :n]) == meta["lists"][j % 5]["amounts"], j
        mine = properties_of(steps, N)
        assert mine == meta["lists"][j % 5]["hits"] == set().union(*(step_properties(s, N) for s in steps)), j
        hits |= mine
        seen |= {s for s in steps if any(s)}
    assert want_skipped[0][0] == 0 and want_skipped[1][-1] == n_steps - 1       # L0 skips the first step, L1 the last
    edges = planted_edges(N, group)
    assert seen == ({(e,) for e in edges} if group == 1 else set(edges))         # every edge runs, nothing else does
    assert len(set(edges)) == len(edges) == (12 if group == 1 else 15)
    assert hits == (PAIR_PROPERTIES if group == 2 else {"odd", "even", "e == N"})
    if group == 2:   # the interleaved lists themselves meet a zero bundle exponent, e = N and a zero part, not only L3 and L4
        interleaved = meta["lists"][0]["hits"] | meta["lists"][1]["hits"]
        assert {"e2 == 0, parts non-zero", "e == N", "one part zero"} <= interleaved
    # bodies: 7 messages on every list, then the raw ones
    assert meta["msg"] == [j // 5 if j // 5 < PLANTED_P else -1 for j in range(PLANTED_ROWS)]
    assert [int(fields[j, n]) for j in range(35, PLANTED_ROWS, 5)] == [0, 1, N - 1, N, 2 * N - 1]
    # fewer steps (what a slow shape may shrink to): twelve still cover the edge set; the lists never shrink
    short = planted_mask_lists(N, 12, group)
    assert {s for lst in short for s in steps_of(lst, 12, group) if any(s)} == ({(e,) for e in edges} if group == 1 else set(edges))


@pytest.mark.parametrize("family", sorted(PLANTED_FAMILIES))
def test_packing_at_the_rotations_width_keeps_every_field(family):
    """what the GPU test hands to fbs_refresh_compact_dev: `pack` (the numpy restatement, tests/test_gpu_compact.py) of the planted
    rows at log2(2N) bits is the format's definition on Python integers, and unpacks to the same fields; at that width the unpack
    re-rounds nothing"""
    from tests.test_gpu_compact import pack
    shape = PLANTED_FAMILIES[family]
    N, n, b = 1 << shape["log_n_poly"], PLANTED_STEPS, shape["log_n_poly"] + 1
    fields, _ = planted_amount_rows(N, n, shape["bsk_group"], np.ones(n, np.int64), PLANTED_P)
    words = pack(fields.astype(np.uint64), b)
    for row, w in zip(fields, words):
        assert [int(x) for x in w] == pack_definition(row, b)
        assert unpack_definition(w, n + 1, b) == [int(f) for f in row] == reround_definition(row, b, b)


def test_the_semantic_body_is_the_phase_it_claims():
    """m_n - <mask, s> is round(msg N / p) + off, off within two of the edge of the message's slot on either side and in its middle"""
    N, n, p = 512, PLANTED_STEPS, PLANTED_P
    sk = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1])
    offs = set()
    for turn in range(3):
        fields, meta = planted_amount_rows(N, n, 2, sk, p, turn)
        for j, msg in enumerate(meta["msg"]):
            if msg < 0:
                continue
            phase = (int(fields[j, n]) - int((fields[j, :n].astype(np.int64) * sk).sum())) % (2 * N)
            off = (phase - (2 * msg * N + p) // (2 * p) + N) % (2 * N) - N
            assert off in (0, N // (2 * p) - 2, -(N // (2 * p) - 2)) and 2 * p * abs(off) + p < N, (j, off)   # inside the slot
            offs.add((j, off))
    assert len(offs) == 3 * 35                                                   # every semantic row at every off


@pytest.mark.parametrize("family", sorted(PLANTED_FAMILIES))
def test_the_reference_decrypts_every_semantic_row(family):
    prm = planted_set(**PLANTED_FAMILIES[family])
    o = orc.Oracle(prm, seed=33)
    N, n, p = o.N, prm["n"], prm["p_msg"]
    tv, post = o.build_tv(list(range(p)))
    sk = o.keys()["sk_lwe"]
    cases = 0
    for turn in range(3):                                                        # 35 semantic rows x 3 offs = 105 cases
        fields, meta = planted_amount_rows(N, n, prm["bsk_group"], sk, p, turn)
        for j, msg in enumerate(meta["msg"]):
            if msg < 0 and turn:
                continue
            out = o.sample_extract(o.blind_rotate(fields[j], tv), post)
            assert int(out.max()) < orc.Q
            if msg >= 0:
                assert int(o.decrypt(out)) == msg, (family, turn, j)
                cases += 1
    assert cases == 105


def test_the_semantic_assertion_runs_on_every_family_of_kernels():
    """tests/test_gpu_rotation_amounts.py asserts `decrypt == msg` where the recipe's parameter set is a usable one: at least six
    standard deviations between a bootstrap output and the edge of its box, by the noise model (params.variances).  The recipes that
    are not: the six instantiations k_blind_rotate_cu<L,1,1> and <L,1,2> (lean ones included), whose template arguments themselves
    mean ONE gadget level of at most 9 and at most 7 bits (FIRST, csrc/fbs_select.cpp) -- 0.2 to 1 sigma at N = 1024 and 2048, with
    any gadget that reaches them.  Every other recipe has more than 12 (k_blind_rotate_cu<L,1,0> takes any beta > 9: its recipe has 20
    bits).  Every family of kernels keeps entries with the assertion; and at the worst of the six the REFERENCE decrypts wrongly."""
    from tfhe_fbs_map_amd import _native
    names = [k for k in _native.kernel_catalog() if k.startswith("k_blind_rotate")]
    margin = {}
    for k in names:
        rec = recipe(k)
        margin[k] = planted_output_margin(planted_set(rec["log_n"], rec.get("k", 1), rec["l"], rec["beta"], rec["group"]))
    unusable = {k for k in names if margin[k] < PLANTED_MARGIN}
    forced = {k for k in names if re.fullmatch(r"k_blind_rotate_cu<\d+,1,[12](,lean)?>", k)}
    assert unusable == forced and len(unusable) == 6
    assert all(recipe(k)["l"] == 1 and recipe(k)["beta"] == (9 if ",1,1" in k else 7) for k in unusable)   # the most bits FIRST admits
    assert max(margin[k] for k in unusable) < 1.5 and min(margin[k] for k in names if k not in unusable) > 12
    assert {k.split("<")[0] for k in names if k not in unusable} == {k.split("<")[0] for k in names}
    rec = recipe("k_blind_rotate_cu<10,1,2>")
    prm = planted_set(rec["log_n"], 1, rec["l"], rec["beta"], rec["group"])
    o = orc.Oracle(prm, seed=33)
    tv, post = o.build_tv(list(range(PLANTED_P)))
    fields, meta = planted_amount_rows(o.N, prm["n"], 1, o.keys()["sk_lwe"], PLANTED_P)
    wrong = sum(int(o.decrypt(o.sample_extract(o.blind_rotate(fields[j], tv), post))) != m for j, m in enumerate(meta["msg"]) if m >= 0)
    assert wrong >= 5                                                            # (20 of 35 with these keys)


def test_sample_extract_is_the_tail_of_the_bootstrap():
    """Oracle.sample_extract(blind_rotate(modswitch(keyswitch(ct)))) is bootstrap_batch, word for word"""
    prm = planted_set(**PLANTED_FAMILIES["k3_n512_g2"])
    o = orc.Oracle(prm, seed=5)
    table = [0, 1, 2, 3, 2, 1, 0]
    tv, post = o.build_tv(table)
    cts = o.encrypt(np.arange(7), nonce0=2)
    want, _ = o.bootstrap_batch(cts, [table])
    for ct, w in zip(cts, want):
        assert np.array_equal(o.sample_extract(o.blind_rotate(o.modswitch(o.keyswitch(ct)), tv), post), w)
