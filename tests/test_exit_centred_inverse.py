"""`SplitNtt::inverse_exit_centred` (csrc/fbs_ntt_split.hpp): the inverse transform k_blind_rotate takes where a wave holds a whole
N = 1024 polynomial and DIG >= 1.  It centres ONE register per group and half, at the group's exit, where `inverse<true>` centres all
eight at the entry of groups 1 and 0.

Without a GPU: a replay on exact integers (the FP64 models of tests/helpers.py: fp_mulmod, and fp_center with the rint of the rounded
float quotient) on inputs AT the entry promise 16 q - 1, which holds every range the header states; and the kernel source calls the new
inverse under the one condition it is proved for.  On the GPU: the device's raw words are the replay's, word for word; reduced mod q they
are what the listed `bounded=1` variant gives; and the two k_blind_rotate shapes of the benchmark parameter set still produce the
oracle's ciphertexts."""
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import N, Q, TWI, TWO53, exact, fp_center, fp_mulmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
NEW_LINE = "class=SplitNtt logn=10 lanes=64 dir=inverse bounded=1 centre=exit"
OLD_LINE = "class=SplitNtt logn=10 lanes=64 dir=inverse bounded=1"
ENTRY = 16 * Q - 1
TWO52 = 1 << 52


def inverse_exit_centred(x, seen=None):
    """SplitNtt::inverse_exit_centred on values by position: Gentleman-Sande stages 9..7 (group 2), 6..4 (group 1), 3..1 (group 0), after each
    group fp_center on register 0 of every lane and half -- the positions whose three index bits of that group are zero -- then the joining
    stage 0; returns N * coefficients.  seen: a dict that receives, per group ("g2", "g1", "g0", "join"), the largest fp_mulmod input, and
    per group the largest register 0 before centring and the largest other register, "peak" (the largest value held anywhere) and "out"."""
    x = list(x)
    seen = {} if seen is None else seen
    peak = max(abs(v) for v in x)
    assert peak < 16 * Q

    def stage(s, key):
        nonlocal peak
        half = N >> (s + 1)
        for blk in range(1 << s):
            w = TWI[(1 << s) + blk]
            for i in range(blk * 2 * half, blk * 2 * half + half):
                u, v = x[i], x[i + half]
                d = exact(int(u) - int(v))
                seen[key] = max(seen.get(key, 0), abs(d))
                x[i] = exact(int(u) + int(v))
                x[i + half] = fp_mulmod(d, w)
                peak = max(peak, abs(d), abs(x[i]), abs(x[i + half]))

    for group, stages in ((2, (9, 8, 7)), (1, (6, 5, 4)), (0, (3, 2, 1))):
        for s in stages:
            stage(s, "g%d" % group)
        lo = 6 - 3 * group                                   # lo_of(G): the group's registers are index bits lo .. lo + 2 of a half
        reg0 = [i for i in range(N) if (i >> lo) & 7 == 0]
        seen["g%d reg0" % group] = max(abs(x[i]) for i in reg0)
        seen["g%d others" % group] = max(abs(x[i]) for i in range(N) if (i >> lo) & 7)
        for i in reg0:
            x[i] = fp_center(x[i])
    stage(0, "join")
    seen["peak"], seen["out"] = peak, max(abs(v) for v in x)
    return x


_cases = {}


def cases():
    """{name: (values by position, replay, what the replay saw)}, made once: helpers.variant_cases at 16 q - 1"""
    if not _cases:
        v = H.parse_variant(OLD_LINE)
        for name, c in H.variant_cases(v, ENTRY):
            seen = {}
            _cases[name] = (c, inverse_exit_centred([float(a) for a in c], seen), seen)
    return _cases


FAMILIES = (["random", "all +", "all -"] + ["alternating, stride 2^%d" % s for s in range(10)] + ["extreme class %d" % c for c in range(4)])


def test_case_list_is_whole():
    names = list(cases())
    assert names and len(names) == 1 + 2 * (len(FAMILIES) - 1)
    for fam in FAMILIES:
        assert fam in names, fam
        if fam != "random":
            assert fam + ", just inside" in names, fam
    for name, (c, _, _) in cases().items():
        assert len(c) == N and max(abs(a) for a in c) <= ENTRY, name
    assert all(abs(a) == ENTRY for a in cases()["all +"][0])


def test_replay_gives_the_residues_of_the_reference():
    for name, (c, out, _) in cases().items():
        assert [int(a) % Q for a in out] == H.reference_intt(c, 10), name


def test_replay_stays_inside_the_ranges_the_header_states():
    top = 0
    for name, (_, _, seen) in cases().items():
        assert seen["peak"] < TWO53, name                               # everything held is an exact integer below 2^53
        assert seen["g2"] < TWO53, name                                 # fp_mulmod inputs: exact there ...
        assert max(seen["g1"], seen["g0"], seen["join"]) < TWO52, name  # ... and in the narrower range, products under 0.8 q, here
        assert seen["g2 reg0"] <= 128 * Q, name
        assert seen["g1 reg0"] <= 40 * Q and seen["g0 reg0"] <= 40 * Q, name
        assert max(seen["g2 others"], seen["g1 others"], seen["g0 others"]) <= 5 * Q, name
        assert seen["out"] <= 8 * Q, name
        top = max(top, seen["g2 reg0"])
    assert top >= 127 * Q, "no case takes group 2's register 0 to the edge: %.2f q" % (top / Q)
    assert cases()["all +"][2]["g2 reg0"] == 8 * ENTRY                   # the planted one: eight equal inputs at the promise


def test_kernel_takes_the_new_inverse_under_the_proved_condition_only():
    br = re.sub(r"\s+", " ", open(os.path.join(CSRC, "fbs_blind_rotate.hip")).read())
    call = ("if constexpr (has_fused_opening<W>::value && BOUNDED) W::inverse_exit_centred(own, xc, t, twi, inv_uni); "
            "else W::template inverse<BOUNDED>(own, xc, t, twi, inv_uni);")
    assert br.count(call) == 1 and br.count("inverse_exit_centred(") == 1
    assert br.count("constexpr bool BOUNDED = DIG >= 1;") == 1
    assert br.index("void k_blind_rotate(BrArgs a)") < br.index(call) < br.index("void k_blind_rotate_pairs(BrArgs a)")
    # a whole polynomial on one wave: the condition is the fused opening's, which only SplitNtt has
    split = re.sub(r"\s+", " ", open(os.path.join(CSRC, "fbs_ntt_split.hpp")).read())
    assert "struct has_fused_opening : std::false_type {};" in split
    assert split.count("struct has_fused_opening<") == 1 and "struct has_fused_opening<SplitNtt<LOGN, LL>> : std::true_type {};" in split
    # nobody else calls it: the pairs, k = 2, general-GLWE and whole-CU kernels and WavesNtt keep inverse<>
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp", ".cpp")) and name not in ("fbs_blind_rotate.hip", "fbs_ntt_split.hpp", "fbs_debug_transform.hip"):
            assert "inverse_exit_centred" not in open(os.path.join(CSRC, name)).read(), name
    assert split.count("inverse_exit_centred(") == 1                     # its definition: WavesNtt does not call it
    # the hook runs it and the list does not name it
    from tfhe_fbs_map_amd import _native
    assert NEW_LINE not in _native.debug_transform_list() and OLD_LINE in _native.debug_transform_list()
    assert '"%s"' % NEW_LINE in open(os.path.join(CSRC, "fbs_debug_transform.hip")).read()


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device():
    """(run, pos): run(line, [values by position]) -> raw words in natural order; pos from the layout probe of the forward variant"""
    from tests import test_gpu_transforms as G
    pos = G.probe(H.parse_variant(OLD_LINE))

    def run(line, polys):
        out = G.context(10).debug_transform(line, np.array([[c[pos[j]] for j in range(N)] for c in polys], dtype=np.int64))
        return [[int(a) for a in row] for row in out]
    return run


@pytest.mark.gpu
def test_device_equals_the_replay_word_for_word(device):
    names = list(cases())
    got = device(NEW_LINE, [cases()[n][0] for n in names])
    for name, out in zip(names, got):
        want = [int(a) for a in cases()[name][1]]
        bad = [j for j in range(N) if out[j] != want[j]]
        assert not bad, "%s: %d words differ, first at coefficient %d: device %d, replay %d" % (name, len(bad), bad[0], out[bad[0]], want[bad[0]])


@pytest.mark.gpu
def test_device_agrees_with_the_listed_inverse_mod_q(device):
    names = list(cases())
    new = device(NEW_LINE, [cases()[n][0] for n in names])
    old = device(OLD_LINE, [cases()[n][0] for n in names])
    for name, a, b in zip(names, new, old):
        assert [x % Q for x in a] == [x % Q for x in b], name
        assert max(abs(x) for x in a) <= 8 * Q, name


@pytest.mark.gpu
@pytest.mark.parametrize("count,kernel", [(2 * H.CUS + 1, "k_blind_rotate<10,6,3,1>"), (7 * 4 * H.CUS // 8, "k_blind_rotate<10,6,3,4>")])
def test_kernels_that_take_it_give_the_oracles_ciphertexts(toy_params, count, kernel):
    """the benchmark's gadget (l = 3, beta = 7: DIG = 3) at n = 12: one launch of the small-workgroup shape (the first size past two
    bootstraps per CU) and one of the whole-CU shape (the smallest last round the launcher still sends there, 7/8 of 1024), sampled rows
    (first, last and every sub-slot of a workgroup, a trivial ciphertext among them) word for word against the oracle"""
    from oracle import tfhe_oracle as orc
    from tfhe_fbs_map_amd import _native
    ctx, o = _native.Context(toy_params, seed=21), orc.Oracle(toy_params, seed=21)
    rng = np.random.default_rng(count)
    tables = [[0, 1, 1, 0, 1, 0, 0], [0, 1, 2, 3, 2, 1, 0]]
    msgs = rng.integers(0, 7, count)
    ids = rng.integers(0, 2, count).astype(np.uint32)
    cts = ctx.encrypt(msgs, nonce0=300)
    cts[2, :-1] = 0                                                       # trivial: every rotation amount zero
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = ctx.bootstrap_batch(ctx.tvset(tables), cts, ids)
    launched = [k for k in ctx.profile_kernels() if "blind_rotate" in k]
    ctx.profile(False)
    assert launched == [kernel]
    pick = [0, 1, 2, 3, 4, 5, 6, 7, count // 2, count // 2 + 1, count - 2, count - 1]
    ref, _ = o.bootstrap_batch(cts[pick], tables, ids[pick])
    assert np.array_equal(got[pick], ref)
    keep = np.ones(count, bool)
    keep[2] = False
    assert np.array_equal(ctx.decrypt(got)[keep], np.array([tables[i][m] for i, m in zip(ids, msgs)])[keep])
    ctx.close()
