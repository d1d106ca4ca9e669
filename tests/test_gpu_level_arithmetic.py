"""The kernels that run between bootstraps -- k_lincomb, k_multi_extract, k_scatter_rows, k_fill_trivial (csrc/fbs_kernels.hip) --
each driven alone on the inputs planted in tests/helpers.py, which tests/test_level_arithmetic_reference.py shows to sit at the
bounds those kernels are exact by: linear combinations of up to 400 terms whose planted columns hold 16 products of one sign just
inside q/2 between two centrings, coefficients and constants at the ends of int64 and at multiples of q; tables whose difference
polynomial has sum |d| = 65534, the most the loader fuses, cut out of accumulators of q - 1 throughout; tables with 65536, which the
loader must keep on a rotation of their own.  Every comparison is word for word against the CPU oracle (pinned to the definition on
Python integers by the reference file); every word the call was not to write must be bit-identical to what was uploaded.

Shapes: every way the 256-thread loop over the D + 1 words of a ciphertext can end (ct_words 257: the second pass has one live lane;
513, 1025, 1537, 2049, 4097), at tiny n so that key generation and the oracle's bootstraps take milliseconds."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (EX_P, EX_TABLES, LC_OUTPUTS, LC_SHAPES, LC_SLOTS, Q, lc_coefs, lc_delta, lc_terms, planted_accumulators,
                           planted_lincomb)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A          # in every word no call may write (not a residue: a kernel that read it would show too)
BEHIND = 0x3C3C3C3C3C3C3C3C            # behind a ciphertext in a row of (k + 1) N words: a copy of the whole row would carry it over
_MADE = {}


@pytest.fixture(scope="module")
def nat():
    from tfhe_fbs_map_amd import _native
    return _native


def made(nat, k, log_n):
    """(context, oracle) of a shape on the same keys, made once: three gadget levels of ten bits, so that a table cut out of a
    shared rotation with |D_F| = 32767 sqrt(2) still decrypts"""
    if (k, log_n) not in _MADE:
        from tfhe_fbs_map_amd import Params
        prm = Params(n=8, log_n_poly=log_n, k=k, l_bsk=3, beta_bsk=10, t_ksk=8, gamma_ksk=2, p_msg=EX_P, sigma_lwe=1 << 8, sigma_glwe=4,
                     bsk_group=1)
        _MADE[(k, log_n)] = (nat.Context(prm, seed=13), orc.Oracle(prm, seed=13))
    return _MADE[(k, log_n)]


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def download(d):
    return d.cpu().numpy().view(np.uint64)


def planted_sources(ctw, T):
    """[LC_SLOTS][T][ctw]: sample s holds the planted words of sign +1 (s even) or -1 (s odd)"""
    return np.stack([planted_lincomb(ctw, LC_SLOTS, 1 - 2 * (s & 1), seed=s)[0] for s in range(T)], axis=1)


# ---- fbs_lincomb_dev ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,log_n", LC_SHAPES)
def test_lincomb_of_up_to_400_planted_terms_word_for_word(nat, k, log_n):
    """One launch: outputs of 0, 1, 15, 16, 17, 31, 32, 33, 48, 100 and 400 terms (a ragged term list with an empty entry, sources
    repeated within an output from 49 terms on), both signs (by sample), T = 5."""
    ctx, o = made(nat, k, log_n)
    ctw, T = ctx.params.ct_words, 5
    assert ctw == k * (1 << log_n) + 1
    coefs = lc_coefs(LC_SLOTS)
    n_out = len(LC_OUTPUTS)
    wires = np.full((LC_SLOTS + n_out + 1, T, ctw), SENTINEL, np.uint64)           # sources, destinations, one slot nobody names
    wires[:LC_SLOTS] = planted_sources(ctw, T)
    dst = [LC_SLOTS + n_out - 1 - g for g in range(n_out)]                          # (not in the order of the outputs)
    off, srcs, cf = [0], [], []
    for first, n, _ in LC_OUTPUTS:
        srcs += lc_terms(first, n)
        cf += [coefs[t] for t in lc_terms(first, n)]
        off.append(len(srcs))
    assert off[1] == 0 and max(np.bincount(srcs[off[-2]:])) >= 8                     # an empty term list; sources repeated
    d = upload(wires)
    ctx.lincomb_dev(d.data_ptr(), T, dst, off, srcs, cf, [c for _, _, c in LC_OUTPUTS])
    ctx.sync()
    got = download(d)
    assert np.array_equal(got[:LC_SLOTS], wires[:LC_SLOTS]) and (got[LC_SLOTS + n_out] == SENTINEL).all()
    assert got[LC_SLOTS:LC_SLOTS + n_out].max() < Q
    for g, (first, n, const) in enumerate(LC_OUTPUTS):
        terms = lc_terms(first, n)
        for s in range(T):
            ref = o.lincomb([wires[t, s] for t in terms], [coefs[t] for t in terms], const)
            bad = np.nonzero(got[dst[g], s] != ref)[0]
            assert bad.size == 0, "%d terms, sample %d: %d words differ, first at %d" % (n, s, bad.size, bad[0])


# ---- fbs_level_lincomb_dev, fbs_eval, fbs_eval_dev ---------------------------------------------------------------------------------
def lincomb_program(nat, ctx):
    """LinearProds on the planted coefficients, no bootstrap: 40 terms; 17 terms; a combination of those two and an input (a second
    stage of the same level: nothing is merged below the facade); a constant alone; 400 terms.  Every one of them is an output, then the
    constants 0, 1 and 2p - 1.  -> (program, instructions as (terms [(coef, wire)], const))"""
    coefs = lc_coefs(LC_SLOTS)
    w = LC_SLOTS                                                                    # wire id of the first instruction
    instr = [([(coefs[t], t) for t in range(40)], 1), ([(coefs[t], t) for t in range(17)], Q),
             ([(1, w), (-1, w + 1), (coefs[11], w), (3, 5)], -1), ([], 2 * EX_P - 1),
             ([(coefs[t % LC_SLOTS], t % LC_SLOTS) for t in range(400)], 0)]
    arg0, term_coef, term_src = [], [], []
    for terms, _ in instr:
        arg0.append(len(term_src))
        term_coef += [c for c, _ in terms]
        term_src += [s for _, s in terms]
    out_wire = [w + 2, w, w + 3, w + 1, w + 4, -1 - 0, -1 - 1, -1 - (2 * EX_P - 1)]
    prog = nat.Program(ctx, ctx.tvset([]), LC_SLOTS, [0] * len(instr), arg0, [len(t) for t, _ in instr], [c for _, c in instr],
                       term_coef, term_src, out_wire)
    return prog, instr, out_wire


def oracle_lincombs(o, instr, inputs, s):
    """the value of every wire of lincomb_program at sample s"""
    vals = [inputs[i, s] for i in range(LC_SLOTS)]
    for terms, const in instr:
        vals.append(o.lincomb([vals[src] for _, src in terms], [c for c, _ in terms], const))
    return vals


@pytest.mark.parametrize("k,log_n", LC_SHAPES)
def test_level_lincomb_on_a_sample_range_and_constant_outputs(nat, k, log_n):
    ctx, o = made(nat, k, log_n)
    ctw, T, s0, sc = ctx.params.ct_words, 7, 2, 3
    prog, instr, out_wire = lincomb_program(nat, ctx)
    assert prog.depth == 0 and prog.n_bootstrap == 0
    inputs = planted_sources(ctw, T)
    # one level call on samples [2, 5) of a buffer of stride 7
    wires = np.full((prog.n_slots + 1, T, ctw), SENTINEL, np.uint64)
    wires[prog.in_slot] = inputs
    d = upload(wires)
    prog.level_lincomb_dev(0, d.data_ptr(), T, s0, sc)
    ctx.sync()
    got = download(d)
    want = wires.copy()
    for s in range(s0, s0 + sc):
        vals = oracle_lincombs(o, instr, inputs, s)
        for wire, slot in zip(out_wire[:5], prog.out_slot[:5]):                     # (every instruction is an output: its slot is known)
            want[slot, s] = vals[wire]
    assert len(set(prog.out_slot[:5].tolist())) == 5 and (prog.out_slot[5:] < 0).all()
    assert (want[prog.out_slot[:5], s0:s0 + sc] < Q).all()
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "(slot, sample) that differ: %s" % bad[:8].tolist()
    # the whole program, host to host and device to device: the constants of the second come from k_fill_trivial
    Te = 3
    ref = np.zeros((len(out_wire), Te, ctw), np.uint64)
    for s in range(Te):
        vals = oracle_lincombs(o, instr, inputs, s)
        for i, wire in enumerate(out_wire):
            if wire >= 0:
                ref[i, s] = vals[wire]
            else:
                ref[i, s, -1] = (-1 - wire) * lc_delta(EX_P) % Q
    cts = np.ascontiguousarray(inputs[:, :Te])
    assert np.array_equal(prog.eval(cts, Te), ref)
    d_in = upload(cts)
    d_out = upload(np.full((len(out_wire) * Te + 1, ctw), SENTINEL, np.uint64))
    prog.eval_dev(d_in.data_ptr(), Te, d_out.data_ptr())
    ctx.sync()
    out = download(d_out)
    assert np.array_equal(out[:-1].reshape(ref.shape), ref) and (out[-1] == SENTINEL).all()
    assert list(ctx.decrypt(ref[5:, 0])) == [0, 1, 2 * EX_P - 1]


# ---- fbs_level_scatter_dev on planted rows ------------------------------------------------------------------------------------
TABLE_NAMES = ["at_limit_a", "at_limit_b", "small", "negative", "c1_long", "over_limit_a"]
TABLES = [EX_TABLES[n] for n in TABLE_NAMES]
LINS = [[(1, 0), (2, 1)], [(1, 0), (2, 2)], [(1, 1), (1, 2)]]                       # wires 3, 4, 5 of inputs 0, 1, 2


def shared_program(nat, ctx, over_limit=False, fuse=True):
    """wire 3 read by the two tables at the limit, the small one and a negative one (and by the table over the limit), wire 4 by two
    tables, wire 5 by one.  -> (program, boots as (output index, source wire, table id))"""
    boots = [(3, 0), (3, 1), (3, 2), (3, 3)] + ([(3, 5)] if over_limit else []) + [(4, 2), (4, 4), (5, 2)]
    kind = [0] * 3 + [1] * len(boots)
    arg0 = [0, 2, 4] + [src for src, _ in boots]
    arg1 = [2, 2, 2] + [tab for _, tab in boots]
    flat = [t for lin in LINS for t in lin]
    prog = nat.Program(ctx, ctx.tvset(TABLES), 3, kind, arg0, arg1, [0] * len(kind), [c for c, _ in flat], [s for _, s in flat],
                       [6 + i for i in range(len(boots))], fuse_tables=fuse)
    return prog, [(i, src, tab) for i, (src, tab) in enumerate(boots)]


def oracle_sources(o, cts, s):
    """{wire 3 | 4 | 5: its ciphertext at sample s}"""
    return {3 + i: o.lincomb([cts[src, s] for _, src in lin], [c for c, _ in lin], 0) for i, lin in enumerate(LINS)}


def match_rows(rows, candidates, ctw):
    """rows [n_gates][samples][row_words], candidates {name: [samples][words]} -> name per gate: every row equals exactly one
    candidate (over its own length) at every sample"""
    names = []
    for g in range(rows.shape[0]):
        hits = [n for n, c in candidates.items() if np.array_equal(rows[g, :, :c.shape[1]], c)]
        assert len(hits) == 1, "row %d matches %s" % (g, hits)
        names.append(hits[0])
    assert len(set(names)) == len(names)
    return names


BITS = np.array([[0, 1, 0, 1, 1, 0, 1], [0, 0, 1, 1, 0, 1, 1], [1, 0, 0, 1, 0, 0, 1]])


@pytest.mark.parametrize("k,log_n", [(1, 8), (2, 10), (3, 9)])
def test_tables_either_side_of_the_fusing_limit(nat, k, log_n):
    """Tables with sum |d| = 65534 share a rotation; one with 65536 on the same source loads, on a rotation of its own; the program
    decrypts to what it decrypts to without sharing, and every ciphertext is the oracle's."""
    ctx, o = made(nat, k, log_n)
    T = BITS.shape[1]
    prog, _ = shared_program(nat, ctx)
    assert (prog.n_bootstrap, prog.n_rotations, prog.n_keyswitch) == (7, 3, 3)
    prog2, boots2 = shared_program(nat, ctx, over_limit=True)
    plain2, _ = shared_program(nat, ctx, over_limit=True, fuse=False)
    assert (prog2.n_bootstrap, prog2.n_rotations) == (8, prog.n_rotations + 1) and plain2.n_rotations == 8
    cts = ctx.encrypt(BITS, nonce0=31)
    got2, ref2 = prog2.eval(cts, T), plain2.eval(cts, T)
    msgs = ctx.decrypt(ref2)
    assert np.array_equal(ctx.decrypt(got2), msgs)
    value = {3: BITS[0] + 2 * BITS[1], 4: BITS[0] + 2 * BITS[2], 5: BITS[1] + BITS[2]}
    for i, src, tab in boots2:
        assert np.array_equal(msgs[i], np.array(TABLES[tab] + [0] * EX_P)[value[src]] % (2 * EX_P)), TABLE_NAMES[tab]
    srcs = {u: np.stack([oracle_sources(o, cts, s)[u] for s in range(T)]) for u in (3, 4, 5)}
    shared = {u: [(i, tab) for i, src, tab in boots2 if src == u and tab != 5] for u in (3, 4)}
    for u, group in shared.items():                                                 # cut out of one rotation of the source
        for (i, tab), ref in zip(group, o.bootstrap_multi(srcs[u], [TABLES[tab] for _, tab in group])):
            assert np.array_equal(got2[i], ref), (u, TABLE_NAMES[tab])
    for i, src, tab in boots2:                                                      # a rotation each: also the table over the limit
        ref = o.bootstrap_batch(srcs[src], [TABLES[tab]])[0]
        assert np.array_equal(ref2[i], ref) and (np.array_equal(got2[i], ref) == (tab == 5 or src == 5)), (src, TABLE_NAMES[tab])


@pytest.mark.parametrize("k,log_n", [(1, 8), (2, 10), (3, 9)])
def test_scatter_of_planted_accumulators_and_ciphertext_rows(nat, k, log_n):
    """fbs_level_scatter_dev of a fused level on rows a test chose: accumulators of q - 1 throughout, of 0, alternating, q - 1 on
    one polynomial, random under the tables at the limit; a planted ciphertext with a sentinel behind it in the ordinary gate's row.
    The order of the rows is taken from one honest run, not assumed."""
    import torch
    ctx, o = made(nat, k, log_n)
    prm = ctx.params
    N, ctw, T, s0, sc = prm.N, prm.ct_words, 7, 2, 3
    prog, boots = shared_program(nat, ctx)
    assert prog.n_rotations == 3 and prog.row_words == (k + 1) * N > ctw and prog.depth == 1 and prog.level_width == [3]
    cts = ctx.encrypt(BITS, nonce0=31)

    # ---- the oracle's side of one honest level on samples [2, 5): accumulators of the shared sources, the single gate's ciphertext
    tv0 = o.tv0()
    acc = {u: np.stack([o.blind_rotate(o.modswitch(o.keyswitch(oracle_sources(o, cts, s)[u])), tv0) for s in range(s0, s0 + sc)])
           for u in (3, 4)}
    single = o.bootstrap_batch(np.stack([oracle_sources(o, cts, s)[5] for s in range(s0, s0 + sc)]), [TABLES[2]])[0]
    wires = np.full((prog.n_slots + 1, T, ctw), SENTINEL, np.uint64)
    wires[prog.in_slot] = cts
    d = upload(wires)
    total = prog.level_width[0] * sc
    rows = torch.full((total + 1, prog.row_words), SENTINEL, dtype=torch.int64, device="cuda")
    prog.level_lincomb_dev(0, d.data_ptr(), T, s0, sc)
    prog.level_bootstrap_dev(0, d.data_ptr(), T, s0, sc, 0, total, d_rows=rows.data_ptr())
    ctx.sync()
    honest = download(rows)
    assert (honest[total] == SENTINEL).all()
    order = match_rows(honest[:total].reshape(-1, sc, prog.row_words), {3: acc[3], 4: acc[4], 5: single}, ctw)

    # ---- planted rows: every accumulator pattern under the tables at the limit, a planted ciphertext with a sentinel behind it ----
    pats = planted_accumulators(k, N, seed=k)
    pats["one polynomial'"] = planted_accumulators(k, N, seed=k + 1)["one polynomial"]
    names = list(pats)
    planted = np.full((total + 1, prog.row_words), BEHIND, np.uint64)
    rows_of = {}
    for g, u in enumerate(order):
        for s in range(sc):
            if u == 5:
                planted[g * sc + s, :ctw] = planted_lincomb(ctw, 3, 1, seed=s)[0][s]
            else:                                                                   # wire 3: all q - 1, all 0, alternating; wire 4: the rest
                planted[g * sc + s] = pats[names[s if u == 3 else 3 + s]]
            rows_of[(u, s)] = planted[g * sc + s]
    assert names[0] == "all q-1" and (planted[order.index(5) * sc:, ctw:][:sc] == BEHIND).all()
    before = download(d).copy()
    d_planted = upload(planted)
    prog.level_scatter_dev(0, d.data_ptr(), T, s0, sc, d_planted.data_ptr(), 0, total)
    ctx.sync()
    got = download(d)
    want = before.copy()
    for i, src, tab in boots:
        slot = prog.out_slot[i]
        for s in range(sc):
            if src == 5:
                want[slot, s0 + s] = rows_of[(5, s)][:ctw]
            else:
                diff, post = o.build_tv_diff(TABLES[tab])
                want[slot, s0 + s] = o.multi_extract(rows_of[(src, s)], diff, post)
    assert len(set(prog.out_slot.tolist())) == len(boots)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "(slot, sample) that differ: %s of out slots %s" % (bad[:8].tolist(), prog.out_slot.tolist())
    assert got[prog.out_slot, s0:s0 + sc].max() < Q


@pytest.mark.parametrize("k,log_n", [(1, 8), (3, 9)])
def test_scatter_of_ciphertext_rows_in_slices(nat, k, log_n):
    """A program loaded without sharing: rows of D + 1 words, scattered in slices that begin inside a gate (f_begin > 0)."""
    import torch
    ctx, o = made(nat, k, log_n)
    ctw, T, s0, sc = ctx.params.ct_words, 7, 2, 3
    prog, boots = shared_program(nat, ctx, fuse=False)
    assert (prog.n_rotations, prog.row_words, prog.level_width) == (7, ctw, [7])
    cts = ctx.encrypt(BITS, nonce0=31)
    wires = np.full((prog.n_slots + 1, T, ctw), SENTINEL, np.uint64)
    wires[prog.in_slot] = cts
    d = upload(wires)
    total = 7 * sc
    rows = torch.full((total + 1, ctw), SENTINEL, dtype=torch.int64, device="cuda")
    prog.level_lincomb_dev(0, d.data_ptr(), T, s0, sc)
    cuts = [(0, 4), (4, 5), (5, 14), (14, total)]
    for f0, f1 in cuts:
        prog.level_bootstrap_dev(0, d.data_ptr(), T, s0, sc, f0, f1, d_rows=rows[f0:].data_ptr())
    ctx.sync()
    honest = download(rows)
    assert (honest[total] == SENTINEL).all()
    srcs = [np.stack([oracle_sources(o, cts, s)[u] for s in range(s0, s0 + sc)]) for u in (3, 4, 5)]
    cand = {i: o.bootstrap_batch(srcs[src - 3], [TABLES[tab]])[0] for i, src, tab in boots}
    order = match_rows(honest[:total].reshape(7, sc, ctw), cand, ctw)                # gate -> output index
    planted = np.full((total + 1, ctw), SENTINEL, np.uint64)
    planted[:total] = planted_lincomb(ctw, total, -1, seed=k)[0]
    before = download(d).copy()
    d_rows = upload(planted)
    for f0, f1 in cuts[::-1]:
        prog.level_scatter_dev(0, d.data_ptr(), T, s0, sc, d_rows[f0:].data_ptr(), f0, f1)
    ctx.sync()
    got = download(d)
    want = before.copy()
    for g, i in enumerate(order):
        want[prog.out_slot[i], s0:s0 + sc] = planted[g * sc:(g + 1) * sc]
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "(slot, sample) that differ: %s" % bad[:8].tolist()
