"""Every blind-rotation kernel with an ENCRYPTED accumulator (include/fbs_exec.h, "encrypted-index reads"), word for word against
tests/lookup_reference.py -- which tests/test_lookup_reference.py ties to the frozen oracle.

One case per rotation entry of fbs_kernel_catalog, at the recipe that reaches it (tests/helpers.py: recipe, planted_set, n = 16),
through fbs_lookup_compact_dev at bits = log2(2N): the fields of a row ARE its rotation amounts (tests/test_gpu_rotation_amounts.py),
so the planted rows of planted_amount_rows drive the prologue's gather through every mask list and every edge of the body amount.
Row f of a launch is planted row f % 60 and names table (f // 5) % 4 of THREE: id 3 is out of range and must read table 0.  The
tables are genuine mapped folds (box map, p = 7) of encryptions of a permutation of 0 .. 6 each, made once per parameter set on
the CPU by tests/fold_reference.py's fold_sample through tests/lookup_reference.py:fold_by_boxes -- from ciphertexts whose masks
are random in 16 columns and zero elsewhere, so that only 16 rows of a fold key have to be made where a whole key is up to 270 MB;
the tables' own mask polynomials are sums of digit x key products and full-size residues all the same.  The counts are the
recipes': ragged last workgroups, several bootstraps per workgroup, calls cut into two launches.

THE SUBSET.  The CPU reference is computed on 23 of the 60 planted rows, REF_ROWS below, and every word of every row f of the launch
with f % 60 among them is compared.  It keeps: all five mask lists (rows 0 .. 4, 45 .. 49, 55 .. 59); a semantic body at each of
the three offsets (rows 0, 1, 2: offsets 0, +edge, -edge); the raw bodies N - 1 (rows 45 .. 49), N (50 .. 52) and 2N - 1
(55 .. 59), where the mask polynomials wrap and change sign; and every table id, 3 included (bodies 0, 1, 2, 3 and 9, 10, 11).  A
row's table depends on f % 60 alone (60 / 5 is a multiple of 4), so EVERY other row of the launch must equal, word for word, the
row 60 before it: all rows are held, through the first 60, and those through the subset.  No entry of the catalog is left out, and
no kernel is kept out of lookups by the selector: every family's numbers stayed where they were (profiles/lookup/resources.txt)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests import lookup_reference as L
from tests.helpers import (PLANTED_DEFAULT_KNOBS, PLANTED_FAMILIES, PLANTED_MARGIN, PLANTED_ROWS, PLANTED_STEPS, planted_amount_rows,
                           planted_output_margin, planted_set, recipe)
from tests.test_gpu_compact import pack
from tests.test_gpu_device_io import dev, host
from tests.test_gpu_rotation_amounts import SENTINEL, refresh_planted, rotation_entries, set_of

pytestmark = pytest.mark.gpu

N_TABLES = 3
REF_ROWS = sorted(set(range(0, 5)) | {5, 6, 10, 15, 16} | set(range(45, 50)) | {50, 51, 52} | set(range(55, 60)))


def pytest_generate_tests(metafunc):
    if "kernel_name" in metafunc.fixturenames:
        metafunc.parametrize("kernel_name", rotation_entries())


def table_of(f):
    return (np.asarray(f) // 5) % 4


def lookup_planted(ctx, fields, tables, count, ids="planted"):
    """rows f % 60 of `fields`, f < count, through fbs_lookup_compact_dev at log2(2N) bits -> [count][D + 1]; the buffer is two rows
    longer than the launch, and those rows stay as they were"""
    import torch
    b = ctx.params.log_n_poly + 1
    words = pack(fields[np.arange(count) % PLANTED_ROWS].astype(np.uint64), b)
    d_t = dev(np.array(tables))
    assert d_t.data_ptr() % 16 == 0
    d_of = None if ids is None else torch.from_numpy(table_of(np.arange(count)).astype(np.int32)).cuda()
    d_c = torch.full((count + 2, ctx.params.ct_words), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.lookup_compact_dev(d_t.data_ptr(), len(tables), 0 if d_of is None else d_of.data_ptr(), dev(words).data_ptr(), count, d_c.data_ptr(),
                           bits=b)
    ctx.sync()
    out = host(d_c)
    assert (out[count:] == SENTINEL).all(), "wrote past the last ciphertext"
    return out[:count]


@pytest.fixture(scope="module")
def planted():
    """per parameter set: context, oracle on the context's keys, the 60 planted rows, their messages, the three tables and their
    entries, the reference outputs of REF_ROWS (computed once, never written to), and whether the set is a usable one"""
    from tfhe_fbs_map_amd import Params, _native as nat
    made = {}

    def get(log_n, k, l, beta, group):
        key = (log_n, k, l, beta, group)
        if key not in made:
            prm = planted_set(*key)
            ctx = nat.Context(Params(**prm), seed=33)
            o = orc.Oracle(prm, seed=33, keygen=False)
            o.set_keys(**ctx.export_keys())
            fields, meta = planted_amount_rows(1 << log_n, PLANTED_STEPS, group, o.keys()["sk_lwe"], prm["p_msg"])
            tables, entries = L.encrypted_tables(o, prm, N_TABLES, seed=11)
            L._keys_of(o)                                        # (before the threads share it)
            eff = [int(t) if t < N_TABLES else 0 for t in table_of(REF_ROWS)]
            with ThreadPoolExecutor(8) as pool:
                ref = np.stack(list(pool.map(lambda jt: L.lookup_reference(o, fields[jt[0]], tables[jt[1]]), zip(REF_ROWS, eff))))
            ref.setflags(write=False)
            tables.setflags(write=False)
            made[key] = (ctx, o, fields, np.array(meta["msg"]), tables, entries, ref, planted_output_margin(prm) >= PLANTED_MARGIN)
        return made[key]

    yield get
    for entry in made.values():
        entry[0].close()


def test_the_subset_keeps_what_it_must():
    lists = {j % 5 for j in REF_ROWS}
    bodies = {j // 5 for j in REF_ROWS}
    assert lists == {0, 1, 2, 3, 4} and {9, 10, 11} <= bodies                      # every mask list; raw N - 1, N, 2N - 1
    assert {j % 3 for j in REF_ROWS if j // 5 < 7} == {0, 1, 2}                    # a semantic body at each offset (turn = 0)
    assert {int(t) for t in table_of(REF_ROWS)} == {0, 1, 2, 3}                    # every id, the out-of-range one included
    assert all((table_of(f) == table_of(f % 60)).all() for f in (np.arange(2000),))
    for j in (45, 50, 55):                                                         # the raw bodies are what the docstring says
        fields, _ = planted_amount_rows(1024, 16, 1, np.ones(16, np.int64), 7)
        assert int(fields[j, 16]) == {45: 1023, 50: 1024, 55: 2047}[j]


def test_encrypted_accumulator_against_the_reference(planted, kernel_name):
    rec = recipe(kernel_name)
    assert rec is not None, "no recipe reaches %s" % kernel_name
    ctx, o, fields, msg, tables, entries, ref, usable = planted(*set_of(rec))
    ctx.tune(**{**PLANTED_DEFAULT_KNOBS, **rec["knobs"]})        # (the context is shared: the knobs are set per case)
    count = rec["count"]
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = lookup_planted(ctx, fields, tables, count)
    launched = ctx.profile_kernels()
    ctx.profile(False)
    assert kernel_name in launched, (kernel_name, sorted(launched))
    assert got.max() < orc.Q
    rows = np.arange(count) % PLANTED_ROWS
    at = {j: i for i, j in enumerate(REF_ROWS)}
    held = np.array([f for f in range(count) if rows[f] in at])
    want = ref[[at[j] for j in rows[held]]]
    wrong = held[(got[held] != want).any(axis=1)]                # ALL words of every row of the subset
    assert wrong.size == 0, (kernel_name, "rows", wrong[:8].tolist(), "lists", sorted(set((wrong % 5).tolist())))
    if count > PLANTED_ROWS:                                     # ... and every other row through the row 60 before it
        again = np.flatnonzero((got[PLANTED_ROWS:] != got[:-PLANTED_ROWS]).any(axis=1)) + PLANTED_ROWS
        assert again.size == 0, (kernel_name, "repeats", again[:8].tolist())
    if usable:                                                   # the entry the row names, of the table it names
        sem = held[msg[rows[held]] >= 0]
        tid = table_of(sem)
        tid[tid >= N_TABLES] = 0
        assert np.array_equal(ctx.decrypt(got[sem]), entries[tid, msg[rows[sem]]]), kernel_name


@pytest.mark.parametrize("family", sorted(PLANTED_FAMILIES))
def test_the_trivial_table_is_the_ordinary_bootstrap(planted, family):
    """table (0, .., 0, tv of the identity): fbs_lookup_compact_dev is fbs_refresh_compact_dev, word for word, on the 60 rows"""
    shape = PLANTED_FAMILIES[family]
    ctx, o, fields, _, _, _, _, _ = planted(shape["log_n_poly"], shape["k"], shape["l_bsk"], shape["beta_bsk"], shape["bsk_group"])
    ctx.tune(**PLANTED_DEFAULT_KNOBS)
    prm = ctx.params
    tv, post = o.build_tv(list(range(prm.p_msg)))
    assert post == 0
    table = np.zeros((1, prm.k + 1, prm.N), np.uint64)
    table[0, prm.k] = tv
    got = lookup_planted(ctx, fields, table, PLANTED_ROWS, ids=None)             # (no ids: row i reads table i, past the set table 0)
    assert np.array_equal(got, refresh_planted(ctx, fields, PLANTED_ROWS))


def test_lookup_of_big_key_indices_runs_the_key_switch_first(planted):
    """fbs_lookup_dev: key switch and modulus switch as fbs_bootstrap_batch_dev runs them (the oracle's, word for word), then the
    rotation from the table -- with ids, and without (index i reads table i; past the set, table 0)"""
    import torch
    ctx, o, _, _, tables, entries, _, usable = planted(10, 2, 1, 20, 2)
    assert usable
    ctx.tune(**PLANTED_DEFAULT_KNOBS)
    p = ctx.params.p_msg
    msgs = np.arange(2 * p) % p
    cts = ctx.encrypt(msgs, nonce0=5)
    ids = (np.arange(2 * p) // 3) % 4
    d_t, d_in = dev(np.array(tables)), dev(cts)                            # (held: a temporary's memory would be handed to the next upload)
    for use_ids in (True, False):
        eff = np.where(ids < N_TABLES, ids, 0) if use_ids else np.where(np.arange(2 * p) < N_TABLES, np.arange(2 * p), 0)
        d_out = torch.full((2 * p + 2, ctx.params.ct_words), SENTINEL, dtype=torch.int64, device="cuda")
        d_of = torch.from_numpy(ids.astype(np.int32)).cuda()
        ctx.lookup_dev(d_t.data_ptr(), N_TABLES, d_of.data_ptr() if use_ids else 0, d_in.data_ptr(), 2 * p, d_out.data_ptr())
        ctx.sync()
        got = host(d_out)
        assert (got[2 * p:] == SENTINEL).all()
        want = np.stack([L.lookup_reference(o, o.modswitch(o.keyswitch(ct)), tables[t]) for ct, t in zip(cts, eff)])
        assert np.array_equal(got[:2 * p], want), use_ids
        assert np.array_equal(ctx.decrypt(got[:2 * p]), entries[eff, msgs])


def test_lookup_refusals_write_nothing(planted):
    import torch
    from tfhe_fbs_map_amd import FbsError
    ctx, _, fields, _, tables, _, _, _ = planted(8, 4, 2, 8, 2)
    b = ctx.params.log_n_poly + 1
    d_t, d_w = dev(np.array(tables)), dev(pack(fields[:4].astype(np.uint64), b))
    d_c = torch.full((6, ctx.params.ct_words), SENTINEL, dtype=torch.int64, device="cuda")
    for call, text in ((lambda: ctx.lookup_compact_dev(d_t.data_ptr() + 8, 3, 0, d_w.data_ptr(), 4, d_c.data_ptr(), bits=b), "16-byte aligned"),
                       (lambda: ctx.lookup_compact_dev(d_t.data_ptr(), 0, 0, d_w.data_ptr(), 4, d_c.data_ptr(), bits=b), "at least one table"),
                       (lambda: ctx.lookup_compact_dev(0, 3, 0, d_w.data_ptr(), 4, d_c.data_ptr(), bits=b), "at least one table"),
                       (lambda: ctx.lookup_compact_dev(d_t.data_ptr(), 3, 0, d_w.data_ptr(), 4, d_c.data_ptr(), bits=b - 1), "compact width"),
                       (lambda: ctx.lookup_dev(d_t.data_ptr() + 8, 3, 0, d_c.data_ptr(), 4, d_c.data_ptr()), "16-byte aligned"),
                       (lambda: ctx.lookup_dev(d_t.data_ptr(), 0, 0, d_c.data_ptr(), 4, d_c.data_ptr()), "at least one table")):
        with pytest.raises(FbsError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value)
    ctx.lookup_compact_dev(d_t.data_ptr(), 3, 0, d_w.data_ptr(), 0, d_c.data_ptr(), bits=b)   # nothing to read: nothing done
    ctx.sync()
    assert (host(d_c) == SENTINEL).all()
