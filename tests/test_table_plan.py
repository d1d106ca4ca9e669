"""`split.plan_table` and the two noise functions of params.py behind it (include/fbs_exec.h, "encrypted tables"), without a GPU:
every admission, every refusal with its text, the bounds and the norm2 bookkeeping through a run of writes."""
import pytest

from tfhe_fbs_map_amd import params as P
from tfhe_fbs_map_amd.split import plan_table


@pytest.fixture(scope="module")
def default_set():
    prm = P.choose_params(15, 70, glwe_dims=(1, 2, 3))
    return prm, P.folded_state_factor(prm, *P.fold_choice(prm, 70, 6.0))


def plan(prm, ff, op, **over):
    args = dict(spread=2, n_entries=prm.p_msg // 2, T_table=8, T_index=8, table_norm2=1.0 + ff, index_out_norm2=1.0, written=False,
                value_norm2=1.0, table_max=1, value_max=1)
    args.update(over)
    return plan_table(prm, ff, op, **args)


def test_the_noise_functions():
    assert P.table_write_norm2(1.5, 1.0, 0.02) == pytest.approx(3.52)
    assert P.table_write_norm2(1.5, 1.0, 0.02, P.TABLE_SET) == pytest.approx(4.52)
    assert P.table_write_norm2(0.0, 0.0, 0.0, P.TABLE_ADD) == 1.0 and P.table_read_norm2(3.52) == pytest.approx(4.52)
    assert (P.TABLE_ADD, P.TABLE_SET) == (0, 1)


def test_create_read_and_writes_keep_the_books(default_set):
    prm, ff = default_set
    p = prm.p_msg
    made = plan(prm, ff, "create", table_norm2=[1.0, 1.0], table_max=2)
    assert made == dict(norm2=pytest.approx(1.0 + ff), max_value=2, out_norm2=None)
    read = plan(prm, ff, "read", table_norm2=made["norm2"])
    assert read["out_norm2"] == pytest.approx(2.0 + ff) and read["norm2"] == made["norm2"]
    norm2, bound, fold = made["norm2"], 2, ff
    for turn in range(3):                                                        # three adds of values up to 3
        w = plan(prm, ff, "add", table_norm2=norm2, table_max=bound, value_max=3, written=turn > 0)
        assert w["norm2"] == pytest.approx(norm2 + 1.0 + fold + 1.0) and w["max_value"] == bound + 3 and w["out_norm2"] is None
        norm2, bound = w["norm2"], w["max_value"]
    assert bound == 11 <= p - 1
    s = plan(prm, ff, "set", table_norm2=norm2, table_max=bound, value_max=5, written=True)
    assert s["norm2"] == pytest.approx(norm2 + 1.0 + fold + 2.0) and s["max_value"] == 5                  # a set REPLACES the bound
    assert plan(prm, ff, "add", T_table=1, T_index=1)["max_value"] == 2                                  # a shared table, one writer
    assert plan(prm, ff, "read", T_table=1, T_index=1000)["out_norm2"] == pytest.approx(2.0 + ff)        # ... and any number of readers


def test_the_index_margin_rule(default_set):
    prm, ff = default_set
    m = P.lookup_index_margin(prm, 1.0)
    need = P.refresh_margin_needed(prm, 1.0)
    assert m >= need > m / 2                                                     # one box admits a read and no more: halving is no option
    # spread 2: a write and a read of a written table stand where a read of an ordinary table stands; an unwritten one has twice that
    assert plan(prm, ff, "add") and plan(prm, ff, "read", written=True) and plan(prm, ff, "read")
    for op, over in (("add", dict(spread=1, n_entries=3)), ("set", dict(spread=1, n_entries=3)), ("read", dict(spread=1, n_entries=3, written=True))):
        with pytest.raises(ValueError, match="the index would be read at %.2f standard deviations" % (m / 2)):
            plan(prm, ff, op, **over)
    assert plan(prm, ff, "read", spread=1, n_entries=3)                          # never written: the ordinary read
    assert plan(prm, ff, "add", spread=1, n_entries=3, min_margin=m / 2)         # a caller's own margin stands in
    noisy = 3.5                                                                  # an index that a bare read refuses, an unwritten wide table takes
    assert P.lookup_index_margin(prm, noisy) < need <= 2 * P.lookup_index_margin(prm, noisy)
    assert plan(prm, ff, "read", index_out_norm2=noisy)
    with pytest.raises(ValueError, match="the index would be read at"):
        plan(prm, ff, "read", index_out_norm2=noisy, written=True)


def test_every_refusal_says_why(default_set):
    prm, ff = default_set
    p = prm.p_msg
    for op, over, text in (("create", dict(spread=0), "at least one box"),
                           ("create", dict(n_entries=0), "at least one entry"),
                           ("create", dict(n_entries=p // 2 + 1), "%d entries of 2 boxes each are more than p = %d boxes hold (%d)" % (p // 2 + 1, p, p // 2)),
                           ("read", dict(spread=3, n_entries=p // 3 + 1), "more than p"),
                           ("read", dict(T_index=4), "an index of 4 samples for tables of 8"),
                           ("add", dict(T_index=4), "an index of 4 samples for tables of 8"),
                           ("add", dict(T_table=1, T_index=8), "a shared table is written by an index of one sample, not 8"),
                           ("set", dict(T_table=1, T_index=8), "a shared table is written by an index of one sample"),
                           ("add", dict(index_out_norm2=1e6), "the index would be read at"),
                           ("read", dict(table_norm2=1e6), "the entry read would refresh at"),
                           ("add", dict(table_max=p - 3, value_max=3), "a sum of entries up to %d and values up to 3 reaches %d, above p - 1 = %d" % (p - 3, p, p - 1)),
                           ("set", dict(value_max=p), "reaches %d, above p - 1" % p),
                           ("add", dict(value_max=-1), "is negative"),
                           ("add", dict(value_max=None), "needs the bounds"),
                           ("add", dict(table_norm2=1e6), "noise budget is spent -- make a new server.table(...) of the refreshed entries()"),
                           ("set", dict(table_norm2=1e6), "noise budget is spent"),
                           ("write", dict(), "none of 'create', 'read', 'add', 'set'")):
        with pytest.raises(ValueError) as e:
            plan(prm, ff, op, **over)
        assert text in str(e.value), (op, over, str(e.value))
    for op in ("create", "read", "add", "set"):
        with pytest.raises(ValueError, match="no fold key"):
            plan_table(prm, None, op, 2, 3, 8, 8, table_max=1, value_max=1)
    assert plan(prm, ff, "add", table_max=p - 4, value_max=3)["max_value"] == p - 1          # the bound itself is admitted


def test_the_budget_runs_out_after_a_number_of_writes(default_set):
    """adds until plan_table says stop: the count is what SET_MARGIN leaves, more than a handful, and the refusal names the cure"""
    prm, ff = default_set
    norm2, writes = 1.0 + ff, 0
    while True:
        try:
            norm2 = plan(prm, ff, "add", table_norm2=norm2, table_max=0, value_max=0, written=writes > 0)["norm2"]
        except ValueError as e:
            assert "server.table(...)" in str(e)
            break
        writes += 1
        assert writes < 1000
    assert P.refresh_margin(prm, None, P.table_read_norm2(norm2)) >= P.SET_MARGIN
    assert P.refresh_margin(prm, None, P.table_read_norm2(P.table_write_norm2(norm2, 1.0, ff))) < P.SET_MARGIN
    assert writes >= 3, writes
