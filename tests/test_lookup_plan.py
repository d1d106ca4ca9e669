"""`split.plan_lookup` and the two noise functions of params.py behind it (include/fbs_exec.h, "encrypted-index reads"), without a
GPU: every refusal with its text, the output's norm2 for one and two digits, the rounds of the cascade, and the default sets."""
import pytest

from tfhe_fbs_map_amd import params as P
from tfhe_fbs_map_amd.split import plan_lookup


@pytest.fixture(scope="module")
def default_set():
    prm = P.choose_params(15, 70, glwe_dims=(1, 2, 3))
    return prm, P.folded_state_factor(prm, *P.fold_choice(prm, 70, 6.0))


def plan(prm, ff, **over):
    args = dict(p=prm.p_msg, T_table=8, T_index=8, n_entries=prm.p_msg, digits=1, table_out_norm2=1.0, index_out_norm2=1.0, axis="rows")
    args.update(over)
    return plan_lookup(prm, ff, **args)


def test_the_noise_functions():
    assert P.lookup_output_norm2(1.0, 0.02) == pytest.approx(2.02)
    assert P.lookup_output_norm2(1.0, 0.02, digits=2) == pytest.approx(3.04)
    assert P.lookup_output_norm2(3.5, 0.0, digits=3) == pytest.approx(6.5)
    prm = P.choose_params(15, 70, glwe_dims=(1, 2, 3))
    for o2 in (1.0, 2.02, 70.0):
        assert P.lookup_index_margin(prm, o2) == P.refresh_margin(prm, None, o2)


def test_out_norm2_for_one_and_two_digits(default_set):
    prm, ff = default_set
    p = prm.p_msg
    assert plan(prm, ff) == ([1], pytest.approx(1.0 + ff + 1.0))
    rounds, o2 = plan(prm, ff, n_entries=p + 2, digits=2)
    assert rounds == [2, 1] and o2 == pytest.approx(1.0 + 2 * (ff + 1.0)) and o2 == P.lookup_output_norm2(1.0, ff, 2)
    assert plan(prm, ff, table_out_norm2=[1.0, 3.0])[1] == pytest.approx(3.0 + ff + 1.0)      # per-row factors: the largest counts


def test_round_counts(default_set):
    prm, ff = default_set
    p = prm.p_msg
    assert plan(prm, ff, n_entries=1)[0] == [1]
    assert plan(prm, ff, n_entries=p)[0] == [1]
    assert plan(prm, ff, n_entries=p + 1, digits=2)[0] == [2, 1]
    assert plan(prm, ff, n_entries=p * p, digits=2)[0] == [p, 1]
    assert plan(prm, ff, n_entries=p, digits=2)[0] == [1, 1]
    assert plan(prm, ff, n_entries=p * p + 1, digits=3)[0] == [p + 1, 2, 1]


def test_every_refusal_says_why(default_set):
    prm, ff = default_set
    p = prm.p_msg
    for over, text in ((dict(n_entries=0), "at least one entry"),
                       (dict(n_entries=p + 1), "%d entries are more than 1 digit(s) base %d name (%d)" % (p + 1, p, p)),
                       (dict(n_entries=p * p + 1, digits=2), "more than 2 digit(s)"),
                       (dict(digits=0), "at least one digit"),
                       (dict(T_table=4), "neither shared (1) nor the index's own (8)"),
                       (dict(axis="samples", T_table=8, n_entries=7), "along the samples a table is its state's 8 samples"),
                       (dict(axis="samples", T_table=p + 1, n_entries=p + 1, digits=2), "at most p = %d" % p),
                       (dict(axis="columns"), "neither 'rows' nor 'samples'"),
                       (dict(index_out_norm2=1e6), "the index would be read at"),
                       (dict(table_out_norm2=1e6), "the entry read would refresh at"),
                       (dict(min_margin=1e3), "the index would be read at")):
        with pytest.raises(ValueError) as e:
            plan(prm, ff, **over)
        assert text in str(e.value), (over, str(e.value))
    with pytest.raises(ValueError) as e:
        plan(prm, None)
    assert "no fold key" in str(e.value)
    assert plan(prm, ff, T_table=1)[0] == [1]                                                 # a shared table
    assert plan(prm, ff, axis="samples", T_table=p, n_entries=p)[0] == [1]                   # ... and one along the samples


@pytest.mark.parametrize("p,norm2", [(15, 70), (8, 30), (4, 10)])
def test_a_bootstrap_output_table_read_by_a_bootstrap_output_index_is_accepted(p, norm2):
    prm = P.choose_params(p, norm2, glwe_dims=(1, 2, 3))
    ff = P.folded_state_factor(prm, *P.fold_choice(prm, norm2, 6.0))
    rounds, o2 = plan_lookup(prm, ff, p, 1000, 1000, p, 1, 1.0, 1.0, "rows")
    assert rounds == [1] and o2 == pytest.approx(2.0 + ff) and ff < 0.03
    assert P.lookup_index_margin(prm, 1.0) >= P.refresh_margin_needed(prm, 1.0) and P.refresh_margin(prm, None, o2) >= P.SET_MARGIN == 6.0
    # (the output against the margin of norm2 = 1 itself could never pass: a fold and a rotation more than a bootstrap output)
    assert P.refresh_margin(prm, None, o2) < P.refresh_margin_needed(prm, 1.0)
