"""The pure Python of the sample-axis operations, on stand-in `ResidentOutputs` (no device): `plan_chain` takes a `SampleView` with
its own T under the names it gives its rows, attaches the map and the fill to the link and applies the full-link refresh rule by
the state's out_norm2; the index arrays of shift, broadcast and stride are what their definitions say; the arithmetic of
`sum_groups` and its refusal; the name check of `Server.fold`."""
import types

import numpy as np
import pytest

from tests.test_chain_abi import A_FROM_S, _adder, _key_params, _sources

NONE = 0xFFFFFFFF
NAMES = [f"s{i}" for i in range(8)] + ["cout"]


class _StubState:
    """stands for a DeviceState: asked whether it is closed, and for its group sums"""

    def __init__(self, closed=False):
        self.closed, self.summed = closed, []

    def sum_groups(self, group):
        self.summed.append(group)
        return _StubState()


def _resident(T=6, fp=bytes(8), out_norm2=1.0, closed=False, p=15):
    from tfhe_fbs_map_amd.split import ResidentOutputs
    server = types.SimpleNamespace(key=types.SimpleNamespace(params=types.SimpleNamespace(p_msg=p)))
    return ResidentOutputs(NAMES, T, fp, None if out_norm2 is None else np.full(9, float(out_norm2)), _StubState(closed), server)


def _setup():
    env = _adder()
    prm, fuse = _key_params(env)
    _, fresh = _sources(prm)          # seeded b0..b7 at T = 4
    return env, prm, fuse, fresh


def test_a_view_counts_with_its_own_T_and_carries_its_map():
    from tfhe_fbs_map_amd.split import SampleView, plan_chain
    env, prm, fuse, fresh = _setup()
    res = _resident(T=6)
    index = [5, 5, NONE, 0]
    view = res.samples(index, fill={"s3": 1})
    assert isinstance(view, SampleView) and view.T == 4 and res.T == 6
    assert view.fingerprint == res.fingerprint and view.out_norm2 is res.out_norm2 and view.output_names == NAMES
    links, T = plan_chain(prm, fuse, bytes(8), env, [view, fresh], rename=A_FROM_S)
    assert T == 4
    for i in range(8):
        ln = links[i]
        assert (ln.kind, ln.source, ln.index, ln.refresh, ln.noise) == ("state", 0, i, False, 1.0)
        assert ln.sample_index.dtype == np.uint32 and ln.sample_index.tolist() == index and ln.fill == (1 if i == 3 else 0)
        assert (links[8 + i].kind, links[8 + i].sample_index, links[8 + i].fill) == ("seeded", None, 0)
    # the unmapped state keeps links without a map, and its own T rule with its old message
    with pytest.raises(ValueError, match="T = 4 samples where the others have 6"):
        plan_chain(prm, fuse, bytes(8), env, [res, fresh], rename=A_FROM_S)
    plain, _ = plan_chain(prm, fuse, bytes(8), env, [_resident(T=4), fresh], rename=A_FROM_S)
    assert all(ln.sample_index is None and ln.fill == 0 for ln in plain)


def test_view_refusals():
    from tfhe_fbs_map_amd.split import plan_chain
    env, prm, fuse, fresh = _setup()
    res = _resident(T=6)
    with pytest.raises(ValueError, match="source 1 has T = 4 samples where the others have 5"):
        plan_chain(prm, fuse, bytes(8), env, [res.samples([0] * 5), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="sample 1 reads sample 6 of a state of 6"):
        res.samples([0, 6, 1, 2])
    with pytest.raises(ValueError, match="at least one"):
        res.samples([])
    with pytest.raises(ValueError, match="not rows of the state"):
        res.samples([0], names={"nope": "x"})
    with pytest.raises(ValueError, match="not rows of the state"):
        res.samples([0], fill={"nope": 1})
    with pytest.raises(ValueError, match="one name"):
        res.samples([0], names={"s0": "s1"})
    with pytest.raises(ValueError, match=r"fill %d outside \[0, 2p\)" % (2 * prm.p_msg)):
        plan_chain(prm, fuse, bytes(8), env, [res.samples([0] * 4, fill=2 * prm.p_msg), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="closed"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(closed=True).samples([0] * 4), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="another server key"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(fp=bytes(range(8))).samples([0] * 4), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="saved without out_norm2"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(out_norm2=None).samples([0] * 4), fresh], rename=A_FROM_S)


def test_two_views_of_one_state_are_ambiguous_until_renamed():
    from tfhe_fbs_map_amd.split import plan_chain
    env, prm, fuse, _ = _setup()
    res = _resident(T=5)
    even, odd = [0, 2, 4], [1, 3, NONE]
    b_from_s = {f"b{i}": f"s{i}" for i in range(8)}
    with pytest.raises(ValueError, match="input a0 \\(as s0\\): ambiguous, held by sources \\[0, 1\\]"):
        plan_chain(prm, fuse, bytes(8), env, [res.samples(even), res.samples(odd)], rename={**A_FROM_S, **b_from_s})
    right = res.samples(odd, fill=1, names={n: n + "@r" for n in NAMES})
    assert right.output_names == [n + "@r" for n in NAMES]
    links, T = plan_chain(prm, fuse, bytes(8), env, [res.samples(even), right],
                          rename={**A_FROM_S, **{f"b{i}": f"s{i}@r" for i in range(8)}})
    assert T == 3
    for i in range(8):
        assert (links[i].source, links[i].index, links[i].sample_index.tolist(), links[i].fill) == (0, i, even, 0)
        assert (links[8 + i].source, links[8 + i].index, links[8 + i].sample_index.tolist(), links[8 + i].fill) == (1, i, odd, 1)


def test_the_refresh_rule_goes_by_the_carried_out_norm2():
    from tfhe_fbs_map_amd.split import plan_chain
    env, prm, fuse, fresh = _setup()
    for o2, refresh in ((1.0, False), (0.0, False), (2.0, True), (7.0, True)):
        view = _resident(T=9, out_norm2=o2).samples([8, 7, 6, 5])
        links, _ = plan_chain(prm, fuse, bytes(8), env, [view, fresh], rename=A_FROM_S)
        same, _ = plan_chain(prm, fuse, bytes(8), env, [_resident(T=4, out_norm2=o2), fresh], rename=A_FROM_S)
        for a, b in zip(links[:8], same[:8]):
            assert (a.refresh, a.noise, a.margin) == (b.refresh, b.noise, b.margin) and a.refresh == refresh, o2
            assert (a.margin is not None) == refresh and a.sample_index is not None and b.sample_index is None
    with pytest.raises(ValueError, match="refresh would keep"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(T=9, out_norm2=1e4).samples([0] * 4), fresh], rename=A_FROM_S)


def test_shift_broadcast_and_stride_are_their_definitions():
    from tfhe_fbs_map_amd.split import shift_index
    res = _resident(T=7)
    for d in (-8, -7, -2, -1, 0, 1, 3, 6, 7, 9):
        want = [s - d if 0 <= s - d < 7 else NONE for s in range(7)]
        view = res.shift(d, fill=1)
        assert view.index.tolist() == want and view.T == 7 and view.fill == [1] * 9, d
        assert shift_index(7, d).tolist() == want and shift_index(7, d).dtype == np.uint32
    assert res.shift(1).fill == [0] * 9
    view = res.broadcast(4, 11)
    assert view.T == 11 and view.index.tolist() == [4] * 11
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            res.broadcast(bad, 3)
    for start, step in ((0, 1), (0, 2), (1, 2), (2, 3), (6, 1), (3, 100)):
        view = res.stride(start, step)
        assert view.index.tolist() == list(range(start, 7, step)) and view.T == len(range(start, 7, step))
    for start, step in ((7, 1), (-1, 1), (0, 0)):
        with pytest.raises(ValueError):
            res.stride(start, step)
    assert res.stride(1, 2, names={"s0": "x"}).output_names[0] == "x"


def test_sum_groups_arithmetic_and_refusal():
    from tfhe_fbs_map_amd.split import ResidentOutputs, plan_sum_groups
    n2 = np.array([1.0, 0.0, 0.5])
    for T, group, want_T in ((28, 7, 4), (37, 7, 6), (37, 1, 37), (37, 37, 1), (5, 14, 1), (4101, 4096, 2)):
        p = 15 if group <= 14 else 2 * 65536
        T2, out = plan_sum_groups(p, T, group, 1, n2)
        assert T2 == want_T and np.array_equal(out, n2 * group), (T, group)
    assert plan_sum_groups(15, 10, 2, 7)[1] is None                      # 2 * 7 = 14 = p - 1, no noise recorded
    assert plan_sum_groups(15, 10, 14, 0) == (1, None)
    for p, group, max_value in ((15, 15, 1), (15, 2, 8), (15, 8, 2), (7, 7, 1), (2, 2, 1)):
        with pytest.raises(ValueError, match="above p - 1 = %d" % (p - 1)):
            plan_sum_groups(p, 30, group, max_value)
    for group in (0, -1, 65537):
        with pytest.raises(ValueError, match=r"outside \[1, 65536\]"):
            plan_sum_groups(1 << 20, 30, group, 0)
    # the method: the plan first, then the state's sums, under the same names and key, with no default widths
    res = _resident(T=28, out_norm2=0.5, p=15)
    out = res.sum_groups(7)
    assert isinstance(out, ResidentOutputs) and out.T == 4 and out.output_names == NAMES and out.fingerprint == res.fingerprint
    assert np.array_equal(out.out_norm2, np.full(9, 3.5)) and out.compact_bits is None and out.packed_bits is None
    assert res.state.summed == [7] and out.state is not res.state and out.server is res.server
    with pytest.raises(ValueError, match="above p - 1 = 14"):
        res.sum_groups(15)
    with pytest.raises(ValueError, match="above p - 1 = 14"):
        res.sum_groups(5, max_value=3)
    assert res.state.summed == [7]
    with pytest.raises(ValueError, match="closed"):
        _resident(closed=True).sum_groups(2)


def test_summed_outputs_are_refreshed_by_a_chain_that_reads_them():
    from tfhe_fbs_map_amd.split import plan_chain
    env, prm, fuse, fresh = _setup()
    summed = _resident(T=8, out_norm2=1.0, p=prm.p_msg).sum_groups(2)
    links, T = plan_chain(prm, fuse, bytes(8), env, [summed, fresh], rename=A_FROM_S)
    assert T == 4 and all(ln.refresh and ln.noise == 1.0 and ln.margin is not None for ln in links[:8])


def test_fold_checks_its_names_up_front():
    from tfhe_fbs_map_amd.split import Server, fold_plan
    env = _adder()
    low = env.lower()
    left, right = dict(A_FROM_S), {f"b{i}": f"s{i}" for i in range(8)}
    got = fold_plan(low, NAMES, left, right)
    assert got == (left, right, {})
    with pytest.raises(ValueError, match=r"the state holds no rows \['s7'\]"):
        fold_plan(low, NAMES[:7] + ["cout"], left, right)
    with pytest.raises(ValueError, match="left and right feed inputs"):
        fold_plan(low, NAMES, left, {k: v for k, v in right.items() if k != "b3"})
    with pytest.raises(ValueError, match=r"\['a0'\] in both"):
        fold_plan(low, NAMES, left, {**right, "a0": "s0"})
    with pytest.raises(ValueError, match=r"back names \['nope'\]"):
        fold_plan(low, NAMES, left, right, {"nope": "s0"})
    # a back that renames a row away: the second round could not find it
    with pytest.raises(ValueError, match=r"renamed through back holds no rows \['s0'\]"):
        fold_plan(low, NAMES, left, right, {"s0": "t0"})
    with pytest.raises(ValueError, match="two outputs one name"):
        fold_plan(low, NAMES, left, right, {"s0": "s1"})
    # rows under other names in the state, and a back that maps the outputs onto them
    rows = [f"acc{i}" for i in range(8)]
    l2, r2 = {f"a{i}": rows[i] for i in range(8)}, {f"b{i}": rows[i] for i in range(8)}
    back = {f"s{i}": rows[i] for i in range(8)}
    assert fold_plan(low, rows, l2, r2, back) == (l2, r2, back)
    with pytest.raises(ValueError, match="renamed through back holds no rows"):
        fold_plan(low, rows, l2, r2)
    # Server.fold makes the check before it touches the server or the GPU
    server = Server.__new__(Server)
    state = _resident(T=5)
    with pytest.raises(ValueError, match=r"renamed through back holds no rows \['s0'\]"):
        server.fold(env, state, left, right, back={"s0": "t0"})
