"""The frame every blind-rotation kernel takes from csrc/fbs_blind_rotate.hpp -- br_job (which bootstrap a thread works on: the
ragged last workgroup, the clamp of device-side table ids), br_acc_init, br_rounding, br_extract (sample extraction, and the whole
accumulator of a shared rotation) -- through ONE instantiation of each of the seven kernels, on toy keys (n = 8), word for word
against the CPU oracle.  tests/helpers.py:recipe gives the parameter set, count and knobs that reach each instantiation
(tests/test_select.py checks that on the CPU); here the per-kernel profile table confirms that it ran.

Two cases per kernel:

* a launch through the device-pointer entry with table ids the host cannot validate (n_tables, 1000, 0xFFFFFFFF, the last of them
  on the last bootstrap, which a ragged workgroup repeats) and, wherever a workgroup holds two bootstraps, an odd count: the
  outputs are the oracle's with those ids read as table 0, and the rows behind the last one of an over-allocated buffer are untouched;
* the fused toy program of tests/test_gpu_fusion.py (T = 8), whose shared rotations leave their whole accumulator through the
  gate_acc branch of br_extract, against oracle_eval_program(..., fuse=True).  Its two levels hold 16 and 8 rotations, and no knob
  makes a launch that small take two bootstraps per workgroup in k_blind_rotate and k_blind_rotate_pairs_k2: there the selection
  gives the program to the one-bootstrap-per-workgroup instantiation of the same kernel (FUSED_KERNEL below: the same source, the
  same br_extract call).  Shared rotations in workgroups of several bootstraps are covered by
  tests/test_gpu_fusion.py::test_shared_rotations_in_a_level_longer_than_a_round (k_blind_rotate<10,6,3,4>); k_blind_rotate_glwe is
  held at two per workgroup by br_glwe_fpw."""
import numpy as np
import pytest

from oracle import lut_oracle, tfhe_oracle as orc
from tests.helpers import oracle_eval_program, recipe
from tests.test_gpu_fusion import MULTI, load

pytestmark = pytest.mark.gpu

TABLES = [[0, 1, 1, 0, 1, 0, 0], [0, 1, 2, 3, 2, 1, 0], [0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1]]
KERNELS = ["k_blind_rotate<8,6,3,2>", "k_blind_rotate_pairs<10,6,4>", "k_blind_rotate_cu<10,3,2>", "k_blind_rotate_cu_pairs<11,1>",
           "k_blind_rotate_pairs_k2<10,2>", "k_blind_rotate_cu_k2", "k_blind_rotate_glwe<8,3,1,2>"]
# knobs beyond the recipe's (they change no launch of the recipe's own count), and what the fused program's small levels reach
EXTRA_KNOBS = {"k_blind_rotate_glwe<8,3,1,2>": dict(br_glwe_fpw=2)}
FUSED_KERNEL = {"k_blind_rotate<8,6,3,2>": "k_blind_rotate<8,6,3,1>", "k_blind_rotate_pairs_k2<10,2>": "k_blind_rotate_pairs_k2<10,1>"}
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


def case_of(name):
    """-> (parameter set, count, knobs): the recipe's, the parameters as tests/test_gpu_dispatch.py:run_case makes them, the count odd"""
    from tfhe_fbs_map_amd import Params
    rec = recipe(name)
    prm = Params(n=8, log_n_poly=rec["log_n"], k=rec.get("k", 1), l_bsk=rec["l"], beta_bsk=rec["beta"], t_ksk=4, gamma_ksk=4, p_msg=7,
                 sigma_lwe=1 << 6, sigma_glwe=1 << 4, bsk_group=rec["group"])
    return prm, rec["count"] | 1, dict(rec["knobs"], **EXTRA_KNOBS.get(name, {}))


@pytest.mark.parametrize("name", KERNELS)
def test_ragged_launch_with_wild_device_side_table_ids(name):
    import torch
    from tfhe_fbs_map_amd import _native as nat
    prm, count, knobs = case_of(name)
    ctx, o = nat.Context(prm, seed=21), orc.Oracle(prm, seed=21)
    ctx.tune(**knobs)
    rng = np.random.default_rng(count)
    ids = rng.integers(0, len(TABLES), count).astype(np.uint32)
    msgs = np.array([rng.integers(0, len(TABLES[i])) for i in ids])
    wild = {1: len(TABLES), count // 2: 1000, count - 1: 0xFFFFFFFF}
    for at, v in wild.items():
        ids[at] = v
        msgs[at] %= len(TABLES[0])
    cts = ctx.encrypt(msgs, nonce0=3)
    d_in = torch.from_numpy(cts.view(np.int64)).cuda()
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_out = torch.full((count + 2, prm.ct_words), UNTOUCHED, dtype=torch.int64, device="cuda")
    ctx.profile(True)
    ctx.profile_read(reset=True)
    ctx.bootstrap_batch_dev(ctx.tvset(TABLES), d_in.data_ptr(), d_ids.data_ptr(), count, d_out.data_ptr())
    ctx.sync()
    launched = ctx.profile_kernels()
    assert name in launched, (name, sorted(launched))
    got = d_out.cpu().numpy().view(np.uint64)
    read_as = np.where(ids < len(TABLES), ids, 0).astype(np.uint32)
    ref, _ = o.bootstrap_batch(cts, TABLES, read_as)
    assert np.array_equal(got[:count], ref), name
    assert (got[count:] == UNTOUCHED).all(), name
    ctx.close()


@pytest.mark.parametrize("name", KERNELS)
def test_shared_rotations_leave_their_accumulator(name):
    from tfhe_fbs_map_amd import _native as nat
    prm, _, knobs = case_of(name)
    T = 8
    ctx, low, tv, prog = load(nat, prm, MULTI, ["a", "b", "c"])
    ctx.tune(**knobs)
    assert (prog.n_bootstrap, prog.n_rotations) == (7, 3)
    bits = np.random.default_rng(5).integers(0, 2, (3, T))
    cts = ctx.encrypt(bits, nonce0=2)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = prog.eval(cts, T)
    launched = ctx.profile_kernels()
    assert FUSED_KERNEL.get(name, name) in launched, (name, sorted(launched))
    ops, outs = lut_oracle.read_fbs(MULTI)
    wires = oracle_eval_program(orc.Oracle(prm, seed=6), ops, outs, {n: cts[i] for i, n in enumerate(low["input_names"])}, fuse=True)
    for k, (out_name, src) in enumerate(outs):
        assert np.array_equal(got[k], wires[src]), (name, out_name)
    ctx.close()
