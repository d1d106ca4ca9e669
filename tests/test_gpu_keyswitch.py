"""Every key-switch kernel on worst-case keys and digits: k_ks_gemm<2,2>, k_keyswitch_fp<8,2,8>, k_keyswitch_lanes<8,2,8>,
k_keyswitch_lanes<8,1,4> and k_keyswitch<8> are exact only because of a stated bound on what their accumulators hold (int32 per
limb plane, FP64 between folds, 64- and 32-bit integer sums), and honest keys and ciphertexts stay orders of magnitude below all of
them.  Here the key comes in through import_keys with its mask columns PLANTED (tests/helpers.py: planted_keys -- a key row's body
is recomputed from its mask, so any mask makes a valid key) and the ciphertext rows hold every digit at either end of its range
(planted_rows); tests/test_keyswitch_reference.py shows on the CPU that these inputs reach at least half of every stated bound, that
the reference used here (the C oracle's key switch, rounded and packed by the restatement of tests/test_gpu_compact.py) is the
definition on Python integers, and that the tuned key words put switched words of the stress rows exactly on rounding boundaries of
the 31-bit fields, where an error of one unit in a sum shows.

Per parameter set of helpers.KS_SETS (each admitted by the selection harness, none replaced), key (planted, mirrored), knob setting
and batch size, fbs_compact_dev at 31 and at log2(2N) bits equals the reference word for word, on the kernel the launcher was
meant to take.  Then the stress rows through a whole bootstrap, and scratch and key rebuilds on re-import."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import KS_SETS, ks_fp_words_per_fold, ks_gemm_admitted, ks_set, planted_keys, planted_rows
from tests.test_gpu_compact import KNOBS, compact_on_device, pack, round_fields

pytestmark = pytest.mark.gpu

ROWS = 131                                           # one full 128-row tile and a ragged one; every tile holds every row pattern
COUNTS = (1, 31, 33, 64, 65, 131)                    # k_keyswitch<8>; lanes<8,1,4>; fp / lanes<8,2,8>
GEMM_COUNTS = (1, 33, 131)
_MADE = {}


def made(name):
    """(context with honest keys, its exported keys, oracle, rows, {mirrored: (planted key dict, switched rows by the oracle)})"""
    if name not in _MADE:
        from tfhe_fbs_map_amd import Context, Params
        prm = ks_set(name)
        ctx = Context(Params(**prm), seed=11)
        honest_keys = ctx.export_keys()
        o = orc.Oracle(prm, seed=11, keygen=False)
        rows = planted_rows(prm, ROWS, ctx.encrypt(np.arange(ROWS // 6 + 1) % prm["p_msg"], nonce0=40))
        planted = {}
        for mirrored in (False, True):
            keys, _ = planted_keys(honest_keys, prm, mirrored=mirrored)
            o.set_keys(**keys)
            planted[mirrored] = (keys, np.stack([o.keyswitch(r) for r in rows]))
        o.set_keys(**honest_keys)
        ctx.profile(True)
        _MADE[name] = (ctx, honest_keys, o, rows, planted)
    return _MADE[name]


def expected_kernel(prm, knobs, count):
    """select_keyswitch, restated"""
    if knobs.get("ks_mfma", 1) and ks_gemm_admitted(prm):
        return "k_ks_gemm<2,2> (int8 MFMA)"
    if count < 32:
        return "k_keyswitch<8>"
    if count <= 64:
        return "k_keyswitch_lanes<8,1,4>"
    return "k_keyswitch_fp<8,2,8>" if knobs.get("ks_fp", 1) and ks_fp_words_per_fold(prm) >= 1 else "k_keyswitch_lanes<8,2,8>"


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name", list(KS_SETS))
def test_every_kernel_on_planted_keys_and_rows(name, mirrored):
    ctx, honest_keys, _, rows, planted = made(name)
    prm = ks_set(name)
    keys, switched = planted[mirrored]
    widths = (31, prm["log_n_poly"] + 1)
    want = {bits: pack(round_fields(switched, bits), bits) for bits in widths}
    ran = set()
    try:
        ctx.import_keys(**keys)
        for knobs in KNOBS:
            ctx.tune(**{**dict(ks_mfma=1, ks_fp=1), **knobs})
            kernel_of = {count: expected_kernel(prm, knobs, count) for count in COUNTS}
            counts = GEMM_COUNTS if len(set(kernel_of.values())) == 1 else COUNTS
            for count in counts:
                for bits in widths:
                    ctx.profile_read(reset=True)
                    got = compact_on_device(ctx, rows[:count], bits)
                    assert ctx.profile_read()["keyswitch"]["kernel"] == kernel_of[count], (name, mirrored, knobs, count)
                    bad = np.argwhere(got != want[bits][:count])
                    assert got.shape == want[bits][:count].shape and bad.size == 0, (name, mirrored, knobs, count, bits, bad[:8].tolist())
                ran.add(kernel_of[count])
    finally:
        ctx.tune(ks_mfma=1, ks_fp=1)
        ctx.import_keys(**honest_keys)
    # what ran is what the set is for: the GEMM only where its digits fit an int8; FP64 only where a word fits between two folds
    assert ("k_ks_gemm<2,2> (int8 MFMA)" in ran) == (name != "g9")
    assert ("k_keyswitch_fp<8,2,8>" in ran) == (name not in ("g9", "g8_t2"))
    assert ran >= {"k_keyswitch<8>", "k_keyswitch_lanes<8,1,4>", "k_keyswitch_lanes<8,2,8>"}


@pytest.mark.parametrize("name", ["n4096", "g8_t1"])
def test_stress_rows_through_a_bootstrap(name):
    ctx, honest_keys, o, rows, planted = made(name)
    p = ks_set(name)["p_msg"]
    tables = [[(3 * m + 1) % (2 * p) for m in range(p)], [m % 2 for m in range(p)]]
    ids = (np.arange(36) % 2).astype(np.uint32)
    keys, _ = planted[False]
    try:
        ctx.import_keys(**keys)
        o.set_keys(**keys)
        got = ctx.bootstrap_batch(ctx.tvset(tables), rows[:36], ids)
        assert np.array_equal(got, o.bootstrap_batch(rows[:36], tables, ids)[0])
    finally:
        ctx.import_keys(**honest_keys)
        o.set_keys(**honest_keys)


@pytest.mark.parametrize("name", ["g9", "k3"])
def test_scratch_is_kept_and_reimported_keys_are_rebuilt(name):
    """after the planted keys: a second identical call allocates nothing, and the honest keys, imported again, give the honest outputs
    on every kernel -- the limb fragments, the FP64 copy and the correction vector all follow the key of the last import"""
    ctx, honest_keys, o, rows, planted = made(name)
    prm = ks_set(name)
    cts = ctx.encrypt(np.arange(ROWS) % prm["p_msg"], nonce0=500)
    want = pack(round_fields(np.stack([o.keyswitch(c) for c in cts]), 31), 31)
    try:
        ctx.import_keys(**planted[True][0])
        assert not np.array_equal(compact_on_device(ctx, cts, 31), want)          # another key: other words
        ctx.import_keys(**honest_keys)
        for knobs in KNOBS:
            ctx.tune(**{**dict(ks_mfma=1, ks_fp=1), **knobs})
            for count in (31, 64, ROWS):
                first = compact_on_device(ctx, cts[:count], 31)
                growths = ctx.stat("scratch_growths")
                assert np.array_equal(compact_on_device(ctx, cts[:count], 31), first) and ctx.stat("scratch_growths") == growths
                assert np.array_equal(first, want[:count]), (name, knobs, count)
    finally:
        ctx.tune(ks_mfma=1, ks_fp=1)
        ctx.import_keys(**honest_keys)
