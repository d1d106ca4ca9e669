"""The compact format's kernels (k_compact_pack, k_compact_unpack, k_decrypt_compact; csrc/fbs_compact.hip) at real key sizes and on
planted rounding boundaries.  tests/test_gpu_compact.py and tests/test_gpu_chain.py compare them word for word at n = 12, where
one pack round, one pass of 64 lanes and a 32-bit sum that never wraps is all that runs; here n = 64, 65, 734 and 4096
(helpers.COMPACT_WIDE_SETS: N = 256, so 9 bits is the narrowest width), and the inputs are CHOSEN:

* pack: the key-switching key comes in through import_keys with a few rows planted (helpers.planted_switch), so that the key switch
  of a one-word ciphertext is exactly a target row -- every mask word the last that rounds down, the first that rounds up, q - 1,
  one below a step (an odd negative error sum), and a body that puts x_n - floor(eps / 2) on a rounding boundary, one either side,
  on 0 and on q - 1.  fbs_compact_dev equals the definition on Python integers, on every key-switch family, alone and mixed with
  honest encryptions;
* unpack: the same patterns as fields, for the re-rounding from w to 9 bits; fbs_compact_fields_dev equals the definition;
* decode: every mask field 2^w - 1 (the sum wraps 2^32 up to 1022 times), zero masks, the phase on every boundary between two
  messages for p = 7 and p = 4096, random fields; host and device decodes equal the definition;
* the grid-stride loops of unpack and decode, entered above 262 144 ciphertexts;
* the refresh of compact ciphertexts at n = 734 against the bootstrap through the identity table.

tests/test_compact_reference.py checks without a GPU that the planted inputs are what they claim and that the numpy
restatements used for the large cases here equal the definitions."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import (COMPACT_PACK_WIDTHS, COMPACT_WIDE_SETS, Q, compact_definition, compact_target_rows, decode_case_batches,
                           decode_cases, decode_definition, lc_delta, load_fixture, planted_switch, reround_definition,
                           reround_field_rows)
from tests.test_gpu_chain import fields_on_device, refresh_on_device, reround
from tests.test_gpu_compact import KNOBS, compact_on_device, pack, unpack
from tests.test_gpu_keyswitch import expected_kernel

pytestmark = pytest.mark.gpu

B = 9                                                # log2(2N) of every set
UNPACK_WIDTHS = (9, 10, 23, 31)
DECODE_WIDTHS = (9, 23, 31)
HONEST = 64                                          # one block of honest encryptions beside the planted ciphertexts
GRID_COUNT = 262144 + 5                              # one more pass of the grid-stride loops (2^16 workgroups of four waves), ragged
SEED = 11
_MADE = {}


def made(name):
    """(context, its honest keys, oracle with the same keys, parameter dict) of a set, made once per module"""
    if name not in _MADE:
        from tfhe_fbs_map_amd import Context, Params
        prm = COMPACT_WIDE_SETS[name]
        ctx = Context(Params(**prm), seed=SEED)
        honest = ctx.export_keys()
        o = orc.Oracle(prm, seed=SEED, keygen=False)
        o.set_keys(**honest)
        ctx.profile(True)
        _MADE[name] = (ctx, honest, o, prm)
    return _MADE[name]


def as_u64(rows):
    return np.array([[int(v) for v in r] for r in rows], dtype=np.uint64)


def decode_fields(fields, sk, bits, two_p):
    """the decode restated in numpy, for the cases too many for Python integers: fields [count][n + 1] -> messages [count]"""
    f = np.asarray(fields, np.int64)
    phase = (f[:, -1] - (f[:, :-1] * np.asarray(sk, np.int64)).sum(axis=1)) % (1 << bits)      # (exact: n 2^31 < 2^63)
    return ((phase * two_p + (1 << (bits - 1))) >> bits) % two_p


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_pack_of_planted_switches_is_the_definition(name):
    """(k_compact_pack's own grid cap of 2^22 workgroups a launch is out of reach of a test: 4 million ciphertexts)"""
    ctx, honest, o, prm = made(name)
    n = prm["n"]
    ordinary = ctx.encrypt(np.arange(HONEST) % (2 * prm["p_msg"]), nonce0=7000)
    ran = set()
    try:
        for bits in COMPACT_PACK_WIDTHS:
            rows = compact_target_rows(n, bits)
            keys, planted = planted_switch(honest, prm, [r for r, _ in rows.values()], [b for _, b in rows.values()], oracle=o)
            cts = np.concatenate([planted, ordinary])
            x = [o.keyswitch(c) for c in cts]                                  # (the oracle holds the planted key now)
            assert [int(v) for r in x[:len(planted)] for v in r] == [int(v) for r, bs in rows.values() for b in bs for v in r + [b]]
            want = pack(as_u64([compact_definition(r, bits) for r in x]), bits)
            ctx.import_keys(**keys)
            for knobs in KNOBS:
                ctx.tune(**{**dict(ks_mfma=1, ks_fp=1), **knobs})
                for count in (1, len(planted), len(cts)):
                    ctx.profile_read(reset=True)
                    got = compact_on_device(ctx, cts[:count], bits)
                    kernel = ctx.profile_read()["keyswitch"]["kernel"]
                    assert kernel == expected_kernel(prm, knobs, count), (name, knobs, count)
                    ran.add(kernel)
                    bad = np.argwhere(got != want[:count])
                    assert got.shape == want[:count].shape and bad.size == 0, (name, bits, knobs, count, bad[:8].tolist())
    finally:
        ctx.tune(ks_mfma=1, ks_fp=1)
        ctx.import_keys(**honest)
        o.set_keys(**honest)
    assert ran == {"k_ks_gemm<2,2> (int8 MFMA)", "k_keyswitch<8>", "k_keyswitch_lanes<8,1,4>", "k_keyswitch_fp<8,2,8>",
                   "k_keyswitch_lanes<8,2,8>"}


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_unpack_of_planted_fields_is_the_definition(name):
    ctx, _, _, prm = made(name)
    n = prm["n"]
    for bits in UNPACK_WIDTHS:
        rows = [r for group in reround_field_rows(n, bits, B).values() for r in group]
        want = as_u64([reround_definition(r, bits, B) for r in rows])
        for count in (1, len(rows)):
            got = fields_on_device(ctx, pack(as_u64(rows[:count]), bits), bits)
            bad = np.argwhere(got != want[:count])
            assert got.shape == want[:count].shape and bad.size == 0, (name, bits, count, bad[:8].tolist())


@pytest.mark.parametrize("name", list(COMPACT_WIDE_SETS))
def test_decodes_on_planted_phases_are_the_definition(name):
    from tfhe_fbs_map_amd import Context, Params
    ctx7, honest, _, prm = made(name)
    n = prm["n"]
    sk = [int(s) for s in honest["sk_lwe"]]
    ctx4096 = Context(Params(**{**prm, "p_msg": 4096}), seed=SEED, keygen=False)   # the same keys, the widest message space
    ctx4096.import_keys(**honest)
    try:
        for ctx, p in ((ctx7, 7), (ctx4096, 4096)):
            for bits in DECODE_WIDTHS:
                for kind, words, want in decode_case_batches(decode_cases(n, sk, bits, 2 * p), sk, bits, 2 * p, pack):
                    on_host = ctx.decrypt_compact(words, bits, device=False)
                    on_dev = ctx.decrypt_compact(words, bits, device=True)
                    assert np.array_equal(on_dev, want), (name, p, bits, kind, np.argwhere(on_dev != want)[:8].tolist())
                    assert np.array_equal(on_host, want), (name, p, bits, kind, np.argwhere(on_host != want)[:8].tolist())
    finally:
        ctx4096.close()


def test_grid_stride_loops_of_unpack_and_decode():
    """more ciphertexts than 2^16 workgroups of four waves take in one pass: both loops go round again, the last pass ragged.
    (k_compact_pack has no such loop; its launcher splits above 2^22 workgroups, out of reach of a test.)"""
    ctx, honest, _, prm = made("n64")
    n, p = prm["n"], prm["p_msg"]
    sk = honest["sk_lwe"].astype(np.int64)
    rng = np.random.default_rng(64)
    words = rng.integers(0, 1 << 64, (GRID_COUNT, ctx.compact_words(B)), dtype=np.uint64)      # every bit random, the padding too
    fields = unpack(words, n, B)
    sample = [0, 1, 262143, 262144, GRID_COUNT - 1]
    assert [decode_definition(fields[i], sk, B, 2 * p) for i in sample] == [int(v) for v in decode_fields(fields[sample], sk, B, 2 * p)]
    got = fields_on_device(ctx, words, B)
    assert got.shape == fields.shape and np.array_equal(got, fields)
    assert np.array_equal(ctx.decrypt_compact(words, B, device=True), decode_fields(fields, sk, B, 2 * p))
    wide = rng.integers(0, 1 << 10, (GRID_COUNT, n + 1), dtype=np.uint64)
    want = reround(wide, n, 10, B)
    assert [int(v) for i in sample for v in want[i]] == [v for i in sample for v in reround_definition(wide[i], 10, B)]
    got = fields_on_device(ctx, pack(wide, 10), 10)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_refresh_at_a_real_key_size():
    """fbs_refresh_compact_dev of fbs_compact_dev at 9 bits is the bootstrap through the identity table word for word, and from 31
    bits it decrypts to the same messages (tests/test_gpu_chain.py at n = 12), at n = 734.  At this n and N = 256 the modulus switch
    alone moves a phase by up to a third of the distance between two messages, so the ciphertexts are chosen beforehand, by the
    definitions: those whose 9-bit phase lies within half of that distance's half (9 of 512) of its message on both paths."""
    ctx, honest, o, prm = made("n734")
    n, p = prm["n"], prm["p_msg"]
    sk = [int(s) for s in honest["sk_lwe"]]
    msgs = np.random.default_rng(734).integers(0, p, 160)
    cts = ctx.encrypt(msgs, nonce0=90_000)

    def off_centre(f, m):
        phase = (f[n] - sum(v for v, s in zip(f, sk) if s)) % (1 << B)
        d = (phase - (m << B) // (2 * p)) % (1 << B)
        return min(d, (1 << B) - d)
    keep = []
    for i, (ct, m) in enumerate(zip(cts, msgs)):
        x = [int(v) for v in o.keyswitch(ct)]
        if max(off_centre(compact_definition(x, B), int(m)), off_centre(reround_definition(compact_definition(x, 31), 31, B), int(m))) <= 9:
            keep.append(i)
    assert len(keep) >= 48
    keep = keep[:48]
    cts, msgs = cts[keep], msgs[keep]
    want = ctx.bootstrap_batch(ctx.tvset([list(range(p))]), cts)
    assert np.array_equal(want, o.bootstrap_batch(cts, [list(range(p))])[0])
    got = refresh_on_device(ctx, compact_on_device(ctx, cts, B), B)
    assert np.array_equal(got, want)
    assert np.array_equal(ctx.decrypt(got), msgs)
    wide = refresh_on_device(ctx, compact_on_device(ctx, cts, 31), 31)
    assert np.array_equal(ctx.decrypt(wide), msgs)


def test_constant_output_that_rounds_up_to_two_to_the_width():
    """a program's constant outputs reach the format through compact_round on the host (fbs_eval_sources, compact outputs), not through
    the key switch: a constant whose body is q - 1 rounds up to 2^w, and the field wraps to 0 up to 27 bits"""
    from tfhe_fbs_map_amd import _native as nat, parse_fbs
    ctx, _, _, prm = made("n64")
    n, p = prm["n"], prm["p_msg"]
    const = (Q - 1) * pow(lc_delta(p), Q - 2, Q) % Q                          # const x Delta = q - 1
    assert const * lc_delta(p) % Q == Q - 1
    rec = load_fixture("edge_outputs")
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    out_wire = list(low["out_wire"])
    at = low["out_names"].index("one")
    assert out_wire[at] == -2
    out_wire[at] = -1 - const
    tv = ctx.tvset(low["tables"])
    prog = nat.Program(ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"], low["term_coef"],
                       low["term_src"], out_wire)
    T = 3
    for bits in COMPACT_PACK_WIDTHS:
        got = prog.eval_sources([("plain", 1), ("plain", 0)], T, bits)
        fields = compact_definition([0] * n + [Q - 1], bits)
        assert fields[n] == (0 if bits <= 27 else (1 << bits) - 15)
        want = pack(as_u64([fields]), bits)
        assert got.shape == (len(out_wire), T, ctx.compact_words(bits))
        assert np.array_equal(got[at], np.repeat(want, T, axis=0)), bits
        zero = pack(as_u64([[0] * (n + 1)]), bits)
        assert np.array_equal(got[low["out_names"].index("z")], np.repeat(zero, T, axis=0)), bits
    prog.close()
