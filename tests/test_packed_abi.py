"""Packed outputs without a GPU (include/fbs_exec.h, "packed outputs"): the new entries are declared, exported and bound;
`params.packing_choice` reaches the margin at every parameter set the golden fixtures select, with no smaller key; the split's
`PackedOutputs` and `ServerKey` files round-trip, old server keys load without a packing key and `plan_chain` refuses a packed
result; the packed format restated in numpy agrees with `split.packed_words`; and the host key generation, import and decode pass
tests/c/packed_harness.cpp under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_compact_abi import _fixture_choices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ENTRIES = ("fbs_packing_keygen", "fbs_packing_key_sizes", "fbs_export_packing_key", "fbs_import_packing_key", "fbs_packed_words",
           "fbs_pack_dev", "fbs_state_fetch_packed", "fbs_decrypt_packed")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    for meth in ("packing_keygen", "export_packing_key", "import_packing_key", "packed_words", "pack_dev", "decrypt_packed"):
        assert callable(getattr(_native.Context, meth)), meth
    assert callable(_native.DeviceState.fetch_packed)
    header = open(os.path.join(ROOT, "include", "fbs_exec.h")).read()
    for word in ("packed outputs", '"pack_slices"', '"packing_key"', '"packing_levels"', '"packing_base_bits"'):
        assert word in header, word


def test_packing_choice_reaches_the_margin_with_the_smallest_key():
    from tfhe_fbs_map_amd.params import (DEFAULT_GLWE_DIMS, choose_params, compact_output_variance, margin_sigmas, packed_margin_needed,
                                         packed_output_margin, packed_output_skew, packed_output_variance, packing_choice)
    pairs = _fixture_choices()
    assert len(pairs) > 10
    for p, norm2 in pairs:
        try:
            prm = choose_params(p, norm2, glwe_dims=DEFAULT_GLWE_DIMS)
        except ValueError:
            prm = choose_params(p, norm2, floor_margin=4.0, glwe_dims=DEFAULT_GLWE_DIMS)
        t_p, gamma_p, bits = packing_choice(prm, norm2, 1.0)
        assert 1 <= gamma_p and t_p * gamma_p <= 31 and prm.log_n_poly + 1 <= bits <= 31
        need = margin_sigmas(prm, norm2) * (1 - 4 * p * packed_output_skew(prm))
        assert need == pytest.approx(packed_margin_needed(prm, norm2), rel=1e-12)
        assert packed_output_margin(prm, t_p, gamma_p, bits, 1.0) >= need * (1 - 1e-12), (p, norm2)
        # no smaller key: fewer levels never reach it, nor a wider digit at these levels, nor a narrower width at this key
        for t in range(1, t_p + 1):
            for g in range(31 // t, 0, -1):
                if (t, g) == (t_p, gamma_p):
                    break
                assert packed_output_margin(prm, t, g, 31, 1.0) < need * (1 - 1e-12), (p, norm2, t, g)
        if bits > prm.log_n_poly + 1:
            assert packed_output_margin(prm, t_p, gamma_p, bits - 1, 1.0) < need * (1 - 1e-12)
        # the four terms
        q, n, N, k = float((1 << 46) - 507903), prm.n, prm.N, prm.k
        terms = (compact_output_variance(prm, 31, 1.0), n * t_p * N * (4.0 ** gamma_p + 2) / 12 * (prm.sigma_glwe / q) ** 2,
                 n / 2 * 4.0 ** (-t_p * gamma_p) / 12, (1 + k * N / 2) / (12 * 4.0 ** bits))
        assert packed_output_variance(prm, t_p, gamma_p, bits, 1.0) == pytest.approx(sum(terms), rel=1e-12)
        # More noise on the outputs never asks for less: the choice is monotone in the order it is made in -- levels up, then
        # digit width down, then transport width up -- and at a FIXED key the width alone is monotone.  (Across a step of gamma_p
        # the width may come down again: a narrower digit leaves the transport more room, e.g. p = 3, norm2 = 11 gives
        # (1, 27, 13) at out_norm2 = 1 and (1, 26, 12) at out_norm2 = 11.)
        noises = (0.0, 1.0, norm2, 4 * norm2, 1e9)
        choices = [packing_choice(prm, norm2, o) for o in noises]
        order = [(t, -g, w) for (t, g, w), o in zip(choices, noises) if packed_output_margin(prm, t, g, w, o) >= need * (1 - 1e-12)]
        assert len(order) >= 3 and order == sorted(order), (p, norm2, choices)
        assert choices[-1][2] == 31, (p, norm2, choices)                             # nothing reaches it: the last resort
        fixed = []
        for o in noises:
            reach = [w for w in range(prm.log_n_poly + 1, 32) if packed_output_margin(prm, t_p, gamma_p, w, o) >= need * (1 - 1e-12)]
            fixed.append(min(reach, default=31))
        assert fixed == sorted(fixed) and fixed[1] == bits, (p, norm2, fixed)


def _packed(T=5, bits=13, seed=0):
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.split import PackedOutputs, packed_words
    prm = Params(n=24, log_n_poly=8, k=2)
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2**63, packed_words(prm, 3 * T, bits), dtype=np.uint64)
    return PackedOutputs(["s0", "s1", "cout"], T, bits, words, bytes(range(8)), np.ones(3))


def test_packed_outputs_round_trip_and_refuse_what_is_not_one(tmp_path):
    from tfhe_fbs_map_amd.split import CompactOutputs, PackedOutputs
    out = _packed()
    path = str(tmp_path / "out.npz")
    out.save(path)
    back = PackedOutputs.load(path)
    assert (back.output_names, back.T, back.bits, back.fingerprint) == (out.output_names, out.T, out.bits, out.fingerprint)
    assert back.words.dtype == np.uint64 and np.array_equal(back.words, out.words) and np.array_equal(back.out_norm2, out.out_norm2)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"kind", "format_version", "output_names", "T", "bits", "words", "fingerprint", "out_norm2"}
        fields = {k: z[k] for k in z.files}
    with pytest.raises(ValueError):
        CompactOutputs.load(path)
    bad = [dict(kind=np.array("compact_outputs")), dict(format_version=np.array(99)), dict(words=fields["words"].astype(np.int64)),
           dict(words=fields["words"].reshape(1, -1)), dict(bits=np.array(32, np.int64)), dict(fingerprint=np.zeros(7, np.uint8)),
           dict(out_norm2=np.ones(2))]
    for i, change in enumerate(bad):
        p = str(tmp_path / f"bad{i}.npz")
        np.savez(p, **{**fields, **change})
        with pytest.raises(ValueError):
            PackedOutputs.load(p)


def test_server_key_files_with_and_without_a_packing_key(tmp_path):
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.split import ServerKey, seeded_key_sizes
    prm = Params(n=6, log_n_poly=8, k=2, l_bsk=1, beta_bsk=18, t_ksk=2, gamma_ksk=3, p_msg=3, sigma_lwe=4, sigma_glwe=4)
    rng = np.random.default_rng(1)
    nb, nk = seeded_key_sizes(prm)
    bsk, ksk = rng.integers(0, 2**40, nb, dtype=np.uint64), rng.integers(0, 2**40, nk, dtype=np.uint64)
    plain = ServerKey(prm, False, bytes(range(32)), bsk, ksk)
    old, new = str(tmp_path / "old.npz"), str(tmp_path / "new.npz")
    plain.save(old)
    with np.load(old, allow_pickle=False) as z:       # a key without a packing key is written as it always was
        assert set(z.files) == {"kind", "format_version", "params", "fuse_tables", "mask_key", "fingerprint", "bsk_bodies", "ksk_bodies"}
    back = ServerKey.load(old)
    assert back.packing_bodies is None and (back.packing_levels, back.packing_base_bits) == (0, 0)
    bodies = rng.integers(0, 2**40, prm.n * 2 * prm.N, dtype=np.uint64)
    packing = ServerKey(prm, False, bytes(range(32)), bsk, ksk, bodies, 2, 7)
    packing.save(new)
    back = ServerKey.load(new)
    assert (back.packing_levels, back.packing_base_bits) == (2, 7) and np.array_equal(back.packing_bodies, bodies)
    assert np.array_equal(back.bsk_bodies, bsk) and back.fingerprint == plain.fingerprint
    for levels, base, b in ((2, 16, bodies), (0, 7, bodies), (2, 7, bodies[:-1])):
        with pytest.raises(ValueError):
            ServerKey(prm, False, bytes(range(32)), bsk, ksk, b, levels, base)


def test_plan_chain_refuses_a_packed_result():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.split import client_choice, plan_chain
    rec = load_fixture("adder8__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    prm, fuse = client_choice(env, ExecConfig())
    with pytest.raises(ValueError, match="PackedOutputs.*client"):
        plan_chain(prm, fuse, bytes(range(8)), env, [_packed()])


def test_the_packed_format_in_numpy_agrees_with_packed_words():
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.split import packed_words
    rng = np.random.default_rng(2)
    for k, log_n in ((1, 8), (2, 8), (3, 9), (2, 10)):
        prm = Params(n=24, log_n_poly=log_n, k=k)
        N = prm.N
        for bits in (log_n + 1, 17, 31):
            for count in (1, 63, N - 1, N, N + 1, 2 * N + 3):
                words, fields = [], []
                for g0 in range(0, count, N):
                    fill = min(N, count - g0)
                    f = rng.integers(0, 1 << bits, k * N + fill)
                    stream = 0
                    for i, x in enumerate(f):
                        stream |= int(x) << (i * bits)
                    n_words = -(-(k * N + fill) * bits // 64)                  # (k N bits is a multiple of 64)
                    words.append([(stream >> (64 * j)) & (2**64 - 1) for j in range(n_words)])
                    fields.append(f)
                flat = np.array([w for s in words for w in s], np.uint64)
                assert flat.size == packed_words(prm, count, bits), (k, log_n, bits, count)
                # ... and unpacks: every sample starts on a word boundary
                at = 0
                for s, f in zip(words, fields):
                    stream = sum(int(x) << (64 * j) for j, x in enumerate(flat[at:at + len(s)]))
                    assert [(stream >> (i * bits)) & ((1 << bits) - 1) for i in range(len(f))] == [int(x) for x in f]
                    assert stream >> (len(f) * bits) == 0                      # zero padding
                    at += len(s)
    assert packed_words(Params(n=690, log_n_poly=10, k=2), 129000, 13) * 8 == 125 * 3 * 1024 * 13 // 8 + (2 * 1024 * 13 // 64 + -(-1000 * 13 // 64)) * 8


def _harness(tmp_path):
    """tests/c/packed_harness.cpp with the product's host sources and the sanitizer flags of tests/c/Makefile"""
    make = open(os.path.join(CDIR, "Makefile")).read()
    san = re.search(r"^SAN\s*:=\s*(.*)$", make, re.M).group(1).split()
    exe = str(tmp_path / "packed_harness")
    srcs = [os.path.join(CDIR, "packed_harness.cpp")] + [os.path.join(CSRC, f) for f in
                                                           ("fbs_plan.cpp", "fbs_host.cpp", "fbs_select.cpp", "fbs_error.cpp")]
    subprocess.check_call(["g++", "-std=c++17", *san, "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread", "-o", exe, *srcs])
    return exe


def test_host_packing_key_and_decode_under_sanitizers(tmp_path):
    exe = _harness(tmp_path)
    for mode, least in (("keys", 9), ("decode", 40)):
        r = subprocess.run([exe, mode], capture_output=True, text=True, env=ENV, timeout=600)
        assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
        assert r.stdout.count("ok %s" % mode) >= least, r.stdout[-2000:]
