"""Compact outputs without a GPU (include/fbs_exec.h, "compact outputs"): the new entries are declared, exported and bound; the
split's `CompactOutputs` file round-trips, refuses what is not one and holds no secret; the noise rule (`params.compact_output_*`)
keeps the blind rotation's own width for every parameter set the golden fixtures are chosen at; and the host decode passes
tests/c/compact_harness.cpp under AddressSanitizer and UBSan and equals a numpy restatement of the format."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ENTRIES = ("fbs_compact_words", "fbs_compact_dev", "fbs_eval_seeded_compact", "fbs_decrypt_compact", "fbs_decrypt_compact_dev")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    for meth in ("compact_words", "compact_dev", "decrypt_compact", "decrypt_compact_dev"):
        assert callable(getattr(_native.Context, meth)), meth
    assert callable(_native.Program.eval_seeded_compact)


def test_compact_sizes_are_the_issue_figures():
    """k = 2, p = 15 (n = 734 at 11 bits): 1 016 bytes against 16 392; p = 31 (n = 766, N = 2048 at 12 bits): 1 152 bytes"""
    from tfhe_fbs_map_amd import Params
    from tfhe_fbs_map_amd.split import compact_words
    assert compact_words(Params(n=734, log_n_poly=10, k=2), 11) * 8 == 1016
    assert compact_words(Params(n=766, log_n_poly=11), 12) * 8 == 1152
    assert Params(n=734, log_n_poly=10, k=2).ct_words * 8 == 16392
    for n in (1, 63, 64, 734):
        for w in range(9, 32):
            assert compact_words(Params(n=n), w) == -(-(n + 1) * w // 64)


def _outputs(T=5, bits=11, W=127, seed=0):
    from tfhe_fbs_map_amd.split import CompactOutputs
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2**63, (3, T, W), dtype=np.uint64)
    return CompactOutputs(["s0", "s1", "cout"], T, bits, words, bytes(range(8)))


def test_compact_outputs_round_trip_and_refuse_what_is_not_one(tmp_path):
    from tfhe_fbs_map_amd.split import FORMAT_VERSION, CompactOutputs, EncryptedOutputs
    out = _outputs()
    path = str(tmp_path / "out.npz")
    out.save(path)
    back = CompactOutputs.load(path)
    assert back.output_names == out.output_names and back.T == out.T and back.bits == out.bits
    assert back.fingerprint == out.fingerprint and back.words.dtype == np.uint64 and np.array_equal(back.words, out.words)
    with np.load(path, allow_pickle=False) as z:
        # names, sizes, the packed ciphertexts and the server key's fingerprint: nothing else, no secret
        assert set(z.files) == {"kind", "format_version", "output_names", "T", "bits", "words", "fingerprint"}
        fields = {k: z[k] for k in z.files}
    assert FORMAT_VERSION == 1
    with pytest.raises(ValueError):
        EncryptedOutputs.load(path)                                     # another kind
    bad = [dict(kind=np.array("encrypted_outputs")), dict(format_version=np.array(FORMAT_VERSION + 1)),
           dict(words=fields["words"][:, :4]), dict(words=fields["words"][:2]), dict(words=fields["words"].astype(np.int64)),
           dict(words=fields["words"][0]), dict(bits=np.array(32, np.int64)), dict(fingerprint=np.zeros(7, np.uint8))]
    for i, change in enumerate(bad):
        p = str(tmp_path / f"bad{i}.npz")
        np.savez(p, **{**fields, **change})
        with pytest.raises(ValueError):
            CompactOutputs.load(p)


def _fixture_choices():
    from tests.helpers import fixture_names, load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    seen = set()
    for name in fixture_names():
        m = re.search(r"_p(\d+)", name)
        if not m:
            continue
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        seen.add((int(m.group(1)), env.stats()["norm2_linprod"]))
    return sorted(seen)


def test_compact_output_bits_keep_the_blind_rotation_width_on_every_fixture_set():
    from tfhe_fbs_map_amd.params import (DEFAULT_GLWE_DIMS, choose_params, compact_output_bits, compact_output_margin,
                                         compact_output_skew, compact_output_variance, margin_sigmas, variances)
    pairs = _fixture_choices()
    assert len(pairs) > 10
    for p, norm2 in pairs:
        try:
            prm = choose_params(p, norm2, glwe_dims=DEFAULT_GLWE_DIMS)
        except ValueError:
            prm = choose_params(p, norm2, floor_margin=4.0, glwe_dims=DEFAULT_GLWE_DIMS)
        w0 = prm.log_n_poly + 1
        w = compact_output_bits(prm, norm2, 1.0)
        assert w <= w0, (p, norm2, prm, w)
        # the margin the set was chosen for, with the 2^46 rounding skew (which the bootstrap inputs carry too) counted on both sides
        skewed = margin_sigmas(prm, norm2) * (1 - 4 * p * compact_output_skew(prm))
        assert compact_output_margin(prm, w, 1.0) >= skewed * (1 - 1e-12), (p, norm2)
        # (margin_sigmas itself leaves the skew out: held to within 1e-3, the skew's share at p = 31 -- DESIGN.md section 4)
        assert compact_output_margin(prm, w, 1.0) >= margin_sigmas(prm, norm2) * (1 - 1e-3), (p, norm2)
        # the variance at log2(2N) with out_norm2 = norm2 is the variance of the phase the next bootstrap reads
        v_br, v_ks, v_ms = variances(prm)
        assert compact_output_variance(prm, w0, norm2) == pytest.approx(norm2 * v_br + v_ks + v_ms, rel=1e-12)
        # more noise on the output asks for no fewer bits; 31 is the last resort
        assert compact_output_bits(prm, norm2, 4 * norm2) >= w
        assert compact_output_bits(prm, norm2, 1e9) == 31


def test_output_noise_factor_follows_the_program():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    from tfhe_fbs_map_amd.split import output_noise_factor
    rec = load_fixture("adder8__search_p7")
    low = parse_fbs(rec["fbs"], inputs=rec["program_inputs"]).lower()
    assert output_noise_factor(low, 7) == 1.0                          # bootstrap outputs
    low = dict(low, out_wire=[0, -3])                                   # an input and a constant
    assert output_noise_factor(low, 7) == 0.0


def _harness(tmp_path):
    """tests/c/compact_harness.cpp with the product's host sources and the sanitizer flags of tests/c/Makefile"""
    make = open(os.path.join(CDIR, "Makefile")).read()
    san = re.search(r"^SAN\s*:=\s*(.*)$", make, re.M).group(1).split()
    exe = str(tmp_path / "compact_harness")
    srcs = [os.path.join(CDIR, "compact_harness.cpp")] + [os.path.join(CSRC, f) for f in
                                                            ("fbs_plan.cpp", "fbs_host.cpp", "fbs_select.cpp", "fbs_error.cpp")]
    subprocess.check_call(["g++", "-std=c++17", *san, "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread", "-o", exe, *srcs])
    return exe


def _decode_numpy(words, sk, bits, p):
    """section 1 of the format, restated: field j at stream bits [j w, j w + w), phase = m_n - sum m_i s_i mod 2^w, round"""
    n = sk.size
    out = []
    for ct in np.asarray(words, np.uint64).reshape(-1, words.shape[-1]):
        stream = sum(int(x) << (64 * k) for k, x in enumerate(ct))
        f = [(stream >> (j * bits)) & ((1 << bits) - 1) for j in range(n + 1)]
        phase = (f[n] - sum(fi for fi, s in zip(f, sk) if s)) % (1 << bits)
        out.append(((phase * 2 * p + (1 << (bits - 1))) >> bits) % (2 * p))
    return np.array(out, np.int64)


def test_host_decode_under_sanitizers(tmp_path):
    exe = _harness(tmp_path)
    r = subprocess.run([exe, "roundtrip"], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok ") > 100
    rng = np.random.default_rng(7)
    for n, log_n, p, bits, count in ((12, 8, 7, 9, 5), (63, 10, 15, 11, 4), (734, 10, 15, 14, 3), (766, 11, 31, 31, 2), (5, 10, 2, 30, 6)):
        from tfhe_fbs_map_amd import Params
        from tfhe_fbs_map_amd.split import compact_words
        W = compact_words(Params(n=n), bits)
        sk = rng.integers(0, 2, n, dtype=np.uint64)
        words = rng.integers(0, 2**63, (count, W), dtype=np.uint64) * 2 + rng.integers(0, 2, (count, W), dtype=np.uint64)
        used = (n + 1) * bits
        if used % 64:
            words[:, -1] &= np.uint64((1 << (used % 64)) - 1)           # bits past the last field are zero
        text = " ".join(str(v) for v in [n, log_n, p, bits, count, *sk.tolist(), *words.reshape(-1).tolist()])
        r = subprocess.run([exe, "decode"], input=text, capture_output=True, text=True, env=ENV, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
        got = np.array([int(v) for v in r.stdout.split()], np.int64)
        assert np.array_equal(got, _decode_numpy(words, sk, bits, p)), (n, bits)
