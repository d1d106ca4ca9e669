"""The seeded path without a GPU: the new entries of include/fbs_exec.h are declared, exported and bound; the seeded streams
have domains of their own; the split's files round-trip, refuse what does not fit their parameters and hold no secret; and the
host code of the seeded keys and inputs passes the seeded mode of tests/c/host_harness.cpp under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ENTRIES = ("fbs_keygen_seeded", "fbs_seeded_key_sizes", "fbs_export_seeded_keys", "fbs_import_seeded_keys", "fbs_encrypt_seeded",
           "fbs_encrypt_seeded_fresh", "fbs_encrypt_seeded_dev", "fbs_encrypt_seeded_fresh_dev", "fbs_expand_seeded",
           "fbs_expand_seeded_dev", "fbs_eval_seeded")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    for meth in ("keygen_seeded", "export_seeded_keys", "import_seeded_keys", "encrypt_seeded", "expand_seeded", "evaluation_only"):
        assert callable(getattr(_native.Context, meth)), meth
    assert callable(_native.Program.eval_seeded)


def _domains():
    text = open(os.path.join(CSRC, "fbs_internal.hpp")).read()
    body = re.search(r"enum Domain : uint64_t \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return {name: int(v) for name, v in re.findall(r"(DOM_\w+)\s*=\s*(\d+)", body)}


def test_seeded_domains_are_new_and_fit_the_stream_id():
    dom = _domains()
    old = {k: v for k, v in dom.items() if v <= 8}
    new = {k: v for k, v in dom.items() if v >= 9}
    assert sorted(old.values()) == list(range(1, 9))
    assert {"DOM_MASK_KEY", "DOM_SBSK_MASK", "DOM_SBSK_NOISE", "DOM_SKSK_MASK", "DOM_SKSK_NOISE", "DOM_SENC_MASK",
            "DOM_SENC_NOISE"} <= set(new)
    assert len(set(dom.values())) == len(dom)                   # no two streams of a key share a domain
    assert all(0 < v < 256 for v in dom.values())                # the 8-bit field of stream_id (bits 56 .. 63)


def _params():
    from tfhe_fbs_map_amd import ExecConfig
    return ExecConfig().params_choice(15, 1)                     # the default 128-bit p = 15 set (k = 2, bsk_group = 2)


def _server_key(prm, seed=0):
    from tfhe_fbs_map_amd.split import ServerKey, seeded_key_sizes
    rng = np.random.default_rng(seed)
    nb, nk = seeded_key_sizes(prm)
    q = (1 << 46) - 62 * (1 << 13) + 1
    return ServerKey(prm, True, rng.bytes(32), rng.integers(0, q, nb, dtype=np.uint64), rng.integers(0, q, nk, dtype=np.uint64))


def test_seeded_key_sizes_follow_the_layout():
    from tfhe_fbs_map_amd.split import seeded_key_sizes
    prm = _params()
    assert (prm.k, prm.log_n_poly, prm.l_bsk, prm.bsk_group) == (2, 10, 1, 2)
    nb, nk = seeded_key_sizes(prm)
    assert nb == prm.n // 2 * 3 * (prm.k + 1) * prm.l_bsk * prm.N and nk == prm.k * prm.N * prm.t_ksk
    full_bsk = nb * (prm.k + 1)
    assert full_bsk * 8 == prm.bytes_per_fbs() - prm.k * prm.N * prm.t_ksk * (prm.n + 1) * 8 - 2 * prm.ct_words * 8 - prm.N * 8


def test_server_key_round_trips_and_holds_no_secret(tmp_path):
    from tfhe_fbs_map_amd.split import ServerKey, mask_key_fingerprint
    prm = _params()
    key = _server_key(prm)
    path = str(tmp_path / "server_key.npz")
    key.save(path)
    back = ServerKey.load(path)
    assert back.params == prm and back.fuse_tables is True and back.mask_key == key.mask_key
    assert np.array_equal(back.bsk_bodies, key.bsk_bodies) and np.array_equal(back.ksk_bodies, key.ksk_bodies)
    assert back.fingerprint == key.fingerprint == mask_key_fingerprint(key.mask_key) and len(key.fingerprint) == 8
    with np.load(path, allow_pickle=False) as z:
        for name in z.files:
            assert not re.search(r"(^|_)sk(_|$)|secret|lwe|glwe", name), name
            assert z[name].size not in (prm.n, prm.big_dim), name     # nothing the size of sk_lwe or sk_glwe


def test_server_key_load_refuses_mismatched_sizes(tmp_path):
    from tfhe_fbs_map_amd.split import ServerKey
    prm = _params()
    key = _server_key(prm)
    for field, cut in (("bsk_bodies", 1), ("ksk_bodies", 7)):
        d = dict(bsk_bodies=key.bsk_bodies, ksk_bodies=key.ksk_bodies)
        d[field] = d[field][:-cut]
        path = str(tmp_path / ("short_%s.npz" % field))
        np.savez(path, kind=np.array("server_key"), format_version=np.array(1),
                 params=np.array([getattr(prm, f) for f in ("n", "log_n_poly", "k", "l_bsk", "beta_bsk", "t_ksk", "gamma_ksk",
                                                             "p_msg", "sigma_lwe", "sigma_glwe", "bsk_group")], np.int64),
                 fuse_tables=np.array(True), mask_key=np.frombuffer(key.mask_key, np.uint8),
                 fingerprint=np.frombuffer(key.fingerprint, np.uint8), **d)
        with pytest.raises(ValueError, match=field):
            ServerKey.load(path)
    other = str(tmp_path / "other.npz")
    key.save(other)
    with np.load(other, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["format_version"] = np.array(99)
    np.savez(other, **d)
    with pytest.raises(ValueError, match="format version"):
        ServerKey.load(other)
    with pytest.raises(ValueError):
        ServerKey(prm, False, b"\0" * 31, key.bsk_bodies, key.ksk_bodies)


def test_encrypted_inputs_and_outputs_round_trip(tmp_path):
    from tfhe_fbs_map_amd.split import EncryptedInputs, EncryptedOutputs
    rng = np.random.default_rng(1)
    ins = EncryptedInputs(["a", "b0", "carry"], 5, (1 << 55) + 17, rng.integers(0, 1 << 46, (3, 5), dtype=np.uint64), b"12345678")
    p_in = str(tmp_path / "in.npz")
    ins.save(p_in)
    back = EncryptedInputs.load(p_in)
    assert back.input_names == ins.input_names and back.T == 5 and back.nonce0 == ins.nonce0 and back.fingerprint == b"12345678"
    assert np.array_equal(back.bodies, ins.bodies) and back.bodies.dtype == np.uint64
    outs = EncryptedOutputs(["s", "c"], 5, rng.integers(0, 1 << 46, (2, 5, 9), dtype=np.uint64), b"abcdefgh")
    p = str(tmp_path / "out.npz")
    outs.save(p)
    back = EncryptedOutputs.load(p)
    assert back.output_names == ["s", "c"] and back.T == 5 and np.array_equal(back.cts, outs.cts)
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, kind=np.array("encrypted_inputs"), format_version=np.array(1), input_names=np.array(["a", "b"]),
             T=np.array(5), nonce0=np.array(0, np.uint64), bodies=np.zeros((3, 5), np.uint64), fingerprint=np.zeros(8, np.uint8))
    with pytest.raises(ValueError, match="bodies"):
        EncryptedInputs.load(bad)
    with pytest.raises(ValueError, match="not a saved"):
        EncryptedOutputs.load(p_in)


def test_seeded_host_code_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "asan"], timeout=600)
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "host_harness"), "seeded"], capture_output=True, text=True, env=ENV,
                       timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.endswith(" ok")]
    assert len(ok) == 6, r.stdout
    for k in (1, 2, 3):
        assert any(ln.startswith("k=%d " % k) for ln in ok)
    assert any("group=1" in ln for ln in ok) and any("group=2" in ln for ln in ok)
    assert any("l=1" in ln for ln in ok) and any("l=2" in ln for ln in ok)
