"""Public-key inputs without a GPU (include/fbs_exec.h, "public-key inputs"): what the entries refuse, with nothing written; the
closed forms of the word counts; libfbspublic.so's export list, dependencies and exception barriers; fresh streams; the files;
and `plan_chain` on a `PublicInputs`."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests.test_client_lib import SETS, toy_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tfhe_fbs_map_amd")
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libfbspublic.so")
Q = (1 << 46) - 62 * (1 << 13) + 1
E_INVALID, E_STATE = -1, -3
HOST_ENTRIES = """fbs_pub_key_words fbs_pub_keygen fbs_pub_create fbs_pub_destroy fbs_pub_last_error fbs_pub_words fbs_pub_encrypt
    fbs_pub_encrypt_fresh fbs_pub_expand""".split()
DEVICE_ENTRIES = ["fbs_pub_expand_dev", "fbs_state_put_public"]
SENTINEL = 0xDEADBEEFDEADBEEF


@pytest.fixture(scope="module", autouse=True)
def libraries():
    subprocess.check_call(["make", "-s", "-C", CSRC, "client", "public"], timeout=900)


@pytest.fixture(scope="module")
def world():
    """k = 1, N = 256: (parameter set, raw library, mask key, bodies, secret, an encryptor's handle)"""
    from tfhe_fbs_map_amd import HostContext, _public_native as pub
    prm = toy_sets()["k1_N256"]
    ctx = HostContext(prm, seed=4)
    ctx.keygen_seeded()
    sk, mask_key = ctx.export_keys()["sk_glwe"], ctx.export_seeded_keys()["mask_key"]
    bodies = pub.keygen(prm, mask_key, sk, bytes(32))
    enc = pub.Encryptor(prm, mask_key, bodies, bytes(range(32)))
    return dict(prm=prm, lib=pub._lib(), mask_key=mask_key, bodies=bodies, sk=sk, enc=enc, ctx=ctx)


def err(lib, handle=None):
    return lib.fbs_pub_last_error(handle).decode()


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_public_target_uses_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "public"], capture_output=True, text=True, check=True).stdout
    assert "fbs_public.cpp" in out and "libfbspublic.so" in out and "-DFBS_HOST_ONLY" in out and "-Wl,-Bsymbolic" in out
    assert "hipcc" not in out and "rocm" not in out.lower() and "__HIP_PLATFORM_AMD__" not in out, out
    for src in ("fbs_plan.cpp", "fbs_select.cpp", "fbs_capi.cpp", "fbs_eval.cpp", "fbs_client_entries.cpp", "fbs_client_capi.cpp", ".hip"):
        assert src not in out, src
    everything = subprocess.run(["make", "-n", "-B", "-C", CSRC], capture_output=True, text=True, check=True).stdout
    assert "libfbspublic.so" in everything and "fbs_public.hip" in everything          # part of `all`, and the kernel is in NAMES
    clean = subprocess.run(["make", "-n", "-C", CSRC, "clean"], capture_output=True, text=True, check=True).stdout
    assert "libfbspublic.so" in clean
    # .gitignore covers the library (read as text: a checkout need not be a git repository)
    import fnmatch
    patterns = [ln.strip() for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip() and not ln.startswith(("#", "!"))]
    assert any("/" not in pat and fnmatch.fnmatch(os.path.basename(LIB), pat) for pat in patterns), patterns


def test_library_exports_exactly_the_nine_host_entries():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native, _public_native
    defined = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in defined.splitlines() if ln.split()[-1].startswith("fbs_"))
    assert exported == sorted(HOST_ENTRIES) and len(HOST_ENTRIES) == 9
    assert sorted(_public_native.EXPORTED_SYMBOLS) == sorted(HOST_ENTRIES)
    assert set(HOST_ENTRIES + DEVICE_ENTRIES) <= set(declared_symbols()) and set(HOST_ENTRIES + DEVICE_ENTRIES) <= set(_native.EXPORTED_SYMBOLS)
    gpu = C.CDLL(_native.LIB_PATH)
    for name in HOST_ENTRIES + DEVICE_ENTRIES:
        assert hasattr(gpu, name), name
    assert callable(_native.DeviceState.put_public) and callable(_native.Context.pub_expand_dev)


def test_library_needs_no_gpu_runtime():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert needed, dyn
    for lib in needed:
        assert not re.search(r"hip|hsa|roc", lib, re.I), lib
    undefined = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for line in undefined.splitlines():
        assert not re.search(r"hip|hsa|roc", line.split()[-1], re.I), line


def test_every_entry_is_an_exception_barrier():
    text = open(os.path.join(CSRC, "fbs_public.cpp")).read()
    body = text[text.index('extern "C" {'):]
    seen = []
    for m in re.finditer(r"^(?:int|void|double|const char \*) ?(fbs_\w+)\(([^{};]*?)\) (try )?\{", body, flags=re.M):
        seen.append(m.group(1))
        assert m.group(3), "%s has no function-try-block" % m.group(1)
    assert sorted(seen) == sorted(HOST_ENTRIES)
    capi = open(os.path.join(CSRC, "fbs_capi.cpp")).read()
    for name in DEVICE_ENTRIES:
        assert re.search(r"^int %s\([^{};]*?\) try \{" % name, capi, flags=re.M), name


def test_binding_imports_neither_torch_nor_the_gpu_binding():
    src = open(os.path.join(PKG, "_public_native.py")).read()
    imports = re.findall(r"^\s*(?:from\s+(\S+)\s+import|import\s+(\S+))", src, flags=re.M)
    assert {a or b for a, b in imports} == {"__future__", "ctypes", "os", "sys", "numpy", "._client_native"}
    code = ("import sys\nfrom tfhe_fbs_map_amd import _public_native as p\nfrom tfhe_fbs_map_amd._client_native import Params\n"
            "prm = Params(n=12, log_n_poly=8, p_msg=7, sigma_lwe=256, sigma_glwe=256)\nassert p.key_words(prm) == 256\n"
            "assert 'torch' not in sys.modules\nprint('ok')\n")
    # (the package itself loads the GPU binding in this tree; the module on its own must not need it)
    probe = ("import sys, types, importlib.util, os\nroot = %r\npkg = types.ModuleType('tfhe_fbs_map_amd'); pkg.__path__ = [os.path.join(root, 'tfhe_fbs_map_amd')]\n"
             "sys.modules['tfhe_fbs_map_amd'] = pkg\n" % ROOT) + code + "assert 'tfhe_fbs_map_amd._native' not in sys.modules\n"
    r = subprocess.run([os.sys.executable, "-c", probe], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


PUBLIC_ONLY_CHILD = r"""
import sys
sys.path.insert(0, HERE)
import numpy as np
import tfhe_fbs_map_amd as pkg
from tfhe_fbs_map_amd import Params, PublicEncryptor, PublicInputs, PublicKey
assert pkg.__file__.startswith(HERE)
assert "torch" not in sys.modules
key = PublicKey.load(HERE + "/key.npz")
enc = PublicEncryptor(key, seed=bytes(32))
ins = enc.encrypt({"a": [0, 1, 1], "b": [1, 1, 0]}, ["a", "b"])
ins.save(HERE + "/ins.npz")
assert PublicInputs.load(HERE + "/ins.npz").samples.shape == (1, key.params.k + 1, key.params.N)
try:
    pkg.Context
except ImportError as e:
    assert "libfbsexec.so is missing" in str(e), str(e)
else:
    raise AssertionError("the GPU library was not asked for")
print("public ok")
"""


def test_package_imports_where_only_the_public_library_exists(tmp_path, world):
    import shutil
    import sys
    from tfhe_fbs_map_amd import PublicKey
    dst = tmp_path / "tfhe_fbs_map_amd"
    shutil.copytree(PKG, dst, ignore=shutil.ignore_patterns("libfbsexec.so", "libfbsclient.so", "csrc", "__pycache__"))
    assert (dst / "libfbspublic.so").exists() and not (dst / "libfbsexec.so").exists() and not (dst / "libfbsclient.so").exists()
    PublicKey(world["prm"], world["mask_key"], world["bodies"]).save(str(tmp_path / "key.npz"))
    code = "HERE = %r\n" % str(tmp_path) + PUBLIC_ONLY_CHILD
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "FBS_LIB", "FBS_CLIENT_LIB", "FBS_PUBLIC_LIB")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0 and "public ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    # what the encryptor wrote there decrypts here
    from tfhe_fbs_map_amd import PublicInputs, _public_native as pub
    ins = PublicInputs.load(str(tmp_path / "ins.npz"))
    got = world["ctx"].decrypt(pub.expand(world["prm"], ins.samples, 6)).reshape(2, 3)
    assert np.array_equal(got, [[0, 1, 1], [1, 1, 0]]) and ins.fingerprint == PublicKey(world["prm"], world["mask_key"], world["bodies"]).fingerprint


# ---- word counts, count = 0 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_word_counts_are_the_closed_forms(name):
    from tfhe_fbs_map_amd import _public_native as pub
    prm = toy_sets()[name]
    N, k = prm.N, prm.k
    assert pub.key_words(prm) == k * N
    for count in (0, 1, N - 1, N, N + 1, 2 * N, 2 * N + 3, 1000 * N + 1):
        assert pub.sample_words(prm, count) == -(-count // N) * (k + 1) * N, count
    lib, w = pub._lib(), C.c_size_t(77)
    assert lib.fbs_pub_words(C.byref(prm.to_c()), (1 << 64) - 1, C.byref(w)) == E_INVALID and w.value == 77 and "overflow" in err(lib)
    assert lib.fbs_pub_words(C.byref(prm.to_c()), 5, None) == E_INVALID and lib.fbs_pub_key_words(C.byref(prm.to_c()), None) == E_INVALID
    assert lib.fbs_pub_words(None, 5, C.byref(w)) == E_INVALID and lib.fbs_pub_key_words(None, C.byref(w)) == E_INVALID and w.value == 77


def test_count_zero_does_nothing(world):
    lib, prm, enc = world["lib"], world["prm"], world["enc"]
    before = enc.encrypt(np.zeros(1, np.int64))[1]
    assert lib.fbs_pub_encrypt(enc._h, None, 0, 5, None) == 0
    first = C.c_uint64(123)
    assert lib.fbs_pub_encrypt_fresh(enc._h, None, 0, None, C.byref(first)) == 0
    assert lib.fbs_pub_expand(C.byref(prm.to_c()), None, 0, None) == 0
    assert enc.encrypt(np.zeros(1, np.int64))[1] == before + 1          # count = 0 took no stream
    glwe, _ = enc.encrypt(np.zeros(0, np.int64), nonce0=1)
    assert glwe.shape == (0, 2, prm.N)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(world):
    lib, prm, enc = world["lib"], world["prm"], world["enc"]
    N, cp = prm.N, prm.to_c()
    out = np.full(2 * 2 * N, SENTINEL, np.uint64)
    good = np.arange(N + 1, dtype=np.int64) % (2 * prm.p_msg)

    def enc_code(msgs, nonce0=5, fresh=False):
        msgs = np.ascontiguousarray(msgs, np.int64)
        if fresh:
            return lib.fbs_pub_encrypt_fresh(enc._h, msgs.ctypes.data, msgs.size, out.ctypes.data, None)
        return lib.fbs_pub_encrypt(enc._h, msgs.ctypes.data, msgs.size, nonce0, out.ctypes.data)

    counter = enc.encrypt(good[:1])[1]
    for fresh in (False, True):
        for bad, where in ((2 * prm.p_msg, 0), (-1, N), (2 * prm.p_msg, N - 1), (1 << 62, 3)):
            msgs = good.copy()
            msgs[where] = bad
            assert enc_code(msgs, fresh=fresh) == E_INVALID and "message %d is outside [0, 2p)" % where in err(lib, enc._h), (bad, where)
    assert enc_code(good, nonce0=1 << 55) == E_INVALID and "below 2^55" in err(lib, enc._h)          # the fresh entries' range
    assert enc_code(good, nonce0=(1 << 55) - 1) == E_INVALID                                           # two samples: the second would be 2^55
    assert enc_code(good, nonce0=(1 << 64) - 1) == E_INVALID
    assert lib.fbs_pub_encrypt(enc._h, None, 3, 5, out.ctypes.data) == E_INVALID and lib.fbs_pub_encrypt(enc._h, good.ctypes.data, 3, 5, None) == E_INVALID
    assert lib.fbs_pub_encrypt(None, good.ctypes.data, 3, 5, out.ctypes.data) == E_INVALID
    assert lib.fbs_pub_encrypt_fresh(None, good.ctypes.data, 3, out.ctypes.data, None) == E_INVALID
    assert (out == SENTINEL).all()
    assert enc.encrypt(good[:1])[1] == counter + 1                                                     # no refused call took a stream

    # expansion: a non-canonical word anywhere in the samples the count covers -- first, last, and in the unfilled part of the last
    cts = np.full((N + 1) * (N + 1), SENTINEL, np.uint64)
    glwe, _ = enc.encrypt(good, nonce0=9)
    for index in (0, glwe.size - 1, 2 * N + 5, 3 * N + 100):
        for value in (Q, (1 << 64) - 1):
            bad = glwe.copy().reshape(-1)
            bad[index] = value
            assert lib.fbs_pub_expand(C.byref(cp), bad.ctypes.data, N + 1, cts.ctypes.data) == E_INVALID
            assert "sample word %d is not a canonical residue" % index in err(lib)
    assert lib.fbs_pub_expand(C.byref(cp), None, 3, cts.ctypes.data) == E_INVALID and lib.fbs_pub_expand(C.byref(cp), glwe.ctypes.data, 3, None) == E_INVALID
    assert lib.fbs_pub_expand(None, glwe.ctypes.data, 3, cts.ctypes.data) == E_INVALID
    assert (cts == SENTINEL).all()
    edge = glwe.copy().reshape(-1)
    edge[0] = Q - 1
    assert lib.fbs_pub_expand(C.byref(cp), edge.ctypes.data, N + 1, cts.ctypes.data) == 0 and cts[0] == Q - 1

    # creation and keygen
    h = C.c_void_p(5)
    bodies = world["bodies"].copy().reshape(-1)
    for index in (0, bodies.size - 1):
        bad = bodies.copy()
        bad[index] = Q
        assert lib.fbs_pub_create(C.byref(cp), world["mask_key"], bad.ctypes.data, bytes(32), C.byref(h)) == E_INVALID and not h.value
        assert "public-key word %d is not a canonical residue" % index in err(lib)
        h = C.c_void_p(5)
    for args in ((None, world["mask_key"], bodies.ctypes.data, bytes(32)), (C.byref(cp), None, bodies.ctypes.data, bytes(32)),
                 (C.byref(cp), world["mask_key"], None, bytes(32)), (C.byref(cp), world["mask_key"], bodies.ctypes.data, None)):
        h = C.c_void_p(5)
        assert lib.fbs_pub_create(*args, C.byref(h)) == E_INVALID and not h.value
    assert lib.fbs_pub_create(C.byref(cp), world["mask_key"], bodies.ctypes.data, bytes(32), None) == E_INVALID
    made = np.full(prm.k * N, SENTINEL, np.uint64)
    sk = world["sk"].copy()
    sk[7] = 2
    assert lib.fbs_pub_keygen(C.byref(cp), world["mask_key"], sk.ctypes.data, bytes(32), made.ctypes.data) == E_INVALID and "binary" in err(lib)
    sk[7] = 1
    for args in ((None, world["mask_key"], sk.ctypes.data, bytes(32), made.ctypes.data), (C.byref(cp), None, sk.ctypes.data, bytes(32), made.ctypes.data),
                 (C.byref(cp), world["mask_key"], None, bytes(32), made.ctypes.data), (C.byref(cp), world["mask_key"], sk.ctypes.data, None, made.ctypes.data)):
        assert lib.fbs_pub_keygen(*args) == E_INVALID
    assert lib.fbs_pub_keygen(C.byref(cp), world["mask_key"], sk.ctypes.data, bytes(32), None) == E_INVALID
    assert (made == SENTINEL).all()
    lib.fbs_pub_destroy(None)
    assert isinstance(lib.fbs_pub_last_error(None), bytes)


def test_parameter_sets_a_context_refuses_are_refused_with_its_code_and_text(world):
    """the shared admission of fbs_api_checks.hpp: each set fbs_ctx_create refuses comes back from every entry that takes a
    parameter set with the code and the text the client library's fbs_ctx_create gives"""
    from tfhe_fbs_map_amd import Params, _client_native, _native
    lib, client, gpu = world["lib"], _client_native._lib(), _native.lib
    w, h = C.c_size_t(77), C.c_void_p()
    one = np.zeros(8, np.uint64)
    for bad in (Params(k=2, log_n_poly=11), Params(k=5, log_n_poly=9), Params(log_n_poly=13), Params(l_bsk=5, beta_bsk=7), Params(p_msg=0),
                Params(log_n_poly=7), Params(sampler=2), Params(bsk_group=2, n=631), Params(bsk_group=2, log_n_poly=9)):
        cp = bad.to_c()
        rc = client.fbs_ctx_create(C.byref(cp), 1, -1, C.byref(h))
        want = client.fbs_last_error(None).decode()
        assert rc == E_INVALID and want
        assert gpu.fbs_ctx_create(C.byref(cp), 1, 0, C.byref(h)) == rc and gpu.fbs_last_error(None).decode() == want
        calls = (lambda: lib.fbs_pub_key_words(C.byref(cp), C.byref(w)), lambda: lib.fbs_pub_words(C.byref(cp), 5, C.byref(w)),
                 lambda: lib.fbs_pub_keygen(C.byref(cp), bytes(32), one.ctypes.data, bytes(32), one.ctypes.data),
                 lambda: lib.fbs_pub_create(C.byref(cp), bytes(32), one.ctypes.data, bytes(32), C.byref(h)),
                 lambda: lib.fbs_pub_expand(C.byref(cp), one.ctypes.data, 1, one.ctypes.data))
        for call in calls:
            assert call() == rc and err(lib) == want, (bad, want)
        assert w.value == 77 and not h.value and not one.any()


def test_fresh_streams_are_never_shared_and_run_out(world):
    from tfhe_fbs_map_amd import _public_native as pub
    prm, lib = world["prm"], world["lib"]
    N = prm.N
    enc = pub.Encryptor(prm, world["mask_key"], world["bodies"], bytes(32))
    _, a = enc.encrypt(np.zeros(N + 1, np.int64))
    _, b = enc.encrypt(np.zeros(1, np.int64))
    _, c = enc.encrypt(np.zeros(2 * N, np.int64))
    assert (a, b, c) == (1 << 55, (1 << 55) + 2, (1 << 55) + 3)                 # a sample takes a stream: ceil(count / N) per call
    taken, lock = [], threading.Lock()

    def worker(seed):
        rng = np.random.default_rng(seed)
        for _ in range(40):
            count = int(rng.integers(1, 3 * N))
            _, first = enc.encrypt(np.zeros(count, np.int64))
            with lock:
                taken.append((first, -(-count // N)))
    threads = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    taken.sort()
    assert len(taken) == 160 and taken[0][0] == (1 << 55) + 5
    for (f0, g0), (f1, _) in zip(taken, taken[1:]):
        assert f0 + g0 == f1                                                    # disjoint, and no stream skipped
    # the same (seed, nonce) gives the same sample -- which is why nobody may reuse one; two fresh calls never do
    x, _ = enc.encrypt(np.ones(3, np.int64), nonce0=12)
    y, _ = enc.encrypt(np.ones(3, np.int64), nonce0=12)
    z, _ = enc.encrypt(np.ones(3, np.int64))
    assert np.array_equal(x, y) and not np.array_equal(x[0, 0], z[0, 0])
    # exhaustion: more samples than [2^55, 2^56) has left is FBS_E_STATE, asked before anything is sized; the counter stays
    nxt = taken[-1][0] + taken[-1][1] + 1
    out, msgs, first = np.full(4, SENTINEL, np.uint64), np.zeros(4, np.int64), C.c_uint64(99)
    left = (1 << 56) - nxt
    assert lib.fbs_pub_encrypt_fresh(enc._h, msgs.ctypes.data, left * N + 1, out.ctypes.data, C.byref(first)) == E_STATE
    assert "used up" in err(lib, enc._h) and first.value == 99 and (out == SENTINEL).all()
    assert enc.encrypt(np.zeros(1, np.int64))[1] == nxt


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def test_public_key_and_inputs_round_trip(tmp_path, world):
    from tfhe_fbs_map_amd import PublicEncryptor, PublicInputs, PublicKey
    from tfhe_fbs_map_amd.split import mask_key_fingerprint
    for prm in (world["prm"], toy_sets()["k2_N256_g2"].replace(sampler=1)):
        bodies = np.random.default_rng(1).integers(0, Q, (prm.k, prm.N), dtype=np.uint64)
        key = PublicKey(prm, world["mask_key"], bodies)
        path = str(tmp_path / "pk.npz")
        key.save(path)
        back = PublicKey.load(path)
        assert back.params == prm and back.mask_key == world["mask_key"] and np.array_equal(back.bodies, bodies)
        assert back.fingerprint == mask_key_fingerprint(world["mask_key"]) == key.fingerprint
        with np.load(path, allow_pickle=False) as z:
            assert str(z["kind"]) == "public_key" and int(z["format_version"]) == 1 and ("sampler" in z.files) == bool(prm.sampler)
            assert sorted(z.files) == sorted(["kind", "format_version", "params", "mask_key", "fingerprint", "bodies"] + (["sampler"] if prm.sampler else []))
    with pytest.raises(ValueError, match="not a saved public_inputs"):
        PublicInputs.load(path)
    with pytest.raises(ValueError, match="words"):
        PublicKey(world["prm"], world["mask_key"], np.zeros(5, np.uint64))
    with pytest.raises(ValueError, match="32 bytes"):
        PublicKey(world["prm"], b"short", world["bodies"])
    key = PublicKey(world["prm"], world["mask_key"], world["bodies"])
    enc = PublicEncryptor(key, seed=bytes(range(32)))
    T = 200
    rng = np.random.default_rng(2)
    values = {"x": rng.integers(0, 2, T), "y": 1, "z": rng.integers(0, 2, T)}
    ins = enc.encrypt(values, ["x", "y", "z"], nonce0=3)
    assert ins.T == T and ins.samples.shape == (3, 2, 256) and ins.fingerprint == key.fingerprint and ins.input_names == ["x", "y", "z"]
    path = str(tmp_path / "in.npz")
    ins.save(path)
    back = PublicInputs.load(path)
    assert back.input_names == ins.input_names and back.T == T and np.array_equal(back.samples, ins.samples) and back.fingerprint == ins.fingerprint
    with pytest.raises(ValueError, match="not a saved public_key"):
        PublicKey.load(path)
    from tfhe_fbs_map_amd import _public_native as pub
    got = world["ctx"].decrypt(pub.expand(key.params, back.samples, 3 * T)).reshape(3, T)
    assert np.array_equal(got, np.stack([np.broadcast_to(values[n], (T,)) for n in ("x", "y", "z")]))
    with pytest.raises(ValueError, match="bits"):
        enc.encrypt({"x": [0, 2]}, ["x"])
    assert not np.array_equal(PublicEncryptor(key).encrypt(values, ["x"]).samples, PublicEncryptor(key).encrypt(values, ["x"]).samples)   # os.urandom seeds


def test_client_public_key_is_reproducible_and_opens_under_the_clients_secret():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, PublicEncryptor, parse_fbs
    from tfhe_fbs_map_amd import _public_native as pub
    rec = load_fixture("full_adder__search_p7")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = dict(fbs_size=7, params=toy_sets()["k3_N256_g2"])
    one, two, other = (Client(env, ExecConfig(seed=s, **cfg), host=True) for s in (5, 5, 6))
    key = one.public_key()
    assert key is one.public_key() and np.array_equal(key.bodies, two.public_key().bodies) and key.mask_key == one.server_key().mask_key
    assert not np.array_equal(key.bodies, other.public_key().bodies) and key.fingerprint == one.fingerprint and key.params == one.params
    names = env.lower()["input_names"]
    vals = {n: np.random.default_rng(i).integers(0, 2, 9) for i, n in enumerate(names)}
    ins = PublicEncryptor(key).encrypt(vals, names)
    got = one.ctx.decrypt(pub.expand(key.params, ins.samples, len(names) * 9)).reshape(len(names), 9)
    assert np.array_equal(got, np.stack([vals[n] for n in names]))


# ---- the noise rule and plan_chain ---------------------------------------------------------------------------------------------------
def test_public_input_noise_is_far_below_a_bootstraps():
    from tfhe_fbs_map_amd import choose_params
    from tfhe_fbs_map_amd.params import public_input_factor, public_input_variance, variances
    for p in (2, 4, 7, 8, 15, 31):
        prm = choose_params(p)
        v = public_input_variance(prm)
        assert v == (1 + prm.k * prm.N) * (prm.sigma_glwe / Q) ** 2
        assert public_input_factor(prm) == v / variances(prm)[0] and 0 < public_input_factor(prm) < 1e-6, p


def _adder():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture("adder8__search_p7")
    return parse_fbs(rec["fbs"], inputs=rec["program_inputs"])


def test_plan_chain_on_public_inputs():
    from tfhe_fbs_map_amd import ExecConfig
    from tfhe_fbs_map_amd.params import public_input_factor, refresh_margin, refresh_margin_needed
    from tfhe_fbs_map_amd.public import PublicInputs, public_sample_shape
    from tfhe_fbs_map_amd.split import EncryptedInputs, PlainInputs, client_choice, plan_chain
    env = _adder()
    prm, fuse = client_choice(env, ExecConfig(), [env])
    fp, T = bytes(8), 70
    a_names, b_names = [f"a{i}" for i in range(8)], [f"b{i}" for i in range(8)]
    shape = public_sample_shape(prm, 8, T)
    assert shape == (-(-8 * T // prm.N), prm.k + 1, prm.N)
    pub_a = PublicInputs(a_names, T, np.zeros(shape, np.uint64), fp)
    seeded_b = EncryptedInputs(b_names[:7], T, 100, np.zeros((7, T), np.uint64), fp)
    plain = PlainInputs(["b7"], None, {"b7": 1})
    links, got_T = plan_chain(prm, fuse, fp, env, [pub_a, seeded_b, plain])
    assert got_T == T and [ln.name for ln in links] == env.lower()["input_names"]
    factor = public_input_factor(prm)
    assert 0 < factor <= 1
    for i in range(8):
        assert (links[i].kind, links[i].source, links[i].index, links[i].refresh, links[i].noise, links[i].margin) == ("public", 0, i, False, factor, None)
    assert [ln.kind for ln in links[8:]] == ["seeded"] * 7 + ["plain"]
    # renamed, and as the only source of everything
    both = PublicInputs([f"x{i}" for i in range(16)], T, np.zeros(public_sample_shape(prm, 16, T), np.uint64), fp)
    links, _ = plan_chain(prm, fuse, fp, env, [both], rename={n: f"x{i}" for i, n in enumerate(env.lower()["input_names"])})
    assert all(ln.kind == "public" and ln.index == i for i, ln in enumerate(links))
    # held to the fingerprint and to T like an EncryptedInputs
    with pytest.raises(ValueError, match="another server key"):
        plan_chain(prm, fuse, fp, env, [PublicInputs(a_names, T, np.zeros(shape, np.uint64), bytes(range(8))), seeded_b, plain])
    with pytest.raises(ValueError, match="T = 71 samples where the others have 70"):
        plan_chain(prm, fuse, fp, env, [pub_a, EncryptedInputs(b_names[:7], 71, 100, np.zeros((7, 71), np.uint64), fp), plain])
    # a sample array that does not fit the parameter set and T
    for wrong in ((shape[0] + 1,) + shape[1:], (shape[0], shape[1] + 1, shape[2]), (shape[0], shape[1], shape[2] // 2), shape[1:]):
        with pytest.raises(ValueError, match=r"input a0: public-key samples of shape .* need \(%d, %d, %d\)" % shape):
            plan_chain(prm, fuse, fp, env, [PublicInputs(a_names, T, np.zeros(wrong, np.uint64), fp), seeded_b, plain])
    with pytest.raises(ValueError, match="ambiguous"):
        plan_chain(prm, fuse, fp, env, [pub_a, pub_a, seeded_b, plain])

    # The refresh rule, at a made-up set whose factor exceeds 1.  (1 + kN) sigma^2 above one blind rotation's output variance takes
    # one key bit, one gadget level of base 2 and a noise of 8 q, which no library would take: plan_chain is arithmetic.  Exactly the
    # full-link rule: refresh_margin(params, None, factor) against refresh_margin_needed at the program's norm2 -- the adder's 11
    # leaves room for the factor, a program of norm2 = 1 does not.
    from tfhe_fbs_map_amd import Params, parse_fbs
    loud = Params(n=1, log_n_poly=8, k=1, l_bsk=1, beta_bsk=1, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1, sigma_glwe=8 * Q)
    factor = public_input_factor(loud)
    assert 1.0 < factor < 1.01
    norm2 = env.stats()["norm2_linprod"]
    margin = refresh_margin(loud, None, factor)
    assert margin >= refresh_margin_needed(loud, norm2) and norm2 > factor
    pub_loud = PublicInputs(a_names, T, np.zeros(public_sample_shape(loud, 8, T), np.uint64), fp)
    links, _ = plan_chain(loud, False, fp, env, [pub_loud, seeded_b, plain], min_margin=0.0)
    assert all((ln.kind, ln.refresh, ln.noise, ln.margin) == ("public", True, 1.0, margin) for ln in links[:8])
    assert [(ln.kind, ln.refresh) for ln in links[8:]] == [("seeded", False)] * 7 + [("plain", False)]
    single = parse_fbs("m1 = 1 * a\nm2 = Bootstrap(m1, [0, 1])\nOutput x = m2\n", inputs=["a"])
    assert single.stats()["norm2_linprod"] == 1 and margin < refresh_margin_needed(loud, 1)
    one = PublicInputs(["a"], T, np.zeros(public_sample_shape(loud, 1, T), np.uint64), fp)
    with pytest.raises(ValueError, match="input a: its refresh would keep .*public-key noise factor"):
        plan_chain(loud, False, fp, single, [one], min_margin=0.0)
    quiet = loud.replace(sigma_glwe=Q // 2)                 # the same shape below 1: in as it is
    assert public_input_factor(quiet) < 1
    links, _ = plan_chain(quiet, False, fp, single, [one], min_margin=0.0)
    assert (links[0].kind, links[0].refresh, links[0].noise) == ("public", False, public_input_factor(quiet))
