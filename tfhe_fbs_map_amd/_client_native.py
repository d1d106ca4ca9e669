"""ctypes binding of libfbsclient.so: the client's part of include/fbs_exec.h ("client library") on a machine with no GPU.

The holder of the secret key makes keys, encrypts inputs and reads results; none of that touches a device.  libfbsclient.so is
the host code of libfbsexec.so built alone (`make -C tfhe_fbs_map_amd/csrc client`: a C++ compiler, no ROCm), and `HostContext`
carries the client's subset of `_native.Context` under the same names, arguments and return shapes.  For the same parameter
set and seed every word it writes is the word the GPU library writes.

This module imports neither torch nor `_native`, and loads its library on first use: `_native` takes `Params`, `FbsError` and
the small helpers from here, and must import where only libfbsexec.so has been built.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import types
from dataclasses import dataclass, asdict

import numpy as np

from .security import MODULUS, MODULUS_BITS, sigma_min      # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FBS_CLIENT_LIB") or os.path.join(_HERE, "libfbsclient.so")
DEVICE_NONE = -1   # FBS_DEVICE_NONE


RANDOMNESS_GRADE = ("test-grade: ChaCha20 streams keyed by the context seed; noise = integer Irwin-Hall(12) stand-in for a discrete "
                    "Gaussian, bounded at 6 sigma.  Bring keys made with a production sampler through Context.import_keys")
# what Params.sampler = 1 / ExecConfig(sampler="gaussian") draws instead (include/fbs_exec.h, RANDOMNESS GRADE); sampler 0, the text
# above, stays the default: the oracle and the known-answer tests pin its streams
GAUSSIAN_SAMPLER_GRADE = ("opt-in: a double-precision rounded Gaussian (Box-Muller on the ChaCha20 stream keyed from the caller's 32 "
                          "bytes, rounded to the nearest integer, tail to 13.3 sigma), bit-identical on host and GPU; not constant-time, "
                          "not a certified discrete Gaussian, not audited")
SAMPLERS = {"irwin_hall": 0, "gaussian": 1}


def sampler_id(sampler):
    """0 / 1 or their names "irwin_hall" / "gaussian" -> fbs_params.sampler"""
    if isinstance(sampler, str):
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler is one of {sorted(SAMPLERS)}, not {sampler!r}")
        return SAMPLERS[sampler]
    return int(sampler)


class FbsError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libfbsexec error {code}: {text}")
        self.code = code


class _Params(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in
                ("n", "log_n_poly", "k", "l_bsk", "beta_bsk", "t_ksk", "gamma_ksk", "p_msg")] + \
               [("sigma_lwe", C.c_uint64), ("sigma_glwe", C.c_uint64), ("bsk_group", C.c_uint32), ("sampler", C.c_uint32)]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


@dataclass(frozen=True)
class Params:
    """Cryptographic parameter set.  The shape defaults to BASELINE.md's synthetic set (n=630 N=1024 k=1 l=3 beta=7
    t=8 gamma=2).  A noise left at None becomes the smallest standard deviation that is 128-bit secure at its
    dimension (`security.sigma_min`); anything lower is an explicit choice -- `reduced_noise()` is the benchmark
    setting (2^-40 q, NOT secure), `params.P1024` the benchmark set built with it, `params.choose_params` the
    selector that returns secure AND correct sets."""
    n: int = 630
    log_n_poly: int = 10
    k: int = 1
    l_bsk: int = 3
    beta_bsk: int = 7
    t_ksk: int = 8
    gamma_ksk: int = 2
    p_msg: int = 15
    sigma_lwe: int | None = None      # key-switching-key noise, absolute units of 1/q
    sigma_glwe: int | None = None     # bootstrapping-key and fresh-input noise
    bsk_group: int = 1                # key bits per blind-rotation step: 1, or 2 (n/2 steps on bundles of 3 GGSW samples)
    sampler: int = 0                  # noise sampler: 0 Irwin-Hall (reproducible / test-grade, the default), 1 rounded Gaussian

    def __post_init__(self):
        if self.sigma_lwe is None:
            object.__setattr__(self, "sigma_lwe", sigma_min(self.n))
        if self.sigma_glwe is None:
            object.__setattr__(self, "sigma_glwe", sigma_min(self.k * (1 << self.log_n_poly)))

    @classmethod
    def for_poly_size(cls, poly_size: int, **kw):
        """Parameter set for polynomial size N.  A non-power-of-two N (BASELINE config 5 names one) raises
        FbsError(FBS_E_POLY_SIZE): see include/fbs_exec.h `fbs_poly_size_check` for why that ring is refused."""
        lib = _any_lib()
        rc = lib.fbs_poly_size_check(int(poly_size))
        if rc != 0:
            raise FbsError(rc, lib.fbs_last_error(None).decode())
        return cls(log_n_poly=int(poly_size).bit_length() - 1, **kw)

    def reduced_noise(self, sigma: int = 1 << 6):
        """The same shape with both noises at `sigma` (default 2^6 = 2^-40 q): throughput benchmarks and parity tests
        only -- far below what any security level needs at these dimensions."""
        return self.replace(sigma_lwe=sigma, sigma_glwe=sigma)

    @property
    def N(self):
        return 1 << self.log_n_poly

    @property
    def big_dim(self):
        return self.k * self.N

    @property
    def ct_words(self):
        return self.big_dim + 1

    def replace(self, **kw):
        d = asdict(self)
        d.update(kw)
        return Params(**d)

    def to_c(self):
        return _Params(**asdict(self))

    def bytes_per_fbs(self):
        """Algorithmic bytes one FBS must consume: every
        bootstrapping-key row and key-switching-key row once, its input and
        output ciphertext and its test vector."""
        N, k, n = self.N, self.k, self.n
        ggsw = (k + 1) * self.l_bsk * (k + 1) * N * 8
        bsk = (n // 2 * 3 if self.bsk_group == 2 else n) * ggsw
        ksk = k * N * self.t_ksk * (n + 1) * 8
        return bsk + ksk + 2 * (k * N + 1) * 8 + N * 8


def gpu_library_path():
    """where `_native` looks for libfbsexec.so (FBS_LIB: kernel-variant experiments)"""
    return os.environ.get("FBS_LIB") or os.path.join(_HERE, "libfbsexec.so")


def gpu_library_missing(path):
    """what importing `_native` says without libfbsexec.so -- and what the first use of anything that needs it says where the
    package was imported with the client library alone"""
    return (f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  tfhe_fbs_map_amd has no CPU fallback.")


_vp, _u64, _u32, _sz, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t, C.c_int
# the client's entries: what libfbsclient.so exports, and libfbsexec.so beside its own
SIGNATURES = {
    "fbs_poly_size_check": (_i32, [_u32]),
    "fbs_ctx_create": (_i32, [C.POINTER(_Params), _u64, _i32, C.POINTER(_vp)]),
    "fbs_ctx_create_seeded": (_i32, [C.POINTER(_Params), _vp, _i32, C.POINTER(_vp)]),
    "fbs_ctx_destroy": (None, [_vp]),
    "fbs_ctx_stat": (_i32, [_vp, C.c_char_p, C.POINTER(C.c_int64)]),
    "fbs_last_error": (C.c_char_p, [_vp]),
    "fbs_device_info": (C.c_char_p, [_vp]),
    "fbs_keygen": (_i32, [_vp]),
    "fbs_key_sizes": (_i32, [_vp, C.POINTER(_sz * 4)]),
    "fbs_export_keys": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "fbs_keygen_seeded": (_i32, [_vp]),
    "fbs_seeded_key_sizes": (_i32, [_vp, C.POINTER(_sz * 2)]),
    "fbs_export_seeded_keys": (_i32, [_vp, _vp, _vp, _vp]),
    "fbs_encrypt": (_i32, [_vp, _vp, _sz, _u64, _vp]),
    "fbs_encrypt_fresh": (_i32, [_vp, _vp, _sz, _vp, C.POINTER(_u64)]),
    "fbs_decrypt": (_i32, [_vp, _vp, _sz, _vp]),
    "fbs_encrypt_seeded": (_i32, [_vp, _vp, _sz, _u64, _vp]),
    "fbs_encrypt_seeded_fresh": (_i32, [_vp, _vp, _sz, _vp, C.POINTER(_u64)]),
    "fbs_expand_seeded": (_i32, [_vp, _vp, _sz, _u64, _vp]),
    "fbs_compact_words": (_i32, [_vp, _u32, C.POINTER(_sz)]),
    "fbs_decrypt_compact": (_i32, [_vp, _vp, _sz, _u32, _vp]),
    "fbs_packing_keygen": (_i32, [_vp, _u32, _u32]),
    "fbs_packing_key_sizes": (_i32, [_vp, _u32, C.POINTER(_sz * 2)]),
    "fbs_export_packing_key": (_i32, [_vp, _vp, _vp]),
    "fbs_packed_words": (_i32, [_vp, _sz, _u32, C.POINTER(_sz)]),
    "fbs_decrypt_packed": (_i32, [_vp, _vp, _sz, _u32, _vp]),
    "fbs_debug_raise": (_i32, [_vp, _i32]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)


_lib_handle = None


def _lib():
    """libfbsclient.so, loaded on first use"""
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C tfhe_fbs_map_amd/csrc client` (a C++17 compiler is all it needs)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not match the header
        fn.restype = res
        fn.argtypes = args
    _lib_handle = lib
    return lib


def _any_lib():
    """a library that serves the entries both have and no context needs (fbs_poly_size_check): the GPU library where `_native`
    has loaded it, as before there was a choice, else the client library"""
    native = sys.modules.get(__package__ + "._native")
    lib = getattr(native, "lib", None) if isinstance(native, types.ModuleType) and not isinstance(native, _GpuLibraryMissing) else None
    return lib if lib is not None else _lib()


def client_library_present():
    return os.path.exists(LIB_PATH)


class _GpuLibraryMissing(types.ModuleType):
    """Stands in for `_native` where the package was imported with the client library alone: what a client needs resolves to
    this module's definitions, anything else raises the ImportError that importing `_native` itself raises there."""
    _SHARED = ("RANDOMNESS_GRADE", "GAUSSIAN_SAMPLER_GRADE", "SAMPLERS", "sampler_id", "FbsError", "Params", "_Params", "_c", "_ptr", "MODULUS", "MODULUS_BITS", "sigma_min")

    def __getattr__(self, name):
        if name in self._SHARED:
            return globals()[name]
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        raise ImportError(gpu_library_missing(gpu_library_path()))


def gpu_library_stand_in(name):
    mod = _GpuLibraryMissing(name, _GpuLibraryMissing.__doc__)
    mod.LIB_PATH = gpu_library_path()
    return mod


class ClientContext:
    """One parameter set, one key set, and what the holder of the secret does with them on host arrays: the entries of
    `SIGNATURES`, written once for `HostContext` (libfbsclient.so) and `_native.Context` (libfbsexec.so, which adds the GPU's).
    A subclass names its library (`_lib`) and closes its handle (`close`)."""

    def __init__(self, params: Params, seed: int | bytes | None = None, keygen: bool = False):
        """seed: as `Context` -- an int is the reproducible form (fbs_ctx_create), None or 32 bytes fbs_ctx_create_seeded (None:
        from os.urandom).  keygen=True: `keygen()` at once."""
        self._create(params, seed, DEVICE_NONE)
        if keygen:
            self.keygen()

    def _create(self, params, seed, device):
        """the context handle, in the seed's form, on `device`"""
        lib = self._lib
        self.params = params
        self.seed = seed
        self._h = C.c_void_p()
        cp = params.to_c()
        if isinstance(seed, int):
            rc = lib.fbs_ctx_create(C.byref(cp), seed, device, C.byref(self._h))
        else:
            raw = os.urandom(32) if seed is None else bytes(seed)
            if len(raw) != 32:
                raise ValueError("a byte seed has 32 bytes")
            rc = lib.fbs_ctx_create_seeded(C.byref(cp), raw, device, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise FbsError(rc, lib.fbs_last_error(None).decode())

    @property
    def _lib(self):
        """the loaded library that serves `SIGNATURES`"""
        raise NotImplementedError("ClientContext is the shared part of HostContext and Context: make one of those")

    def close(self):
        """fbs_ctx_destroy through the subclass's library, once"""
        raise NotImplementedError

    def _check(self, rc):
        if rc != 0:
            raise FbsError(rc, self._lib.fbs_last_error(self._h).decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self.close()

    @property
    def device_info(self):
        return self._lib.fbs_device_info(self._h).decode()

    def stat(self, name):
        v = C.c_int64()
        self._check(self._lib.fbs_ctx_stat(self._h, name.encode(), C.byref(v)))
        return v.value

    def keygen(self):
        self._check(self._lib.fbs_keygen(self._h))

    def export_keys(self):
        sizes = (C.c_size_t * 4)()
        self._check(self._lib.fbs_key_sizes(self._h, C.byref(sizes)))
        arrs = [np.empty(sizes[i], np.uint64) for i in range(4)]
        self._check(self._lib.fbs_export_keys(self._h, *[_ptr(a) for a in arrs]))
        return dict(sk_lwe=arrs[0], sk_glwe=arrs[1], bsk=arrs[2], ksk=arrs[3])

    # ---- seeded path: masks under a public key, only bodies travel (include/fbs_exec.h) ----
    def keygen_seeded(self):
        """fbs_keygen_seeded: keys whose masks a server regenerates from the public mask key (`export_seeded_keys`)."""
        self._check(self._lib.fbs_keygen_seeded(self._h))

    def seeded_key_sizes(self):
        sizes = (C.c_size_t * 2)()
        self._check(self._lib.fbs_seeded_key_sizes(self._h, C.byref(sizes)))
        return int(sizes[0]), int(sizes[1])

    def export_seeded_keys(self):
        """The server key: dict(mask_key=32 bytes, bsk_bodies, ksk_bodies).  Holds no secret."""
        nb, nk = self.seeded_key_sizes()
        mk = np.zeros(32, np.uint8)
        bsk, ksk = np.empty(nb, np.uint64), np.empty(nk, np.uint64)
        self._check(self._lib.fbs_export_seeded_keys(self._h, _ptr(mk), _ptr(bsk), _ptr(ksk)))
        return dict(mask_key=mk.tobytes(), bsk_bodies=bsk, ksk_bodies=ksk)

    def encrypt(self, msgs, nonce0=None):
        """nonce0=None: streams nobody has used (the context counts them: no two calls share mask or noise); an int: ciphertext
        i takes stream nonce0 + i -- reproducible, for tests and checkers."""
        msgs = _c(msgs, np.int64)
        cts = np.empty(msgs.shape + (self.params.ct_words,), np.uint64)
        if nonce0 is None:
            self._check(self._lib.fbs_encrypt_fresh(self._h, _ptr(msgs), msgs.size, _ptr(cts), None))
        else:
            self._check(self._lib.fbs_encrypt(self._h, _ptr(msgs), msgs.size, nonce0, _ptr(cts)))
        return cts

    def decrypt(self, cts):
        cts = _c(cts, np.uint64)
        out = np.empty(cts.shape[:-1], np.int64)
        self._check(self._lib.fbs_decrypt(self._h, _ptr(cts), out.size, _ptr(out)))
        return out

    def encrypt_seeded(self, msgs, nonce0=None):
        """Seeded encryption: (bodies with the shape of msgs, first stream).  Ciphertext i takes stream nonce0 + i; None = streams
        nobody has used (the counter of `encrypt`)."""
        msgs = _c(msgs, np.int64)
        bodies = np.empty(msgs.shape, np.uint64)
        if nonce0 is None:
            first = C.c_uint64()
            self._check(self._lib.fbs_encrypt_seeded_fresh(self._h, _ptr(msgs), msgs.size, _ptr(bodies), C.byref(first)))
            return bodies, first.value
        self._check(self._lib.fbs_encrypt_seeded(self._h, _ptr(msgs), msgs.size, int(nonce0), _ptr(bodies)))
        return bodies, int(nonce0)

    def expand_seeded(self, bodies, nonce0):
        """fbs_expand_seeded (host): bodies of streams nonce0, nonce0 + 1, .. -> full ciphertexts [..][D+1]"""
        bodies = _c(bodies, np.uint64)
        cts = np.empty(bodies.shape + (self.params.ct_words,), np.uint64)
        self._check(self._lib.fbs_expand_seeded(self._h, _ptr(bodies), bodies.size, int(nonce0), _ptr(cts)))
        return cts

    # ---- compact outputs (include/fbs_exec.h) ----
    @property
    def default_compact_bits(self):
        """log2(2N): the width the blind rotation reads, and the narrowest compact width"""
        return self.params.log_n_poly + 1

    def compact_words(self, bits=None):
        """W, the uint64 words of one compact ciphertext at width `bits` (None: log2(2N)); FbsError(FBS_E_INVALID) outside
        [log2(2N), 31]"""
        w = C.c_size_t()
        self._check(self._lib.fbs_compact_words(self._h, self.default_compact_bits if bits is None else int(bits), C.byref(w)))
        return int(w.value)

    def _compact_io(self, words, bits):
        """(the width, the words as uint64 [..][W], empty messages [..]) of a compact decryption; ValueError on another W"""
        bits = self.default_compact_bits if bits is None else int(bits)
        words = _c(words, np.uint64)
        W = words.shape[-1] if words.ndim else 0
        out = np.empty(words.shape[:-1], np.int64)
        if out.size and W != self.compact_words(bits):
            raise ValueError(f"compact ciphertexts of {W} words at {bits} bits (the parameter set needs {self.compact_words(bits)})")
        return bits, words, out

    def decrypt_compact(self, words, bits=None):
        """Compact ciphertexts [..][W] -> messages [..] (fbs_decrypt_compact, on the host)"""
        bits, words, out = self._compact_io(words, bits)
        self._check(self._lib.fbs_decrypt_compact(self._h, _ptr(words), out.size, bits, _ptr(out)))
        return out

    # ---- packed outputs (include/fbs_exec.h, "packed outputs") ----
    def packing_keygen(self, t_p, gamma_p):
        """fbs_packing_keygen: the packing key (t_p levels of gamma_p bits) beside the keys of `keygen_seeded`"""
        self._check(self._lib.fbs_packing_keygen(self._h, int(t_p), int(gamma_p)))

    def _gadget_key_sizes(self, noun, t):
        """fbs_<noun>_key_sizes: the sizes of the packing key or (the GPU library's) of the fold key"""
        sizes = (C.c_size_t * 2)()
        self._check(getattr(self._lib, f"fbs_{noun}_key_sizes")(self._h, int(t), C.byref(sizes)))
        return int(sizes[0]), int(sizes[1])

    def _export_gadget_key(self, noun, rows, full):
        """fbs_export_<noun>_key: dict(<noun>_levels, <noun>_base_bits, <noun>_bodies [rows][t][N]), and `full` [rows][t][k+1][N]"""
        nb, nf = self._gadget_key_sizes(noun, 0)
        bodies = np.empty(nb, np.uint64)
        whole = np.empty(nf, np.uint64) if full else None
        self._check(getattr(self._lib, f"fbs_export_{noun}_key")(self._h, _ptr(bodies), _ptr(whole)))
        out = {f"{noun}_levels": self.stat(f"{noun}_levels"), f"{noun}_base_bits": self.stat(f"{noun}_base_bits"), f"{noun}_bodies": bodies}
        if full:
            out["full"] = whole.reshape(rows, out[f"{noun}_levels"], self.params.k + 1, self.params.N)
        return out

    def packing_key_sizes(self, t_p=0):
        """(bodies, whole key) in words for t_p levels (0: the context's own key)"""
        return self._gadget_key_sizes("packing", t_p)

    def export_packing_key(self, full=False):
        """dict(packing_levels, packing_base_bits, packing_bodies [n][t_p][N]); full=True adds `full`, the whole key
        [n][t_p][k+1][N] in the coefficient domain (a test hook)"""
        return self._export_gadget_key("packing", self.params.n, full)

    def packed_words(self, count, bits):
        """uint64 words of `count` outputs packed at width `bits` (fbs_packed_words)"""
        w = C.c_size_t()
        self._check(self._lib.fbs_packed_words(self._h, int(count), int(bits), C.byref(w)))
        return int(w.value)

    def decrypt_packed(self, words, count, bits):
        """Packed words of `count` outputs -> messages [count] (fbs_decrypt_packed, on the host)"""
        words = _c(words, np.uint64).ravel()
        if words.size != self.packed_words(count, bits):
            raise ValueError(f"{words.size} packed words for {count} outputs at {bits} bits (the parameter set needs {self.packed_words(count, bits)})")
        out = np.empty(int(count), np.int64)
        self._check(self._lib.fbs_decrypt_packed(self._h, _ptr(words), int(count), int(bits), _ptr(out)))
        return out


class HostContext(ClientContext):
    """One parameter set, one key set, on the host: the client's subset of `_native.Context` (libfbsclient.so)."""

    @property
    def _lib(self):
        return _lib()

    def close(self):
        if getattr(self, "_h", None) and _lib_handle is not None:      # (None while the interpreter shuts down)
            _lib_handle.fbs_ctx_destroy(self._h)
            self._h = None
