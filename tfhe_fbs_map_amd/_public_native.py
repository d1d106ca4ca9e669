"""ctypes binding of libfbspublic.so: the public-key encryptor's part of include/fbs_exec.h ("public-key inputs").

A data owner who holds neither the secret key nor a GPU encrypts inputs under a public key the key holder published.
libfbspublic.so is the host code of those entries built alone (`make -C tfhe_fbs_map_amd/csrc public`: a C++ compiler, no ROCm)
and exports the nine host `fbs_pub_*` entries and nothing else; libfbsexec.so holds the same code, so where only that library
has been built -- and `_native` has loaded it -- the entries are taken from there.

This module imports numpy, ctypes and `_client_native` (itself numpy and ctypes only): neither torch nor `_native`.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from ._client_native import FbsError, _c, _Params, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FBS_PUBLIC_LIB") or os.path.join(_HERE, "libfbspublic.so")

_vp, _u64, _sz, _i32 = C.c_void_p, C.c_uint64, C.c_size_t, C.c_int
# the host entries: what libfbspublic.so exports, and libfbsexec.so beside its own two
SIGNATURES = {
    "fbs_pub_key_words": (_i32, [C.POINTER(_Params), C.POINTER(_sz)]),
    "fbs_pub_keygen": (_i32, [C.POINTER(_Params), _vp, _vp, _vp, _vp]),
    "fbs_pub_create": (_i32, [C.POINTER(_Params), _vp, _vp, _vp, C.POINTER(_vp)]),
    "fbs_pub_destroy": (None, [_vp]),
    "fbs_pub_last_error": (C.c_char_p, [_vp]),
    "fbs_pub_words": (_i32, [C.POINTER(_Params), _sz, C.POINTER(_sz)]),
    "fbs_pub_encrypt": (_i32, [_vp, _vp, _sz, _u64, _vp]),
    "fbs_pub_encrypt_fresh": (_i32, [_vp, _vp, _sz, _vp, C.POINTER(_u64)]),
    "fbs_pub_expand": (_i32, [C.POINTER(_Params), _vp, _sz, _vp]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def bind(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not match the header
        fn.restype = res
        fn.argtypes = args
    return lib


def public_library_present():
    return os.path.exists(LIB_PATH)


_lib_handle = None


def _lib():
    """libfbspublic.so, loaded on first use; where it has not been built, the GPU library `_native` has loaded"""
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if os.path.exists(LIB_PATH):
        _lib_handle = bind(C.CDLL(LIB_PATH))
        return _lib_handle
    native = sys.modules.get(__package__ + "._native")
    lib = native.__dict__.get("lib") if native is not None else None
    if lib is None:
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C tfhe_fbs_map_amd/csrc public` (a C++17 compiler is all it needs)")
    _lib_handle = bind(lib)
    return _lib_handle


def _fail(rc, handle=None):
    raise FbsError(rc, (_lib().fbs_pub_last_error(handle) or b"").decode())


def _bytes32(b, what):
    b = bytes(b)
    if len(b) != 32:
        raise ValueError(f"{what} has 32 bytes")
    return b


def key_words(prm):
    """k N, the words of a public key's bodies (fbs_pub_key_words)"""
    w = C.c_size_t()
    rc = _lib().fbs_pub_key_words(C.byref(prm.to_c()), C.byref(w))
    if rc:
        _fail(rc)
    return int(w.value)


def sample_words(prm, count):
    """ceil(count / N) (k + 1) N, the words of `count` encrypted messages (fbs_pub_words)"""
    w = C.c_size_t()
    rc = _lib().fbs_pub_words(C.byref(prm.to_c()), int(count), C.byref(w))
    if rc:
        _fail(rc)
    return int(w.value)


def keygen(prm, mask_key, sk_glwe, noise_seed):
    """fbs_pub_keygen: the bodies [k][N] of the public key for the GLWE secret `sk_glwe` (as `export_keys` returns it) under the
    public mask key, the noise drawn under the 32-byte `noise_seed`"""
    sk = _c(sk_glwe, np.uint64).reshape(-1)
    if sk.size != prm.k * prm.N:
        raise ValueError(f"a GLWE secret of {sk.size} words, the parameter set has {prm.k * prm.N}")
    bodies = np.empty((prm.k, prm.N), np.uint64)
    rc = _lib().fbs_pub_keygen(C.byref(prm.to_c()), _bytes32(mask_key, "a mask key"), _ptr(sk), _bytes32(noise_seed, "a noise seed"), _ptr(bodies))
    if rc:
        _fail(rc)
    return bodies


def expand(prm, glwe, count):
    """fbs_pub_expand (host): samples [ceil(count / N)][k+1][N] -> big-key ciphertexts [count][D+1]"""
    glwe = _c(glwe, np.uint64).reshape(-1)
    count = int(count)
    if glwe.size != sample_words(prm, count):
        raise ValueError(f"{glwe.size} sample words for {count} messages (the parameter set needs {sample_words(prm, count)})")
    cts = np.empty((count, prm.ct_words), np.uint64)
    rc = _lib().fbs_pub_expand(C.byref(prm.to_c()), _ptr(glwe), count, _ptr(cts))
    if rc:
        _fail(rc)
    return cts


class Encryptor:
    """fbs_pub: a public key and the key the encryptor's own randomness is expanded from (32 bytes; None: from os.urandom)."""

    def __init__(self, prm, mask_key, bodies, seed=None):
        self.params = prm
        self._h = None
        bodies = _c(bodies, np.uint64).reshape(-1)
        if bodies.size != prm.k * prm.N:
            raise ValueError(f"public-key bodies of {bodies.size} words, the parameter set needs {prm.k * prm.N}")
        h = C.c_void_p()
        rc = _lib().fbs_pub_create(C.byref(prm.to_c()), _bytes32(mask_key, "a mask key"), _ptr(bodies),
                                   _bytes32(os.urandom(32) if seed is None else seed, "a seed"), C.byref(h))
        if rc:
            _fail(rc)
        self._h = h

    def encrypt(self, msgs, nonce0=None):
        """messages in [0, 2p), flattened in C order -> (samples [G][k+1][N], first stream).  Sample g takes stream nonce0 + g;
        None: streams this encryptor has not used."""
        msgs = _c(msgs, np.int64).reshape(-1)
        prm = self.params
        glwe = np.empty((-(-msgs.size // prm.N), prm.k + 1, prm.N), np.uint64)
        if nonce0 is None:
            first = C.c_uint64()
            rc = _lib().fbs_pub_encrypt_fresh(self._h, _ptr(msgs), msgs.size, _ptr(glwe), C.byref(first))
            nonce0 = first.value
        else:
            rc = _lib().fbs_pub_encrypt(self._h, _ptr(msgs), msgs.size, int(nonce0), _ptr(glwe))
        if rc:
            _fail(rc, self._h)
        return glwe, int(nonce0)

    def close(self):
        if getattr(self, "_h", None) and _lib_handle is not None:      # (None while the interpreter shuts down)
            _lib_handle.fbs_pub_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()
