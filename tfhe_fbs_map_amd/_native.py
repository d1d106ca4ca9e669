"""ctypes binding of libfbsexec.so (C ABI: include/fbs_exec.h).

There is deliberately no fallback: if the shared library is missing or cannot be
loaded, importing this module raises, and if no gfx950 GPU is present
`Context(...)` raises `FbsError` -- the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FBS_LIB") or os.path.join(_HERE, "libfbsexec.so")   # FBS_LIB: kernel-variant experiments

from .security import MODULUS, MODULUS_BITS, sigma_min      # noqa: E402,F401
# what a client shares with this module lives in `_client_native`, which needs neither this library nor a GPU
from . import _client_native, _public_native      # noqa: E402
from ._client_native import GAUSSIAN_SAMPLER_GRADE, RANDOMNESS_GRADE, SAMPLERS, ClientContext, FbsError, Params, _Params, _c, _ptr, gpu_library_missing      # noqa: E402,F401


class _Layout(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("n_slots", "n_levels", "max_width", "max_sources", "n_bootstrap", "n_keyswitch",
                                          "n_inputs", "n_outputs", "n_rotations", "row_words")]


class _ProgramDesc(C.Structure):
    _fields_ = [("n_inputs", C.c_uint32), ("n_instr", C.c_uint32), ("n_terms", C.c_uint32),
                ("n_outputs", C.c_uint32),
                ("kind", C.c_void_p), ("arg0", C.c_void_p), ("arg1", C.c_void_p),
                ("const_coef", C.c_void_p), ("term_coef", C.c_void_p), ("term_src", C.c_void_p),
                ("out_wire", C.c_void_p)]


class _InputSrc(C.Structure):   # fbs_input_src (include/fbs_exec.h, "chained evaluation")
    _fields_ = [("kind", C.c_uint32), ("bits", C.c_uint32), ("refresh", C.c_uint32), ("nonce0", C.c_uint64),
                ("data", C.c_void_p)]


class _ResidentSrc(C.Structure):   # fbs_resident_src (include/fbs_exec.h, "resident state")
    _fields_ = [("state", C.c_void_p), ("row", C.c_uint32), ("refresh", C.c_uint32)]


class _SampleMap(C.Structure):   # fbs_sample_map (include/fbs_exec.h, "sample-axis operations")
    _fields_ = [("index", C.c_void_p), ("fill", C.c_int64)]


SAMPLE_NONE = 0xFFFFFFFF   # FBS_SAMPLE_NONE
MAX_SUM_GROUP = 65536      # FBS_MAX_SUM_GROUP


class _AuditRow(C.Structure):   # fbs_audit_row (include/fbs_exec.h, "audited evaluation")
    _fields_ = [("count", C.c_uint64), ("over", C.c_uint64), ("max_abs", C.c_uint64), ("sum", C.c_int64),
                ("sumsq_lo", C.c_uint64), ("sumsq_hi", C.c_uint64)]


AUDIT_INPUTS, AUDIT_LINCOMB, AUDIT_ROTATION_INPUT, AUDIT_BOOTSTRAP = 0, 1, 2, 3   # FBS_AUDIT_*
AUDIT_MAX_SAMPLES = 1 << 18   # samples a row one fbs_audit_level_dev call takes

SRC_SEEDED, SRC_FULL, SRC_COMPACT, SRC_PLAIN = 0, 1, 2, 3   # FBS_SRC_*


def _input_src(source, T, ctw):
    """one feed tuple of `Program.eval_sources` -> (fbs_input_src, the array it points into)"""
    kind = source[0]
    if kind == "plain":
        _, data = source
        if np.ndim(data) == 0:   # one message for every sample
            a = np.array([operator.index(data)], np.int64)
            return _InputSrc(SRC_PLAIN, 1, 0, 0, a.ctypes.data), a
        a = _c(data, np.int64).reshape(T)
        return _InputSrc(SRC_PLAIN, 0, 0, 0, a.ctypes.data), a
    _, data, arg = source
    if kind == "seeded":
        a = _c(data, np.uint64).reshape(T)
        return _InputSrc(SRC_SEEDED, 0, 0, int(arg), a.ctypes.data), a
    if kind == "full":
        a = _c(data, np.uint64).reshape(T, ctw)
        return _InputSrc(SRC_FULL, 0, int(bool(arg)), 0, a.ctypes.data), a
    if kind == "compact":
        a = _c(data, np.uint64).reshape(T, -1)
        return _InputSrc(SRC_COMPACT, int(arg), 1, 0, a.ctypes.data), a
    raise ValueError(f"unknown source kind {kind!r}")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(gpu_library_missing(LIB_PATH))
    # PyTorch ships its own copy of the HIP runtime; if it is going to be used in this process (device
    # tensors, RCCL) it has to be the first one loaded, or torch later finds "No HIP GPUs".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, u64, u32, sz, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t, C.c_int
    sig = dict(_public_native.SIGNATURES)   # the host entries of "public-key inputs": the same code as libfbspublic.so's
    sig.update(_client_native.SIGNATURES)   # the client's entries: the same code as libfbsclient.so's, or this library's form of it
    sig.update({
        "fbs_ctx_reserve": (i32, [vp, sz, sz, sz]),
        "fbs_ctx_tune": (i32, [vp, C.c_char_p, C.c_int64]),
        "fbs_import_keys": (i32, [vp, vp, vp, vp, vp]),
        "fbs_encrypt_dev": (i32, [vp, vp, sz, u64, vp, vp]),
        "fbs_encrypt_fresh_dev": (i32, [vp, vp, sz, vp, C.POINTER(u64), vp]),
        "fbs_decrypt_dev": (i32, [vp, vp, sz, vp, vp]),
        "fbs_import_seeded_keys": (i32, [vp, vp, vp, vp]),
        "fbs_encrypt_seeded_dev": (i32, [vp, vp, sz, u64, vp, vp]),
        "fbs_encrypt_seeded_fresh_dev": (i32, [vp, vp, sz, vp, C.POINTER(u64), vp]),
        "fbs_expand_seeded_dev": (i32, [vp, vp, sz, u64, vp, vp]),
        "fbs_eval_seeded": (i32, [vp, vp, vp, sz, u64, vp]),
        "fbs_compact_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_eval_seeded_compact": (i32, [vp, vp, vp, sz, u64, u32, vp]),
        "fbs_decrypt_compact_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_compact_fields_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_refresh_compact_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_eval_sources": (i32, [vp, vp, vp, sz, u32, vp]),
        "fbs_import_packing_key": (i32, [vp, u32, u32, vp]),
        "fbs_pack_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_state_fetch_packed": (i32, [vp, vp, sz, sz, u32, vp]),
        "fbs_state_create": (i32, [vp, sz, sz, C.POINTER(vp)]),
        "fbs_state_destroy": (None, [vp]),
        "fbs_state_info": (i32, [vp, C.POINTER(sz), C.POINTER(sz)]),
        "fbs_eval_resident": (i32, [vp, vp, vp, vp, sz, u32, vp, vp]),
        "fbs_eval_resident_mapped": (i32, [vp, vp, vp, vp, vp, sz, u32, vp, vp]),
        "fbs_state_sum_groups": (i32, [vp, vp, sz, sz, sz, vp, sz]),
        "fbs_state_fetch": (i32, [vp, vp, sz, sz, u32, vp]),
        "fbs_state_put": (i32, [vp, vp, sz, sz, vp]),
        "fbs_pub_expand_dev": (i32, [vp, vp, sz, vp, vp]),
        "fbs_state_put_public": (i32, [vp, vp, sz, sz, vp]),
        "fbs_fold_keygen": (i32, [vp, u32, u32]),
        "fbs_fold_key_sizes": (i32, [vp, u32, C.POINTER(sz * 2)]),
        "fbs_export_fold_key": (i32, [vp, vp, vp]),
        "fbs_import_fold_key": (i32, [vp, u32, u32, vp]),
        "fbs_fold_dev": (i32, [vp, vp, sz, vp, vp]),
        "fbs_state_fold": (i32, [vp, vp, sz, sz, vp]),
        "fbs_state_fold_dev": (i32, [vp, vp, sz, sz, vp]),
        "fbs_state_unfold_dev": (i32, [vp, vp, sz, sz, vp]),
        "fbs_debug_fold_front_dev": (i32, [vp, vp, sz, u32, u32, vp, vp]),
        "fbs_lookup_map": (i32, [u32, u32, u32, u32, u32, vp]),
        "fbs_fold_mapped_dev": (i32, [vp, vp, sz, vp, sz, vp, vp]),
        "fbs_lookup_dev": (i32, [vp, vp, u32, vp, vp, sz, vp, vp]),
        "fbs_lookup_compact_dev": (i32, [vp, vp, u32, vp, vp, sz, u32, vp, vp]),
        "fbs_state_lookup": (i32, [vp, vp, vp, u32, u32, u32, vp, sz, vp, sz]),
        "fbs_table_map": (i32, [u32, u32, u32, u32, u32, u32, vp]),
        "fbs_rotate_dev": (i32, [vp, vp, u32, vp, vp, sz, u32, vp, vp]),
        "fbs_rotate_compact_dev": (i32, [vp, vp, u32, vp, vp, sz, u32, u32, vp, vp]),
        "fbs_glwe_add_dev": (i32, [vp, vp, sz, vp, vp, sz, vp]),
        "fbs_table_create": (i32, [vp, vp, vp, u32, u32, u32, C.POINTER(vp)]),
        "fbs_table_free": (None, [vp]),
        "fbs_table_stat": (i32, [vp, C.c_char_p, C.POINTER(C.c_int64)]),
        "fbs_table_words": (i32, [vp, vp, vp]),
        "fbs_table_read": (i32, [vp, vp, vp, sz, vp, sz]),
        "fbs_table_write": (i32, [vp, vp, vp, sz, vp, vp, u32, vp]),
        "fbs_tvset_create": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
        "fbs_tvset_destroy": (None, [vp]),
        "fbs_bootstrap_batch": (i32, [vp, vp, vp, vp, sz, vp]),
        "fbs_bootstrap_batch_dev": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "fbs_lincomb_dev": (i32, [vp, vp, sz, u32, vp, vp, vp, vp, vp, vp]),
        "fbs_bootstrap_wires_dev": (i32, [vp, vp, vp, sz, u32, vp, vp, vp, sz, sz, vp]),
        "fbs_program_load": (i32, [vp, C.POINTER(_ProgramDesc), vp, C.POINTER(vp)]),
        "fbs_program_load_ex": (i32, [vp, C.POINTER(_ProgramDesc), vp, u32, C.POINTER(vp)]),
        "fbs_table_fusion_norms": (i32, [vp, u32, C.POINTER(u64), C.POINTER(u64)]),
        "fbs_program_destroy": (None, [vp]),
        "fbs_program_info": (i32, [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "fbs_eval": (i32, [vp, vp, vp, sz, vp]),
        "fbs_eval_dev": (i32, [vp, vp, vp, sz, vp, vp]),
        "fbs_eval_messages": (i32, [vp, vp, vp, sz, i32, C.POINTER(u64), vp]),
        "fbs_program_layout": (i32, [vp, C.POINTER(_Layout)]),
        "fbs_program_level": (i32, [vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        "fbs_program_io_slots": (i32, [vp, vp, vp]),
        "fbs_level_lincomb_dev": (i32, [vp, vp, u32, vp, sz, sz, sz, vp]),
        "fbs_level_bootstrap_dev": (i32, [vp, vp, u32, vp, sz, sz, sz, sz, sz, vp, vp]),
        "fbs_level_scatter_dev": (i32, [vp, vp, u32, vp, sz, sz, sz, vp, sz, sz, vp]),
        "fbs_audit_rows": (i32, [vp, u32, u32, C.POINTER(u32), vp]),
        "fbs_audit_level_dev": (i32, [vp, vp, u32, u32, vp, sz, sz, sz, vp, vp, vp, vp]),
        "fbs_profile_enable": (i32, [vp, i32]),
        "fbs_profile_read": (i32, [vp, C.POINTER(C.c_double * 3), C.POINTER(u64 * 3), i32]),
        "fbs_profile_kernel": (C.c_char_p, [vp, i32]),
        "fbs_kernel_catalog": (C.c_char_p, []),
        "fbs_profile_kernels": (i32, [vp, vp, sz, C.POINTER(sz)]),
        "fbs_sync": (i32, [vp, vp]),
        "fbs_debug_polymul": (i32, [vp, vp, vp, vp]),
        "fbs_debug_field": (i32, [vp, i32, vp, vp, sz, vp]),
        "fbs_debug_gauss": (i32, [vp, vp, sz, u64, vp]),
        "fbs_debug_gauss_dev": (i32, [vp, vp, sz, u64, vp, vp]),
        "fbs_debug_pack_fields_dev": (i32, [vp, vp, sz, u32, vp, vp]),
        "fbs_debug_transform_list": (C.c_char_p, []),
        "fbs_debug_transform": (i32, [vp, C.c_char_p, vp, vp, sz]),
        "fbs_searcher_create": (i32, [i32, C.POINTER(vp)]),
        "fbs_searcher_destroy": (None, [vp]),
        "fbs_searcher_last_error": (C.c_char_p, [vp]),
        "fbs_searcher_last_kernel_ms": (C.c_double, [vp]),
        "fbs_search_lincomb_coefs": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, C.POINTER(i32)]),
    })
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not match the header
        fn.restype = res
        fn.argtypes = args
    return lib


EXPORTED_SYMBOLS = (
    "fbs_poly_size_check", "fbs_ctx_create", "fbs_ctx_create_seeded", "fbs_ctx_reserve", "fbs_ctx_tune", "fbs_ctx_stat",
    "fbs_import_keys", "fbs_encrypt_fresh", "fbs_ctx_destroy", "fbs_last_error", "fbs_device_info", "fbs_keygen",
    "fbs_key_sizes", "fbs_export_keys", "fbs_encrypt", "fbs_decrypt", "fbs_encrypt_dev", "fbs_encrypt_fresh_dev",
    "fbs_decrypt_dev", "fbs_tvset_create",
    "fbs_tvset_destroy", "fbs_bootstrap_batch", "fbs_bootstrap_batch_dev", "fbs_lincomb_dev",
    "fbs_bootstrap_wires_dev", "fbs_program_load", "fbs_program_load_ex", "fbs_table_fusion_norms", "fbs_program_destroy",
    "fbs_program_info",
    "fbs_searcher_create", "fbs_searcher_destroy", "fbs_searcher_last_error", "fbs_searcher_last_kernel_ms",
    "fbs_search_lincomb_coefs", "fbs_eval", "fbs_eval_dev", "fbs_eval_messages", "fbs_program_layout", "fbs_program_level", "fbs_program_io_slots",
    "fbs_level_lincomb_dev", "fbs_level_bootstrap_dev", "fbs_level_scatter_dev", "fbs_profile_enable", "fbs_profile_kernel", "fbs_kernel_catalog", "fbs_profile_kernels", "fbs_profile_read", "fbs_sync", "fbs_debug_polymul", "fbs_debug_raise",
    "fbs_debug_field", "fbs_debug_transform_list", "fbs_debug_transform", "fbs_debug_gauss", "fbs_debug_gauss_dev", "fbs_debug_pack_fields_dev",
    "fbs_keygen_seeded", "fbs_seeded_key_sizes", "fbs_export_seeded_keys", "fbs_import_seeded_keys", "fbs_encrypt_seeded",
    "fbs_encrypt_seeded_fresh", "fbs_encrypt_seeded_dev", "fbs_encrypt_seeded_fresh_dev", "fbs_expand_seeded",
    "fbs_expand_seeded_dev", "fbs_eval_seeded",
    "fbs_compact_words", "fbs_compact_dev", "fbs_eval_seeded_compact", "fbs_decrypt_compact", "fbs_decrypt_compact_dev",
    "fbs_compact_fields_dev", "fbs_refresh_compact_dev", "fbs_eval_sources",
    "fbs_state_create", "fbs_state_destroy", "fbs_state_info", "fbs_eval_resident", "fbs_state_fetch", "fbs_state_put",
    "fbs_packing_keygen", "fbs_packing_key_sizes", "fbs_export_packing_key", "fbs_import_packing_key", "fbs_packed_words",
    "fbs_pack_dev", "fbs_state_fetch_packed", "fbs_decrypt_packed",
    "fbs_pub_expand_dev", "fbs_state_put_public",
    "fbs_fold_keygen", "fbs_fold_key_sizes", "fbs_export_fold_key", "fbs_import_fold_key", "fbs_fold_dev", "fbs_state_fold",
    "fbs_state_fold_dev", "fbs_state_unfold_dev", "fbs_debug_fold_front_dev",
    "fbs_lookup_map", "fbs_fold_mapped_dev", "fbs_lookup_dev", "fbs_lookup_compact_dev", "fbs_state_lookup",
    "fbs_table_map", "fbs_rotate_dev", "fbs_rotate_compact_dev", "fbs_glwe_add_dev",
    "fbs_table_create", "fbs_table_free", "fbs_table_stat", "fbs_table_words", "fbs_table_read", "fbs_table_write",
    "fbs_eval_resident_mapped", "fbs_state_sum_groups",
    "fbs_audit_rows", "fbs_audit_level_dev",
) + _public_native.EXPORTED_SYMBOLS

lib = _load()

MAP_NONE, MAP_NEG = 0xFFFFFFFF, 0x80000000   # FBS_MAP_NONE, FBS_MAP_NEG of a mapped fold's map


def lookup_map(p, N, length, base=0, stride=1):
    """fbs_lookup_map: the box map of a table of `length` <= p entries, uint32 [N] (host side, pure)"""
    out = np.zeros(max(1, int(N)), dtype=np.uint32)
    rc = lib.fbs_lookup_map(int(p), int(N), int(length), int(base), int(stride), out.ctypes.data)
    if rc != 0:
        raise FbsError(rc, lib.fbs_last_error(None).decode())
    return out

ROTATE_NEGATE = 1   # FBS_ROTATE_NEGATE of fbs_rotate_dev's flags


def table_map(p, N, spread, length, base=0, stride=1):
    """fbs_table_map: the map of a writable table of `length` <= p // spread entries, `spread` boxes an entry, uint32 [N] (host side,
    pure); spread = 1 is `lookup_map`, length = 1 the unit box of a write"""
    out = np.zeros(max(1, int(N)), dtype=np.uint32)
    rc = lib.fbs_table_map(int(p), int(N), int(spread), int(length), int(base), int(stride), out.ctypes.data)
    if rc != 0:
        raise FbsError(rc, lib.fbs_last_error(None).decode())
    return out


def kernel_catalog():
    """Names of every kernel instantiation the launchers can pick (fbs_kernel_catalog)."""
    return [n for n in lib.fbs_kernel_catalog().decode().split("\n") if n]


def debug_transform_list():
    """One line per transform variant the blind-rotation kernels instantiate (fbs_debug_transform_list); needs no GPU."""
    return [n for n in lib.fbs_debug_transform_list().decode().split("\n") if n]


class TvSet:
    def __init__(self, ctx, tables):
        self.ctx = ctx
        self.tables = [list(map(int, t)) for t in tables]
        vals = _c([v for t in self.tables for v in t] or [0], np.int32)
        off = np.zeros(len(self.tables) + 1, np.uint32)
        off[1:] = np.cumsum([len(t) for t in self.tables])
        h = C.c_void_p()
        ctx._check(lib.fbs_tvset_create(ctx._h, _ptr(vals), _ptr(off), len(self.tables), C.byref(h)))
        self._h = h

    def fusion_norms(self, table):
        """(|D_F|^2, |G_F|^2) of table `table` (include/fbs_exec.h, fbs_table_fusion_norms): what sharing a blind rotation
        does to its output noise."""
        d, g = C.c_uint64(), C.c_uint64()
        self.ctx._check(lib.fbs_table_fusion_norms(self._h, table, C.byref(d), C.byref(g)))
        return d.value, g.value

    def __del__(self):
        if getattr(self, "_h", None) and self.ctx._h and lib is not None:
            lib.fbs_tvset_destroy(self._h)
            self._h = None


class Program:
    FUSE_TABLES = 1    # FBS_LOAD_FUSE_TABLES

    def __init__(self, ctx, tvset, n_inputs, kind, arg0, arg1, const_coef, term_coef, term_src, out_wire, fuse_tables=False):
        """fuse_tables: the tables of a source that several Bootstraps read share ONE blind rotation
        (include/fbs_exec.h, FBS_LOAD_FUSE_TABLES)."""
        self.ctx, self.tvset = ctx, tvset
        self.fused = bool(fuse_tables)
        self._keep = [_c(kind, np.uint8), _c(arg0, np.uint32), _c(arg1, np.uint32), _c(const_coef, np.int64),
                      _c(term_coef, np.int64), _c(term_src, np.uint32), _c(out_wire, np.int64)]
        k = self._keep
        desc = _ProgramDesc(n_inputs, len(k[0]), len(k[4]), len(k[6]), *[_ptr(a) for a in k])
        h = C.c_void_p()
        ctx._check(lib.fbs_program_load_ex(ctx._h, C.byref(desc), tvset._h, self.FUSE_TABLES if fuse_tables else 0, C.byref(h)))
        self._h = h
        self.n_inputs, self.n_outputs = n_inputs, len(k[6])
        lay = _Layout()
        ctx._check(lib.fbs_program_layout(h, C.byref(lay)))
        self.depth, self.max_width, self.n_bootstrap = lay.n_levels, lay.max_width, lay.n_bootstrap
        self.n_slots, self.n_keyswitch, self.max_sources = lay.n_slots, lay.n_keyswitch, lay.max_sources
        self.n_rotations = lay.n_rotations
        self.row_words = lay.row_words          # words per row of the d_rows arrays of the level calls (2N for a fused program)
        self.in_slot = np.empty(self.n_inputs, np.uint32)
        self.out_slot = np.empty(self.n_outputs, np.int64)
        ctx._check(lib.fbs_program_io_slots(h, _ptr(self.in_slot), _ptr(self.out_slot)))
        self.level_width, self.level_sources = [], []
        for L in range(self.depth):
            a, b = C.c_uint32(), C.c_uint32()
            ctx._check(lib.fbs_program_level(h, L, C.byref(a), C.byref(b)))
            self.level_width.append(a.value)
            self.level_sources.append(b.value)

    def eval(self, in_cts, T):
        ctw = self.ctx.params.ct_words
        in_cts = _c(in_cts, np.uint64).reshape(self.n_inputs, T, ctw)
        out = np.empty((self.n_outputs, T, ctw), np.uint64)
        self.ctx._check(lib.fbs_eval(self.ctx._h, self._h, _ptr(in_cts), T, _ptr(out)))
        return out

    def eval_messages(self, msgs, nonce0=None):
        """Messages in, messages out (fbs_eval_messages): msgs [n_inputs][T] -> np.ndarray [n_outputs][T], with the inputs
        encrypted and the outputs decrypted on the GPU.  The same as ctx.decrypt(self.eval(ctx.encrypt(msgs, nonce0), T)):
        nonce0=None takes n_inputs * T streams nobody has used, an int pins input i, sample s to stream nonce0 + i*T + s."""
        msgs = _c(msgs, np.int64)
        T = msgs.shape[-1] if msgs.ndim else 1
        msgs = msgs.reshape(self.n_inputs, T)
        out = np.empty((self.n_outputs, T), np.int64)
        first = C.c_uint64(0 if nonce0 is None else int(nonce0))
        self.ctx._check(lib.fbs_eval_messages(self.ctx._h, self._h, _ptr(msgs), T, int(nonce0 is None), C.byref(first), _ptr(out)))
        return out

    def eval_seeded(self, bodies, T, nonce0):
        """Seeded inputs, full outputs (fbs_eval_seeded): bodies [n_inputs][T] from `Context.encrypt_seeded` of a [n_inputs][T]
        array whose first stream is nonce0 -> output ciphertexts [n_outputs][T][D+1], as `eval` returns them.  Needs no
        secret: an evaluation-only context (`Context.evaluation_only`) runs it."""
        bodies = _c(bodies, np.uint64).reshape(self.n_inputs, T)
        out = np.empty((self.n_outputs, T, self.ctx.params.ct_words), np.uint64)
        self.ctx._check(lib.fbs_eval_seeded(self.ctx._h, self._h, _ptr(bodies), T, int(nonce0), _ptr(out)))
        return out

    def eval_seeded_compact(self, bodies, T, nonce0, bits=None):
        """Seeded inputs, compact outputs (fbs_eval_seeded_compact): as `eval_seeded`, but each output comes back key-switched to
        the small key, rounded to `bits` bits a field (None: log2(2N)) and packed -> words [n_outputs][T][W]
        (`Context.compact_words`).  Needs no secret; `Context.decrypt_compact` reads the words."""
        bits = self.ctx.default_compact_bits if bits is None else int(bits)
        bodies = _c(bodies, np.uint64).reshape(self.n_inputs, T)
        out = np.empty((self.n_outputs, T, self.ctx.compact_words(bits)), np.uint64)
        self.ctx._check(lib.fbs_eval_seeded_compact(self.ctx._h, self._h, _ptr(bodies), T, int(nonce0), bits, _ptr(out)))
        return out

    def eval_sources(self, sources, T, bits=0):
        """Inputs from any mix of sources (fbs_eval_sources), one per input in input order:
            ("seeded", bodies [T], nonce0)     -- sample s on stream nonce0 + s (`Context.encrypt_seeded`)
            ("full", cts [T][D+1], refresh)    -- outputs of an earlier evaluation; refresh=True: through the identity table first
            ("compact", words [T][W], bits)    -- compact outputs of an earlier evaluation, always refreshed
            ("plain", msgs int64 [T])          -- the server's own cleartext messages in [0, 2p), written on the GPU as trivial
            ("plain", int)                        ciphertexts (zero mask, body m * Delta); an int serves every sample
        bits = 0: full outputs [n_outputs][T][D+1] (as `eval_seeded`); else compact [n_outputs][T][W] at that width (as
        `eval_seeded_compact`).  Needs no secret."""
        if len(sources) != self.n_inputs:
            raise ValueError(f"{len(sources)} sources for {self.n_inputs} inputs")
        arr, keep = (_InputSrc * max(1, self.n_inputs))(), []
        ctw = self.ctx.params.ct_words
        for i, source in enumerate(sources):
            arr[i], a = _input_src(source, T, ctw)
            keep.append(a)
        bits = int(bits)
        shape = (self.n_outputs, T, self.ctx.compact_words(bits) if bits else ctw)
        out = np.empty(shape, np.uint64)
        self.ctx._check(lib.fbs_eval_sources(self.ctx._h, self._h, C.byref(arr), T, bits, _ptr(out)))
        return out

    def eval_resident(self, sources, T, out_bits=0, out_state=None):
        """`eval_sources` with resident state (fbs_eval_resident).  A source may also be
            ("state", state, row, refresh)     -- row `row` of a `DeviceState`; refresh=True: through the identity table first
            ("state", state, row, refresh, index, fill)
                                               -- the same through a sample map (fbs_eval_resident_mapped): sample s is sample
                                                  index[s] of the row (uint32 [T]; the state may hold any number of samples), or,
                                                  where index[s] == SAMPLE_NONE, the trivial ciphertext of the message `fill`
        out_state=None: returns the outputs as `eval_sources` does at `out_bits`.  out_state: a `DeviceState` of n_outputs rows and
        T samples a row that takes the full outputs, row o = output o; returns it.  With out_state and only state and seeded
        sources (and plain ones) the call does not wait for the evaluation: whatever reads the state next is queued behind it."""
        if len(sources) != self.n_inputs:
            raise ValueError(f"{len(sources)} sources for {self.n_inputs} inputs")
        arr, res, keep = (_InputSrc * max(1, self.n_inputs))(), (_ResidentSrc * max(1, self.n_inputs))(), []
        maps, mapped = (_SampleMap * max(1, self.n_inputs))(), False
        ctw = self.ctx.params.ct_words
        for i, source in enumerate(sources):
            kind = source[0]
            if kind == "state":
                _, state, row, refresh = source[:4]
                if not isinstance(state, DeviceState) or state.closed:
                    raise ValueError(f"input {i}: a closed state")
                res[i] = _ResidentSrc(state._h.value, int(row), int(bool(refresh)))
                keep.append(state)
                if len(source) > 4 and source[4] is not None:
                    _, _, _, _, index, fill = source
                    index = np.asarray(index)
                    if index.shape != (T,) or (index.size and (index.min() < 0 or index.max() > SAMPLE_NONE)):
                        raise ValueError(f"input {i}: a sample map is {T} indices that fit 32 bits")
                    index = _c(index, np.uint32)
                    maps[i], mapped = _SampleMap(index.ctypes.data, operator.index(fill)), True
                    keep.append(index)
                continue
            arr[i], a = _input_src(source, T, ctw)
            keep.append(a)
        bits = int(out_bits)

        def run(ctx, prog, arr, res, *rest):   # (the feed of before goes through the entry of before)
            if mapped:
                return lib.fbs_eval_resident_mapped(ctx, prog, arr, res, C.byref(maps), *rest)
            return lib.fbs_eval_resident(ctx, prog, arr, res, *rest)

        if out_state is not None:
            if not isinstance(out_state, DeviceState) or out_state.closed:
                raise ValueError("out_state is a closed state")
            self.ctx._check(run(self.ctx._h, self._h, C.byref(arr), C.byref(res), T, bits, None, out_state._h))
            return out_state
        out = np.empty((self.n_outputs, T, self.ctx.compact_words(bits) if bits else ctw), np.uint64)
        self.ctx._check(run(self.ctx._h, self._h, C.byref(arr), C.byref(res), T, bits, _ptr(out), None))
        return out

    # device-pointer entry points (ints from torch.Tensor.data_ptr()); asynchronous on `stream`, no host copies
    def eval_dev(self, d_in, T, d_out, stream=0):
        self.ctx._check(lib.fbs_eval_dev(self.ctx._h, self._h, d_in or None, T, d_out or None, stream or None))

    def level_lincomb_dev(self, level, d_wires, T, s_begin, s_count, stream=0):
        self.ctx._check(lib.fbs_level_lincomb_dev(self.ctx._h, self._h, level, d_wires, T, s_begin, s_count, stream or None))

    def level_bootstrap_dev(self, level, d_wires, T, s_begin, s_count, f_begin, f_end, d_rows=0, stream=0):
        self.ctx._check(lib.fbs_level_bootstrap_dev(self.ctx._h, self._h, level, d_wires, T, s_begin, s_count, f_begin, f_end,
                                                    d_rows or None, stream or None))

    def level_scatter_dev(self, level, d_wires, T, s_begin, s_count, d_rows, f_begin, f_end, stream=0):
        self.ctx._check(lib.fbs_level_scatter_dev(self.ctx._h, self._h, level, d_wires, T, s_begin, s_count, d_rows, f_begin,
                                                  f_end, stream or None))

    def audit_rows(self, level, point):
        """The program wire ids (fbs_program_desc numbering: inputs, then instructions) of the rows that point `point`
        (AUDIT_*) of level `level` reports, in reporting order (fbs_audit_rows) -> np.ndarray uint32"""
        n = C.c_uint32()
        self.ctx._check(lib.fbs_audit_rows(self._h, int(level), int(point), C.byref(n), None))
        ids = np.empty(n.value, np.uint32)
        self.ctx._check(lib.fbs_audit_rows(self._h, int(level), int(point), C.byref(n), _ptr(ids)))
        return ids

    def audit_level_dev(self, level, point, d_wires, T, s_begin, s_count, d_expected, errors=False, stream=0):
        """fbs_audit_level_dev: the exact error statistics of one point of one level of a stepped program.  d_expected: device
        pointer to int64 [n_rows][s_count], the cleartext value of each row per sample (taken mod 2p).  Blocks.  Returns
        (stats, errors): stats a list of dicts of Python ints (count, over, max_abs, sum, sumsq -- the 128-bit sum of squares),
        one per row of `audit_rows(level, point)`; errors int64 [n_rows][s_count] when asked for, else None."""
        n = C.c_uint32()
        self.ctx._check(lib.fbs_audit_rows(self._h, int(level), int(point), C.byref(n), None))
        rows = (_AuditRow * max(1, n.value))()
        err = np.empty((n.value, int(s_count)), np.int64) if errors else None
        self.ctx._check(lib.fbs_audit_level_dev(self.ctx._h, self._h, int(level), int(point), d_wires or None, int(T), int(s_begin),
                                                int(s_count), d_expected or None, C.byref(rows), _ptr(err), stream or None))
        live = n.value if int(s_count) else 0
        stats = [dict(count=int(r.count), over=int(r.over), max_abs=int(r.max_abs), sum=int(r.sum),
                      sumsq=(int(r.sumsq_hi) << 64) | int(r.sumsq_lo)) for r in rows[:live]]
        return stats, err

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h and lib is not None:
            lib.fbs_program_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


class DeviceState:
    """Resident state (fbs_state, include/fbs_exec.h): [rows][T][D+1] big-key ciphertexts that stay in the context's device
    memory between evaluations.  `Program.eval_resident` writes its outputs into one and reads inputs from its rows; `fetch`
    brings rows to the host, full or compact, and `put` takes full ones back.  `close()` frees it (also as a context manager);
    closing the context closes its states."""

    def __init__(self, ctx, rows, T):
        self.ctx, self.rows, self.T = ctx, int(rows), int(T)
        self._h = None
        h = C.c_void_p()
        ctx._check(lib.fbs_state_create(ctx._h, self.rows, self.T, C.byref(h)))
        self._h = h
        ctx._states.add(self)

    @property
    def closed(self):
        return self._h is None or not self.ctx._h

    def _live(self):
        if self.closed:
            raise ValueError("the state is closed")
        return self._h

    def fetch(self, row0=0, rows=None, bits=0):
        """rows [row0, row0 + rows) -> np.ndarray: bits=0 the full ciphertexts [rows][T][D+1]; else compact words [rows][T][W] at
        that width, compacted on the GPU (fbs_state_fetch).  Waits for the evaluations queued before it."""
        rows = self.rows - int(row0) if rows is None else int(rows)
        bits = int(bits)
        out = np.empty((max(0, rows), self.T, self.ctx.compact_words(bits) if bits else self.ctx.params.ct_words), np.uint64)
        self.ctx._check(lib.fbs_state_fetch(self.ctx._h, self._live(), int(row0), rows, bits, _ptr(out)))
        return out

    def fetch_packed(self, bits, row0=0, rows=None):
        """rows [row0, row0 + rows), flattened [row][sample], packed on the GPU into GLWE samples at width `bits`
        (fbs_state_fetch_packed) -> the packed words, `Context.packed_words(rows * T, bits)` of them"""
        rows = self.rows - int(row0) if rows is None else int(rows)
        out = np.empty(self.ctx.packed_words(max(0, rows) * self.T, bits), np.uint64)
        self.ctx._check(lib.fbs_state_fetch_packed(self.ctx._h, self._live(), int(row0), rows, int(bits), _ptr(out)))
        return out

    def put(self, cts, row0=0):
        """full ciphertexts [rows][T][D+1] (canonical words) -> rows row0 onwards (fbs_state_put)"""
        cts = _c(cts, np.uint64).reshape(-1, self.T, self.ctx.params.ct_words)
        self.ctx._check(lib.fbs_state_put(self.ctx._h, self._live(), int(row0), cts.shape[0], _ptr(cts)))
        return self

    def lookup(self, rows, index, index_row, out=None, out_row0=0, axis=0):
        """This state as encrypted tables read by an encrypted index (fbs_state_lookup).  axis=0: `rows` is [planes][len] row
        numbers, plane m's entry e being row rows[m][e] at the query's own sample (or at sample 0 where this state has T = 1: a
        shared table); axis=1: `rows` is [planes], plane m's entries being the samples of row rows[m].  Sample s of row
        out_row0 + m of `out` <- the entry that row `index_row` of `index` names at sample s.  out=None: a new `DeviceState` of
        `planes` rows and the index's T.  Queued on the context; needs a fold key, no secret.  Returns `out`."""
        if axis == 0:
            rows = _c(rows, np.uint32)
            if rows.ndim != 2 or rows.size == 0:
                raise ValueError("rows is [planes][len]")
            planes, length = rows.shape
        else:
            rows = _c(rows, np.uint32).reshape(-1)
            planes, length = rows.size, self.T
        if not isinstance(index, DeviceState) or index.closed:
            raise ValueError("index is a closed state")
        made = out is None
        if made:
            out = DeviceState(self.ctx, max(1, planes), index.T)
        try:
            if not isinstance(out, DeviceState) or out.closed:
                raise ValueError("out is a closed state")
            self.ctx._check(lib.fbs_state_lookup(self.ctx._h, self._live(), _ptr(rows), int(planes), int(length), int(axis), index._h,
                                                 int(index_row), out._h, int(out_row0)))
        except Exception:
            if made:
                out.close()
            raise
        return out

    def sum_groups(self, group, row0=0, rows=None, out=None, out_row0=0):
        """Sample j of row out_row0 + r of `out` <- the sum of samples [j group, (j + 1) group) of row row0 + r, word by word modulo q
        (fbs_state_sum_groups): the ciphertext of the sum of their messages.  out=None: a new `DeviceState` of `rows` rows;
        either way ceil(T / group) samples a row.  Queued on the context, no secret needed.  Returns `out`."""
        rows = self.rows - int(row0) if rows is None else int(rows)
        group = operator.index(group)
        made = out is None
        if made:
            if not 1 <= group <= MAX_SUM_GROUP:
                raise ValueError(f"group {group} outside [1, {MAX_SUM_GROUP}]")
            out = DeviceState(self.ctx, rows, -(-self.T // group))
        try:
            if not isinstance(out, DeviceState) or out.closed:
                raise ValueError("out is a closed state")
            self.ctx._check(lib.fbs_state_sum_groups(self.ctx._h, self._live(), int(row0), rows, group, out._h, int(out_row0)))
        except Exception:
            if made:
                out.close()
            raise
        return out

    def put_public(self, glwe, row0=0, rows=None):
        """public-key samples [ceil(rows * T / N)][k+1][N] (host; `_public_native.Encryptor.encrypt` of the rows' messages flattened
        [row][sample]) -> rows [row0, row0 + rows), expanded on the GPU (fbs_state_put_public).  Needs no key."""
        rows = self.rows - int(row0) if rows is None else int(rows)
        prm = self.ctx.params
        glwe = _c(glwe, np.uint64).reshape(-1)
        want = -(-max(0, rows) * self.T // prm.N) * (prm.k + 1) * prm.N
        if glwe.size != want:
            raise ValueError(f"{glwe.size} sample words for {rows} rows of {self.T} samples (the parameter set needs {want})")
        self.ctx._check(lib.fbs_state_put_public(self.ctx._h, self._live(), int(row0), rows, _ptr(glwe)))
        return self

    def _fold_words(self, rows):
        prm = self.ctx.params
        return -(-max(0, rows) * self.T // prm.N) * (prm.k + 1) * prm.N

    def fold(self, row0=0, rows=None, device=False):
        """rows [row0, row0 + rows), flattened [row][sample], folded on the GPU into full-precision GLWE samples
        [ceil(rows * T / N)][k+1][N] (include/fbs_exec.h, "folded state"): a numpy array (fbs_state_fold), or with device=True an
        int64 torch tensor that stays on the card (fbs_state_fold_dev; the call waits for the fold).  Needs a fold key, no secret."""
        rows = self.rows - int(row0) if rows is None else int(rows)
        words = self._fold_words(rows)
        if not device:
            out = np.empty(words, np.uint64)
            self.ctx._check(lib.fbs_state_fold(self.ctx._h, self._live(), int(row0), rows, _ptr(out)))
            return out
        import torch
        out = torch.empty(max(2, words), dtype=torch.int64, device=f"cuda:{self.ctx.device}")
        torch.cuda.synchronize(out.device)
        self.ctx._check(lib.fbs_state_fold_dev(self.ctx._h, self._live(), int(row0), rows, out.data_ptr()))
        self.ctx.sync()
        return out[:words]

    def unfold(self, glwe, row0=0, rows=None):
        """The way back: folded samples -> rows [row0, row0 + rows), by sample extraction on the GPU, no key.  A numpy array goes
        through `put_public` (checked word by word on the host); a torch tensor on the context's device is expanded where it lies
        (fbs_state_unfold_dev; the call waits for it)."""
        if isinstance(glwe, np.ndarray):
            return self.put_public(glwe, row0, rows)
        rows = self.rows - int(row0) if rows is None else int(rows)
        import torch
        if glwe.dtype != torch.int64 or not glwe.is_cuda or glwe.device.index != self.ctx.device or not glwe.is_contiguous():
            raise ValueError("folded samples on the device are a contiguous int64 tensor on the context's device")
        if glwe.numel() != self._fold_words(rows):
            raise ValueError(f"{glwe.numel()} sample words for {rows} rows of {self.T} samples (the parameter set needs {self._fold_words(rows)})")
        torch.cuda.synchronize(glwe.device)
        self.ctx._check(lib.fbs_state_unfold_dev(self.ctx._h, self._live(), int(row0), rows, glwe.data_ptr() if rows else None))
        self.ctx.sync()
        return self

    def close(self):
        if not self.closed and lib is not None:
            lib.fbs_state_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class DeviceTable:
    """Resident tables (fbs_table, include/fbs_exec.h, "encrypted tables"): folded samples that stay in the context's device memory,
    made once of rows of a `DeviceState` (`rows` [planes][len]: plane m's entry e is row rows[m][e], at every sample of the state,
    or one shared table per plane where the state has T = 1), `spread` boxes an entry; read and written by an encrypted index.
    `close()` frees them (also as a context manager); closing the context closes its tables."""
    ADD, SET = 0, 1

    def __init__(self, state, rows, spread=2):
        self._h, self.ctx = None, getattr(state, "ctx", None)   # (before anything can fail: __del__ closes)
        rows = _c(rows, np.uint32)
        if rows.ndim != 2 or rows.size == 0:
            raise ValueError("rows is [planes][len]")
        if not isinstance(state, DeviceState) or state.closed:
            raise ValueError("state is a closed state")
        self.planes, self.len, self.spread, self.T = rows.shape[0], rows.shape[1], int(spread), state.T
        h = C.c_void_p()
        self.ctx._check(lib.fbs_table_create(self.ctx._h, state._h, _ptr(rows), self.planes, self.len, self.spread, C.byref(h)))
        self._h = h
        self.ctx._states.add(self)

    @property
    def closed(self):
        return self._h is None or self.ctx is None or not self.ctx._h

    def _live(self):
        if self.closed:
            raise ValueError("the table is closed")
        return self._h

    def stat(self, name):
        """fbs_table_stat: one of tables, planes, samples, len, spread, writes, words"""
        v = C.c_int64()
        self.ctx._check(lib.fbs_table_stat(self._live(), name.encode(), C.byref(v)))
        return v.value

    def words(self):
        """every table, uint64 [tables][k+1][N] (fbs_table_words; waits for the writes queued before it)"""
        prm = self.ctx.params
        out = np.empty((self.stat("tables"), prm.k + 1, prm.N), np.uint64)
        self.ctx._check(lib.fbs_table_words(self.ctx._h, self._live(), _ptr(out)))
        return out

    def read(self, index, index_row, out=None, out_row0=0):
        """Sample s of row out_row0 + m of `out` <- the entry of plane m's table that row `index_row` of `index` names at sample s
        (fbs_table_read).  out=None: a new `DeviceState` of `planes` rows and the index's T.  Returns `out`."""
        if not isinstance(index, DeviceState) or index.closed:
            raise ValueError("index is a closed state")
        made = out is None
        if made:
            out = DeviceState(self.ctx, self.planes, index.T)
        try:
            if not isinstance(out, DeviceState) or out.closed:
                raise ValueError("out is a closed state")
            self.ctx._check(lib.fbs_table_read(self.ctx._h, self._live(), index._h, int(index_row), out._h, int(out_row0)))
        except Exception:
            if made:
                out.close()
            raise
        return out

    def write(self, index, index_row, values, value_rows, mode=ADD, identity=None):
        """entry[index] += value (mode ADD) or = value (SET) in every table: the value of plane m's table at sample s is row
        value_rows[m] of `values` at sample s (fbs_table_write).  identity: a `TvSet` whose table 0 is the identity, for a SET's
        refresh (None: the context's own)."""
        if not isinstance(index, DeviceState) or index.closed or not isinstance(values, DeviceState) or values.closed:
            raise ValueError("index and values are live states")
        value_rows = _c(value_rows, np.uint32).reshape(-1)
        if value_rows.size != self.planes:
            raise ValueError("one value row a plane")
        self.ctx._check(lib.fbs_table_write(self.ctx._h, self._live(), index._h, int(index_row), values._h, _ptr(value_rows), int(mode),
                                            identity._h if identity is not None else None))
        return self

    def close(self):
        if not self.closed and lib is not None:
            lib.fbs_table_free(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def debug_gauss(words, sigma):
    """The host's rounded Gaussian (sampler 1) of windows of six uint64 words [count][6] at standard deviation sigma -> int64 [count]
    (fbs_debug_gauss: no context, no GPU)."""
    words = _c(words, np.uint64).reshape(-1, 6)
    out = np.empty(words.shape[0], np.int64)
    rc = lib.fbs_debug_gauss(None, _ptr(words), words.shape[0], int(sigma), _ptr(out))
    if rc != 0:
        raise FbsError(rc, lib.fbs_last_error(None).decode())
    return out


class Context(ClientContext):
    """One GPU, one parameter set, one key set.  What the holder of the secret does on host arrays is `ClientContext`'s, the same
    wrappers `HostContext` has; here is what needs the GPU."""
    _lib = property(lambda self: lib)

    def __init__(self, params: Params, seed: int | bytes | None = None, device: int = 0, keygen: bool = True,
                 device_keys: bool = False):
        """seed: what all key material and encryption randomness derive from.
        * an int: the REPRODUCIBLE form (fbs_ctx_create, 64 bits) -- tests and benchmarks pass a constant so that the CPU
          oracle can be keyed identically.  Not a way to make production keys.
        * None or 32 bytes: fbs_ctx_create_seeded -- 256 bits (None: from os.urandom) with the parameter set mixed into the
          derivation.
        Either way the noise sampler is the one `params.sampler` names: 0, the default, a test-grade stand-in for a discrete
        Gaussian (`RANDOMNESS_GRADE`); 1 a rounded Gaussian (`GAUSSIAN_SAMPLER_GRADE`: not certified, not audited).  A deployment
        that needs more brings its own keys with `import_keys`.  keygen=False leaves the context without keys (for
        `import_keys`).
        device_keys=True: the evaluation keys are made -- and a server key is expanded -- on the GPU (knob "keys_on_device",
        include/fbs_exec.h) instead of on the host and uploaded; the same words either way (`stat("keys_made_on_device")`)."""
        self.device = device
        self._states = weakref.WeakSet()   # its DeviceStates and DeviceTables: closed with it
        self._create(params, seed, device)
        if device_keys:
            self.tune(keys_on_device=1)
        if keygen:
            self.keygen()

    def close(self):
        if getattr(self, "_h", None) and lib is not None:      # `lib` is None while the interpreter shuts down
            for st in list(getattr(self, "_states", ())):      # fbs_ctx_destroy frees the states and tables still alive
                st._h = None
            lib.fbs_ctx_destroy(self._h)
            self._h = None

    def import_keys(self, sk_lwe, sk_glwe, bsk, ksk):
        """Keys made elsewhere (layout of `export_keys`) instead of `keygen`: a caller's own CSPRNG and sampler, or a checker's."""
        arrs = [_c(a, np.uint64).ravel() for a in (sk_lwe, sk_glwe, bsk, ksk)]
        sizes = (C.c_size_t * 4)()
        self._check(lib.fbs_key_sizes(self._h, C.byref(sizes)))
        for a, want, name in zip(arrs, sizes, ("sk_lwe", "sk_glwe", "bsk", "ksk")):
            if a.size != want:
                raise ValueError(f"{name} has {a.size} words, the parameter set needs {want}")
        self._check(lib.fbs_import_keys(self._h, *[_ptr(a) for a in arrs]))

    # ---- seeded path: masks under a public key, only bodies travel (include/fbs_exec.h) ----
    def import_seeded_keys(self, mask_key, bsk_bodies, ksk_bodies):
        """fbs_import_seeded_keys: expands the server key and leaves the context evaluation-only."""
        mk = np.frombuffer(bytes(mask_key), np.uint8).copy()
        if mk.size != 32:
            raise ValueError("a mask key has 32 bytes")
        bsk, ksk = _c(bsk_bodies, np.uint64).ravel(), _c(ksk_bodies, np.uint64).ravel()
        for a, want, name in zip((bsk, ksk), self.seeded_key_sizes(), ("bsk_bodies", "ksk_bodies")):
            if a.size != want:
                raise ValueError(f"{name} has {a.size} words, the parameter set needs {want}")
        self._check(lib.fbs_import_seeded_keys(self._h, _ptr(mk), _ptr(bsk), _ptr(ksk)))

    @classmethod
    def evaluation_only(cls, params: Params, mask_key, bsk_bodies, ksk_bodies, device: int = 0, device_keys: bool = False):
        """A context that holds the evaluation keys of a server key and no secret: it evaluates (`Program.eval_seeded`,
        `Program.eval`, the batch and level entries) and refuses to encrypt or decrypt.  device_keys=True: only the bodies are
        uploaded and the masks are regenerated on the GPU."""
        ctx = cls(params, seed=None, device=device, keygen=False, device_keys=device_keys)
        ctx.import_seeded_keys(mask_key, bsk_bodies, ksk_bodies)
        return ctx

    def encrypt_seeded(self, msgs, nonce0=None, device=True):
        """Seeded encryption: (bodies with the shape of msgs, first stream).  Ciphertext i takes stream nonce0 + i; None = streams
        nobody has used (the counter of `encrypt`).  device=True (default): on the GPU (fbs_encrypt_seeded_dev), False: on the
        host -- the same words."""
        if not device:
            return super().encrypt_seeded(msgs, nonce0)
        msgs = _c(msgs, np.int64)
        import torch
        d_m = torch.from_numpy(msgs.reshape(-1)).to("cuda:%d" % self.device)
        d_b = torch.empty(max(1, msgs.size), dtype=torch.int64, device=d_m.device)
        torch.cuda.synchronize(d_m.device)
        first = self.encrypt_seeded_dev(d_m.data_ptr(), msgs.size, d_b.data_ptr(), nonce0=nonce0)
        self.sync()
        return d_b[:msgs.size].cpu().numpy().view(np.uint64).reshape(msgs.shape), first

    def encrypt_seeded_dev(self, d_msgs, count, d_bodies, nonce0=None, stream=0):
        """fbs_encrypt_seeded_dev / fbs_encrypt_seeded_fresh_dev; returns the first stream taken"""
        if nonce0 is None:
            first = C.c_uint64()
            self._check(lib.fbs_encrypt_seeded_fresh_dev(self._h, d_msgs or None, count, d_bodies or None, C.byref(first),
                                                         stream or None))
            return first.value
        self._check(lib.fbs_encrypt_seeded_dev(self._h, d_msgs or None, count, int(nonce0), d_bodies or None, stream or None))
        return int(nonce0)

    def expand_seeded_dev(self, d_bodies, count, nonce0, d_cts, stream=0):
        self._check(lib.fbs_expand_seeded_dev(self._h, d_bodies or None, count, int(nonce0), d_cts or None, stream or None))

    def pub_expand_dev(self, d_glwe, count, d_cts, stream=0):
        """fbs_pub_expand_dev: public-key samples [ceil(count / N)][k+1][N] at d_glwe -> [count][D+1] ciphertexts at d_cts"""
        self._check(lib.fbs_pub_expand_dev(self._h, d_glwe or None, count, d_cts or None, stream or None))

    def pub_expand(self, glwe, count):
        """`pub_expand_dev` on host arrays: samples -> np.ndarray [count][D+1] (the host form is `_public_native.expand`)"""
        import torch
        glwe = _c(glwe, np.uint64).reshape(-1)
        dev = torch.device("cuda", self.device)
        d_g = torch.from_numpy(glwe.view(np.int64)).to(dev)
        d_c = torch.empty((max(1, int(count)), self.params.ct_words), dtype=torch.int64, device=dev)
        self.pub_expand_dev(d_g.data_ptr() if glwe.size else None, int(count), d_c.data_ptr(), None)
        self.sync()
        return d_c[:int(count)].cpu().numpy().view(np.uint64)

    def reserve(self, max_keyswitches=0, max_shared_rows=0, wire_words=0):
        """Size the scratch up front so that no later `*_dev` call has to grow it (growing blocks): include/fbs_exec.h."""
        self._check(lib.fbs_ctx_reserve(self._h, int(max_keyswitches), int(max_shared_rows), int(wire_words)))

    def tune(self, **knobs):
        """Launcher knobs (`fbs_ctx_tune`): which kernel shape a launch takes; results never depend on them."""
        for k, v in knobs.items():
            self._check(lib.fbs_ctx_tune(self._h, k.encode(), int(v)))

    def tvset(self, tables):
        return TvSet(self, tables)

    def state(self, rows, T):
        """A `DeviceState` of [rows][T][D+1] ciphertexts in this context's device memory (fbs_state_create)."""
        return DeviceState(self, rows, T)

    def table(self, state, rows, spread=2):
        """A `DeviceTable` of rows of `state` ([planes][len] row numbers), `spread` boxes an entry (fbs_table_create)."""
        return DeviceTable(state, rows, spread)

    # ---- compact outputs: key-switched to the small key, rounded to `bits` bits a field, bit-packed (include/fbs_exec.h) ----
    def compact_dev(self, d_cts, count, d_words, bits=None, stream=0):
        """fbs_compact_dev: `count` big-key ciphertexts at d_cts -> [count][W] words at d_words, asynchronous on `stream`; needs
        no secret"""
        self._check(lib.fbs_compact_dev(self._h, d_cts or None, count, self.default_compact_bits if bits is None else int(bits),
                                        d_words or None, stream or None))

    def decrypt_compact(self, words, bits=None, device=True):
        """Compact ciphertexts [..][W] -> messages [..].  device=True: on the GPU (fbs_decrypt_compact_dev), False: on the host
        (fbs_decrypt_compact) -- the same messages."""
        if not device:
            return super().decrypt_compact(words, bits)
        bits, words, out = self._compact_io(words, bits)
        import torch
        d_w = torch.from_numpy(words.reshape(-1).view(np.int64)).to("cuda:%d" % self.device) if words.size else None
        d_m = torch.empty(max(1, out.size), dtype=torch.int64, device="cuda:%d" % self.device)
        torch.cuda.synchronize(d_m.device)
        self._check(lib.fbs_decrypt_compact_dev(self._h, d_w.data_ptr() if d_w is not None else None, out.size, bits, d_m.data_ptr(),
                                                None))
        self.sync()
        return d_m[:out.size].cpu().numpy().reshape(out.shape)

    def compact_fields_dev(self, d_words, count, d_fields, bits=None, stream=0):
        """fbs_compact_fields_dev: [count][W] words at width `bits` -> uint32 fields [count][n + 1] at log2(2N) bits (what the
        blind rotation reads), asynchronous on `stream`"""
        self._check(lib.fbs_compact_fields_dev(self._h, d_words or None, count, self.default_compact_bits if bits is None else int(bits),
                                               d_fields or None, stream or None))

    def refresh_compact_dev(self, d_words, count, d_cts, bits=None, stream=0):
        """fbs_refresh_compact_dev: [count][W] words -> fresh big-key ciphertexts [count][D+1] (one bootstrap through the identity
        table each), asynchronous on `stream`; needs no secret"""
        self._check(lib.fbs_refresh_compact_dev(self._h, d_words or None, count, self.default_compact_bits if bits is None else int(bits),
                                                d_cts or None, stream or None))

    def decrypt_compact_dev(self, d_words, count, d_msgs, bits=None, stream=0):
        self._check(lib.fbs_decrypt_compact_dev(self._h, d_words or None, count, self.default_compact_bits if bits is None else int(bits),
                                                d_msgs or None, stream or None))

    # ---- packed outputs: up to N outputs in one GLWE sample under the big key (include/fbs_exec.h, "packed outputs") ----
    def _import_gadget_key(self, noun, t, gamma, bodies):
        """fbs_import_<noun>_key, once the bodies are as many as `t` levels need"""
        bodies = _c(bodies, np.uint64).reshape(-1)
        if 1 <= int(t) <= 31 and bodies.size != self._gadget_key_sizes(noun, t)[0]:
            raise ValueError(f"{noun}_bodies has {bodies.size} words, the parameter set needs {self._gadget_key_sizes(noun, t)[0]}")
        self._check(getattr(lib, f"fbs_import_{noun}_key")(self._h, int(t), int(gamma), _ptr(bodies)))

    def import_packing_key(self, t_p, gamma_p, bodies):
        """fbs_import_packing_key: the masks come from the context's mask key; works on evaluation-only contexts"""
        self._import_gadget_key("packing", t_p, gamma_p, bodies)

    # ---- folded state: N resident ciphertexts in one full-precision GLWE sample (include/fbs_exec.h, "folded state") ----
    def fold_keygen(self, t_f, gamma_f):
        """fbs_fold_keygen: the fold key (t_f levels of gamma_f bits) beside the keys of `keygen_seeded`"""
        self._check(lib.fbs_fold_keygen(self._h, int(t_f), int(gamma_f)))

    def fold_key_sizes(self, t_f=0):
        """(bodies, whole key) in words for t_f levels (0: the context's own key)"""
        return self._gadget_key_sizes("fold", t_f)

    def export_fold_key(self, full=False):
        """dict(fold_levels, fold_base_bits, fold_bodies [D][t_f][N]); full=True adds `full`, the whole key [D][t_f][k+1][N] in the
        coefficient domain (a test hook)"""
        return self._export_gadget_key("fold", self.params.k * self.params.N, full)

    def import_fold_key(self, t_f, gamma_f, bodies):
        """fbs_import_fold_key: the masks come from the context's mask key; works on evaluation-only contexts"""
        self._import_gadget_key("fold", t_f, gamma_f, bodies)

    def fold_dev(self, d_cts, count, d_glwe, stream=0):
        """fbs_fold_dev: `count` big-key ciphertexts at d_cts -> folded samples at d_glwe, asynchronous on `stream`; no secret"""
        self._check(lib.fbs_fold_dev(self._h, d_cts or None, int(count), d_glwe or None, stream or None))

    # ---- encrypted-index reads: a folded table rotated by an encrypted index (include/fbs_exec.h, "encrypted-index reads") ----
    def fold_mapped_dev(self, d_cts, n_src, d_map, count, d_glwe, stream=0):
        """fbs_fold_mapped_dev: fold position j takes ciphertext d_map[j] of the `n_src` at d_cts (MAP_NEG: negated, MAP_NONE: none)
        -> folded samples at d_glwe, asynchronous on `stream`; no secret"""
        self._check(lib.fbs_fold_mapped_dev(self._h, d_cts or None, int(n_src), d_map or None, int(count), d_glwe or None, stream or None))

    def lookup_dev(self, d_tables, n_tables, d_table_of, d_cts_index, count, d_cts_out, stream=0):
        """fbs_lookup_dev: big-key index ciphertexts [count][D+1] -> the entries they name of the folded tables at d_tables
        ([n_tables][k+1][N]; d_table_of [count] or 0: index i reads table i), asynchronous on `stream`; no secret, no fold key"""
        self._check(lib.fbs_lookup_dev(self._h, d_tables or None, int(n_tables), d_table_of or None, d_cts_index or None, int(count),
                                       d_cts_out or None, stream or None))

    def lookup_compact_dev(self, d_tables, n_tables, d_table_of, d_words, count, d_cts_out, bits=None, stream=0):
        """fbs_lookup_compact_dev: the same lookup with the indices as compact ciphertexts [count][W] at width `bits`"""
        self._check(lib.fbs_lookup_compact_dev(self._h, d_tables or None, int(n_tables), d_table_of or None, d_words or None, int(count),
                                               self.default_compact_bits if bits is None else int(bits), d_cts_out or None, stream or None))

    # ---- encrypted tables: the rotated sample itself, and sums of samples (include/fbs_exec.h, "encrypted tables") ----
    def rotate_dev(self, d_tables, n_tables, d_table_of, d_cts_index, count, d_glwe_out, negate=False, stream=0):
        """fbs_rotate_dev: `lookup_dev` without the sample extraction -- the whole rotated sample of every index at d_glwe_out
        ([count][k+1][N]); negate: by the negated amounts, X^{+r} instead of X^{-r}"""
        self._check(lib.fbs_rotate_dev(self._h, d_tables or None, int(n_tables), d_table_of or None, d_cts_index or None, int(count),
                                       ROTATE_NEGATE if negate else 0, d_glwe_out or None, stream or None))

    def rotate_compact_dev(self, d_tables, n_tables, d_table_of, d_words, count, d_glwe_out, bits=None, negate=False, stream=0):
        """fbs_rotate_compact_dev: the same with the indices as compact ciphertexts [count][W] at width `bits`"""
        self._check(lib.fbs_rotate_compact_dev(self._h, d_tables or None, int(n_tables), d_table_of or None, d_words or None, int(count),
                                               self.default_compact_bits if bits is None else int(bits), ROTATE_NEGATE if negate else 0,
                                               d_glwe_out or None, stream or None))

    def glwe_add_dev(self, d_dst, n_dst, dst_of, d_src, stream=0):
        """fbs_glwe_add_dev: sample dst_of[f] of the `n_dst` at d_dst += sample f of d_src, modulo q; dst_of is a host array, checked
        (in range, no target twice)"""
        dst_of = _c(dst_of, np.uint32).reshape(-1)
        self._check(lib.fbs_glwe_add_dev(self._h, d_dst or None, int(n_dst), _ptr(dst_of), d_src or None, dst_of.size, stream or None))

    def debug_fold_front_dev(self, d_cts, count, cols, tg, d_fields, stream=0):
        """fbs_debug_fold_front_dev (a test hook): the fold's front kernel alone"""
        self._check(lib.fbs_debug_fold_front_dev(self._h, d_cts or None, int(count), int(cols), int(tg), d_fields or None, stream or None))

    def fold(self, cts):
        """Host ciphertexts [..][D+1] -> folded samples (through `fold_dev`); for tests and one-off calls"""
        import torch
        cts = _c(cts, np.uint64).reshape(-1, self.params.ct_words)
        count, prm = cts.shape[0], self.params
        words = -(-count // prm.N) * (prm.k + 1) * prm.N
        dev = f"cuda:{self.device}"
        d_c = torch.from_numpy(cts.view(np.int64)).to(dev) if count else torch.zeros(1, dtype=torch.int64, device=dev)
        d_w = torch.zeros(max(2, words), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(d_w.device)
        self.fold_dev(d_c.data_ptr(), count, d_w.data_ptr())
        self.sync()
        return d_w[:words].cpu().numpy().view(np.uint64)

    def pack_dev(self, d_cts, count, d_words, bits, stream=0):
        """fbs_pack_dev: `count` big-key ciphertexts at d_cts -> packed words at d_words, asynchronous on `stream`; no secret"""
        self._check(lib.fbs_pack_dev(self._h, d_cts or None, int(count), int(bits), d_words or None, stream or None))

    def debug_pack_fields_dev(self, d_fields, count, d_words, bits, stream=0):
        """fbs_debug_pack_fields_dev (a test hook): uint32 fields [count][n + 1] at 31 bits at d_fields, as the key switch of
        `pack_dev` leaves them, -> packed words at d_words; one pass at the most, no key switch"""
        self._check(lib.fbs_debug_pack_fields_dev(self._h, d_fields or None, int(count), int(bits), d_words or None, stream or None))

    def pack(self, cts, bits):
        """Host ciphertexts [..][D+1] -> packed words (through `pack_dev`); for tests and one-off calls"""
        import torch
        cts = _c(cts, np.uint64).reshape(-1, self.params.ct_words)
        count = cts.shape[0]
        d_c = torch.from_numpy(cts.view(np.int64)).to("cuda:%d" % self.device)
        d_w = torch.zeros(max(1, self.packed_words(count, bits)), dtype=torch.int64, device=d_c.device)
        torch.cuda.synchronize(d_c.device)
        self.pack_dev(d_c.data_ptr(), count, d_w.data_ptr(), bits)
        self.sync()
        return d_w[:self.packed_words(count, bits)].cpu().numpy().view(np.uint64)

    def bootstrap_batch(self, tvset, cts, table_ids=None):
        cts = _c(cts, np.uint64)
        count = cts.size // self.params.ct_words
        ids = None if table_ids is None else _c(table_ids, np.uint32)
        out = np.empty_like(cts)
        self._check(lib.fbs_bootstrap_batch(self._h, tvset._h, _ptr(cts), _ptr(ids), count, _ptr(out)))
        return out

    # device-pointer entry points (ints from torch.Tensor.data_ptr()); asynchronous on `stream`
    def encrypt_dev(self, d_msgs, count, d_cts, nonce0=None, stream=0):
        """fbs_encrypt_dev / fbs_encrypt_fresh_dev: `count` int64 messages at d_msgs -> [count][D+1] ciphertexts at d_cts,
        word-identical to `encrypt`.  Returns the first stream taken (nonce0, or the first fresh one when nonce0 is None)."""
        if nonce0 is None:
            first = C.c_uint64()
            self._check(lib.fbs_encrypt_fresh_dev(self._h, d_msgs or None, count, d_cts or None, C.byref(first), stream or None))
            return first.value
        self._check(lib.fbs_encrypt_dev(self._h, d_msgs or None, count, int(nonce0), d_cts or None, stream or None))
        return int(nonce0)

    def decrypt_dev(self, d_cts, count, d_msgs, stream=0):
        """fbs_decrypt_dev: [count][D+1] ciphertexts at d_cts -> `count` int64 messages at d_msgs, what `decrypt` returns."""
        self._check(lib.fbs_decrypt_dev(self._h, d_cts or None, count, d_msgs or None, stream or None))

    def bootstrap_batch_dev(self, tvset, d_in, d_table_ids, count, d_out, stream=0):
        self._check(lib.fbs_bootstrap_batch_dev(self._h, tvset._h, d_in, d_table_ids or None, count, d_out,
                                                stream or None))

    def lincomb_dev(self, d_wires, T, dst, term_off, srcs, coefs, consts, stream=0):
        dst, term_off, srcs = _c(dst, np.uint32), _c(term_off, np.uint32), _c(srcs, np.uint32)
        coefs, consts = _c(coefs, np.int64), _c(consts, np.int64)
        self._check(lib.fbs_lincomb_dev(self._h, d_wires, T, len(dst), _ptr(dst), _ptr(term_off), _ptr(srcs),
                                        _ptr(coefs), _ptr(consts), stream or None))

    def bootstrap_wires_dev(self, tvset, d_wires, T, src, dst, table_ids, s_begin, s_end, stream=0):
        src, dst, table_ids = _c(src, np.uint32), _c(dst, np.uint32), _c(table_ids, np.uint32)
        self._check(lib.fbs_bootstrap_wires_dev(self._h, tvset._h, d_wires, T, len(src), _ptr(src), _ptr(dst),
                                                _ptr(table_ids), s_begin, s_end, stream or None))

    def profile(self, on=True):
        self._check(lib.fbs_profile_enable(self._h, int(on)))

    def profile_read(self, reset=True):
        ms = (C.c_double * 3)()
        cnt = (C.c_uint64 * 3)()
        self._check(lib.fbs_profile_read(self._h, C.byref(ms), C.byref(cnt), int(reset)))
        names = ("keyswitch", "blind_rotate", "lincomb")
        return {n: dict(ms=ms[i], launches=int(cnt[i]), kernel=lib.fbs_profile_kernel(self._h, i).decode())
                for i, n in enumerate(names)}

    def profile_kernels(self):
        """{kernel instantiation: dict(kind, launches, ms)} since the last reset -- a launch cut into a whole-round part and a
        remainder shows as two entries."""
        need = C.c_size_t()
        self._check(lib.fbs_profile_kernels(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._check(lib.fbs_profile_kernels(self._h, buf, need.value, None))
        out = {}
        for line in buf.value.decode().splitlines():
            kind, name, launches, ms = line.split("\t")
            out[name] = dict(kind=("keyswitch", "blind_rotate", "lincomb")[int(kind)], launches=int(launches), ms=float(ms))
        return out

    def sync(self, stream=0):
        self._check(lib.fbs_sync(self._h, stream or None))

    def debug_polymul(self, a, b):
        a, b = _c(a, np.uint64), _c(b, np.uint64)
        c = np.empty_like(a)
        self._check(lib.fbs_debug_polymul(self._h, _ptr(a), _ptr(b), _ptr(c)))
        return c

    DEBUG_FIELD_OPS = ("fp_mulmod", "fp_mulmod_exact", "fp_center", "fp_canon", "fp_canon_near", "fp_u64_round_trip")

    def debug_field(self, op, x, w=None):
        """The device's raw result of a field primitive (DEBUG_FIELD_OPS) on int64 arrays, element by element."""
        x = _c(x, np.int64)
        w = None if w is None else _c(w, np.int64)
        out = np.empty_like(x)
        self._check(lib.fbs_debug_field(self._h, self.DEBUG_FIELD_OPS.index(op), _ptr(x), _ptr(w), x.size, _ptr(out)))
        return out

    def debug_gauss_dev(self, words, sigma):
        """The device's rounded Gaussian (sampler 1) of windows of six uint64 words [count][6] at standard deviation sigma -> int64
        [count], whatever the context's own sampler (fbs_debug_gauss_dev; `debug_gauss` is the host's)."""
        import torch
        words = _c(words, np.uint64).reshape(-1, 6)
        dev = torch.device("cuda", self.device)
        d_words = torch.from_numpy(words.view(np.int64)).to(dev)
        d_out = torch.empty(words.shape[0], dtype=torch.int64, device=dev)
        self._check(lib.fbs_debug_gauss_dev(self._h, d_words.data_ptr(), words.shape[0], int(sigma), d_out.data_ptr(), None))
        self.sync()
        return d_out.cpu().numpy()

    def debug_transform(self, variant, values):
        """One transform variant (a line of debug_transform_list) on [polys][N] int64 values, unreduced in and out."""
        values = _c(values, np.int64).reshape(-1, 1 << self.params.log_n_poly)
        out = np.empty_like(values)
        self._check(lib.fbs_debug_transform(self._h, variant.encode(), _ptr(values), _ptr(out), values.shape[0]))
        return out
