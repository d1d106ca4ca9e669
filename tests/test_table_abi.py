"""Encrypted tables without a GPU (include/fbs_exec.h, "encrypted tables"): the entries are declared, exported by libfbsexec.so and
bound with the header's argument counts and types, neither the client nor the public library carries them, and the header's
constants are the binding's."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ctypes
# the header's parameter types, in order, as the ctypes image the binding must give them
ENTRIES = {
    "fbs_table_map": ["uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t *"],
    "fbs_rotate_dev": ["fbs_ctx *", "const uint64_t *", "uint32_t", "const uint32_t *", "const uint64_t *", "size_t", "uint32_t", "uint64_t *", "void *"],
    "fbs_rotate_compact_dev": ["fbs_ctx *", "const uint64_t *", "uint32_t", "const uint32_t *", "const uint64_t *", "size_t", "uint32_t", "uint32_t",
                               "uint64_t *", "void *"],
    "fbs_glwe_add_dev": ["fbs_ctx *", "uint64_t *", "size_t", "const uint32_t *", "const uint64_t *", "size_t", "void *"],
    "fbs_table_create": ["fbs_ctx *", "const fbs_state *", "const uint32_t *", "uint32_t", "uint32_t", "uint32_t", "fbs_table **"],
    "fbs_table_stat": ["const fbs_table *", "const char *", "int64_t *"],
    "fbs_table_words": ["fbs_ctx *", "const fbs_table *", "uint64_t *"],
    "fbs_table_read": ["fbs_ctx *", "const fbs_table *", "const fbs_state *", "size_t", "fbs_state *", "size_t"],
    "fbs_table_write": ["fbs_ctx *", "fbs_table *", "const fbs_state *", "size_t", "const fbs_state *", "const uint32_t *", "uint32_t",
                        "const fbs_tvset *"],
}
IMAGE = {"uint32_t": C.c_uint32, "size_t": C.c_size_t, "const char *": C.c_char_p, "fbs_table **": C.POINTER(C.c_void_p),
         "int64_t *": C.POINTER(C.c_int64)}


def _header():
    return open(os.path.join(ROOT, "include", "fbs_exec.h")).read()


def test_entries_are_declared_exported_and_bound_with_the_headers_signatures():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, types in ENTRIES.items():
        assert name in declared_symbols() and hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        declared = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip() for a in args.split(",")]
        assert declared == types, (name, declared)
        bound = getattr(_native.lib, name)
        assert bound.restype is C.c_int32 or bound.restype is C.c_int
        assert list(bound.argtypes) == [IMAGE.get(t, C.c_void_p) for t in types], name
    assert re.search(r"\bvoid\s+fbs_table_free\s*\(\s*fbs_table \*table\s*\)\s*;", text) and hasattr(lib, "fbs_table_free")
    assert _native.lib.fbs_table_free.restype is None and list(_native.lib.fbs_table_free.argtypes) == [C.c_void_p]
    assert re.search(r"typedef struct fbs_table fbs_table;", text)
    # the lookups keep their signatures
    assert len(_native.lib.fbs_lookup_dev.argtypes) == 8 and len(_native.lib.fbs_lookup_compact_dev.argtypes) == 9
    assert len(_native.lib.fbs_lookup_map.argtypes) == 6
    assert _native.ROTATE_NEGATE == 1 and re.search(r"#define FBS_ROTATE_NEGATE 1u\b", _header())


def test_no_entry_is_in_the_client_or_the_public_library():
    from tfhe_fbs_map_amd import _client_native, _public_native
    for mod in (_client_native, _public_native):
        assert os.path.exists(mod.LIB_PATH), mod.LIB_PATH
        lib = ctypes.CDLL(mod.LIB_PATH)
        for name in ENTRIES:
            assert not hasattr(lib, name), (mod.__name__, name)
            assert name not in mod.EXPORTED_SYMBOLS, (mod.__name__, name)


def test_the_section_says_what_the_entries_refuse():
    text = _header()
    at = text.index("encrypted tables: the primitives of a write by an encrypted index")
    section = text[at:text.index("a loaded program, one level at a time")]
    for phrase in ("floor((2 p c + s N) / (2 s N))", "W(j - N) == 0", "len > floor(p / spread)", "16-byte aligned", "named twice",
                   "(2N - a) mod 2N", "Every entry writes nothing when it fails"):
        assert phrase in section, phrase
