"""Sample-axis operations without a GPU (include/fbs_exec.h, "sample-axis operations"): the two entries are declared, exported by
libfbsexec.so and bound with the header's argument counts, neither the client nor the public library carries them, and the ctypes
image of fbs_sample_map has the header's layout."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"fbs_eval_resident_mapped": 9, "fbs_state_sum_groups": 7}


def _header():
    return open(os.path.join(ROOT, "include", "fbs_exec.h")).read()


def test_entries_are_declared_exported_and_bound_with_the_headers_argument_counts():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, n_args in ENTRIES.items():
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, (name, args)
        assert len(getattr(_native.lib, name).argtypes) == n_args, name
    # the old entry keeps its eight arguments
    assert len(_native.lib.fbs_eval_resident.argtypes) == 8
    assert callable(_native.DeviceState.sum_groups)
    assert _native.SAMPLE_NONE == 0xFFFFFFFF and re.search(r"#define FBS_SAMPLE_NONE 0xFFFFFFFFu\b", _header())
    assert _native.MAX_SUM_GROUP == 65536 and re.search(r"#define FBS_MAX_SUM_GROUP 65536u\b", _header())


def test_neither_entry_is_in_the_client_or_the_public_library():
    from tfhe_fbs_map_amd import _client_native, _public_native
    for mod in (_client_native, _public_native):
        assert os.path.exists(mod.LIB_PATH), mod.LIB_PATH
        lib = ctypes.CDLL(mod.LIB_PATH)
        for name in ENTRIES:
            assert not hasattr(lib, name), (mod.__name__, name)
            assert name not in mod.EXPORTED_SYMBOLS, (mod.__name__, name)


def test_sample_map_has_the_layout_of_the_header():
    from tfhe_fbs_map_amd import _native
    body = re.search(r"typedef struct fbs_sample_map \{(.*?)\} fbs_sample_map;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t.strip(), n) for t, n in re.findall(r"([\w \*]+?)\b(\w+);", body)]
    assert fields == [("const uint32_t *", "index"), ("int64_t", "fill")]
    want = {"const uint32_t *": ctypes.c_void_p, "int64_t": ctypes.c_int64}
    assert [(n, want[t]) for t, n in fields] == list(_native._SampleMap._fields_)
    S = _native._SampleMap
    assert ctypes.sizeof(S) == 16 and (S.index.offset, S.fill.offset) == (0, 8)
    # fbs_resident_src and fbs_input_src are unchanged
    assert ctypes.sizeof(_native._ResidentSrc) == 16 and ctypes.sizeof(_native._InputSrc) == 32
