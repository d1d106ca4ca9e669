"""Each entry of include/fbs_exec.h is written once.  libfbsexec.so and libfbsclient.so serve the client's entries from one text
(csrc/fbs_client_entries.cpp), and `_native.Context` and `HostContext` wrap them with one set of methods (`ClientContext`), so that
the two libraries say the same words, codes and texts by construction.  Only what differs on a machine with no device is written
per library."""
import glob
import os
import re

import pytest

from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")

# what a library without a device does differently: one definition in fbs_capi.cpp, one in fbs_client_capi.cpp
PER_LIBRARY = ["fbs_ctx_create", "fbs_ctx_stat", "fbs_ctx_destroy", "fbs_device_info", "fbs_keygen", "fbs_keygen_seeded",
               "fbs_packing_keygen"]
# the wrappers both bindings have: defined on the base, and nowhere else but for the GPU forms below
SHARED_METHODS = ["__init__", "_check", "stat", "keygen", "export_keys", "keygen_seeded", "seeded_key_sizes", "export_seeded_keys",
                  "encrypt", "decrypt", "encrypt_seeded", "expand_seeded", "default_compact_bits", "compact_words", "decrypt_compact",
                  "packing_keygen", "packing_key_sizes", "export_packing_key", "packed_words", "decrypt_packed"]
GPU_FORMS = {"__init__", "encrypt_seeded", "decrypt_compact"}   # the device part, the device=True branches


def test_each_entry_is_written_once():
    where = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        for m in re.finditer(r"^(?:int|void|double|const char \*) ?(fbs_\w+)\(([^{};]*?)\) (try )?\{", open(path).read(), flags=re.M):
            where.setdefault(m.group(1), []).append(os.path.basename(path))
    declared = declared_symbols()
    assert set(PER_LIBRARY) <= set(declared)
    assert set(PER_LIBRARY) <= {"fbs_ctx_create", "fbs_ctx_create_seeded", "fbs_ctx_stat", "fbs_ctx_destroy", "fbs_device_info", "fbs_keygen",
                                "fbs_keygen_seeded", "fbs_packing_keygen"}
    for name in declared:
        if name in PER_LIBRARY:
            assert sorted(where.get(name, [])) == ["fbs_capi.cpp", "fbs_client_capi.cpp"], (name, where.get(name))
        else:
            assert len(where.get(name, [])) == 1, (name, where.get(name))
    # and the shared text is in both libraries, and only there
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    lists = {var: re.findall(r"^%s\s*:=(.*)$" % var, makefile, flags=re.M) for var in ("NAMES", "CLIENT_NAMES", "PUBLIC_NAMES")}
    assert all(len(found) == 1 for found in lists.values()), lists
    lists = {var: found[0].split() for var, found in lists.items()}
    assert "fbs_client_entries.cpp" in lists["NAMES"] and "fbs_client_entries.cpp" in lists["CLIENT_NAMES"]
    assert "fbs_client_entries.cpp" not in lists["PUBLIC_NAMES"]
    assert "fbs_client_capi.cpp" not in lists["NAMES"] and "fbs_capi.cpp" not in lists["CLIENT_NAMES"]


def _csrc(name):
    return open(os.path.join(CSRC, name)).read()


def _function_bodies(text):
    """{name: body} of the functions defined at the left margin or one namespace level in: a line that ends in ") {" or ") try {"
    up to the next line that is "}" alone"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^[\w:<>*&, ]*?\b(\w+)\((?:[^;{}]|\n)*?\)(?: const)? (?:try )?\{\n(.*?)^\}", text, flags=re.M | re.S)}


def test_the_frame_of_a_sample_is_written_once():
    """Every LWE row and every GLWE zero sample comes from one generator on each side: csrc/fbs_rows.hpp on the
    device, mask_words / lwe_body / glwe_zero_sample in csrc/fbs_host.cpp on the host."""
    rows, io, keygen = _csrc("fbs_rows.hpp"), _csrc("fbs_io.hip"), _csrc("fbs_keygen.hip")
    # the three-way block store and the vector type it stores, once across the sample kernels' files
    ladder = r"& 15u\) == 0\) \{\n[^\n]*u64x2[^\n]*w\[i\], w\[i \+ 1\]"
    typedef = r"typedef uint64_t u64x2\b"
    assert len(re.findall(ladder, rows)) == 1 and len(re.findall(typedef, rows)) == 1
    for text in (io, keygen):
        assert not re.search(r"& 15u\) == 0", text) and not re.search(typedef, text)
        assert '#include "fbs_rows.hpp"' in text
    for name in ("fbs_public.hip", "fbs_state.hip"):   # (their own alignment code stores something else; the type is the shared one)
        assert not re.search(typedef, _csrc(name)) and '#include "fbs_rows.hpp"' in _csrc(name), name
    # the block loop over a ChaCha stream is in the frame and in k_glwe_key_rows (mask columns, noise), nowhere else in the two files
    assert "chacha_block" not in io
    assert len(re.findall(r"chacha_block\(", keygen)) == 2 and len(re.findall(r"chacha_block\(", rows)) == 2
    # one wave sum, and no butterfly spelled out where it is a drop-in (k_audit_reduce propagates carries: its own)
    sums = {name: len(re.findall(r"\+= __shfl_xor\(", _csrc(name))) for name in os.listdir(CSRC) if name.endswith((".hip", ".hpp"))}
    assert {name: n for name, n in sums.items() if n} == {"fbs_rows.hpp": 1, "fbs_audit.hip": 2}, sums
    assert "k_audit_reduce" in _csrc("fbs_audit.hip") and not re.search(r"\w*wave_sum\(\w+ \w+\) \{", io + keygen)


def test_one_key_transform_kernel():
    kernels = {}
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        text = open(path).read()
        for old in ("k_bsk_transform", "k_pack_key_transform", "k_secret_transform"):
            assert old not in text, (old, os.path.basename(path))
        for m in re.finditer(r"__global__[^;{]*?\bvoid (k_\w*transform\w*)\(", text):
            kernels.setdefault(m.group(1), []).append(os.path.basename(path))
    kernels.pop("k_debug_transform", None)   # (a test hook that runs one named transform variant: not a key's)
    assert kernels == {"k_key_transform": ["fbs_blind_rotate.hpp"]}, kernels
    launches = {name: len(re.findall(r"\(k_key_transform<", _csrc(name))) for name in ("fbs_blind_rotate.hip", "fbs_pack.hip", "fbs_keygen.hip")}
    assert launches == {"fbs_blind_rotate.hip": 2, "fbs_pack.hip": 1, "fbs_keygen.hip": 1}, launches


def test_one_gadget_key_path():
    """The packing key and the fold key are one family (GadgetKind, csrc/fbs_internal.hpp): no per-key wrapper is left, their
    ChaCha20 domains are named in the kind table alone, and the bracket of the shared scratch is written once."""
    texts = {name: _csrc(name) for name in sorted(os.listdir(CSRC)) if name.endswith((".cpp", ".hip", ".hpp", ".h")) or name == "Makefile"}
    for old in ("host_packing_keygen", "host_fold_keygen", "host_expand_packing_key", "host_expand_fold_key", "dev_packing_bodies",
                "dev_fold_bodies", "dev_upload_packing_key", "dev_upload_fold_key", "install_fold_key", "fold_passes", "check_fold_params"):
        assert [name for name, text in texts.items() if old in text] == [], old
    internal = texts["fbs_internal.hpp"]
    table = re.findall(r"^constexpr GadgetKindInfo GADGET_KINDS\[2\] = .*$", internal, flags=re.M)
    assert len(table) == 1
    for dom in ("DOM_FOLD_MASK", "DOM_PACK_MASK"):
        assert [name for name, text in texts.items() if dom in text] == ["fbs_internal.hpp"], dom
        assert len(re.findall(r"\b%s\b" % dom, internal)) == 2 and len(re.findall(r"\b%s\b" % dom, table[0])) == 1   # the enum, the table
        assert re.search(r"\b%s = \d+" % dom, internal)
    capi = texts["fbs_capi.cpp"]
    bodies = _function_bodies(capi)
    callers = sorted(name for name, body in bodies.items() if "scratch_wait(" in body)
    assert callers == ["scratch_section"], callers
    assert len(re.findall(r"scratch_wait\(", capi)) == 2                              # its definition, and that call
    assert len(re.findall(r"^int scratch_wait\(", capi, flags=re.M)) == 1


def test_the_host_draws_masks_and_products_in_one_place():
    host, public = _csrc("fbs_host.cpp"), _csrc("fbs_public.cpp")
    # no negacyclic add of its own in the public-key library: the shift-and-subtract idiom and the old name are gone
    assert "add_times_bits" not in public and not re.search(r"\[j \+ sh - N\]", public)
    assert "add_times_key(" in public and len(re.findall(r"^void add_times_key\(", host, flags=re.M)) == 1
    assert "rand_words" not in public.replace("rand_words(pub->key, stream_id(DOM_PUB_ENC_U", "")   # (u: bits, not a mask)
    # rand_words: its definition, the secrets, noise_sample and mask_words; every other caller goes through the helpers
    bodies = _function_bodies(host)
    assert {"rand_words", "noise_sample", "mask_words", "lwe_body", "glwe_zero_sample", "draw_secrets", "host_keygen", "host_encrypt"} <= set(bodies)
    callers = sorted(name for name, body in bodies.items() if "rand_words(" in body)
    assert callers == ["draw_secrets", "mask_words", "noise_sample"], callers
    # and the fold of a mask word and the product by the secret are the helpers' alone
    assert sorted(name for name, body in bodies.items() if "fq_fold(" in body) == ["mask_words"]
    users = sorted(name for name, body in bodies.items() if "add_times_key(" in body)
    assert users == ["glwe_zero_sample"], users
    assert "std::fill(s.begin(), s.end(), 0u)" in public   # fbs_pub_keygen still wipes the secret's positions


def test_no_library_exports_what_allocates_a_context():
    """sizeof(fbs_ctx) is each library's own, and libfbsexec.so is not linked -Bsymbolic: were admit_params, params_admitted or
    ctx_create in a dynamic symbol table, a process with two of the libraries could allocate a context with one and fill it with
    the other"""
    import subprocess
    pkg = os.path.join(ROOT, "tfhe_fbs_map_amd")
    subprocess.check_call(["make", "-s", "-C", CSRC, "client", "public"], timeout=600)
    for lib in ("libfbsexec.so", "libfbsclient.so", "libfbspublic.so"):
        names = subprocess.run(["nm", "-D", os.path.join(pkg, lib)], capture_output=True, text=True, check=True).stdout
        assert names and not re.search(r"admit_params|params_admitted|3fbs10ctx_create", names), lib


def test_both_bindings_wrap_the_client_entries_once():
    from tfhe_fbs_map_amd import HostContext, _client_native, _native
    from tfhe_fbs_map_amd._native import Context
    base = _client_native.ClientContext
    assert issubclass(Context, base) and issubclass(HostContext, base) and HostContext is _client_native.HostContext
    assert Context.__mro__[1] is base and HostContext.__mro__[1] is base
    for name in SHARED_METHODS:
        assert name in base.__dict__, name
        assert name not in HostContext.__dict__, name
        assert (name in Context.__dict__) == (name in GPU_FORMS), name
    # the one hook, and each closes its own handle (the GPU's with its states)
    assert "_lib" in Context.__dict__ and "_lib" in HostContext.__dict__
    assert "close" in Context.__dict__ and "close" in HostContext.__dict__
    from tfhe_fbs_map_amd import Params
    with pytest.raises(NotImplementedError):                            # the base alone names no library
        base(Params(n=12, log_n_poly=8, p_msg=7, sigma_lwe=256, sigma_glwe=256), seed=1)
    # one signature table: what the client library binds is what the GPU library binds under the same name
    assert tuple(_client_native.SIGNATURES) == _client_native.EXPORTED_SYMBOLS and len(_client_native.SIGNATURES) == 27
    for name, (res, args) in _client_native.SIGNATURES.items():
        fn = getattr(_native.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    src = open(os.path.join(ROOT, "tfhe_fbs_map_amd", "_native.py")).read()
    load = src[src.index("def _load():"):src.index("EXPORTED_SYMBOLS = (")]
    for name in _client_native.SIGNATURES:
        assert '"%s"' % name not in load, name                          # not typed out a second time
    assert "_client_native.SIGNATURES" in load
