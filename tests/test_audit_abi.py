"""Audited evaluation without a GPU (include/fbs_exec.h, "audited evaluation"): the two entries and the struct are declared,
exported and bound, the ctypes image of fbs_audit_row has the header's layout, the point codes agree, the plan keeps the wire ids the
audit reports, and the client and public-key libraries export what they exported before."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ENTRIES = ("fbs_audit_rows", "fbs_audit_level_dev")


def header():
    return open(os.path.join(ROOT, "include", "fbs_exec.h")).read()


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
        assert getattr(_native.lib, name).argtypes is not None, name
    assert callable(_native.Program.audit_rows) and callable(_native.Program.audit_level_dev)
    assert len(_native.lib.fbs_audit_level_dev.argtypes) == 12 and len(_native.lib.fbs_audit_rows.argtypes) == 5


def test_audit_row_has_the_layout_of_the_header():
    from tfhe_fbs_map_amd import _native
    body = re.search(r"typedef struct fbs_audit_row \{(.*?)\} fbs_audit_row;", header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in names.split(",")]
    assert fields == [("uint64_t", "count"), ("uint64_t", "over"), ("uint64_t", "max_abs"), ("int64_t", "sum"),
                      ("uint64_t", "sumsq_lo"), ("uint64_t", "sumsq_hi")]
    want = {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64}
    assert [(n, want[t]) for t, n in fields] == list(_native._AuditRow._fields_)
    R = _native._AuditRow
    assert ctypes.sizeof(R) == 48 and [getattr(R, n).offset for _, n in fields] == [0, 8, 16, 24, 32, 40]


def test_point_codes_and_sample_bound_agree_with_the_sources():
    from tfhe_fbs_map_amd import _native, audit
    codes = dict(re.findall(r"#define FBS_AUDIT_(\w+)\s+(\d+)u", header()))
    assert codes == dict(INPUTS="0", LINCOMB="1", ROTATION_INPUT="2", BOOTSTRAP="3")
    assert (_native.AUDIT_INPUTS, _native.AUDIT_LINCOMB, _native.AUDIT_ROTATION_INPUT, _native.AUDIT_BOOTSTRAP) == (0, 1, 2, 3)
    assert audit.POINTS == ("inputs", "lincomb", "rotation_input", "bootstrap")      # the names, in the order of the codes
    internal = open(os.path.join(CSRC, "fbs_internal.hpp")).read()
    assert "AUDIT_MAX_SAMPLES = (size_t)1 << 18" in internal and _native.AUDIT_MAX_SAMPLES == 1 << 18
    # |e| <= (q - 1) / 2 < 2^45: 2^18 of them stay below 2^63, their squares below 2^108
    from tfhe_fbs_map_amd import MODULUS
    assert _native.AUDIT_MAX_SAMPLES * ((MODULUS - 1) // 2) < 1 << 63
    assert _native.AUDIT_MAX_SAMPLES * ((MODULUS - 1) // 2) ** 2 < 1 << 128


def test_every_audit_entry_is_an_exception_barrier_and_outside_the_kernel_catalog():
    from tfhe_fbs_map_amd import _native
    text = open(os.path.join(CSRC, "fbs_capi.cpp")).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\([^{};]*?\) try \{" % name, text, flags=re.M), name
    assert not [k for k in _native.kernel_catalog() if "audit" in k]
    assert "fbs_audit.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_client_and_public_libraries_export_what_they_did():
    """the audit needs the GPU and the secret at once: it is part of neither host library"""
    from tests.test_client_lib import CLIENT_ENTRIES
    from tfhe_fbs_map_amd import _client_native, _public_native
    subprocess.check_call(["make", "-s", "-C", CSRC, "client", "public"], timeout=600)
    for lib, want in (("libfbsclient.so", CLIENT_ENTRIES), ("libfbspublic.so", None)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tfhe_fbs_map_amd", lib)], capture_output=True, text=True,
                             check=True).stdout
        exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("fbs_"))
        assert not [n for n in exported if "audit" in n], lib
        if want is not None:
            assert exported == sorted(want)
    assert sorted(_client_native.EXPORTED_SYMBOLS) == sorted(CLIENT_ENTRIES)
    assert not [n for n in _public_native.EXPORTED_SYMBOLS if "audit" in n]
    # ... while the GPU library defines both
    from tfhe_fbs_map_amd import _native
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines()}


PLAN_PROBE = r"""
#include <cstdio>
#include "fbs_plan.hpp"
using namespace fbs;
int main() {
    // wires: 0 a, 1 b | 2 = a + b, 3 = T0(2), 4 = T1(2), 5 = T0(b), 6 = 3 + 2 * 4, 7 = 6 + 5, 8 = T1(7)
    const uint8_t kind[] = {0, 1, 1, 1, 0, 0, 1};
    const uint32_t arg0[] = {0, 2, 2, 1, 2, 4, 7}, arg1[] = {2, 0, 1, 0, 2, 2, 1};
    const int64_t cst[] = {0, 0, 0, 0, 0, 0, 0}, coef[] = {1, 1, 1, 2, 1, 1}, out[] = {8};
    const uint32_t src[] = {0, 1, 3, 4, 6, 5};
    fbs_program_desc d{};
    d.n_inputs = 2; d.n_instr = 7; d.n_terms = 6; d.n_outputs = 1;
    d.kind = kind; d.arg0 = arg0; d.arg1 = arg1; d.const_coef = cst; d.term_coef = coef; d.term_src = src; d.out_wire = out;
    const uint8_t fusable[] = {1, 1};
    for (int fuse = 0; fuse < 2; fuse++) {
        ProgramPlan plan;
        std::string why;
        if (plan_program(&d, 2, fuse ? fusable : nullptr, &plan, &why) != FBS_OK) { std::printf("error %s\n", why.c_str()); return 1; }
        for (uint32_t L = 0; L <= plan.depth; L++)
            for (size_t s = 0; s < plan.lin[L].size(); s++) {
                std::printf("fuse %d lin %u.%zu:", fuse, L, s);
                for (uint32_t w : plan.lin[L][s].dst_wire) std::printf(" %u", w);
                std::printf("\n");
            }
        for (uint32_t L = 0; L < plan.depth; L++) {
            const BootPlan &b = plan.boot[L];
            std::printf("fuse %d boot %u: src", fuse, L);
            for (uint32_t w : b.src_wire) std::printf(" %u", w);
            std::printf(" dst");
            for (uint32_t w : b.dst_wire) std::printf(" %d", (int)w);
            std::printf(" x");
            for (uint32_t w : b.x_wire) std::printf(" %u", w);
            std::printf(" sizes %zu %zu %zu\n", b.src_slot.size(), b.dst.size(), b.x_dst.size());
        }
    }
    return 0;
}
"""


def test_the_plan_keeps_the_wire_id_of_every_writer_and_every_source(tmp_path):
    """`plan_program` (host code, no device): the wire id beside every slot it hands out -- per LinearProd sub-stage, per distinct
    key-switch source, per gate (a shared rotation writes no wire: -1) and per extraction of a fused plan."""
    (tmp_path / "probe.cpp").write_text(PLAN_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(tmp_path / "probe.cpp"), os.path.join(CSRC, "fbs_plan.cpp"),
                           "-o", exe], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    assert out == [
        "fuse 0 lin 0.0: 2",
        "fuse 0 lin 1.0: 6",
        "fuse 0 lin 1.1: 7",
        "fuse 0 boot 0: src 1 2 dst 5 3 4 x sizes 2 3 0",
        "fuse 0 boot 1: src 7 dst 8 x sizes 1 1 0",
        "fuse 1 lin 0.0: 2",
        "fuse 1 lin 1.0: 6",
        "fuse 1 lin 1.1: 7",
        "fuse 1 boot 0: src 1 2 dst 5 -1 x 3 4 sizes 2 2 2",
        "fuse 1 boot 1: src 7 dst 8 x sizes 1 1 0",
    ], out
