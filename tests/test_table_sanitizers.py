"""The host side of encrypted tables under AddressSanitizer and UBSan: tests/c/table_harness.cpp, a stand-alone program with the host
sources compiled in, writes the wide-box map of every (p, N, spread) the tests use into exactly-sized buffers, with len = 1 and
floor(p / spread) and a base and stride that reach index 2^31 - 1, checks every entry against the rule in signed arithmetic, spread 1
against the box map, and every refusal.  Nothing is loaded into the interpreter under a sanitizer: the program is built and run as a
process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_table_maps_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "table.mk", "table_asan"], timeout=900)
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "table_harness")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines == ["ok table maps: 306 cases", "table ok"], r.stdout[-2000:]


def test_harness_build_uses_the_sanitizers_and_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "tests", "c"), "-f", "table.mk", "table_asan"], capture_output=True, text=True, check=True).stdout
    assert "-fsanitize=address,undefined" in out and "-fno-sanitize-recover=undefined" in out and "-DFBS_HOST_ONLY" in out
    assert "hipcc" not in out and "rocm" not in out.lower() and "__HIP_PLATFORM_AMD__" not in out, out
    for src in ("table_harness.cpp", "fbs_error.cpp", "fbs_host.cpp"):
        assert src in out, src
