"""The client library's sources under AddressSanitizer and UBSan: tests/c/client_harness.c, a stand-alone C program, drives
csrc/fbs_error.cpp, fbs_host.cpp, fbs_client_entries.cpp and fbs_client_capi.cpp through the C ABI -- contexts in both seed forms, both key generations,
every export into exactly-sized malloc buffers, every kind of encryption and decryption, the refusals.  Nothing is loaded into the
interpreter under a sanitizer: the program is built and run as a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_client_sources_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "client.mk", "client_asan"], timeout=600)
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "client_harness")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.endswith(" ok")]
    assert ok == ["k=1 N=256 group=1 ok", "k=2 N=256 group=2 ok"], r.stdout
    assert "FAIL" not in r.stdout


def test_harness_build_uses_the_sanitizers_and_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "tests", "c"), "-f", "client.mk", "client_asan"], capture_output=True, text=True, check=True).stdout
    assert "-fsanitize=address,undefined" in out and "-fno-sanitize-recover=undefined" in out
    assert "hipcc" not in out and "rocm" not in out.lower() and "__HIP_PLATFORM_AMD__" not in out, out
    for src in ("fbs_error.cpp", "fbs_host.cpp", "fbs_client_entries.cpp", "fbs_client_capi.cpp", "client_harness.c"):
        assert src in out, src
    assert "fbs_plan.cpp" not in out and "fbs_select.cpp" not in out
