"""The rounded-Gaussian sampler under AddressSanitizer and UBSan: tests/c/sampler_harness.cpp, a stand-alone program, runs
csrc/fbs_sampler.hpp's gauss_sample on the planted windows of tests/test_sampler.py and 2^16 random ones at sigma = 1, 2^30 and q.
Nothing is loaded into the interpreter under a sanitizer: the program is built and run as a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_sampler_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "sampler.mk", "sampler_asan"], timeout=600)
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "sampler_harness")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "sampler ok" and "FAIL" not in r.stdout, r.stdout[-2000:]
    assert [ln.split(":")[0] for ln in lines[:3]] == ["sigma 1", "sigma 1073741824", "sigma 70368743669761"], r.stdout


def test_harness_build_uses_the_sanitizers_and_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "tests", "c"), "-f", "sampler.mk", "sampler_asan"], capture_output=True, text=True, check=True).stdout
    assert "-fsanitize=address,undefined" in out and "-fsanitize=float-cast-overflow" in out and "-fno-sanitize-recover=undefined" in out
    assert "hipcc" not in out and "rocm" not in out.lower() and "__HIP_PLATFORM_AMD__" not in out, out
    assert "sampler_harness.cpp" in out and "LD_PRELOAD" not in out
