"""The public-key encryptor under AddressSanitizer and UBSan: tests/c/public_harness.cpp, a stand-alone program with the three host
sources of libfbspublic.so compiled in, runs key generation, encryption and expansion at exactly-sized buffers for the four toy
sets, with partly filled last samples.  Nothing is loaded into the interpreter under a sanitizer: the program is built and run as a
process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_public_entries_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "public.mk", "public_asan"], timeout=900)
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "public_harness")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "public ok" and "FAIL" not in r.stdout, r.stdout[-2000:]
    assert [ln.split(":")[0] for ln in lines[:5]] == ["k1_N256 sampler 0", "k1_N1024 sampler 0", "k2_N256 sampler 0", "k3_N256 sampler 0",
                                                      "k1_N256 sampler 1"], r.stdout


def test_harness_build_uses_the_sanitizers_and_no_gpu_toolchain():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "tests", "c"), "-f", "public.mk", "public_asan"], capture_output=True, text=True, check=True).stdout
    assert "-fsanitize=address,undefined" in out and "-fno-sanitize-recover=undefined" in out and "-DFBS_HOST_ONLY" in out
    assert "hipcc" not in out and "rocm" not in out.lower() and "__HIP_PLATFORM_AMD__" not in out, out
    for src in ("public_harness.cpp", "fbs_error.cpp", "fbs_host.cpp", "fbs_public.cpp"):
        assert src in out, src
    assert "LD_PRELOAD" not in out
    assert "LD_PRELOAD" not in open(os.path.join(ROOT, "tests", "c", "public.mk")).read()
