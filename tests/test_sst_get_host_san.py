"""AddressSanitizer + UndefinedBehaviorSanitizer run of the host SSTable get (no GPU):
tests/cpp/test_sst_get_host.cpp, a stand-alone program linked with the sanitized host runtime
(Makefile target `sanitize-sst-get`; device code is not instrumented and nothing is launched)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sst_get_host_clean_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tinykvpp_amd", "csrc"), "-j8", "sanitize-sst-get"], check=True)
    exe = os.path.join(ROOT, "tests", "cpp", "build", "test_sst_get_host_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
