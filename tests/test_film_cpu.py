"""No GPU: the film type of the library (nano-kazen_amd/csrc/kz_film.h: KzFilm, the running tap sums of a film and the texels resolved from them) under AddressSanitizer
and UBSan. tests/host_cpp/film_test.cpp includes the header unchanged and stands in for kzMalloc, hipFree, hipMemset and hipMemsetAsync - nothing of the HIP runtime is
linked -, logging every call. A replica's four films go through upload, renders with and without accumulation, AOV mask changes, a clear and the release; the logged
allocations, memsets and frees are compared literally with what a call did before the four films shared one type, bytes() after each step with the totals
tests/test_aov_gpu.py expects, and an allocation failing at each position leaves every film whole or as it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-kazen_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_film_life_cycle_allocates_and_clears_as_before(tmp_path):
    exe = str(tmp_path / "film_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I" + ROCM_INCLUDE, "-I" + CSRC, os.path.join(ROOT, "tests", "host_cpp", "film_test.cpp"), "-o", exe])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "Sanitizer" not in r.stderr, r.stdout + r.stderr
