"""No GPU: the four move-only owners of the library's device resources (nano-kazen_amd/csrc/kz_own.h: DevBuf, PinnedBuf, Event, Stream) under AddressSanitizer
and UBSan. tests/host_cpp/own_test.cpp includes the header unchanged and stands in for the HIP functions it calls - nothing of the HIP runtime is linked -, counting
what is live: nothing after scope exit, nothing freed by a moved-from owner, never two buffers during a regrow, an empty owner and the allocation's error code after
a failure, one creation per ensure(), and a PassCtx-shaped aggregate with nested views released exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-kazen_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owners_release_everything_exactly_once(tmp_path):
    exe = str(tmp_path / "own_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I" + ROCM_INCLUDE, "-I" + CSRC, os.path.join(ROOT, "tests", "host_cpp", "own_test.cpp"), "-o", exe])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "Sanitizer" not in r.stderr, r.stdout + r.stderr
