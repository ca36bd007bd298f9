"""The compiled C++ test program of the host mirror (tests/host_cpp/host_mirror_test.cpp) as a fixture, and the scene it builds, built through Python's own
path: what tests/test_host_mirror.py and tests/test_output.py share. A support module beside the tests, like sample_corners.py: imported, never collected."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_cpp", "host_mirror_test.cpp")
LIBDIR = os.path.join(ROOT, "nano-kazen_amd", "csrc")
HOST = os.path.join(ROOT, "nano-kazen_amd", "host")
# the two files INTEGRATION.md adds to a kazen tree, compiled unchanged against the mirror (mirror_tree/kazen/*.h answer to the reference's header names)
ADAPTER = os.path.join(HOST, "adapter", "renderer_mi355x.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HOST, "mirror_tree"), "-I" + os.path.join(HOST, "adapter")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory, kz):
    kz.abi.load_library()
    out = str(tmp_path_factory.mktemp("host") / "host_mirror_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + INCLUDES + ["-o", out, SRC, ADAPTER, "-L" + LIBDIR, "-lkazen_mi355x", "-Wl,-rpath," + LIBDIR])
    return out


def python_twin(kz):
    S = kz.scenes
    s = S.SceneDescription()

    def q(p, n):
        P = np.array(p, np.float32)
        return P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.tile(np.array(n, np.float32), (4, 1)), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    s.add_mesh(*q([(-2, -1, -2), (2, -1, -2), (2, -1, 2), (-2, -1, 2)], (0, 1, 0)))
    s.add_mesh(*q([(-2, -1, -2), (-2, 2, -2), (2, 2, -2), (2, -1, -2)], (0, 0, 1)), bsdf=S.diffuse((0.7, 0.3, 0.3)))
    s.add_mesh(*q([(-0.8, -0.6, 0), (0.8, -0.6, 0), (0.8, 0.6, -0.6), (-0.8, 0.6, -0.6)], (0, 0.70710678, 0.70710678)),
               bsdf=S.kazenstandard((0.8, 0.6, 0.2), roughness=0.4, metallic=0.0, clearcoat=1.0, sheen=0.5))
    s.add_mesh(*q([(-0.5, 1.5, -0.5), (-0.5, 1.5, 0.5), (0.5, 1.5, 0.5), (0.5, 1.5, -0.5)], (0, -1, 0)), light=S.area((1.0, 0.9, 0.8), 12.0, False))
    s.background = {"color": (0.5, 0.6, 1.0), "intensity": 0.25}
    s.camera.update(width=64, height=48, fov=40.0, nearClip=0.1, farClip=100.0, toWorld=S.look_at((0, 0.5, 3.0), (0, 0, 0), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": 8, "seed": 0}
    s.integrator["maxDepth"] = 4
    return s
