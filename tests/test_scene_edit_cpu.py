"""No-GPU tests of scene editing (include/kazen_mi355x_edit.h): the export list, every refusal (its code, its message, the host tables untouched), and the
host refit - bit for bit the build's tables for unchanged vertices; conservative BVH2 and dequantised BVH4 boxes, the light CDFs and the invisible-light box
after random deformations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scene_tables import P_BEAMOK, P_ILHI, P_ILLO, P_NIL, P_SIZE, check_refit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(sc):
    return {t: sc.table(t).copy() for t in range(8)}


def bvh(sc):
    b = sc.bvh_info()
    b.pop("buildSeconds")
    return b


def test_edit_header_exports_exactly_its_declarations(kz):
    lib = kz.abi.load_library()
    text = open(os.path.join(ROOT, "include", "kazen_mi355x_edit.h")).read()
    assert '#include "kazen_mi355x.h"' in text
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?(kz_[a-z0-9_]+)\s*\(", text, re.M))
    assert declared == set(kz.abi.EDIT_EXPORTS), declared ^ set(kz.abi.EDIT_EXPORTS)
    exported = set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", kz.abi.LIB_PATH], text=True)))
    assert declared <= exported
    for sym in declared:
        assert getattr(lib, sym) is not None
    assert not (declared & set(kz.abi.EXPORTS)) and "kz_scene_table" in kz.abi.EXPORTS


def test_param_offsets_and_update_struct(kz, tmp_path):
    src = tmp_path / "off.cpp"
    src.write_text('#include "kz_internal.h"\n#include <cstddef>\n#include <cstdio>\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(KzParams, nIlTris), '
                   'offsetof(KzParams, ilLo), offsetof(KzParams, ilHi), offsetof(KzParams, beamOk), sizeof(KzParams), sizeof(KzVertexUpdate));}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "nano-kazen_amd", "csrc"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [P_NIL, P_ILLO, P_ILHI, P_BEAMOK, P_SIZE, C.sizeof(kz.abi.KzVertexUpdate)]
    assert C.sizeof(kz.abi.KzVertexUpdate) == 24


def _update(lib, sc, rows):
    arr = (lib.kz_scene_set_vertices.argtypes[1]._type_ * max(1, len(rows)))(*rows)
    return lib.kz_scene_set_vertices(sc.h, arr, len(rows))


def test_every_refusal_has_a_code_a_message_and_changes_nothing(kz):
    a = kz.abi
    d = kz.scenes.cornell_box(32, 32, 4)
    sc = kz.Scene(d)
    lib = sc.lib
    before, info = tables(sc), bvh(sc)
    V, N = d.meshes[5]["V"], d.meshes[5]["N"]
    fp = lambda x: x.ctypes.data_as(a.f32p)
    nan = V.copy(); nan[3, 1] = np.nan
    inf = V.copy(); inf[0, 0] = np.inf
    cases = {
        "mesh out of range": [a.KzVertexUpdate(len(d.meshes), V.shape[0], fp(V), fp(N))],
        "mesh twice": [a.KzVertexUpdate(5, V.shape[0], fp(V), fp(N)), a.KzVertexUpdate(5, V.shape[0], fp(V), fp(N))],
        "wrong count": [a.KzVertexUpdate(5, V.shape[0] - 1, fp(V), fp(N))],
        "missing N": [a.KzVertexUpdate(5, V.shape[0], fp(V), None)],
        "null V": [a.KzVertexUpdate(5, V.shape[0], None, fp(N))],
        "nan": [a.KzVertexUpdate(5, V.shape[0], fp(nan), fp(N))],
        "inf": [a.KzVertexUpdate(5, V.shape[0], fp(inf), fp(N))],
        "good then bad": [a.KzVertexUpdate(6, d.meshes[6]["V"].shape[0], fp(d.meshes[6]["V"] + np.float32(0.1)), fp(d.meshes[6]["N"])),
                          a.KzVertexUpdate(5, V.shape[0], fp(nan), fp(N))],
    }
    for name, rows in cases.items():
        assert _update(lib, sc, rows) == a.KZ_ERR_INVALID_ARG, name
        assert len(lib.kz_last_error()) >= 25, name
        assert all(np.array_equal(v, before[k]) for k, v in tables(sc).items()) and bvh(sc) == info, name
    # a mesh without normals given N: a scene whose mesh has none
    d2 = kz.scenes.SceneDescription()
    d2.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    sc2 = kz.Scene(d2)
    V2 = d2.meshes[0]["V"]
    b2 = tables(sc2)
    assert _update(lib, sc2, [a.KzVertexUpdate(0, 3, fp(V2), fp(V2))]) == a.KZ_ERR_INVALID_ARG and len(lib.kz_last_error()) >= 25
    assert all(np.array_equal(v, b2[k]) for k, v in tables(sc2).items())
    # the camera: another size, another filter, an unsupported type
    for name, cam in {"width": {"width": 33}, "height": {"height": 31}, "rfilter": {"rfilter": {"type": "tent"}},
                      "stddev": {"rfilter": dict(d.camera["rfilter"], stddev=0.25)}, "type": {"type": "orthographic"}}.items():
        with pytest.raises(a.KzError) as e:
            sc.set_camera(cam)
        assert e.value.code in (a.KZ_ERR_INVALID_ARG, a.KZ_ERR_UNSUPPORTED) and len(str(e.value)) - len("kazen_mi355x error 1: ") >= 25, name
        assert all(np.array_equal(v, before[k]) for k, v in tables(sc).items()), name
    assert sc.desc.camera is d.camera


@pytest.mark.parametrize("name", ["cornell", "soup", "materials"])
def test_unchanged_vertices_leave_every_host_table_as_built(kz, name):
    d = {"cornell": lambda: kz.scenes.cornell_box(32, 32, 4), "soup": lambda: kz.scenes.random_triangles(20000, 64, 48, 4, sampler="independent"),
         "materials": lambda: kz.scenes.materials_scene(32, 24, 4)}[name]()
    sc = kz.Scene(d)
    before, info = tables(sc), bvh(sc)
    sc.set_vertices({m: (x["V"], x["N"]) if x["N"] is not None else x["V"] for m, x in enumerate(d.meshes)})
    after = tables(sc)
    assert [k for k in before if not np.array_equal(before[k], after[k])] == []
    assert bvh(sc) == info
    sc.set_camera({})
    assert np.array_equal(sc.table(kz.abi.KZ_TABLE_PARAMS), before[kz.abi.KZ_TABLE_PARAMS])


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_random_deformations_keep_every_box_conservative(kz, name):
    rng = np.random.default_rng(5)
    make = {"cornell": lambda: kz.scenes.cornell_box(32, 32, 4), "soup": lambda: kz.scenes.random_triangles(4000, 64, 48, 4, sampler="independent")}[name]
    sc = kz.Scene(make())
    sah0 = sc.bvh_info()["sahCost"]
    for frame in range(6):
        upd = {}
        for m, x in enumerate(sc.desc.meshes):
            V = x["V"].astype(np.float64)
            c = V.mean(axis=0)
            a = rng.normal() * 0.2
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            V = ((V - c) @ R.T + c + rng.normal(size=3) * 0.05 + rng.normal(size=V.shape) * 0.01).astype(np.float32)
            upd[m] = (V, x["N"]) if x["N"] is not None else V
        sc.set_vertices(upd)
        check_refit(kz, sc)
    info = sc.bvh_info()
    assert info["sahCost"] != sah0 and info["sahCost"] > 0
    # the refit tables are what the host refit of the same final vertices gives from the build's tables, whatever came in between
    once = kz.Scene(make())                                  # (the build's tree: sc.desc holds the deformed vertices now)
    once.set_vertices({m: (x["V"], x["N"]) if x["N"] is not None else x["V"] for m, x in enumerate(sc.desc.meshes)})
    assert all(np.array_equal(once.table(t), sc.table(t)) for t in range(8))


def test_python_keeps_the_description_in_step(kz):
    d = kz.scenes.cornell_box(32, 32, 4)
    sc = kz.Scene(d)
    V0 = d.meshes[5]["V"].copy()
    V = V0 + np.float32(0.05)
    sc.set_vertices({5: (V, d.meshes[5]["N"])})
    assert np.array_equal(sc.desc.meshes[5]["V"], V) and np.array_equal(V0, V0)
    sc.set_camera({"fov": 50.0, "type": "thinlens", "apertureRadius": 0.1, "focusDistance": 3.0})
    assert sc.desc.camera["fov"] == 50.0 and sc.desc.camera["type"] == "thinlens"
    fresh = kz.Scene(sc.desc)
    assert all(np.array_equal(fresh.table(t), sc.table(t)) for t in (kz.abi.KZ_TABLE_SHADE, kz.abi.KZ_TABLE_CDF, kz.abi.KZ_TABLE_LIGHTS))
    pf, ps = fresh.table(kz.abi.KZ_TABLE_PARAMS), sc.table(kz.abi.KZ_TABLE_PARAMS)
    for a, b in ((0, 144), (212, 224), (P_ILLO, P_ILHI + 12), (P_BEAMOK, P_SIZE)):      # the camera's words (s2c c2w invW invH clips, type aperture focus, beams), the invisible-light box
        assert np.array_equal(pf[a:b], ps[a:b]), (a, b)
