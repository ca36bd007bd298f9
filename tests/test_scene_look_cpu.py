"""No-GPU tests of kz_scene_set_bsdfs / kz_scene_set_lights / kz_scene_set_transforms (include/kazen_mi355x_edit.h) on the host tables: the export list and
the struct sizes, every refusal (its code, its message, tables 0..8 untouched), and after every edit the tables a fresh kz_scene_create of the edited
description builds - byte for byte. A transform is held against kz_scene_set_vertices of scenes.transform_vertices' arrays on a twin scene."""
import ctypes as C
import json
import os
import re
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# offsets into KzParams (tests/test_scene_edit_cpu.py pins the first three and the size)
P_SHADOWFAST, P_NIL, P_ILLO, P_ILHI, P_ANYINV, P_BSDFEXT = 296, 300, 304, 316, 328, 396
NTAB = 9


def tables(sc, which=range(NTAB)):
    return {t: sc.table(t).copy() for t in which}


def differing_tables(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def bvh(sc):
    b = sc.bvh_info()
    b.pop("buildSeconds")
    return b


def prm_i32(sc, off):
    return int(sc.table(7)[off:off + 4].view(np.int32)[0])


def rot_scale_trans(ang=0.4, s=(1.1, 0.8, 1.3), t=(0.05, -0.02, 0.1)):
    c, sn = np.cos(ang), np.sin(ang)
    R = np.array([[c, 0, sn, 0], [0, 1, 0, 0], [-sn, 0, c, 0], [0, 0, 0, 1]])
    M = np.array([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1.0]]) @ R @ np.diag([s[0], s[1], s[2], 1.0])
    return M.astype(np.float32)


def test_param_offsets_used_here(kz, tmp_path):
    src = tmp_path / "off.cpp"
    src.write_text('#include "kz_internal.h"\n#include <cstddef>\n#include <cstdio>\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(KzParams, shadowFast), '
                   'offsetof(KzParams, nIlTris), offsetof(KzParams, ilLo), offsetof(KzParams, ilHi), offsetof(KzParams, anyInvisibleLight), offsetof(KzParams, bsdfExt));}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "nano-kazen_amd", "csrc"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [P_SHADOWFAST, P_NIL, P_ILLO, P_ILHI, P_ANYINV, P_BSDFEXT]


def test_edit_header_declares_five_calls_and_the_structs_have_gccs_sizes(kz, tmp_path):
    a = kz.abi
    lib = a.load_library()
    text = open(os.path.join(ROOT, "include", "kazen_mi355x_edit.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?(kz_[a-z0-9_]+)\s*\(", text, re.M))
    assert declared == set(a.EDIT_EXPORTS) and len(a.EDIT_EXPORTS) == 5
    assert {"kz_scene_set_bsdfs", "kz_scene_set_lights", "kz_scene_set_transforms"} <= declared
    exported = set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", a.LIB_PATH], text=True)))
    assert declared <= exported
    if os.path.exists(a.DEV_LIB_PATH):                          # the development variant exports the same calls
        dev = set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", a.DEV_LIB_PATH], text=True)))
        assert declared <= dev
    for sym in declared:
        assert getattr(lib, sym) is not None
    src = tmp_path / "sz.c"
    src.write_text('#include "kazen_mi355x_edit.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu\\n", sizeof(KzBsdfUpdate), sizeof(KzLightUpdate), sizeof(KzTransformUpdate));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(a.KzBsdfUpdate), C.sizeof(a.KzLightUpdate), C.sizeof(a.KzTransformUpdate)] == [132, 24, 68]
    assert a.KZ_TABLE_BSDFS == 8 and a.KZ_TABLE_PARAMS == 7


def _row(a, cdesc, i, **kw):
    b = a.KzBSDF.from_buffer_copy(bytes(cdesc.bsdfs[i]))
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _call(fn, sc, typ, rows):
    arr = (typ * max(1, len(rows)))(*rows)
    return fn(sc.h, arr, len(rows))


def _refused(sc, fn, typ, rows, code, name, before, info):
    lib = sc.lib
    assert _call(fn, sc, typ, rows) == code, (name, lib.kz_last_error())
    msg = lib.kz_last_error().decode()
    assert len(msg) >= 25 and fn.__name__ in msg, (name, msg)
    assert differing_tables(before, tables(sc)) == [] and bvh(sc) == info, name
    return msg


def test_every_refusal_has_a_code_a_message_and_changes_nothing(kz):
    a, S = kz.abi, kz.scenes
    # ---- bsdfs: a textured scene (textures 1.., a normalmap row) under path_mis
    d = S.textured_scene(32, 20, 4)
    sc = kz.Scene(d)
    lib = sc.lib
    cd = d.to_c()
    nrows, ntex = cd.nBsdfs, cd.nTextures
    assert ntex >= 1
    types = [cd.bsdfs[i].type for i in range(nrows)]
    nm = types.index(a.KZ_BSDF_NORMALMAP)
    plain = next(i for i, t in enumerate(types) if t != a.KZ_BSDF_NORMALMAP)
    before, info = tables(sc), bvh(sc)
    U = a.KzBsdfUpdate
    mirror = a.KzBSDF()
    mirror.type = a.KZ_BSDF_MIRROR
    mirror_tex = a.KzBSDF.from_buffer_copy(bytes(mirror))
    mirror_tex.albedoTex = 1
    cases = {
        "row out of range": ([U(nrows, mirror)], a.KZ_ERR_INVALID_ARG, str(nrows)),
        "row twice": ([U(plain, mirror), U(plain, mirror)], a.KZ_ERR_INVALID_ARG, str(plain)),
        "type 99": ([U(plain, _row(a, cd, plain, type=99))], a.KZ_ERR_UNSUPPORTED, str(plain)),
        "texture id beyond nTextures": ([U(plain, _row(a, cd, plain, type=a.KZ_BSDF_DIFFUSE, albedoTex=ntex + 1, roughnessTex=0, metallicTex=0))], a.KZ_ERR_INVALID_ARG, str(plain)),
        "albedoTex on a mirror": ([U(plain, mirror_tex)], a.KZ_ERR_INVALID_ARG, str(plain)),
        "normalmap without normalTex": ([U(nm, _row(a, cd, nm, normalTex=0))], a.KZ_ERR_INVALID_ARG, str(nm)),
        "normalmap nested in a normalmap": ([U(nm, _row(a, cd, nm, nested=nm))], a.KZ_ERR_INVALID_ARG, str(nm)),
        "alphaResolved 2": ([U(plain, _row(a, cd, plain, alphaResolved=2))], a.KZ_ERR_INVALID_ARG, str(plain)),
        "good then bad": ([U(plain, mirror), U(nm, _row(a, cd, nm, normalTex=0))], a.KZ_ERR_INVALID_ARG, str(nm)),
    }
    for name, (rows, code, index) in cases.items():
        msg = _refused(sc, lib.kz_scene_set_bsdfs, U, rows, code, name, before, info)
        assert index in msg, (name, msg)
    # a normalmap row under path_mats (LAB_NOTES H16)
    dm = S.textured_scene(32, 20, 4)
    for m in dm.meshes:
        if m["bsdf"] is not None and m["bsdf"]["type"] == "normalmap":
            m["bsdf"] = m["bsdf"]["nested"]
    dm.integrator["type"] = "path_mats"
    scm = kz.Scene(dm)
    cdm = dm.to_c()
    assert cdm.nTextures >= 1
    nmrow = a.KzBSDF()
    nmrow.type, nmrow.normalTex, nmrow.nested = a.KZ_BSDF_NORMALMAP, 1, 1
    _refused(scm, lib.kz_scene_set_bsdfs, U, [U(0, nmrow)], a.KZ_ERR_UNSUPPORTED, "normalmap under path_mats", tables(scm), bvh(scm))
    # the Python wrapper refuses what needs a new scene
    with pytest.raises(ValueError):
        sc.set_bsdfs({0: S.diffuse(S.constanttexture((0.1, 0.2, 0.3)))})          # a texture the scene does not have
    assert differing_tables(before, tables(sc)) == []

    # ---- lights and transforms: cornell (mesh 7 is its light)
    d = S.cornell_box(32, 32, 4)
    sc = kz.Scene(d)
    before, info = tables(sc), bvh(sc)
    L, T = a.KzLightUpdate, a.KzTransformUpdate
    kl = a.KzLight((1.0, 1.0, 1.0), 2.0, 1)
    for name, rows, index in (("light out of range", [L(1, kl)], "1"), ("light twice", [L(0, kl), L(0, kl)], "0")):
        assert index in _refused(sc, lib.kz_scene_set_lights, L, rows, a.KZ_ERR_INVALID_ARG, name, before, info)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    nan = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    nan[6] = float("nan")
    w0 = (C.c_float * 16)(*np.diag([1, 1, 1, 0]).astype(np.float32).reshape(-1))
    assert d.meshes[7]["light"] is not None and d.meshes[5]["light"] is None
    for name, rows, index in (("mesh out of range", [T(len(d.meshes), eye)], str(len(d.meshes))), ("mesh twice", [T(5, eye), T(5, eye)], "5"),
                              ("a NaN entry", [T(5, nan)], "5"), ("w = 0 on a light mesh", [T(7, w0)], "7"),
                              ("w = 0 on another mesh of a scene no replica holds", [T(6, eye), T(5, w0)], "5")):
        assert index in _refused(sc, lib.kz_scene_set_transforms, T, rows, a.KZ_ERR_INVALID_ARG, name, before, info)
    with pytest.raises(ValueError):
        sc.set_lights({5: S.area()})                                               # which meshes emit does not change


def q1(kz):
    return kz.scenes.load_npz(os.path.join(GOLDEN, "q1_default_m0_r0.5.npz"), {"camera": {"width": 48, "height": 27}, "sampler": {"sampleCount": 4}})


def test_q1_all_22_parameter_sets_on_one_scene(kz):
    """The reference's material study: one scene, set_bsdfs on mesh 4 for each of its 22 parameter sets; table 8 = the fresh scene's, tables 0..7 unchanged
    (= the fresh scene's: checked here too, so that "unchanged" and "equal to fresh" are both asserted). The last step restores the default set's bits."""
    params = json.load(open(os.path.join(GOLDEN, "q1_params.json")))["params"]
    assert len(params) == 22
    sc = kz.Scene(q1(kz))
    start = tables(sc)
    default = dict(sc.desc.meshes[4]["bsdf"])
    seen = set()
    for name, p in params.items():
        b = {k: v for k, v in p.items() if not k.startswith("_")}
        sc.set_bsdfs({4: b})
        d = q1(kz)
        d.meshes[4]["bsdf"] = b
        fresh = tables(kz.Scene(d))
        now = tables(sc)
        assert differing_tables(fresh, now) == [], name
        assert differing_tables(start, now) in ([], [8]), name
        seen.add(now[8].tobytes())
    assert len(seen) >= 20                                      # (the study's sets differ from one another)
    sc.set_bsdfs({4: default})
    assert differing_tables(start, tables(sc)) == []


def test_bsdf_ext_transitions_and_row_swaps(kz):
    S = kz.scenes
    # lean -> models -> lean
    sc = kz.Scene(S.cornell_box(32, 32, 4))
    start = tables(sc)
    ext0 = prm_i32(sc, P_BSDFEXT)
    wall = next(m for m, x in enumerate(sc.desc.meshes) if x["bsdf"] is not None and x["bsdf"]["type"] == "diffuse")
    old = sc.desc.meshes[wall]["bsdf"]
    sc.set_bsdfs({wall: S.mirror()})
    assert prm_i32(sc, P_BSDFEXT) == ext0 | 1 and ext0 & 1 == 0
    assert differing_tables(tables(kz.Scene(sc.desc)), tables(sc)) == []
    sc.set_bsdfs({wall: old})
    assert prm_i32(sc, P_BSDFEXT) == ext0 and differing_tables(start, tables(sc)) == []
    # rough models are resolved as at creation (alpha = max(0.001, x^2))
    sc.set_bsdfs({wall: S.roughconductor(0.3, "Cu")})
    assert differing_tables(tables(kz.Scene(sc.desc)), tables(sc)) == []
    # rows swapped among a scene's existing textures / models
    for make in (lambda: S.textured_scene(32, 20, 4), lambda: S.materials_scene(32, 24, 4)):
        sc = kz.Scene(make())
        have = [m for m, x in enumerate(sc.desc.meshes) if x["bsdf"] is not None and x["bsdf"]["type"] != "normalmap"]
        rolled = {m: sc.desc.meshes[have[(i + 1) % len(have)]]["bsdf"] for i, m in enumerate(have)}
        t0 = tables(sc)
        sc.set_bsdfs(rolled)
        now = tables(sc)
        assert differing_tables(tables(kz.Scene(sc.desc)), now) == []
        assert 8 in differing_tables(t0, now) and [t for t in differing_tables(t0, now) if t < 7] == []


def _big_light_scene(kz):
    d = kz.scenes.cornell_box(32, 32, 4)
    g = np.linspace(-0.3, 0.3, 8, dtype=np.float32)
    xx, zz = np.meshgrid(g, g, indexing="ij")
    V = np.stack([xx.ravel(), np.full(64, 0.5, np.float32), zz.ravel()], 1)
    F = []
    for i in range(7):
        for j in range(7):
            q = i * 8 + j
            F += [[q, q + 1, q + 9], [q, q + 9, q + 8]]
    d.add_mesh(V, np.array(F, np.uint32), bsdf=kz.scenes.diffuse(), light=kz.scenes.area((1, 1, 1), 3.0, True))
    return d


@pytest.mark.parametrize("name", ["cornell", "soup", "q1", "big"])
def test_lights_scale_and_visibility_toggles_equal_fresh_scenes(kz, name):
    S = kz.scenes
    d = {"cornell": lambda: S.cornell_box(32, 32, 4), "soup": lambda: S.random_triangles(20000, 64, 48, 4, sampler="independent"), "q1": lambda: q1(kz),
         "big": lambda: _big_light_scene(kz)}[name]()
    sc = kz.Scene(d)
    start = tables(sc)
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    assert len(lights) == {"cornell": 1, "soup": 8, "q1": 3, "big": 2}[name]

    def step(upd, what):
        sc.set_lights(upd)
        now, fresh = tables(sc), tables(kz.Scene(sc.desc))
        assert differing_tables(fresh, now) == [], (what, differing_tables(fresh, now))
        assert [t for t in differing_tables(start, now) if t not in (5, 6, 7)] == [], what
        return now

    original = {m: dict(d.meshes[m]["light"]) for m in lights}
    step({m: dict(l, intensity=l["intensity"] * 1.75, color=(0.9, 0.5, 0.25)) for m, l in original.items()}, "scaled")
    step({lights[0]: dict(original[lights[0]], lightPrimaryVisibility=not original[lights[0]]["lightPrimaryVisibility"])}, "one toggled")
    step({m: dict(l, lightPrimaryVisibility=True) for m, l in original.items()}, "all visible")
    assert prm_i32(sc, P_NIL) == 0 and prm_i32(sc, P_ANYINV) == 0 and sc.table(6).size == 0
    step({m: dict(l, lightPrimaryVisibility=False) for m, l in original.items()}, "all invisible")
    assert prm_i32(sc, P_ANYINV) == 1
    if name == "big":                                           # an emissive mesh of 98 triangles: no list, the literal closest-hit shadow test
        assert prm_i32(sc, P_SHADOWFAST) == 0 and prm_i32(sc, P_NIL) == 0 and sc.table(6).size == 0
    else:
        assert prm_i32(sc, P_SHADOWFAST) == 1 and prm_i32(sc, P_NIL) == sum(d.meshes[m]["F"].shape[0] for m in lights)
    assert differing_tables(start, step(original, "back")) == []


def _with_bare_triangle(kz):
    d = kz.scenes.cornell_box(32, 32, 4)
    d.add_mesh(np.array([[-0.2, -0.3, 0.1], [0.2, -0.3, 0.1], [0.0, 0.1, 0.2]], np.float32), np.array([[0, 1, 2]], np.uint32), bsdf=kz.scenes.diffuse((0.2, 0.6, 0.3)))
    return d


def _arrays(kz, desc, m, M):
    V, N = kz.scenes.transform_vertices(M, desc.meshes[m]["V"], desc.meshes[m]["N"])
    return V if N is None else (V, N)


def _equal_to_fresh(kz, sc):
    """What tests/test_scene_edit_cpu.py claims of an edited scene against a fresh one of its arrays: shading records, CDFs, light rows, the invisible-light
    triangles and their box (the trees differ: a refit keeps the build's topology)."""
    fresh = kz.Scene(sc.desc)
    assert all(np.array_equal(fresh.table(t), sc.table(t)) for t in (3, 4, 5, 6, 8))
    pf, ps = fresh.table(7), sc.table(7)
    assert np.array_equal(pf[P_SHADOWFAST:P_ANYINV + 4], ps[P_SHADOWFAST:P_ANYINV + 4])


def test_transforms_equal_set_vertices_of_the_numpy_arithmetic(kz):
    make = lambda: _with_bare_triangle(kz)
    d0 = make()
    bare = len(d0.meshes) - 1
    assert d0.meshes[5]["N"] is not None and d0.meshes[bare]["N"] is None and d0.meshes[7]["light"] is not None
    proj = np.eye(4, dtype=np.float32)
    proj[3] = (0.02, 0.1, -0.03, 1.2)
    proj[0, 3] = 0.1
    singular = np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32)
    singular[1, 3] = -0.4
    batches = [{5: rot_scale_trans(), 6: rot_scale_trans(-0.7, (0.9, 1.2, 0.7), (-0.1, 0.0, 0.05))},          # rotation + non-uniform scale + translation
               {5: proj},                                                                                      # projective (w != 1); does not compose with the batch before
               {6: singular},                                                                                  # singular 3x3 on a mesh with normals: the normals stay
               {7: rot_scale_trans(0.2, (0.8, 1.0, 1.1), (0.05, -0.01, 0.0)), bare: rot_scale_trans(1.0, (2.0, 0.5, 1.0), (0, 0.2, 0))},   # the light, a mesh without normals
               {7: rot_scale_trans(0.3), 5: np.eye(4, dtype=np.float32)}]
    sc = kz.Scene(make())
    for i, batch in enumerate(batches):
        sc.set_transforms(batch)
        twin = kz.Scene(make())                                 # every step from the build: a transform applies to the BASE data, whatever came before
        state = {}
        for b in batches[:i + 1]:
            state.update(b)
        twin.set_vertices({m: _arrays(kz, d0, m, M) for m, M in state.items()})
        assert differing_tables(tables(twin, range(8)), tables(sc, range(8))) == [], i
        assert bvh(twin) == bvh(sc), i
        for m, M in state.items():
            want = _arrays(kz, d0, m, M)
            want = want if isinstance(want, tuple) else (want, None)
            assert np.array_equal(sc.desc.meshes[m]["V"], want[0]) and (want[1] is None or np.array_equal(sc.desc.meshes[m]["N"], want[1]))
        _equal_to_fresh(kz, sc)
    # the same batch again: idempotent
    t = tables(sc)
    sc.set_transforms(batches[-1])
    assert differing_tables(t, tables(sc)) == []
    # the singular matrix left the normals as they were (normalised); the projective one moved w
    V, N = kz.scenes.transform_vertices(singular, d0.meshes[6]["V"], d0.meshes[6]["N"])
    n0 = d0.meshes[6]["N"]
    assert np.allclose(N, n0 / np.linalg.norm(n0, axis=1, keepdims=True), atol=1e-6) and (V[:, 1] == np.float32(-0.4)).all()


def test_transform_then_set_vertices_then_transform(kz):
    """kz_scene_set_vertices replaces the base data and drops the transform: the next transform applies to the NEW arrays."""
    d0 = kz.scenes.cornell_box(32, 32, 4)
    A, B = rot_scale_trans(0.5), rot_scale_trans(-0.3, (1.0, 1.1, 0.9), (0.0, 0.05, 0.0))
    sc, twin = kz.Scene(kz.scenes.cornell_box(32, 32, 4)), kz.Scene(kz.scenes.cornell_box(32, 32, 4))
    sc.set_transforms({5: A, 7: A})
    newV = {m: (d0.meshes[m]["V"] + np.float32(0.03), d0.meshes[m]["N"]) for m in (5, 7)}
    sc.set_vertices(newV)
    twin.set_vertices(newV)
    assert differing_tables(tables(twin), tables(sc)) == []
    sc.set_transforms({5: B, 7: B})
    twin.set_vertices({m: kz.scenes.transform_vertices(B, *newV[m]) for m in (5, 7)})
    assert differing_tables(tables(twin), tables(sc)) == []
    assert np.array_equal(sc.desc.meshes[5]["V"], kz.scenes.transform_vertices(B, *newV[5])[0])


def test_mini_xml_identity_load_plus_transform_equals_the_loaders_transform(kz):
    """tests/golden/xml/mini.xml places cube.obj by scale + rotate + translate at load. Loading the cube with the identity and then set_transforms(toWorld)
    gives the loader's arrays to the bit (cube.obj holds no negative zero, and its normals are unit axes, which the identity load leaves as they are) - and so
    every table a twin scene gets from set_vertices of the loader's arrays."""
    X = kz.xmlscene
    path = os.path.join(GOLDEN, "xml", "mini.xml")
    loaded = X.load_xml(path)
    node = [n for n in ET.parse(path).getroot() if n.tag == "mesh"][1]
    M = X._transform(next(c for c in node if c.tag == "transform"))
    assert not np.array_equal(M, np.eye(4, dtype=np.float32))
    V, F, N, UV = X.load_obj(os.path.join(GOLDEN, "xml", "cube.obj"), None)
    assert not np.signbit(V[V == 0]).any()
    ident = X.load_xml(path)
    ident.meshes[1] = dict(ident.meshes[1], V=V, N=N)
    sc = kz.Scene(ident)
    sc.set_transforms({1: M})
    assert np.array_equal(sc.desc.meshes[1]["V"], loaded.meshes[1]["V"]) and np.array_equal(sc.desc.meshes[1]["N"], loaded.meshes[1]["N"])
    twin = kz.Scene(ident_copy(X, path, V, N))
    twin.set_vertices({1: (loaded.meshes[1]["V"], loaded.meshes[1]["N"])})
    assert differing_tables(tables(twin), tables(sc)) == []
    fresh = kz.Scene(loaded)
    assert all(np.array_equal(fresh.table(t), sc.table(t)) for t in (3, 4, 5, 6, 8))


def ident_copy(X, path, V, N):
    d = X.load_xml(path)
    d.meshes[1] = dict(d.meshes[1], V=V, N=N)
    return d


def test_lazy_host_sync_equals_syncing_after_every_edit(kz):
    """A scene no replica holds, edited five times: querying once at the end gives the tables that querying after each edit gives."""
    S = kz.scenes
    lazy, eager = kz.Scene(S.cornell_box(32, 32, 4)), kz.Scene(S.cornell_box(32, 32, 4))
    d0 = S.cornell_box(32, 32, 4)
    edits = [lambda s: s.set_transforms({5: rot_scale_trans(0.3), 6: rot_scale_trans(-0.2)}),
             lambda s: s.set_bsdfs({5: S.mirror()}),
             lambda s: s.set_vertices({6: (d0.meshes[6]["V"] * np.float32(0.9), d0.meshes[6]["N"])}),
             lambda s: s.set_lights({7: S.area((1.0, 0.8, 0.6), 9.0, True)}),
             lambda s: s.set_transforms({6: rot_scale_trans(0.6), 7: rot_scale_trans(0.1, (0.9, 1, 0.9), (0, -0.01, 0))})]
    for e in edits:
        e(lazy)
        e(eager)
        tables(eager)
        eager.bvh_info()
    assert differing_tables(tables(eager), tables(lazy)) == [] and bvh(eager) == bvh(lazy)
