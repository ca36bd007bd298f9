import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def kz():
    return importlib.import_module("nano-kazen_amd")


@pytest.fixture(scope="session")
def O():
    """The CPU oracle (test infrastructure). Builds oracle/liboracle.so on first use."""
    import oracle
    oracle.lib()
    return oracle


@pytest.fixture(scope="session")
def gpu_lib(kz):
    """The product library on a GPU box; fails loudly (no silent skip) if the HIP extension is missing."""
    lib = kz.abi.load_library()
    assert lib.kz_device_count() >= 1, "no HIP device visible: -m gpu tests must run on the GPU box"
    return lib


def _write_scene_file(xml_path, d, mesh_names):
    """SceneDescription -> nano-kazen XML + one Wavefront OBJ per mesh under meshes/ (the loader's input formats, xmlscene.py): every vertex of a mesh is its own
    (p, uv, n) triple, written with 9 significant digits (float32 round-trips), and the camera's toWorld as a matrix. Colours and the matrix are comma-separated
    and an integrator on the loader's defaults is a self-closing element, as in the reference's scene files."""
    base = os.path.dirname(xml_path)
    os.makedirs(os.path.join(base, "meshes"), exist_ok=True)
    num = lambda v: repr(float(v))
    vec = lambda v: ", ".join(num(x) for x in v)
    prop = lambda tag, name, v: '<%s name="%s" value="%s"/>' % (tag, name, v)
    it, sa, cam = d.integrator, d.sampler, d.camera
    out = ['<?xml version="1.0" ?>', "<scene>"]
    if (it["maxDepth"], it["traceBias"], it["regularization"], it["accumulatedRoughness"]) == (5, 0.001, False, 0.5):
        out.append('<integrator type="%s"/>' % it["type"])
    else:
        out += ['<integrator type="%s">' % it["type"], prop("integer", "maxDepth", it["maxDepth"]), prop("float", "traceBias", num(it["traceBias"])),
                prop("boolean", "regularization", str(bool(it["regularization"])).lower()), prop("float", "accumulatedRoughness", num(it["accumulatedRoughness"])), "</integrator>"]
    out += ['<sampler type="%s">' % sa["type"], prop("integer", "sampleCount", sa["sampleCount"]), prop("integer", "seed", sa["seed"]), prop("integer", "resolution", sa["resolution"]),
           "</sampler>", '<camera type="%s">' % cam["type"], prop("float", "fov", num(cam["fov"])), prop("float", "nearClip", num(cam["nearClip"])),
           prop("float", "farClip", num(cam["farClip"])), prop("integer", "width", cam["width"]), prop("integer", "height", cam["height"]),
           '<transform name="toWorld"><matrix value="%s"/></transform>' % vec(np.asarray(cam["toWorld"]).reshape(-1))]
    rf = cam.get("rfilter")
    if rf:
        out += ['<rfilter type="%s">' % rf["type"]] + [prop("float", k, num(rf[k])) for k in ("radius", "stddev", "B", "C")] + ["</rfilter>"]
    out.append("</camera>")
    if d.background:
        out += ['<texture type="background" id="background">', prop("float", "intensity", num(d.background["intensity"])),
                '<texture type="constanttexture">%s</texture>' % prop("color", "color", vec(d.background["color"])), "</texture>"]
    for m, name in zip(d.meshes, mesh_names):
        V, F, N, UV = m["V"], m["F"], m["N"], m["UV"]
        lines = ["v %.9g %.9g %.9g" % tuple(p) for p in V]
        lines += ["vt %.9g %.9g" % tuple(t) for t in UV] if UV is not None else []
        lines += ["vn %.9g %.9g %.9g" % tuple(n) for n in N] if N is not None else []
        corner = "%d/%d/%d" if UV is not None and N is not None else "%d//%d" if N is not None else "%d/%d" if UV is not None else "%d"
        k = corner.count("%d")
        lines += ["f " + " ".join(corner % ((i + 1,) * k) for i in f) for f in F]
        with open(os.path.join(base, "meshes", name + ".obj"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        out += ['<mesh type="obj">', prop("string", "filename", "meshes/%s.obj" % name)]
        b = m["bsdf"]
        if b and b["type"] == "diffuse":
            out += ['<bsdf type="diffuse">', prop("color", "albedo", vec(b["albedo"])), "</bsdf>"]
        elif b and b["type"] == "kazenstandard":
            out += ['<bsdf type="kazenstandard">'] + ['<texture type="constanttexture" id="%s">%s</texture>' % (t, prop("color", "color", vec(c))) for t, c in
                                                      (("baseColor", b["baseColor"]), ("roughness", (b["roughness"], 0, 0)), ("metallic", (b["metallic"], 0, 0)))]
            out += [prop("float", k, num(b[k])) for k in ("anisotropy", "specular", "specularTint", "clearcoat", "clearcoatRoughness", "sheen", "sheenTint")] + ["</bsdf>"]
        elif b:
            raise ValueError("no writer for bsdf %s" % b["type"])
        if m["light"]:
            lt = m["light"]
            out += ['<light type="area">', prop("color", "color", vec(lt["color"])), prop("float", "intensity", num(lt["intensity"])),
                    prop("boolean", "lightPrimaryVisibility", str(bool(lt["lightPrimaryVisibility"])).lower()), "</light>"]
        out.append("</mesh>")
    with open(xml_path, "w") as fh:
        fh.write("\n".join(out + ["</scene>"]) + "\n")


@pytest.fixture(scope="session")
def q1_scene_dir(tmp_path_factory, kz):
    """Files EQUIVALENT to the reference's scene/2022_q1 tree, in _write_scene_file's form, written from the committed fixtures (tests/golden/make_q1_scene.py,
    make_q1_files.py: what xmlscene.load_xml made of the reference's files): parameters/<name>.xml for the 22 parameter sets of q1_params.json on the
    geometry, lights and camera of q1_default_m0_r0.5.npz, and WarmStudio/WarmStudio.xml from q1_warmstudio.npz (its mesh files' names keep their spaces).
    They load to the same scenes (the normals to within an ulp: the loader normalises them again), but they are not the reference's text: every sampler and
    camera property is spelled out, an OBJ has one vertex per (p, uv, n) triple (no position shared between corners with other normals) and there are no
    comments. Comments, lookat and OBJ faces that share positions are exercised by the hand-written files under tests/golden/xml."""
    import json
    golden = os.path.join(ROOT, "tests", "golden")
    root = str(tmp_path_factory.mktemp("2022_q1"))
    params = json.load(open(os.path.join(golden, "q1_params.json")))["params"]
    for name, p in params.items():
        d = kz.scenes.load_npz(os.path.join(golden, "q1_default_m0_r0.5.npz"))
        d.meshes[4]["bsdf"] = {k: v for k, v in p.items() if not k.startswith("_")}
        d.sampler["sampleCount"] = p["_sampleCount"]
        _write_scene_file(os.path.join(root, "parameters", name + ".xml"), d, ["Light_back", "Light_right", "Light_left", "Backdrop", "PlaceHolder_Object"])
    d = kz.scenes.load_npz(os.path.join(golden, "q1_warmstudio.npz"))
    _write_scene_file(os.path.join(root, "WarmStudio", "WarmStudio.xml"), d, ["REPLACE ME", "Backdrop", "Light Array"])
    return root


def wait_for_wipe(lib, limit_s=30.0):
    """Memory a process releases is wiped by the driver (~33 GB/s) before it is reported free again, and whoever allocates before the wipe is through waits for it
    (profiles/r05a_alloc). A test whose point is the TIMING of a growing context waits here until the free memory has stopped rising."""
    import ctypes as C
    import time
    f, t = C.c_uint64(), C.c_uint64()
    last, still, t0 = -1, 0, time.perf_counter()
    while time.perf_counter() - t0 < limit_s:
        assert lib.kz_device_mem_info(0, C.byref(f), C.byref(t)) == 0
        still = still + 1 if f.value <= last + (64 << 20) else 0
        last = max(last, f.value)
        if still >= 4:
            break
        time.sleep(0.1)
    return last


@pytest.fixture(scope="session")
def dev_lib(kz, gpu_lib):
    """The development variant of the library (-DKZ_EXPERIMENTS: same sources + the hooks that are process-global state - failure injection, growth delay,
    trace, device aliasing - and the kernels of rejected experiments). A second copy of the library in this process: its replicas, pools and device state are its
    own. The product library is asked to give its pooled path state back first (the two copies share one card)."""
    if not os.path.exists(kz.abi.DEV_LIB_PATH):
        pytest.fail("development variant not built: python -c 'import __graft_entry__ as g; g.build()'")
    gpu_lib.kz_device_trim(0)
    wait_for_wipe(gpu_lib)
    lib = kz.abi.load_dev_library()
    assert lib.kz_build_flags() & 1 and lib.kz_device_count() >= 1
    return lib
