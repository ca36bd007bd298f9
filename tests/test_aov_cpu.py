"""Feature films (include/kazen_mi355x_aov.h) without a GPU: the header against the library's exports, the refusals that need no device, sanity checks of the
test-only CPU reference (tests/cpu_ref/kz_aov_ref.cpp) the GPU tests compare against, the layered EXR writer, and the precondition of the cross-check scene."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_SRC = os.path.join(HERE, "cpu_ref", "kz_aov_ref.cpp")
AOVS = ("albedo", "normal", "depth")
W, H, SPP = 96, 72, 8          # wider and taller than one 64-px resolve cell and than two 32-px reference blocks; 55 296 items

# ---------------------------------------------------------------- the CPU reference (also imported by test_aov_gpu.py)
_ref = {}


def aov_ref_lib(tmpdir):
    """Compiles the CPU reference with the oracle's flags into `tmpdir` once per process."""
    if "lib" not in _ref:
        out = os.path.join(str(tmpdir), "libkz_aov_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                               "-o", out, REF_SRC])
        L = C.CDLL(out)
        import oracle
        abi = oracle.abi
        L.kzo_last_error.restype = C.c_char_p
        L.kzo_scene_create.argtypes = [C.POINTER(abi.KzSceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.kzo_scene_destroy.argtypes = [C.c_void_p]
        L.kzo_scene_destroy.restype = None
        L.kzo_film_dims.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 3
        L.kza_samples.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_int32), abi.u32p, abi.f32p]
        L.kza_samples.restype = None
        L.kza_render_canonical.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, abi.f32p]
        _ref["lib"] = L
    return _ref["lib"]


class AovRef:
    """A scene of the CPU reference: created through the oracle's kzo_scene_create with the path_mis tag; the integrator named in the description (or here)
    decides whether a first hit on an invisible light is walked through."""

    def __init__(self, L, desc, integrator=None):
        import oracle
        self.L, self.abi = L, oracle.abi
        self.integ = desc.integrator["type"] if integrator is None else integrator
        d = copy.copy(desc)
        d.integrator = dict(desc.integrator, type="path_mis")
        self._c = d.to_c()
        h = C.c_void_p()
        rc = L.kzo_scene_create(C.byref(self._c), 0, C.byref(h))
        if rc != 0:
            raise self.abi.KzError(rc, L.kzo_last_error().decode())
        self.h = h
        w, hh, b = C.c_int(), C.c_int(), C.c_int()
        L.kzo_film_dims(self.h, C.byref(w), C.byref(hh), C.byref(b))
        self.width, self.height, self.border = w.value, hh.value, b.value
        self.tag = {"path_mis": 0, "normals": 1, "ao": 2, "path_mats": 3}[self.integ]

    def __del__(self):
        if getattr(self, "h", None):
            self.L.kzo_scene_destroy(self.h)

    def samples(self, pxy, idx):
        pxy = np.ascontiguousarray(pxy, np.int32)
        idx = np.ascontiguousarray(idx, np.uint32)
        out = np.zeros((idx.shape[0], 10), np.float32)
        self.L.kza_samples(self.h, self.tag, idx.shape[0], pxy.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(self.abi.u32p), out.ctypes.data_as(self.abi.f32p))
        return out

    def film(self, aov, s0=0, s1=0, threads=16, grid=64):
        film = np.zeros((self.height + 2 * self.border, self.width + 2 * self.border, 4), np.float32)
        bit = {"albedo": 1, "normal": 2, "depth": 4}[aov]
        assert self.L.kza_render_canonical(self.h, self.tag, bit, s0, s1, threads, grid, film.ctypes.data_as(self.abi.f32p)) == 0
        return film


def with_integrator(desc, name):
    d = copy.copy(desc)
    d.integrator = dict(desc.integrator, type=name)
    return d


def grid_of(desc, S=None):
    """Every (pixel, sample) of the frame."""
    w, h = desc.camera["width"], desc.camera["height"]
    S = S or desc.sampler["sampleCount"]
    yy, xx, ii = np.meshgrid(np.arange(h), np.arange(w), np.arange(S), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)


def octant_scene(kz, width=W, height=H, spp=SPP, n_tris=200, seed=5):
    """The cross-check scene: `n_tris` triangles WITHOUT vertex normals, each built in a plane whose unit normal has all components >= 0.2 and wound so that
    cross(e1, e2) points along it; the camera looks down (-1, -1, -1), so it sees their front sides. The shading normal of such a triangle is its geometric one
    (accel.cpp:231-233) with no negative component, so |n_geo| - what `normals` renders - and the signed NORMAL feature are the same numbers."""
    S = kz.scenes
    rng = np.random.default_rng(seed)
    s = S.SceneDescription()
    V, F = [], []
    for k in range(n_tris):
        n = rng.uniform(0.2, 1.0, 3)
        n /= np.linalg.norm(n)
        while n.min() < 0.25:                                         # (margin: the float32 normal the renderers form stays >= 0.2)
            n = rng.uniform(0.2, 1.0, 3)
            n /= np.linalg.norm(n)
        a = np.cross(n, [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(n, a)                                            # (a, b, n) right-handed: cross(a, b) = n
        c = rng.uniform(-1.0, 1.0, 3)
        r = rng.uniform(0.25, 0.6)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        V += [c + r * (np.cos(t) * a + np.sin(t) * b) for t in ang]   # counter-clockwise about n
        F.append([3 * k, 3 * k + 1, 3 * k + 2])
    s.add_mesh(np.array(V, np.float32), np.array(F, np.uint32), bsdf=S.diffuse((0.6, 0.5, 0.4)))
    q = S.quad((-0.5, 3.0, -0.5), (-0.5, 3.0, 0.5), (0.5, 3.0, 0.5), (0.5, 3.0, -0.5), flip=True)
    s.add_mesh(q[0], q[3], N=None, UV=None, bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 1, 1), 10.0, True))      # (behind the camera's view: n = -y)
    s.camera.update(width=width, height=height, fov=45.0, nearClip=0.1, farClip=100.0, toWorld=S.look_at((3.2, 3.2, 3.2), (0, 0, 0), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": spp, "seed": 3}
    s.integrator["maxDepth"] = 3
    return s


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return aov_ref_lib(tmp_path_factory.mktemp("kza"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    lib = a.load_library()
    src = open(os.path.join(ROOT, "include", "kazen_mi355x_aov.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?(kz_[a-z0-9_]+)\s*\(", src, re.M))
    assert declared == set(a.AOV_EXPORTS) and len(a.AOV_EXPORTS) == 6, declared ^ set(a.AOV_EXPORTS)
    exported = set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", a.LIB_PATH], text=True)))
    assert declared <= exported, declared - exported
    if os.path.exists(a.DEV_LIB_PATH):
        dev = set(re.findall(r" T (kz_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", a.DEV_LIB_PATH], text=True)))
        assert declared <= dev, declared - dev
    # a surface of its own: nothing added to the pinned lists or to the two existing headers
    assert not (declared & (set(a.EXPORTS) | set(a.PRODUCT_EXPORTS) | set(a.EDIT_EXPORTS)))
    for name in ("kazen_mi355x.h", "kazen_mi355x_dev.h", "kazen_mi355x_edit.h"):
        assert "aov" not in open(os.path.join(ROOT, "include", name)).read().lower(), name
    assert lib.kz_abi_version() == a.KZ_ABI_VERSION == 6
    assert (a.KZ_AOV_ALBEDO, a.KZ_AOV_NORMAL, a.KZ_AOV_DEPTH, a.KZ_AOV_ALL) == tuple(int(re.search(r"#define %s\s+(\d+)u" % n, src).group(1)) for n in ("KZ_AOV_ALBEDO", "KZ_AOV_NORMAL", "KZ_AOV_DEPTH", "KZ_AOV_ALL"))


def _refused(kz, fn, code, *words):
    with pytest.raises(kz.abi.KzError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_without_a_device(kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert sc.aovs() == []
    for bad in (8, 15, 1 << 31):
        _refused(kz, lambda: sc.set_aovs(bad), a.KZ_ERR_INVALID_ARG, "kz_scene_set_aovs")
    assert sc.aovs() == []
    sc.set_aovs(["albedo", "depth"])                                  # (a scene on no device: the mask alone)
    assert sc.aovs() == ["albedo", "depth"]
    with pytest.raises(ValueError):
        sc.set_aovs(["position"])
    # exactly one enabled bit
    for bad in (0, 2, 3, 5, 8):
        _refused(kz, lambda: sc.aov_film(bad), a.KZ_ERR_INVALID_ARG, "kz_aov_download")
    _refused(kz, lambda: sc.aov_film("albedo"), a.KZ_ERR_STATE)       # one enabled bit, but no device
    tiles = [(0, 0, 16, 16)]
    counter = np.zeros(2, np.uint32)
    _refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "pipeline = 1")
    _refused(kz, lambda: sc.render_multi([0]), a.KZ_ERR_UNSUPPORTED, "kz_render_multi")
    _refused(kz, lambda: sc.render_dealt(tiles, counter, device=0), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "KzTileDealer")
    _refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "packedOutput")
    _refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_UNSUPPORTED, "kz_film_download_tiles")
    # with the mask 0 the same calls get as far as they got before: the scene is on no device
    sc.set_aovs(())
    assert sc.aovs() == []
    _refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_STATE)
    _refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_STATE)
    _refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_STATE)


# ---------------------------------------------------------------- the reference itself
def test_reference_sanity(kz, ref):
    d = kz.scenes.cornell_box(32, 24, 4)
    d.camera["fov"] = 80.0                                            # (wide enough to look past the box: misses)
    pxy, idx = grid_of(d)
    s = AovRef(ref, d).samples(pxy, idx)
    hit = s[:, 9] == 1.0
    assert hit.any() and (~hit).any() and set(np.unique(s[:, 9])) == {0.0, 1.0}
    assert not s[~hit][:, 2:].any()                                   # a miss: every feature 0
    assert (s[hit][:, 8] > 0).all() and np.isfinite(s).all()
    assert np.array_equal(np.floor(s[:, :2]).astype(np.int32), pxy)
    # albedo of a constant row is its constant: the rows of the box
    consts = np.array([(0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.75, 0.75, 0.75), (0.9, 0.6, 0.2), (0, 0, 0)], np.float32)
    alb = s[hit][:, 2:5]
    assert (alb[:, None, :] == consts[None]).all(axis=2).any(axis=1).all()
    assert len(np.unique(alb, axis=0)) >= 4
    # unit normals to 4 ulp (of 1: 4 x 2^-23 on the squared length's square root)
    n = s[hit][:, 5:8].astype(np.float64)
    assert np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0).max() <= 4 * 2.0 ** -23
    assert (s[hit][:, 5:8] < 0).any()                                 # signed: the right wall and the ceiling face -x / -y
    # a single constant diffuse row in front of the whole frame
    one = kz.scenes.SceneDescription()
    q = kz.scenes.quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    one.add_mesh(q[0], q[3], N=q[1], UV=q[2], bsdf=kz.scenes.diffuse((0.25, 0.5, 0.125)))
    one.camera.update(width=8, height=8, fov=40.0, nearClip=0.1, farClip=100.0, toWorld=kz.scenes.look_at((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    one.sampler = {"type": "independent", "sampleCount": 2, "seed": 0}
    s1 = AovRef(ref, one).samples(*grid_of(one))
    assert (s1[:, 9] == 1).all() and (s1[:, 2:5] == np.array([0.25, 0.5, 0.125], np.float32)).all() and (s1[:, 5:8] == np.array([0, 0, 1], np.float32)).all()
    f = AovRef(ref, one).film("albedo")
    b = (f.shape[0] - 8) // 2
    inner = f[b:b + 8, b:b + 8]
    assert np.allclose(inner[:, :, :3] / inner[:, :, 3:], [0.25, 0.5, 0.125], rtol=1e-6)


def test_octant_scene_has_no_negative_normal_component(kz, ref):
    """The precondition of the GPU cross-check (NORMAL film of path_mis == picture of `normals`): over the whole grid, zero samples with a negative component."""
    d = octant_scene(kz)
    assert d.meshes[0]["F"].shape[0] == 200 and d.meshes[0]["N"] is None
    s = AovRef(ref, d).samples(*grid_of(d))
    hit = s[:, 9] == 1.0
    assert hit.sum() > len(hit) // 4 and (~hit).sum() > 0
    assert int((s[:, 5:8] < 0).sum()) == 0
    assert s[hit][:, 5:8].min() >= 0.2


def test_exr_layers_round_trip(kz, tmp_path):
    out = kz.output
    rng = np.random.default_rng(1)
    layers = {"": rng.random((9, 13, 3), dtype=np.float32), "albedo": rng.random((9, 13, 3), dtype=np.float32),
              "normal": rng.random((9, 13, 3), dtype=np.float32) * 2 - 1, "depth": np.repeat(rng.random((9, 13, 1), dtype=np.float32) * 50, 3, axis=2)}
    layers["normal"][0, 0] = (-0.0, np.float32(1e-42), -1.0)          # bit for bit: a negative zero and a subnormal survive
    p = out.save_exr_layers(str(tmp_path / "frame"), layers)
    assert p.endswith(".exr")
    raw = open(p, "rb").read()
    names = [n.decode() for n in re.findall(rb"((?:[a-z]+\.)?[RGBZ])\0\x02\0\0\0", raw)]
    assert names == ["B", "G", "R", "albedo.B", "albedo.G", "albedo.R", "depth.Z", "normal.B", "normal.G", "normal.R"] and names == sorted(names)
    back = out.load_exr_layers(p)
    assert sorted(back) == ["", "albedo", "depth", "normal"]
    for k in ("", "albedo", "normal"):
        assert back[k].tobytes() == layers[k].tobytes(), k
    assert back["depth"].tobytes() == np.ascontiguousarray(layers["depth"][:, :, 0]).tobytes()
    # the plain pair is untouched and reads the beauty layer of a one-layer file
    q = out.save_exr_layers(str(tmp_path / "rgb.exr"), {"": layers[""]})
    assert np.array_equal(out.load_exr(q), layers[""]) and open(q, "rb").read() == out.exr_bytes(layers[""])
