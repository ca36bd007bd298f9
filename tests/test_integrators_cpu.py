"""normals / ao / path_mats without a GPU: the C ABI accepts the three tags (and still refuses whitted), the Python and XML plumbing, the C++ mirror's
describe() rows, and sanity checks of the test-only CPU reference (tests/cpu_ref/kz_integrators_ref.cpp) the GPU tests compare against."""
import os
import subprocess

import numpy as np
import pytest

from cpu_refs import RefScene, lib
from film_cases import INTEGRATORS, with_integrator

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MINI = os.path.join(HERE, "golden", "xml", "mini.xml")
LIBDIR = os.path.join(ROOT, "nano-kazen_amd", "csrc")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("integrators", tmp_path_factory.mktemp("kzi"))


def _scene_grid(desc):
    """Every (pixel, sample) of the frame."""
    W, H, S = desc.camera["width"], desc.camera["height"], desc.sampler["sampleCount"]
    yy, xx, ii = np.meshgrid(np.arange(H), np.arange(W), np.arange(S), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)


# ---------------------------------------------------------------- ABI, plumbing
@pytest.mark.parametrize("name,tag", [("normals", 1), ("ao", 2), ("path_mats", 3)])
def test_scene_create_accepts_the_new_integrators(kz, name, tag):
    d = with_integrator(kz.scenes.cornell_box(16, 16, 1), name)
    assert getattr(kz.abi, {"normals": "KZ_INTEGRATOR_NORMALS", "ao": "KZ_INTEGRATOR_AO", "path_mats": "KZ_INTEGRATOR_PATH_MATS"}[name]) == tag
    assert kz.scenes.INTEGRATOR_TAGS[name] == tag
    cd = d.to_c()
    assert cd.integrator.type == tag
    assert kz.Scene(d).bvh_info()["nTris"] == d.n_tris()


@pytest.mark.parametrize("name", ["whitted", "direct", "path_mis2"])
def test_other_integrators_are_still_refused(kz, name):
    d = with_integrator(kz.scenes.cornell_box(16, 16, 1), name)
    assert d.to_c().integrator.type == 99
    with pytest.raises(kz.abi.KzError) as e:
        kz.Scene(d)
    assert e.value.code == 2 and "not on the hot path" in str(e.value)


def test_path_mats_refuses_normal_maps(kz):
    d = with_integrator(kz.scenes.textured_scene(16, 16, 1), "path_mats")
    with pytest.raises(kz.abi.KzError) as e:
        kz.Scene(d)
    assert e.value.code == 2 and "normalmap" in str(e.value) and "path_mats" in str(e.value)
    for name in ("normals", "ao", "path_mis"):                  # the other integrators take the same scene
        kz.Scene(with_integrator(d, name))


def test_new_integrators_ignore_the_integrator_fields(kz):
    """maxDepth 0, a negative traceBias: path_mis reads them, normals / ao / path_mats read nothing but the type (include/kazen_mi355x.h)."""
    d = with_integrator(kz.scenes.cornell_box(16, 16, 1), "path_mats")
    d.integrator.update(maxDepth=0, traceBias=-1.0, regularization=True)
    kz.Scene(d)


@pytest.mark.parametrize("name", INTEGRATORS)
def test_xml_loader_takes_the_new_integrators(kz, tmp_path, name):
    """The loader maps the type and ignores the properties (the reference's constructors read none); the integrator dict keeps its keys."""
    txt = open(MINI).read()
    here = os.path.join(HERE, "golden", "xml")
    txt = txt.replace('type="path_mis"', 'type="%s"' % name).replace('value="floor.obj"', 'value="%s"' % os.path.join(here, "floor.obj")) \
             .replace('value="cube.obj"', 'value="%s"' % os.path.join(here, "cube.obj")).replace('value="light.obj"', 'value="%s"' % os.path.join(here, "light.obj"))
    p = tmp_path / "s.xml"
    p.write_text(txt)
    d = kz.xmlscene.load_xml(str(p))
    assert d.integrator["type"] == name
    assert set(d.integrator) >= {"maxDepth", "traceBias", "regularization", "accumulatedRoughness"}
    assert d.integrator["maxDepth"] == 5 and d.integrator["traceBias"] == 0.001          # mini.xml sets maxDepth 4 / traceBias: ignored here
    assert d.to_c().integrator.type == kz.scenes.INTEGRATOR_TAGS[name]


def test_mirror_describes_the_new_integrators(tmp_path):
    """The C++ mirror registers normals / ao / path_mats and describe() fills the type alone."""
    src = tmp_path / "m.cpp"
    src.write_text(r'''#include <kazen/scene.h>
#include <cstdio>
#include <memory>
int main() {
    const char *names[4] = {"normals", "ao", "path_mats", "path_mis"};
    const int tags[4] = {KZ_INTEGRATOR_NORMALS, KZ_INTEGRATOR_AO, KZ_INTEGRATOR_PATH_MATS, KZ_INTEGRATOR_PATH_MIS};
    for (int i = 0; i < 4; ++i) {
        kazen::PropertyList p;
        std::unique_ptr<kazen::Object> o(kazen::ObjectFactory::createInstance(names[i], p));
        auto *it = dynamic_cast<kazen::Integrator *>(o.get());
        KzIntegrator row; row.type = -1; row.maxDepth = -7;
        if (!it || !it->describe(row) || row.type != tags[i]) { std::printf("FAIL %s\n", names[i]); return 1; }
        if (i < 3 && (row.maxDepth != 0 || row.traceBias != 0.f)) { std::printf("FAIL fields %s\n", names[i]); return 1; }
        std::printf("%s %s\n", names[i], it->toString().c_str());
    }
    return 0;
}
''')
    exe = tmp_path / "m"
    host = os.path.join(ROOT, "nano-kazen_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(host, "mirror_tree"), "-I" + os.path.join(host, "adapter"), str(src),
                           os.path.join(host, "adapter", "renderer_mi355x.cpp"), "-L" + LIBDIR, "-lkazen_mi355x", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert "normals NormalIntegrator[]" in out and "ao AmbientOcculusionIntegrator[]" in out and "path_mats PathMatsIntegrator[]" in out


# ---------------------------------------------------------------- CPU reference sanity
def test_ao_on_a_lone_plane_averages_one(kz, ref):
    """E[2 cos theta] = 1 over the uniform hemisphere: on an unoccluded plane the mean of the samples is 1 within 3 sigma."""
    s = kz.scenes.SceneDescription()
    s.add_mesh(*kz.scenes._vfnuv(kz.scenes.quad((-50, 0, -50), (50, 0, -50), (50, 0, 50), (-50, 0, 50), flip=True)), bsdf=kz.scenes.diffuse())
    s.camera.update(width=16, height=16, fov=30.0, nearClip=0.1, farClip=100.0, toWorld=kz.scenes.look_at((0, 3, 3), (0, 0, 0), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": 64, "seed": 0}
    r = RefScene(ref, with_integrator(s, "ao"))
    v = r.render_samples(*_scene_grid(s))[:, 2:]
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 0], v[:, 2]) and (v >= 0).all()
    m, se = float(v[:, 0].mean()), float(v[:, 0].std() / np.sqrt(len(v)))
    assert abs(m - 1.0) <= 3 * se, (m, se)


def test_normals_on_an_axis_aligned_box(kz, ref):
    """Seen from inside an axis-aligned box every sample is exactly one of (1,0,0), (0,1,0), (0,0,1)."""
    s = kz.scenes.SceneDescription()
    s.add_mesh(*kz.scenes._vfnuv(kz.scenes.box((-2, -2, -2), (2, 2, 2), inward=True)), bsdf=kz.scenes.diffuse())
    s.camera.update(width=24, height=24, fov=100.0, nearClip=0.01, farClip=100.0, toWorld=kz.scenes.look_at((0.3, 0.2, 0.1), (1, -0.5, -1), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": 4, "seed": 0}
    v = RefScene(ref, with_integrator(s, "normals")).render_samples(*_scene_grid(s))[:, 2:]
    assert ((v == 0) | (v == 1)).all() and (v.sum(1) == 1).all()
    assert len({tuple(x) for x in v}) == 3                        # (the wide view sees three faces)


def test_path_mats_without_lights_is_zero(kz, ref):
    s = kz.scenes.cornell_box(16, 16, 16)
    s.meshes = [m for m in s.meshes if m["light"] is None]
    v = RefScene(ref, with_integrator(s, "path_mats")).render_samples(*_scene_grid(s))[:, 2:]
    assert (v == 0).all()


def test_path_mats_depth_cap(kz, ref):
    """Roulette alone (p = min(t.x, 0.95)) ends an albedo-1 path after ~20 bounces; a NaN throughput is never stopped by it (next1D() >= NaN is false),
    so there the 512-bounce cap (H15) is what ends the path. Closed box, no light: 0 either way."""
    s = kz.scenes.SceneDescription()
    s.add_mesh(*kz.scenes._vfnuv(kz.scenes.box((-2, -2, -2), (2, 2, 2), inward=True)), bsdf=kz.scenes.diffuse((1.0, 1.0, 1.0)))
    s.camera.update(width=8, height=8, fov=60.0, nearClip=0.01, farClip=100.0, toWorld=kz.scenes.look_at((0, 0, 0), (0, 0, -1), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": 64, "seed": 0}
    r = RefScene(ref, with_integrator(s, "path_mats"))
    depths = np.array([r.mats_depth(x, y, i) for y in range(8) for x in range(8) for i in range(64)])
    assert depths.max() < 512 and 15 < depths.mean() < 25          # geometric with p = 0.05: mean 20
    s.meshes[0]["bsdf"] = kz.scenes.diffuse((float("nan"),) * 3)
    r = RefScene(ref, with_integrator(s, "path_mats"))
    depths = {r.mats_depth(x, 3, 0) for x in range(8)}
    assert 512 in depths and depths <= {1, 512}                 # (a path the first roulette ends - t.x = 1, p = 0.95 - has depth 1)
    assert (r.render_samples(*_scene_grid(s))[:, 2:] == 0).all()
