"""normals / ao / path_mats on the MI355X: every sample of kz_render_samples has the CPU reference's bits (tests/cpu_ref), the default (wavefront)
pipeline's film is the megakernel's and the CPU reference's canonical film texel for texel under every schedule, and path_mats converges to path_mis."""
import copy

import numpy as np
import pytest

from checks import same_bits
from cpu_refs import RefScene, lib
from film_cases import INTEGRATORS, with_integrator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("integrators", tmp_path_factory.mktemp("kzi"))


def _visible(desc):
    d = copy.deepcopy(desc)
    for m in d.meshes:
        if m["light"] is not None:
            m["light"] = dict(m["light"], lightPrimaryVisibility=True)
    return d


def _thinlens(desc):
    d = copy.deepcopy(desc)
    d.camera.update(type="thinlens", apertureRadius=0.1, focusDistance=3.5)
    return d


def _no_normalmaps(desc):
    """path_mats refuses normal maps: each normalmap row replaced by the row it wraps."""
    d = copy.deepcopy(desc)
    for m in d.meshes:
        if m["bsdf"] is not None and m["bsdf"]["type"] == "normalmap":
            m["bsdf"] = m["bsdf"]["nested"]
    return d


def _cases(kz):
    S = kz.scenes
    return [("cornell/independent", S.cornell_box(24, 20, 8)),
            ("cornell/pmj02bn/visible", _visible(S.cornell_box(24, 20, 8, sampler="pmj02bn"))),
            ("cornell/stratified/thinlens", _thinlens(S.cornell_box(24, 20, 9, sampler="stratified"))),
            ("glass/correlated", S.glass_scene(24, 20, 8, sampler="correlated")),
            ("materials/independent", S.materials_scene(32, 20, 8)),
            ("textured/pmj02bn", S.textured_scene(32, 20, 8, sampler="pmj02bn"))]


def _grid(desc, S=None):
    W, H = desc.camera["width"], desc.camera["height"]
    S = S or desc.sampler["sampleCount"]
    yy, xx, ii = np.meshgrid(np.arange(H), np.arange(W), np.arange(S), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_samples_have_the_cpu_references_bits(gpu_lib, kz, ref, integ):
    """Diffuse, kiss, mirror / dielectric / rough models, textures (normal maps for normals / ao), the four samplers, pinhole and thin lens, invisible
    and visible lights: every sample's pixel position and radiance equal to the CPU reference's to the last bit (> 20 000 samples per integrator)."""
    total = 0
    for name, desc in _cases(kz):
        if integ == "path_mats":
            desc = _no_normalmaps(desc)
        d = with_integrator(desc, integ)
        sc = kz.Scene(d, device=0)
        pxy, idx = _grid(d)
        g = sc.render_samples(pxy, idx)
        c = RefScene(ref, d).render_samples(pxy, idx)
        bad = ~((g.view(np.uint32) == c.view(np.uint32)) | (np.isnan(g) & np.isnan(c))).all(axis=1)
        assert not bad.any(), (name, int(bad.sum()), g[bad][:3], c[bad][:3])
        assert np.isfinite(g).all() and g[:, 2:].max() > 0, name
        total += len(idx)
    assert total >= 20000


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_films_equal_the_megakernel_and_the_cpu_reference(gpu_lib, kz, ref, integ):
    """The default pipeline's film at several pass sizes, with passes in flight, with a tile dealer and accumulated over split sample ranges is the
    pipeline-1 (megakernel) film and the CPU reference's canonical film, texel for texel."""
    for desc in (kz.scenes.cornell_box(72, 40, 16, sampler="pmj02bn"), _no_normalmaps(kz.scenes.materials_scene(64, 40, 8))):
        d = with_integrator(desc, integ)
        cpu = RefScene(ref, d).render_canonical()
        sc = kz.Scene(d, device=0)
        sc.render()
        whole = sc.film()
        assert np.array_equal(whole, cpu)
        assert whole[..., :3].max() > 0
        sc.render(pipeline=1)
        assert np.array_equal(sc.film(), cpu)
        for kw in ({"pass_items": 64 * 16}, {"pass_items": 40 * 64 * 3, "passes_in_flight": 2}, {"passes_in_flight": 3, "pass_items": 4096}, {"shadow_beside": 2},
                   {"pass_halves": 2}):
            sc.render(**kw)
            assert np.array_equal(sc.film(), cpu), kw
        S = d.sampler["sampleCount"]
        sc.render(sample_begin=0, sample_end=S // 2)
        assert np.array_equal(sc.film(), RefScene(ref, d).render_canonical(0, S // 2))
        sc.render(sample_begin=S // 2, sample_end=S, accumulate=True)
        acc = sc.film()
        sc.render(sample_begin=0, sample_end=S // 2, pipeline=1)
        sc.render(sample_begin=S // 2, sample_end=S, accumulate=True, pipeline=1)
        assert np.array_equal(sc.film(), acc)
        assert np.allclose(acc, cpu, rtol=1e-5, atol=1e-6)
        tiles = kz.shard.deal_tiles(d.camera["width"], d.camera["height"], 1, 0, 32)
        counter = np.zeros(1, np.uint32)
        assert sc.render_dealt(tiles, counter, takers=1, batch_tiles=2, pass_items=32 * 32 * 2 * 4) == tiles
        assert np.array_equal(sc.film(), cpu)


def test_path_mats_stops_at_the_cap(gpu_lib, kz, ref):
    """NaN albedo in a closed box without a light: roulette never ends such a path (next1D() >= NaN is false), so every path runs to the 512-bounce cap
    (H15) - on the wavefront pipeline through the survivor read-back every 4th bounce - and the film is the CPU reference's on both pipelines."""
    S = kz.scenes
    s = S.SceneDescription()
    s.add_mesh(*S._vfnuv(S.box((-2, -2, -2), (2, 2, 2), inward=True)), bsdf=S.diffuse((float("nan"),) * 3))
    s.camera.update(width=16, height=16, fov=60.0, nearClip=0.01, farClip=100.0, toWorld=S.look_at((0, 0, 0), (0, 0, -1), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": 4, "seed": 0}
    d = with_integrator(s, "path_mats")
    r = RefScene(ref, d)
    depths = {r.mats_depth(x, 5, 1) for x in range(16)}
    assert 512 in depths and depths <= {1, 512}                 # (a path the first roulette ends - t.x = 1, p = 0.95 - has depth 1)
    sc = kz.Scene(d, device=0)
    sc.render()
    f = sc.film()
    assert same_bits(f, r.render_canonical()) and f[..., 3].sum() > 0
    sc.render(pipeline=1)
    assert same_bits(sc.film(), f)


def _mats_vs_mis_scene(kz, depth, spp):
    """Grey albedos (roulette on t.x is unbiased), no background, lights seen by the camera and black diffuse on the light meshes."""
    S = kz.scenes
    s = S.cornell_box(48, 48, spp, sampler="independent", seed=3, maxDepth=depth)
    for m in s.meshes:
        b = m["bsdf"]
        if m["light"] is not None:
            m["light"] = dict(m["light"], lightPrimaryVisibility=True)
        elif b["type"] == "diffuse":
            a = float(np.mean(b["albedo"]))
            m["bsdf"] = S.diffuse((a, a, a))
        else:
            m["bsdf"] = S.diffuse((0.6, 0.6, 0.6))
    return s


def _region_stats(sc, d):
    pxy, idx = _grid(d)
    v = sc.render_samples(pxy, idx)[:, 2:].mean(axis=1)
    W, H, S = d.camera["width"], d.camera["height"], d.sampler["sampleCount"]
    v = v.reshape(H // 8, 8, W // 8, 8, S).transpose(0, 2, 1, 3, 4).reshape(H // 8, W // 8, -1)
    return v.mean(-1), v.var(-1, ddof=1) / v.shape[-1]


def test_path_mats_converges_to_path_mis(gpu_lib, kz):
    """8x8-pixel region means at 1024 spp: |path_mats - path_mis (maxDepth 64)| <= 4 sigma in every region. The same test against path_mis at maxDepth 2
    (a biased estimate: most indirect light is cut) fails, so it can see a bias."""
    spp = 1024
    dm = with_integrator(_mats_vs_mis_scene(kz, 64, spp), "path_mats")
    m_mean, m_var = _region_stats(kz.Scene(dm, device=0), dm)
    dp = with_integrator(_mats_vs_mis_scene(kz, 64, spp), "path_mis")
    p_mean, p_var = _region_stats(kz.Scene(dp, device=0), dp)
    z = np.abs(m_mean - p_mean) / np.sqrt(m_var + p_var)
    assert (z <= 4).all(), z.max()
    db = with_integrator(_mats_vs_mis_scene(kz, 2, spp), "path_mis")
    b_mean, b_var = _region_stats(kz.Scene(db, device=0), db)
    zb = np.abs(m_mean - b_mean) / np.sqrt(m_var + b_var)
    assert (zb > 4).any(), zb.max()
