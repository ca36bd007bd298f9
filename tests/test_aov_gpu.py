"""-m gpu: the feature films of include/kazen_mi355x_aov.h on the MI355X. Every sample of kz_aov_samples has the CPU reference's bits (tests/cpu_ref/kz_aov_ref.cpp),
every AOV film is the reference's canonical film texel for texel under every filter and schedule, the NORMAL film equals the oracle-pinned `normals` picture where
the two are the same numbers, the picture does not notice the AOVs, and the films follow the picture's through clears, accumulation and edits."""
import copy

import numpy as np
import pytest

from checks import same_bits_strict
from cpu_refs import AovRef, lib
from film_cases import AOVS, FILTERS, H, SCHEDULES, SPP, W, _looks_at_the_light, _thinlens, _visible, _with_filter, grid_of, octant_scene, with_integrator

pytestmark = pytest.mark.gpu

INTEGRATORS = ("path_mis", "normals", "ao", "path_mats")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("aov", tmp_path_factory.mktemp("kza"))


_films = {}


def ref_films(ref, key, desc, s0=0, s1=0):
    """The three reference films of a description, computed once per (key, sample range) and shared."""
    k = (key, s0, s1)
    if k not in _films:
        r = AovRef(ref, desc)
        _films[k] = {a: r.film(a, s0, s1) for a in AOVS}
        for f in _films[k].values():
            f.setflags(write=False)
    return _films[k]


def gpu_films(sc):
    return {a: sc.aov_film(a) for a in AOVS}


# ---------------------------------------------------------------- samples
def _sample_cases(kz):
    S = kz.scenes
    return {"cornell": S.cornell_box(W, H, SPP), "materials": S.materials_scene(W, H, SPP), "textured": S.textured_scene(W, H, SPP, sampler="pmj02bn"),
            "thinlens": _thinlens(S.cornell_box(W, H, SPP, sampler="stratified")), "invisible light/path_mis": _looks_at_the_light(kz),
            "invisible light/normals": with_integrator(_looks_at_the_light(kz), "normals")}


@pytest.mark.parametrize("name", ["cornell", "materials", "textured", "thinlens", "invisible light/path_mis", "invisible light/normals"])
def test_samples_have_the_references_bits(gpu_lib, kz, ref, name):
    d = _sample_cases(kz)[name]
    pxy, idx = grid_of(d)
    sc = kz.Scene(d, device=0)
    g, c = sc.aov_samples(pxy, idx), AovRef(ref, d).samples(pxy, idx)
    bad = ~(g.view(np.uint32) == c.view(np.uint32)).all(axis=1)
    assert not bad.any(), (name, int(bad.sum()), g[bad][:3], c[bad][:3])
    assert np.isfinite(g).all() and (g[:, 9] == 1).any() and g[:, 2:5].max() > 0 and g[:, 8].max() > 0
    sc.set_aovs(AOVS)                                                 # it works whatever the mask is
    assert same_bits_strict(sc.aov_samples(pxy[:4096], idx[:4096]), g[:4096])
    if name == "materials":
        assert (g[:, 2:5] == 1).all(axis=1).any()                     # the models without a diffuse colour are white
    if name == "textured":
        assert len(np.unique(g[g[:, 9] == 1][:, 2:5], axis=0)) > 1000 # texture lookups, not constants


def test_an_invisible_light_is_walked_through_by_path_mis_only(gpu_lib, kz, ref):
    d = _looks_at_the_light(kz)
    pxy, idx = grid_of(d)
    mis = kz.Scene(d, device=0).aov_samples(pxy, idx)
    nrm = kz.Scene(with_integrator(d, "normals"), device=0).aov_samples(pxy, idx)
    on_light = (nrm[:, 2:5] == 0).all(axis=1) & (nrm[:, 9] == 1)      # the light mesh's own row: black diffuse
    assert on_light.sum() > 1000
    assert (mis[on_light][:, 2:5] == np.float32(0.73)).all()          # the ceiling behind it
    assert (mis[on_light][:, 8] < 0.05).all() and (nrm[on_light][:, 8] > 0.5).all()      # depth from the restart origin (the stated limitation) / from the camera
    assert same_bits_strict(mis[~on_light], nrm[~on_light])


# ---------------------------------------------------------------- films
@pytest.mark.parametrize("scene", ["cornell", "textured"])
@pytest.mark.parametrize("filt", list(FILTERS))
def test_films_equal_the_reference(gpu_lib, kz, ref, scene, filt):
    base = kz.scenes.cornell_box(W, H, SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    d = _with_filter(base, FILTERS[filt])
    want = ref_films(ref, (scene, filt), d)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(AOVS)
    sc.render()
    for a, f in gpu_films(sc).items():
        assert np.array_equal(f, want[a]), (a, float(np.abs(f - want[a]).max()))
        assert f[..., 3].max() > 0 and np.abs(f[..., :3]).max() > 0
    assert sc.aov("normal").min() < 0                                 # signed values survive the film
    dz = sc.aov("depth")
    assert np.array_equal(dz[..., 0], dz[..., 1]) and np.array_equal(dz[..., 0], dz[..., 2])


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_films_do_not_depend_on_the_schedule(gpu_lib, kz, ref, integ):
    """One film per AOV whatever the pass size, the sample chunking, passes in flight, halves, shadow rays beside, the split of the sample range over calls -
    and whatever the integrator (a scene whose light camera rays see: nothing is walked through)."""
    base = _visible(kz.scenes.cornell_box(W, H, SPP))
    want = ref_films(ref, "cornell/visible", base)
    sc = kz.Scene(with_integrator(base, integ), device=0)
    sc.set_aovs(AOVS)
    for kw in SCHEDULES:
        sc.render(**kw)
        info = sc.last_pass_info()
        if "passes_in_flight" in kw:
            # the AOV stage of a pass waits for the one before it on another stream (its own event chain): the passes did run in flight, several pixel chunks each
            assert info["passesInFlight"] == 2 and info["passes"] >= 6, info
        if "tune" in kw:
            assert info["sppPerPass"] == 4 and info["passes"] >= 2, info
        if "pass_halves" in kw and integ == "path_mis":
            assert info["shadowBeside"] == 2, info
        for a, f in gpu_films(sc).items():
            assert np.array_equal(f, want[a]), (integ, kw, a)
    sc.render(sample_begin=0, sample_end=4)
    sc.render(sample_begin=4, sample_end=8, accumulate=True)
    for a, f in gpu_films(sc).items():
        assert np.array_equal(f, want[a]), (integ, "two calls", a)


def test_passes_in_flight_repeat(gpu_lib, kz, ref):
    """The ordering hazard again, on the textured scene with three passes in flight and the smallest chunks: a missing wait shows as a film that differs."""
    d = kz.scenes.textured_scene(W, H, SPP)
    want = ref_films(ref, ("textured", "gaussian r=2"), _with_filter(d, FILTERS["gaussian r=2"]))
    sc = kz.Scene(d, device=0)
    sc.set_aovs(AOVS)
    for kw in ({"passes_in_flight": 3, "pass_items": 512 * SPP}, {"passes_in_flight": 2, "pass_items": 256 * 4, "tune": {"sppPerPass": 4}}):
        sc.render(**kw)
        info = sc.last_pass_info()
        # (the planner does not cut a pass below 864 pixels here: 8 chunks of the frame's pixels, and twice as many passes with the samples in two ranges)
        assert info["passesInFlight"] == kw["passes_in_flight"] and info["passes"] >= 8, info
        for a, f in gpu_films(sc).items():
            assert np.array_equal(f, want[a]), (kw, a)


# ---------------------------------------------------------------- against the oracle-pinned path
def test_normal_film_equals_the_normals_picture(gpu_lib, kz, ref):
    """On triangles without vertex normals whose geometric normal has no negative component, |n_geo| (the `normals` integrator, pinned against the oracle by
    tests/test_integrators_gpu.py) and the signed NORMAL feature are the same numbers: the two films are the same bits, rgb * w and w."""
    d = octant_scene(kz)
    nrm = kz.Scene(with_integrator(d, "normals"), device=0)
    nrm.set_aovs(["normal"])
    nrm.render()
    picture = nrm.film()
    assert picture[..., :3].max() > 0
    assert np.array_equal(nrm.aov_film("normal"), picture)
    mis = kz.Scene(d, device=0)
    mis.set_aovs(["normal"])
    mis.render()
    assert np.array_equal(mis.aov_film("normal"), picture)
    assert not np.array_equal(mis.film(), picture)


# ---------------------------------------------------------------- the picture does not notice
@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_picture_untouched_and_memory(gpu_lib, kz, scene):
    d = kz.scenes.cornell_box(W, H, SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    sc = kz.Scene(d, device=0)
    assert sc.aov_info() == 0
    sc.render()
    plain = sc.film()
    sc.set_aovs(AOVS)
    assert sc.aov_info() == 0                                         # allocated on first use
    sc.render()
    assert np.array_equal(sc.film(), plain)
    b = sc.border
    taps = 5                                                          # gaussian r = 2: tapLo = -2, tapHi = 2
    assert sc.aov_info() == 3 * (taps * taps * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16)
    sc.set_aovs(["normal"])
    assert sc.aov_info() == taps * taps * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16
    sc.set_aovs(())
    assert sc.aov_info() == 0
    sc.render()
    assert np.array_equal(sc.film(), plain)


# ---------------------------------------------------------------- lifecycle
def test_clear_and_late_enable(gpu_lib, kz, ref):
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(["albedo", "normal"])
    assert not sc.aov_film("albedo").any()                            # enabled, nothing rendered: zeros
    sc.render(sample_begin=0, sample_end=4)
    assert np.array_equal(sc.aov_film("albedo"), ref_films(ref, "cornell", d, 0, 4)["albedo"])
    # an AOV that enters the mask covers the samples rendered from then on
    sc.set_aovs(AOVS)
    sc.render(sample_begin=4, sample_end=8, accumulate=True)
    assert np.array_equal(sc.aov_film("depth"), ref_films(ref, "cornell", d, 4, 8)["depth"])
    assert np.array_equal(sc.aov_film("albedo"), ref_films(ref, ("cornell", "gaussian r=2"), d)["albedo"])      # (the ones that stayed: all 8 samples)
    picture = sc.film()
    sc.film_clear()
    sc.sync()
    for a in AOVS:
        assert not sc.aov_film(a).any(), a
    assert not sc.film().any()
    # a render that does not accumulate clears them too
    sc.render(sample_begin=0, sample_end=4)
    sc.render(sample_begin=4, sample_end=8)
    assert np.array_equal(sc.aov_film("normal"), ref_films(ref, "cornell", d, 4, 8)["normal"])
    assert picture[..., 3].max() > 0


def test_set_bsdfs_switches_the_kernel_variant(gpu_lib, kz):
    """A lean scene (constant diffuse / kiss rows: kz_wf_aov<0>) taken to a texture-backed row and back gives the albedo films of fresh scenes of each description."""
    S = kz.scenes
    chk = S._test_images()[0]
    tex = S.imagetexture(chk, scale=6.0, colorspace="srgb")
    lean = S.cornell_box(W, H, SPP)
    lean._tex_seed = [tex]                                            # the texture is in the scene's table from the start; no row names it
    plain = lean.meshes[2]["bsdf"]
    textured = copy.copy(lean)
    textured.meshes = list(lean.meshes)
    textured.meshes[2] = dict(lean.meshes[2], bsdf=S.lambertian(tex))

    def albedo_of(desc):
        fresh = kz.Scene(desc, device=0)
        fresh.set_aovs(["albedo"])
        fresh.render()
        return fresh.aov_film("albedo")

    want_lean, want_tex = albedo_of(lean), albedo_of(textured)
    assert not np.array_equal(want_lean, want_tex)
    sc = kz.Scene(copy.copy(lean), device=0)                          # (set_bsdfs rewrites Scene.desc.meshes)
    sc.set_aovs(["albedo"])
    sc.render()
    assert np.array_equal(sc.aov_film("albedo"), want_lean)
    sc.set_bsdfs({2: S.lambertian(tex)})
    assert np.array_equal(sc.aov_film("albedo"), want_lean)           # an edit leaves the films alone
    sc.render()
    assert np.array_equal(sc.aov_film("albedo"), want_tex)
    sc.set_bsdfs({2: plain})
    sc.render()
    assert np.array_equal(sc.aov_film("albedo"), want_lean)


def test_set_camera(gpu_lib, kz, ref):
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(AOVS)
    sc.render()
    before = gpu_films(sc)
    cam = {"toWorld": kz.scenes.look_at((0.8, 0.3, 3.2), (0, -0.2, 0), (0, 1, 0)), "fov": 45.0}
    sc.set_camera(cam)
    for a in AOVS:
        assert np.array_equal(sc.aov_film(a), before[a])              # left alone by the edit
    sc.render()
    moved = kz.scenes.cornell_box(W, H, SPP)
    moved.camera.update(cam)
    want = ref_films(ref, "cornell/moved", moved)
    for a, f in gpu_films(sc).items():
        assert np.array_equal(f, want[a]), a
        assert not np.array_equal(f, before[a]), a


# ---------------------------------------------------------------- refusals
def test_refusals_with_a_device(gpu_lib, kz):
    a = kz.abi
    d = kz.scenes.cornell_box(64, 64, 4)
    sc = kz.Scene(d, device=0)
    tiles = kz.shard.deal_tiles(64, 64, 1, 0, 32)

    def refused(fn, *words):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == a.KZ_ERR_UNSUPPORTED, str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def all_work():
        sc.render(pipeline=1)
        film, _ = sc.render_multi([0])
        assert film[..., 3].max() > 0
        assert sc.render_dealt(tiles, np.zeros(1, np.uint32), takers=1, batch_tiles=2) == tiles
        assert sc.render_tiles(tiles, packed=True).size == sc.packed_floats(tiles)
        assert sc.film_tiles(tiles).size == sc.packed_floats(tiles)

    all_work()
    sc.set_aovs(["depth"])
    refused(lambda: sc.render(pipeline=1), "kz_render", "pipeline = 1")
    refused(lambda: sc.render_multi([0]), "kz_render_multi")
    refused(lambda: sc.render_dealt(tiles, np.zeros(1, np.uint32), takers=1, batch_tiles=2), "kz_render_tiles", "KzTileDealer")
    refused(lambda: sc.render_tiles(tiles, packed=True), "kz_render_tiles", "packedOutput")
    refused(lambda: sc.film_tiles(tiles), "kz_film_download_tiles")
    # a plain render and a static kz_render_tiles on one replica work
    sc.render()
    whole = sc.aov_film("depth")
    sc.render_tiles(tiles)
    assert np.array_equal(sc.aov_film("depth"), whole) and whole[..., 3].max() > 0
    sc.set_aovs(0)
    all_work()
