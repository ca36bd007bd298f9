"""-m gpu: the roulette-ahead test of the shade kernels (kz_wavefront.h wfShadeSurvivor) leaves every film as it was, bit for bit. The development library renders
each scene with the test as the scene has it and with it switched off (kz_debug_rr_ahead) in ONE process: the two films are equal, and equal to the oracle's
(kzo_render_canonical) - with the product kernels and with the statistics kernels (which take the test only when asked to), with the shadow rays beside the bounce rays, as two halves, and over two sample
ranges. The ray counters say that the test did something where it should and nothing where the scene switches it off."""
import numpy as np
import pytest

import rr_ahead_scenes as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def rr(dev_lib):
    """rr(False): no roulette-ahead test; rr(True): as the scene has it; rr(2): counted renders (kz_set_stats) take it too - by default they trace every ray."""
    yield lambda on: dev_lib.kz_debug_rr_ahead(int(on))
    dev_lib.kz_debug_rr_ahead(1)


def _mats(S):
    d = R.room(S)
    d.integrator["type"] = "path_mats"
    return d


# name -> (description, what the hook does to the ray counter, is there an oracle film)
SCENES = {
    "room_whole_ceiling": (lambda S: R.room(S, 64, 48, 8, maxDepth=8), "less", True),
    "room_64_triangles": (lambda S: R.room(S, 48, 40, 8, grid=(8, 4)), "less", True),
    "c4_like_pmj": (lambda S: S.random_triangles(20000, 96, 64, 16, sampler="pmj02bn", seed=1), "less", True),
    "room_65_triangles": (lambda S: R.room(S, 48, 40, 8, grid=(8, 4), extra_light=True), "equal", True),
    "room_background": (lambda S: R.room(S, 48, 40, 8, background={"color": (0.2, 0.3, 0.5), "intensity": 1.0}), "equal", True),
    "room_path_mats": (_mats, "equal", False),
    "no_lights_no_background": (lambda S: R.room(S, 48, 40, 8, lit=False), "less", True),
    "room_independent_ragged": (lambda S: R.room(S, 45, 37, 5, sampler="independent", seed=3), "less", True),
    "room_stratified": (lambda S: R.room(S, 48, 40, 9, sampler="stratified", seed=1), "less", True),
    "room_correlated": (lambda S: R.room(S, 48, 40, 12, sampler="correlated", seed=3), "less", True),
    "room_pmj": (lambda S: R.room(S, 48, 40, 16, sampler="pmj02bn", seed=1), "less", True),
    "glass_regularised": (lambda S: R.glass_room(S, 48, 40, 8), "less", True),
    "invisible_panel": (lambda S: R.panel_room(S, 48, 40, 8), "less", True),
    "textured": (lambda S: S.textured_scene(64, 40, 8), "less", True),
}


def film_of(sc, **kw):
    sc.render(**kw)
    return sc.film()


@pytest.mark.parametrize("name", list(SCENES))
def test_films_are_the_same_bits_with_and_without(dev_lib, kz, O, rr, name):
    make, effect, has_oracle = SCENES[name]
    desc = make(kz.scenes)
    sc = kz.Scene(desc, device=0, lib=dev_lib)
    n = sc.sample_count
    want = O.OracleScene(desc).render_canonical(threads=0) if has_oracle else None
    rr(True)
    on = film_of(sc)
    rr(False)
    off = film_of(sc)
    assert np.array_equal(on, off)
    if want is not None:
        assert np.array_equal(on, want)
    if name != "no_lights_no_background":
        assert np.abs(on[..., :3]).max() > 0
    # the other ways a pass is launched, with the test on and off
    for flag in (True, False):
        rr(flag)
        assert np.array_equal(film_of(sc, shadow_beside=2), on), flag
        assert np.array_equal(film_of(sc, pass_halves=2), on), flag
        sc.render(0, n // 2)
        sc.render(n // 2, n, accumulate=True)
        assert np.array_equal(sc.film(), on), flag
        assert np.array_equal(film_of(sc, pass_items=4096, passes_in_flight=3), on), flag
    # the statistics kernels: the same films, and the ray counter says what the test did. A counted render leaves the test out unless it is asked to take it
    # (rr(2)): the counters then state the work of the reference's loop, which tests/test_gpu_parity.py bounds against the oracle's
    sc.set_stats(True)
    rays = {}
    for flag in (2, True, False):
        rr(flag)
        sc.stats(reset=True)
        assert np.array_equal(film_of(sc), on), flag
        rays[flag] = sc.stats(reset=True)["rays"]
    print("%s: rays %d with the test, %d without (%.4f)" % (name, rays[2], rays[False], rays[2] / max(1, rays[False])))
    assert rays[True] == rays[False], rays
    if effect == "less":
        assert rays[2] < rays[False], rays
    else:
        assert rays[2] == rays[False], rays
    # the megakernel is not touched: the same film
    rr(True)
    sc.set_stats(False)
    assert np.array_equal(film_of(sc, pipeline=1), on)
    sc.close()


def test_product_library_renders_the_same_films(gpu_lib, dev_lib, kz, rr):
    """The product library has no switch: its films are the development library's with the test off."""
    for name in ("room_whole_ceiling", "c4_like_pmj", "glass_regularised"):
        desc = SCENES[name][0](kz.scenes)
        a = kz.Scene(desc, device=0)
        fa = film_of(a)
        a.close()
        rr(False)
        b = kz.Scene(desc, device=0, lib=dev_lib)
        assert np.array_equal(film_of(b), fa), name
        b.close()
        rr(True)


def test_edits_keep_the_resident_scene_equal_to_a_fresh_one(dev_lib, kz, O, rr):
    S = kz.scenes
    rr(True)
    sc = kz.Scene(R.room(S, 48, 40, 8, grid=(2, 2), extra_light=True), device=0, lib=dev_lib)
    T = kz.abi.KZ_TABLE_EM_TRIS

    def check(what):
        fresh = kz.Scene(sc.desc, device=0, lib=dev_lib)
        assert np.array_equal(sc.table(T, 0), sc.table(T)), what                       # the replica's table is the host's ...
        assert np.array_equal(sc.table(T), fresh.table(T)) and np.array_equal(fresh.table(T, 0), fresh.table(T)), what      # ... and a fresh scene's
        got = film_of(sc)
        assert np.array_equal(got, film_of(fresh)), what
        assert np.array_equal(got, O.OracleScene(sc.desc).render_canonical(threads=0)), what
        rr(False)
        assert np.array_equal(film_of(sc), got), what
        rr(True)
        fresh.close()

    check("as created")
    M = np.eye(4, dtype=np.float32)
    M[:3, 3] = (0.1, -0.3, 0.05)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = np.cos(0.3), np.sin(0.3), -np.sin(0.3), np.cos(0.3)
    sc.set_transforms({R.CEILING: M})                                                     # a light mesh under a transform: the ceiling comes down and turns
    check("light mesh transformed")
    sc.set_vertices({9: (sc.desc.meshes[9]["V"] + np.float32([0.3, 0.2, 0.0]), sc.desc.meshes[9]["N"])})
    check("emitter vertices moved")
    sc.set_lights({9: S.area((1, 1, 1), 0.0, False)})                                     # a light goes dark and invisible (it stays an emitter: a hit on it ends the path) ...
    check("light switched off")
    sc.set_lights({9: S.area((0.9, 1, 1), 6.0, True)})                                    # ... and comes back
    check("light switched on")
    sc.set_bsdfs({6: S.kazenstandard(baseColor=(0.2, 0.3, 0.9), roughness=0.2, metallic=1.0)})
    sc.set_vertices({8: (sc.desc.meshes[8]["V"] + np.float32([0.2, -0.2, 0.1]), sc.desc.meshes[8]["N"])})      # the slab: other rays reach the ceiling now
    check("material and occluder")
    sc.close()
