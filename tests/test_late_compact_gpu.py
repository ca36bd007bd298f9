"""-m gpu: the compaction in front of the first roulette bounce (kz_wavefront.h kz_wf_compact; kz_render.hip wfMis) leaves every film as it was, bit for bit.
The development library renders each scene with the compaction and with it switched off (kz_debug_compact_late) in ONE process: the two films are equal - whole
passes, the shadow rays beside the bounce rays, a pass as two halves, two small passes in flight, and counted renders, whose counters are equal too. What a pass
did with its late bounces is read from the library's trace (kz_debug_trace: one line per path_mis pass), so every case is known to have taken the way it is
there for: the dense set, or - when the survivors of bounce 2 do not fit it - the pass's own arrays."""
import re

import numpy as np
import pytest

import rr_ahead_scenes as R

pytestmark = pytest.mark.gpu

W = H = SPP = 64                # 2^18 items
COMPACTED, TOO_SMALL = "compacted", "in the pass's arrays: the dense set is too small"


def _dim(S, d, walls=0.3):
    """The scene's surfaces made dark: three diffuse bounces leave a throughput of ~walls^3, which is what the roulette of bounce 3 keeps of the paths."""
    for i, m in enumerate(d.meshes):
        if m["light"] is None:
            m["bsdf"] = S.diffuse((walls, walls * (0.7 + 0.1 * (i % 3)), walls * 0.8))
    return d


def _room(S, depth, **kw):
    """The dark room lit by ONE small triangle on its back wall (the ceiling is a wall like the others): a bounce ray that the next roulette draw will end is
    still queued when it hits an emitter triangle at all (the roulette-ahead test), so a room under a ceiling of light keeps far more than walls^3 of its paths."""
    return _dim(S, R.room(S, W, H, SPP, maxDepth=depth, lit=False, extra_light=True, **kw))


def _two_panels(S, depth):
    """... and two small invisible light panels, one above the other: a shadow ray towards the upper one crosses the lower one and is walked through it (MODE 2 of
    kz_wf_trace, behind the any-hit kernel that hands such rays on)."""
    d = _room(S, depth)
    for y, colour, power in ((0.3, (1, 1, 1), 6.0), (0.45, (1, 0.9, 0.8), 5.0)):
        q = S.quad((-0.2, y, -0.3), (-0.2, y, 0.1), (0.2, y, 0.1), (0.2, y, -0.3), flip=True)
        d.add_mesh(q[0], q[3], q[1], q[2], bsdf=S.diffuse((0, 0, 0)), light=S.area(colour, power, False))
    d.camera.update(toWorld=S.look_at((0.05, -0.2, 0.95), (0, 0.5, -1), (0, 1, 0)))
    return d


def _open_floor(S, depth):
    """The room's floor, its two blocks and the small light under a sky: most bounce rays leave the scene (a path must hit three times to reach bounce 3), the misses of
    the late bounces add the background through the dense set's throughput and origin, and kz_wf_final takes what is left after the last bounce."""
    d = _room(S, depth, background={"color": (0.2, 0.3, 0.5), "intensity": 1.0})
    d.meshes = [m for i, m in enumerate(d.meshes) if i in (0, 6, 7, 9)]
    return d


def _glass(S, depth):
    """... with a glass sphere and regularisation: eta != 1 along a path, the path state with its misc record, the kernel variant of the other BSDF models. (Such a
    scene does not play the roulette ahead; under the sky most of its paths have left before bounce 3, and the sphere, whose every path gets there, is small.)"""
    d = _open_floor(S, depth)
    P, N, UV, F = S.uv_sphere((0.3, -0.3, 0.0), 0.07, 20, 21)
    d.add_mesh(P, F, N, UV, bsdf=S.dielectric())
    d.integrator.update(regularization=True, accumulatedRoughness=0.5)
    return d


# name -> (description, what the pass does with its late bounces (None: not pinned), compare with the oracle's film)
SCENES = {
    "dark_room_depth5": (lambda S: _room(S, 5), COMPACTED, True),
    "dark_room_depth8": (lambda S: _room(S, 8), COMPACTED, False),
    "dark_room_pmj": (lambda S: _room(S, 6, sampler="pmj02bn", seed=1), COMPACTED, False),
    "open_glass_regularised": (lambda S: _glass(S, 8), COMPACTED, False),
    "bright_room_overflows": (lambda S: R.room(S, W, H, SPP, maxDepth=8), TOO_SMALL, False),
    "black_room_nothing_survives": (lambda S: _dim(S, R.room(S, W, H, SPP, maxDepth=5), walls=0.0), COMPACTED, False),
    "invisible_panels": (lambda S: _two_panels(S, 6), COMPACTED, False),
    "open_floor_background": (lambda S: _open_floor(S, 6), COMPACTED, False),
}


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind(dev_lib, gpu_lib):
    """The tests that follow in the same process compare free device memory before and after their own calls: what these tests' scenes held goes back first."""
    yield
    import gc
    gc.collect()
    dev_lib.kz_device_trim(0)
    gpu_lib.kz_device_trim(0)


@pytest.fixture
def late(dev_lib):
    """late(False): every bounce in the pass's own arrays, as before the compaction; late(True): the default."""
    yield lambda on: dev_lib.kz_debug_compact_late(int(on))
    dev_lib.kz_debug_compact_late(1)


def dense_entries(desc, items):
    """Entries of a pass's dense set: it lies in the pass's hit array (16 B per item) and an entry is seven 16-B records and the origin word, + 16 B each for the
    misc record (kernels of the other BSDF models, regularisation) and the sampler words (every sampler but pmj02bn)."""
    lean = not desc.integrator["regularization"] and all(m["bsdf"]["type"] in ("diffuse", "kazenstandard") for m in desc.meshes)
    return 16 * items // (116 + (0 if lean else 16) + (0 if desc.sampler["type"] == "pmj02bn" else 16))


def film_of(sc, **kw):
    sc.render(**kw)
    return sc.film()


def traced_film(dev_lib, capfd, sc, **kw):
    """The film of one render and what its passes did with their late bounces: [(verdict, paths queued for bounce 3, entries of the dense set)]."""
    capfd.readouterr()
    dev_lib.kz_debug_trace(1)
    try:
        film = film_of(sc, **kw)
    finally:
        dev_lib.kz_debug_trace(0)
    err = capfd.readouterr().err
    return film, [(m.group(1).strip(), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"late bounces ([^(]+)\((\d+) paths, dense set of (\d+)\)", err)]


@pytest.mark.parametrize("name", list(SCENES))
def test_films_are_the_same_bits_with_and_without(dev_lib, kz, O, late, capfd, name):
    make, verdict, has_oracle = SCENES[name]
    desc = make(kz.scenes)
    sc = kz.Scene(desc, device=0, lib=dev_lib)
    late(True)
    on, passes = traced_film(dev_lib, capfd, sc)
    print("%s: %s" % (name, passes))
    assert len(passes) == 1 and passes[0][2] == dense_entries(desc, W * H * SPP), passes
    if verdict is not None:
        assert passes[0][0] == verdict, passes
    if name == "black_room_nothing_survives":
        assert passes[0][1] == 0, passes
    elif verdict == COMPACTED:
        assert 0 < passes[0][1] <= passes[0][2], passes
    late(False)
    off, passes_off = traced_film(dev_lib, capfd, sc)
    assert [p[0] for p in passes_off] == ["in the pass's arrays: no compaction"] and passes_off[0][1] == passes[0][1], (passes_off, passes)
    assert np.array_equal(on, off)
    assert np.abs(on[..., :3]).max() > 0
    if has_oracle:
        assert np.array_equal(on, O.OracleScene(desc).render_canonical(threads=0))
    # the other ways a pass is launched: the same film with the compaction, and without it
    for flag in (True, False):
        late(flag)
        assert np.array_equal(film_of(sc, shadow_beside=2), on), flag
        assert np.array_equal(film_of(sc, pass_halves=2), on), flag
        assert np.array_equal(film_of(sc, pass_items=16384, passes_in_flight=2), on), flag
    # ... small passes decide one by one: each has a dense set of its own
    late(True)
    small, passes = traced_film(dev_lib, capfd, sc, pass_items=16384, passes_in_flight=2)
    assert np.array_equal(small, on) and len(passes) == W * H * SPP // 16384 and all(p[2] == dense_entries(desc, 16384) for p in passes), passes
    if verdict is not None:
        assert any(p[0] == verdict for p in passes), passes
    # counted renders: the same film and the same counters
    # (a counted render leaves the roulette-ahead test out and queues every bounce ray - more paths than the dense set holds in most of these scenes; with
    # kz_debug_rr_ahead(2) it takes the test, and its late bounces go the way the uncounted render's do)
    sc.set_stats(True)
    try:
        for ahead in (1, 2):
            dev_lib.kz_debug_rr_ahead(ahead)
            counted = {}
            for flag in (True, False):
                late(flag)
                sc.stats(reset=True)
                assert np.array_equal(film_of(sc), on), (ahead, flag)
                counted[flag] = sc.stats(reset=True)
            # (node visits and triangle tests vary from run to run with the order in which the workgroups of a shade launch filled the queues, compaction or
            # not - tests/test_gpu_configs.py leaves them out of its comparison for the same reason; here the two runs must agree on them to 2 %)
            loose = ("nodeVisits", "triTests")
            assert {k: v for k, v in counted[True].items() if k not in loose} == {k: v for k, v in counted[False].items() if k not in loose}, (ahead, counted)
            assert all(abs(counted[True][k] - counted[False][k]) <= 0.02 * counted[False][k] for k in loose), (ahead, counted)
            assert counted[True]["samples"] == W * H * SPP and counted[True]["rays"] >= counted[True]["samples"]
        late(True)
        _, passes = traced_film(dev_lib, capfd, sc)
        if verdict is not None:
            assert [p[0] for p in passes] == [verdict], passes
    finally:
        dev_lib.kz_debug_rr_ahead(1)
    sc.close()


def test_product_library_renders_the_same_films(gpu_lib, dev_lib, kz, late):
    """The product library has no switch: its films are the development library's without the compaction."""
    for name in ("dark_room_depth5", "bright_room_overflows", "invisible_panels"):
        desc = SCENES[name][0](kz.scenes)
        a = kz.Scene(desc, device=0)
        fa = film_of(a)
        a.close()
        late(False)
        b = kz.Scene(desc, device=0, lib=dev_lib)
        assert np.array_equal(film_of(b), fa), name
        b.close()
        late(True)


def test_a_shallow_path_is_not_compacted(dev_lib, kz, late, capfd):
    """maxDepth 3: no roulette bounce follows, the pass has no use for a dense set."""
    late(True)
    sc = kz.Scene(R.room(kz.scenes, 32, 32, 16, maxDepth=3), device=0, lib=dev_lib)
    _, passes = traced_film(dev_lib, capfd, sc)
    assert [p[0] for p in passes] == ["in the pass's arrays: no compaction"], passes
    sc.close()
