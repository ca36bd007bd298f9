"""-m gpu: the fast history and the clamp of include/kazen_mi355x_responsive.h on the MI355X. kz_denoise_responsive_films - the picture, the new history, v_last and
the fast plane - has the bits of the C++ restatement (tests/cpu_ref/kz_responsive_ref.cpp) over frames, borders, histories, fast planes, radii, guide subsets and row
tables; the header's identities hold between the device's own calls; a replica's chain across a camera turn, a mesh transform and a light edit has the bits of the
reference chain; mixing the calls on one history and the fast plane's life follow the header. Comparisons are same_bits / array_equal, never a tolerance."""
import copy

import numpy as np
import pytest

from checks import differing, same_bits_strict
from cpu_refs import lib, ref_denoise_motion, ref_denoise_responsive
from film_cases import (FRAMES, GUIDES, LAMP, MISS, NEW_LIGHT, SHORT_BOX, _orbit, random_fast, random_history, random_ids, rotate, row_tables, synthetic_films, synthetic_moment,
                        translate, view_pairs)

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 72, 1


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("responsive", tmp_path_factory.mktemp("kzr"))


def check(kz, ref, films, b, cur, prev, history, fast, ids, rows, tag, **kw):
    got, gh, gf, gv = kz.denoise_responsive_films(*films, border=b, samples=4, current=cur, previous=prev, history=history, fast=fast, ids=ids, rows=rows, return_variance=True, **kw)
    want, wh, wf, wv = ref_denoise_responsive(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=history, fast=fast, ids=ids, rows=rows, **kw)
    assert same_bits_strict(got, want), (tag, kw, "film", differing(got, want))
    assert same_bits_strict(gh, wh), (tag, kw, "history", differing(gh, wh))
    assert same_bits_strict(gv, wv), (tag, kw, "variance", differing(gv, wv))
    assert same_bits_strict(gf, wf), (tag, kw, "fast", differing(gf, wf))
    return wh, wf


# frames: one pixel; more rows than a block of pass B (4); more columns than one (64); several blocks on both axes, so that aprons cross tiles
@pytest.mark.parametrize("frame", FRAMES)
def test_films_entry_has_the_references_bits(gpu_lib, kz, ref, frame):
    w, h = frame
    clamped = 0                                                       # pixels whose count the clamp changed
    tables = row_tables(kz, w)
    lenient = dict(depth_tolerance=20.0, normal_tolerance=3.0)
    for b in (0, 2):
        colour, albedo, normal, depth = synthetic_films(w, h, b, seed=300 * w + h + b)      # (with z = 0 pixels and pixels that are not valid)
        moment = synthetic_moment(colour, seed=5 * w + h + b)
        full = (colour, moment, albedo, normal, depth)
        views = view_pairs(kz, w, h)
        ids = random_ids(w, h, 4, seed=11 * w + h + b, misses=0.15 if w * h >= 64 else 0.0)
        junk = random_history(w, h, seed=w + h + b)
        junk_fast = random_fast(junk, seed=2 * w + h + b)
        # without a history (a fast plane given is ignored), then with the call's own history and fast plane, and with random ones
        own, own_fast = check(kz, ref, full, b, views["same"][0], None, None, None, ids, tables["mixed"], (frame, b, "none"), iterations=1)
        check(kz, ref, full, b, views["same"][0], None, None, junk_fast, ids, tables["mixed"], (frame, b, "none, fast given"), iterations=5)
        for tname in ("static", "mixed"):                             # a static row and moved ones
            rows = tables[tname]
            for hname, hist, fast in (("own", own, own_fast), ("own, absent", own, None), ("random", junk, junk_fast), ("random, absent", junk, None)):
                for vname in ("same", "fraction"):
                    for kw in (dict(iterations=1, fast_history=2, clamp_sigma=0.5, radius=1, **lenient), dict(iterations=1, fast_history=3, clamp_sigma=1.0, radius=2, **lenient),
                               dict(iterations=1, fast_history=2, clamp=False, **lenient), dict(iterations=1)):
                        wh, _ = check(kz, ref, full, b, *views[vname], hist, fast, ids, rows, (frame, b, tname, hname, vname), **kw)
                        if kw.get("clamp", True) and "fast_history" in kw:
                            off = ref_denoise_responsive(ref, kz, *full, border=b, samples=4, current=views[vname][0], previous=views[vname][1], history=hist, fast=fast,
                                                         ids=ids, rows=rows, **dict(kw, clamp=False))[1]
                            clamped += int((wh[..., 8] != off[..., 8]).sum())
        check(kz, ref, full, b, *views["fraction"], junk, junk_fast, ids, tables["mixed"], (frame, b, "five iterations"), iterations=5, fast_history=2, clamp_sigma=0.5, **lenient)
        # guide subsets that hold depth, with and without demodulation
        for al, no, demodulate in ((False, False, True), (True, False, False), (False, True, True), (True, True, False)):
            films = (colour, moment, albedo if al else None, normal if no else None, depth)
            check(kz, ref, films, b, *views["fraction"], junk, junk_fast, ids, tables["mixed"], (frame, b, al, no), iterations=1, demodulate=demodulate, fast_history=2, clamp_sigma=0.5,
                  **lenient)
        check(kz, ref, full, b, *views["fraction"], junk, junk_fast, ids, tables["mixed"], (frame, b, "guides"), iterations=1, guides=["normal", "depth"], use_guides=False, fast_history=2)
        # only misses, and no table
        check(kz, ref, full, b, *views["fraction"], junk, junk_fast, np.full((h, w), MISS, np.uint32), tables["mixed"], (frame, b, "misses"), iterations=1, n_rows=0, fast_history=2)
    assert clamped > 0 or w * h < 4, frame


def test_identities_on_the_device(gpu_lib, kz):
    """CLAMP_OFF gives kz_denoise_motion_films' bits - picture, history, v_last -; a first call gives kz_denoise_variance_films' bits, and its fast plane is (e, v)."""
    b, w, h = 2, 70, 45
    colour, albedo, normal, depth = synthetic_films(w, h, b, seed=19)
    moment = synthetic_moment(colour, seed=20)
    films = (colour, moment, albedo, normal, depth)
    cur, prev = view_pairs(kz, w, h)["fraction"]
    ids, tables = random_ids(w, h, 4, seed=3), row_tables(kz, w)
    junk = random_history(w, h, seed=4)
    fast = random_fast(junk, seed=5)
    for kw in (dict(), dict(iterations=3, demodulate=False, sigma_variance=1.5, depth_tolerance=20.0, normal_tolerance=3.0)):
        common = dict(border=b, samples=8, current=cur, previous=prev, ids=ids, rows=tables["mixed"], return_variance=True, **kw)
        want = kz.denoise_motion_films(*films, history=junk, **common)
        for f, more in ((fast, dict(fast_history=2, clamp_sigma=0.3, radius=1)), (None, dict())):
            got = kz.denoise_responsive_films(*films, history=junk, fast=f, clamp=False, **more, **common)
            assert same_bits_strict(got[0], want[0]) and same_bits_strict(got[1], want[1]) and same_bits_strict(got[3], want[2]), (kw, more)
        on = kz.denoise_responsive_films(*films, history=junk, fast=fast, fast_history=2, clamp_sigma=0.3, radius=1, **common)
        assert not same_bits_strict(on[1], want[1])                          # (the clamp matters)
        want, wv = kz.denoise_variance_films(*films, border=b, samples=8, return_variance=True, **{k: v for k, v in kw.items() if "tolerance" not in k})
        got, hist, f1, gv = kz.denoise_responsive_films(*films, fast=fast, **dict(common, previous=None))
        assert same_bits_strict(got, want) and same_bits_strict(gv, wv) and set(np.unique(hist[..., 8])) == {0.0, 1.0}
        assert same_bits_strict(f1, hist[..., :4])


# ---------------------------------------------------------------- a replica
def _films(sc):
    return [sc.film(), sc.moment_film()] + [sc.aov_film(g) for g in GUIDES]


def _scene(kz, spp):
    sc = kz.Scene(kz.scenes.cornell_box(W, H, spp), device=0)
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    return sc


def test_replica_chain_equals_the_reference_chain(gpu_lib, kz, ref):
    """Six frames of 1 spp: the camera turns by 1.5 degrees each frame, the short box moves at frame 3, the lamp changes colour at frame 5 (kz_scene_set_lights).
    kz_denoise_responsive's picture, history and fast plane have the bits of the reference chain fed the downloaded films, motion_ids() and kz_motion_rows of the
    matrices this test keeps itself - with a fast history of 2 and a narrow clamp, so that the clamp bites -; after the light edit the history counts on: nothing was
    reset."""
    sc = _scene(kz, 6 * SPP)
    n_meshes = len(sc.desc.meshes)
    b = sc.border
    start = copy.copy(sc.desc)
    start.camera = dict(sc.desc.camera)
    box = (translate((-0.08, 0.0, 0.05)) @ rotate((0, 1, 0), 0.1)).astype(np.float32)
    mats = np.tile(np.eye(4, dtype=np.float32), (n_meshes, 1, 1))
    ropts = dict(fast_history=2, clamp_sigma=1.0, radius=2)
    history = fast = prev = prev_mats = None
    bitten = 0
    assert sc.responsive_info() == 0
    for f in range(6):
        if f:
            sc.set_camera({"toWorld": _orbit(kz, start, 1.5 * f).camera["toWorld"]})
        if f == 3:
            sc.set_transforms({SHORT_BOX: box})
            mats[SHORT_BOX] = box
        if f == 5:
            sc.set_lights({LAMP: kz.scenes.area(NEW_LIGHT["color"], NEW_LIGHT["intensity"], False)})
        sc.render(sample_begin=SPP * f, sample_end=SPP * (f + 1), accumulate=False)
        films = _films(sc)
        sc.denoise_responsive(**ropts)
        ids = sc.motion_ids()
        view = kz.temporal_view(sc.desc.camera)
        rows = kz.motion_rows(mats, prev_mats)
        kw = dict(border=b, samples=SPP, current=view, previous=prev, history=history, fast=fast, ids=ids, rows=rows)
        off = ref_denoise_responsive(ref, kz, *films, clamp=False, **ropts, **kw)[1]
        want, history, fast, _ = ref_denoise_responsive(ref, kz, *films, **ropts, **kw)
        bitten += int((off[..., 8] != history[..., 8]).sum())
        prev, prev_mats = view, mats.copy()
        got, gh, gf = sc.denoised_film(), sc.temporal_history(), sc.responsive_fast()
        assert same_bits_strict(got, want), (f, differing(got, want))
        assert same_bits_strict(gh, history), (f, differing(gh, history))
        assert same_bits_strict(gf, fast), (f, differing(gf, fast))
        assert sc.temporal_info() == (2 * W * H * 36, f + 1)          # (f = 5: the light edit reset nothing)
        assert sc.responsive_info() == 2 * W * H * 16
    assert bitten > 0
    assert sc.denoised_srgb8().shape == (H, W, 3)


def test_mixing_calls_on_one_history(gpu_lib, kz, ref):
    """A kz_denoise_motion between two kz_denoise_responsive calls: the third call reads the history the second stored and treats the fast plane as absent - the
    reference called that way has its bits, the reference handed the first call's fast plane has not."""
    sc = _scene(kz, 3 * SPP)
    b = sc.border
    n_meshes = len(sc.desc.meshes)
    rows, view = kz.motion_rows(np.tile(np.eye(4, dtype=np.float32), (n_meshes, 1, 1)), None), kz.temporal_view(sc.desc.camera)
    ropts = dict(fast_history=2, clamp_sigma=1.0)
    frames = []
    for f in range(3):
        sc.render(sample_begin=SPP * f, sample_end=SPP * (f + 1), accumulate=False)
        frames.append(_films(sc))
        if f == 1:
            sc.denoise_motion()
            with pytest.raises(kz.abi.KzError) as e:                  # the plane is there, but it is not this history's
                sc.responsive_fast()
            assert e.value.code == kz.abi.KZ_ERR_STATE
        else:
            sc.denoise_responsive(**ropts)
    ids = sc.motion_ids()
    kw = dict(border=b, samples=SPP, current=view, ids=ids, rows=rows)
    _, h0, f0, _ = ref_denoise_responsive(ref, kz, *frames[0], **ropts, **kw)
    _, h1, _ = ref_denoise_motion(ref, kz, *frames[1], previous=view, history=h0, **kw)
    want, h2, f2, _ = ref_denoise_responsive(ref, kz, *frames[2], previous=view, history=h1, fast=None, **ropts, **kw)
    assert same_bits_strict(sc.denoised_film(), want) and same_bits_strict(sc.temporal_history(), h2) and same_bits_strict(sc.responsive_fast(), f2)
    other = ref_denoise_responsive(ref, kz, *frames[2], previous=view, history=h1, fast=f0, **ropts, **kw)
    assert not same_bits_strict(other[2], f2)
    assert sc.temporal_info() == (2 * W * H * 36, 3)


def test_lifecycle(gpu_lib, kz):
    sc = _scene(kz, 2 * SPP)
    a = kz.abi
    assert sc.responsive_info() == 0
    buf = np.zeros(W * H * 4, np.float32)
    assert sc.lib.kz_responsive_download(sc.h, -1, buf.ctypes.data_as(a.f32p), buf.size) == a.KZ_ERR_STATE      # before the first call
    sc.render(sample_begin=0, sample_end=SPP, accumulate=False)
    sc.denoise_motion()
    assert sc.responsive_info() == 0 and sc.temporal_info() == (2 * W * H * 36, 1)      # a replica that only calls kz_denoise_motion holds no fast plane
    assert sc.lib.kz_responsive_download(sc.h, -1, buf.ctypes.data_as(a.f32p), buf.size) == a.KZ_ERR_STATE
    sc.denoise_responsive()
    assert sc.responsive_info() == 2 * W * H * 16 and sc.temporal_info() == (2 * W * H * 36, 2)
    fast, hist = sc.responsive_fast(), sc.temporal_history()
    assert fast.shape == (H, W, 4) and np.isfinite(fast).all() and not fast[hist[..., 8] == 0].any()
    assert sc.lib.kz_responsive_download(sc.h, -1, buf.ctypes.data_as(a.f32p), buf.size - 4) == a.KZ_ERR_INVALID_ARG
    sc.temporal_reset()
    assert sc.responsive_info() == 0 and sc.temporal_info() == (0, 0)
    assert sc.lib.kz_responsive_download(sc.h, -1, buf.ctypes.data_as(a.f32p), buf.size) == a.KZ_ERR_STATE      # after a reset
    sc.render(sample_begin=SPP, sample_end=2 * SPP, accumulate=False)
    sc.denoise_responsive()
    assert sc.responsive_info() == 2 * W * H * 16 and sc.temporal_info() == (2 * W * H * 36, 1)
    with pytest.raises(a.KzError) as e:                               # refusals with a device, under the call's own name
        sc.denoise_responsive(demodulate=False)
    assert e.value.code == a.KZ_ERR_STATE and "kz_denoise_responsive" in str(e.value) and "kz_temporal_reset" in str(e.value)
