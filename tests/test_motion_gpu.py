"""-m gpu: motion vectors for the denoiser's history (include/kazen_mi355x_motion.h) on the MI355X. kz_motion_ids equals the CPU reference's ids exactly - through
refits, camera edits and ragged frames; kz_denoise_motion_films - the result, the new history and v_last - has the bits of the C++ restatement
(tests/cpu_ref/kz_motion_ref.cpp) over frames, borders, guide subsets, histories, ids and row tables; a replica's chain of calls across kz_scene_set_transforms has the
bits of the reference chain on what it downloads; the history's life follows the header. Comparisons are same_bits / array_equal, never a tolerance."""
import copy

import numpy as np
import pytest

from checks import differing, same_bits_strict
from cpu_refs import lib, ref_denoise_motion, ref_ids
from film_cases import (GUIDES, H, MISS, SHORT_BOX, SPP, W, _looks_at_the_light, _orbit, _thinlens, random_history, random_ids, rotate, row_tables, synthetic_films,
                        synthetic_moment, translate, view_pairs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("motion", tmp_path_factory.mktemp("kzm"))


# ---------------------------------------------------------------- the ids
def _id_cases(kz):
    S = kz.scenes
    return {"cornell": S.cornell_box(W, H, 1), "textured": S.textured_scene(W, H, 1), "invisible light": _looks_at_the_light(kz), "thinlens": _thinlens(S.cornell_box(W, H, 1))}


@pytest.mark.parametrize("name", ["cornell", "textured", "invisible light", "thinlens"])
def test_ids_equal_the_reference(gpu_lib, kz, ref, name):
    """The device's ids are the reference's, every pixel: as created, after kz_scene_set_transforms of one mesh - the refit BVH2 is the one walked - and after
    kz_scene_set_camera. (Scene.desc follows the edits with the arithmetic the library uses, so the reference is handed the edited description.)"""
    d = _id_cases(kz)[name]
    sc = kz.Scene(d, device=0)
    assert sc.motion_info() == (0, (0, 0, 0))
    got, want = sc.motion_ids(), ref_ids(ref, sc.desc)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert sc.motion_info()[0] == W * H * 4
    n_meshes = len(d.meshes)
    hit = got[got != MISS]
    varied = name != "invisible light"                                # (that view is filled by the ceiling: moving it changes no id)
    assert hit.size and hit.max() < n_meshes and (len(np.unique(hit)) >= 3 or not varied)
    if name == "invisible light":                                     # the light is walked through: the ceiling behind it, never the light itself
        light = next(i for i, m in enumerate(d.meshes) if m["light"] is not None)
        assert not (got == light).any() and (got == 1).any()
    # the mesh most of the frame's centre shows, moved by a fifth of a unit and turned
    centre = got[H // 3:2 * H // 3, W // 3:2 * W // 3]
    m = max((i for i in range(n_meshes) if d.meshes[i]["light"] is None), key=lambda i: int((centre == i).sum()))
    sc.set_transforms({m: translate((0.2, 0.05, -0.1)) @ rotate((0, 1, 0), 0.3)})
    moved, want = sc.motion_ids(), ref_ids(ref, sc.desc)
    assert np.array_equal(moved, want), (name, "transform", int((moved != want).sum()))
    assert not varied or not np.array_equal(moved, got)
    start = copy.copy(d)
    start.camera = dict(sc.desc.camera)
    sc.set_camera({"toWorld": _orbit(kz, start, 4.0).camera["toWorld"]})
    turned, want = sc.motion_ids(), ref_ids(ref, sc.desc)
    assert np.array_equal(turned, want), (name, "camera", int((turned != want).sum()))
    assert not varied or not np.array_equal(turned, moved)


@pytest.mark.parametrize("frame", [(1, 1), (7, 5), (65, 3)])
def test_ids_of_ragged_frames(gpu_lib, kz, ref, frame):
    """Frames whose sides are no multiples of the 8 x 8 tile: one pixel, ragged tiles in both directions, one pixel into a second block of a row."""
    w, h = frame
    d = kz.scenes.cornell_box(w, h, 1)
    sc = kz.Scene(d, device=0)
    got, want = sc.motion_ids(), ref_ids(ref, d)
    assert got.shape == (h, w) and np.array_equal(got, want), (frame, got, want)
    assert (got != MISS).all()                                        # the box is closed


# ---------------------------------------------------------------- the films entry
def check(kz, ref, films, b, cur, prev, history, ids, rows, tag, **kw):
    got, gh, gv = kz.denoise_motion_films(*films, border=b, samples=4, current=cur, previous=prev, history=history, ids=ids, rows=rows, return_variance=True, **kw)
    want, wh, wv = ref_denoise_motion(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=history, ids=ids, rows=rows, **kw)
    assert same_bits_strict(got, want), (tag, kw, "film", differing(got, want))
    assert same_bits_strict(gh, wh), (tag, kw, "history", differing(gh, wh))
    assert same_bits_strict(gv, wv), (tag, kw, "variance", differing(gv, wv))
    return wh


# frames: test_temporal_gpu's
@pytest.mark.parametrize("frame", [(1, 1), (2, 2), (7, 5), (64, 33), (65, 3), (130, 20)])
def test_films_entry_has_the_references_bits(gpu_lib, kz, ref, frame):
    w, h = frame
    blended = 0                                                       # pixels of a MOVED row (flags 0) that found a history
    tables = row_tables(kz, w)
    for b in (0, 2):
        colour, albedo, normal, depth = synthetic_films(w, h, b, seed=200 * w + h + b)      # (with z = 0 pixels and pixels that are not valid)
        moment = synthetic_moment(colour, seed=3 * w + h + b)
        full = (colour, moment, albedo, normal, depth)
        views = view_pairs(kz, w, h)
        ids = random_ids(w, h, 4, seed=7 * w + h + b, misses=0.15 if w * h >= 64 else 0.0)
        junk = random_history(w, h, seed=w + h + b)
        own = check(kz, ref, full, b, views["same"][0], None, None, ids, tables["mixed"], (frame, b, "none"), iterations=1)
        check(kz, ref, full, b, views["same"][0], None, None, ids, tables["mixed"], (frame, b, "none"), iterations=5)
        lenient = dict(depth_tolerance=20.0, normal_tolerance=3.0, max_history=7)
        for tname, rows in tables.items():
            flags = np.array([r.flags for r in rows] + [1], np.uint32)[np.where(ids == MISS, 4, ids)]      # per pixel: its row's flags, STATIC for a miss
            for hname, hist in (("random", junk), ("own", own)):
                for vname in ("same", "fraction"):
                    kws = [dict(iterations=1, **lenient)]
                    if tname in ("static", "mixed"):
                        kws += [dict(iterations=1), dict(iterations=5, **lenient)] if vname == "fraction" else [dict(iterations=1)]
                    for kw in kws:
                        out = check(kz, ref, full, b, *views[vname], hist, ids, rows, (frame, b, tname, hname, vname), **kw)
                        blended += int(((out[..., 8] > 1) & (flags == 0)).sum())
                        assert not ((out[..., 8] > 1) & (flags == 2)).any(), (frame, b, tname)      # untracked: no history
        # every guide subset that holds depth, with and without demodulation
        for al in (False, True):
            for no in (False, True):
                films = (colour, moment, albedo if al else None, normal if no else None, depth)
                for demodulate in (True, False):
                    cur, prev = views["fraction"]
                    check(kz, ref, films, b, cur, prev, own, ids, tables["mixed"], (frame, b, al, no), iterations=1, demodulate=demodulate, depth_tolerance=20.0)
                    check(kz, ref, films, b, cur, prev, junk, ids, tables["mixed"], (frame, b, al, no), iterations=1, demodulate=demodulate, use_guides=False, normal_tolerance=3.0)
        check(kz, ref, full, b, *views["fraction"], own, ids, tables["mixed"], (frame, b, "guides"), iterations=1, guides=["normal", "depth"])
        # only misses, and no table
        check(kz, ref, full, b, *views["fraction"], own, np.full((h, w), MISS, np.uint32), tables["mixed"], (frame, b, "misses"), iterations=1, n_rows=0)
    assert blended > 0 or w * h < 4, frame


def test_identities_on_the_device(gpu_lib, kz):
    """All rows STATIC (and any ids) gives kz_denoise_temporal_films' bits; maxHistory = 1 gives kz_denoise_variance_films' bits whatever the rows."""
    b, w, h = 2, 70, 45
    colour, albedo, normal, depth = synthetic_films(w, h, b, seed=9)
    moment = synthetic_moment(colour, seed=10)
    films = (colour, moment, albedo, normal, depth)
    cur, prev = view_pairs(kz, w, h)["fraction"]
    ids, tables = random_ids(w, h, 4, seed=2), row_tables(kz, w)
    _, own = kz.denoise_motion_films(*films, border=b, samples=8, current=prev, ids=ids, rows=tables["static"])      # the frame's own history, from the other view
    for history in (None, own):
        for kw in (dict(), dict(iterations=3, demodulate=False, sigma_variance=1.5, depth_tolerance=20.0, normal_tolerance=3.0)):
            want = kz.denoise_temporal_films(*films, border=b, samples=8, current=cur, previous=prev, history=history, return_variance=True, **kw)
            got = kz.denoise_motion_films(*films, border=b, samples=8, current=cur, previous=prev, history=history, ids=ids, rows=tables["static"], return_variance=True, **kw)
            assert all(same_bits_strict(g, x) for g, x in zip(got, want)), (history is None, kw)
            if history is not None:
                other = kz.denoise_motion_films(*films, border=b, samples=8, current=cur, previous=prev, history=history, ids=ids, rows=tables["mixed"], return_variance=True, **kw)
                assert not same_bits_strict(other[1], want[1])               # (the rows matter)
            want, wv = kz.denoise_variance_films(*films, border=b, samples=8, return_variance=True, **{k: v for k, v in kw.items() if "tolerance" not in k})
            got, hist1, gv = kz.denoise_motion_films(*films, border=b, samples=8, current=cur, previous=prev, history=history, ids=ids, rows=tables["mixed"], max_history=1,
                                                     return_variance=True, **kw)
            assert same_bits_strict(got, want) and same_bits_strict(gv, wv) and set(np.unique(hist1[..., 8])) == {0.0, 1.0}


# ---------------------------------------------------------------- a replica across transform edits
def _films(sc):
    return [sc.film(), sc.moment_film()] + [sc.aov_film(g) for g in GUIDES]


def _scene(kz, spp):
    sc = kz.Scene(kz.scenes.cornell_box(W, H, spp), device=0)
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    return sc


def _box_at(f):
    """The short box's matrix in frame f: slid across the floor and turned a little."""
    return (translate((-0.06 * f, 0.0, 0.04 * f)) @ rotate((0, 1, 0), 0.05 * f)).astype(np.float32)


def test_replica_chain_equals_the_reference_chain(gpu_lib, kz, ref):
    """Three frames of SPP samples; each moves the short box by kz_scene_set_transforms and turns the camera by 1.5 degrees. kz_denoise_motion's result and history
    have the bits of the reference chain fed the downloaded films, motion_ids() and kz_motion_rows of the matrices this test keeps itself; the history grows
    (frames = f + 1) where kz_denoise_temporal, on the same sequence, starts afresh after every transform (pinned old behaviour)."""
    sc, old = _scene(kz, 3 * SPP), _scene(kz, 3 * SPP)
    n_meshes = len(sc.desc.meshes)
    b = sc.border
    start = copy.copy(sc.desc)
    start.camera = dict(sc.desc.camera)
    mats = np.tile(np.eye(4, dtype=np.float32), (n_meshes, 1, 1))
    history, prev, prev_mats = None, None, None
    for f in range(3):
        for s in (sc, old):
            if f:
                s.set_transforms({SHORT_BOX: _box_at(f)})
                s.set_camera({"toWorld": _orbit(kz, start, 1.5 * f).camera["toWorld"]})
            s.render(sample_begin=SPP * f, sample_end=SPP * (f + 1), accumulate=False)
        mats[SHORT_BOX] = _box_at(f) if f else np.eye(4, dtype=np.float32)
        films = _films(sc)
        sc.denoise_motion()
        old.denoise_temporal()
        ids = sc.motion_ids()
        view = kz.temporal_view(sc.desc.camera)
        rows = kz.motion_rows(mats, prev_mats)
        want, history, _ = ref_denoise_motion(ref, kz, *films, border=b, samples=SPP, current=view, previous=prev, history=history, ids=ids, rows=rows)
        prev, prev_mats = view, mats.copy()
        got, gh = sc.denoised_film(), sc.temporal_history()
        assert same_bits_strict(got, want), (f, differing(got, want))
        assert same_bits_strict(gh, history), (f, differing(gh, history))
        assert sc.temporal_info() == (2 * W * H * 36, f + 1)
        assert old.temporal_info() == (2 * W * H * 36, 1)             # kz_denoise_temporal: afresh after every transform
        for x, y in zip(films, _films(sc)):                           # the films do not notice
            assert same_bits_strict(x, y)
        if f:
            assert sc.motion_info() == (W * H * 4 + n_meshes * 96, (n_meshes - 1, 1, 0))
            assert rows[SHORT_BOX].flags == 0
            on_box = ids == SHORT_BOX
            found_box, found = float((history[..., 8][on_box] > 1).mean()), float((history[..., 8] > 1).mean())
            print("motion chain frame %d: %.1f %% of the box's %d pixels and %.1f %% of all pixels found a history" % (f + 1, 100 * found_box, int(on_box.sum()), 100 * found))
            assert on_box.any() and found_box > 0 and found > 0
            assert (old.temporal_history()[..., 8] <= 1).all()
    assert sc.denoised_srgb8().shape == (H, W, 3)


# ---------------------------------------------------------------- lifecycle
def test_lifecycle(gpu_lib, kz, ref):
    d = kz.scenes.cornell_box(W, H, 2 * SPP)                          # (the frames below take its two halves in turn)
    sc = kz.Scene(d, device=0)
    n_meshes = len(d.meshes)
    sc.render()
    plain = sc.film()
    base = {m: (d.meshes[m]["V"].copy(), None if d.meshes[m]["N"] is None else d.meshes[m]["N"].copy()) for m in (SHORT_BOX,)}
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    tp_bytes, mt_bytes = 2 * W * H * 36, W * H * 4 + n_meshes * 96
    N = lambda: sc.temporal_history()[..., 8]

    def frame(call, f):
        sc.render(sample_begin=SPP * (f % 2), sample_end=SPP * (f % 2 + 1), accumulate=False)
        call()

    # nothing has moved: the call is kz_denoise_temporal, no id plane
    frame(sc.denoise_motion, 0)
    frame(sc.denoise_motion, 1)
    assert sc.temporal_info() == (tp_bytes, 2) and sc.motion_info() == (0, (n_meshes, 0, 0))
    # a transform keeps the history: the box's pixels blend with where the box was
    sc.set_transforms({SHORT_BOX: translate((-0.05, 0, 0.03))})
    frame(sc.denoise_motion, 2)
    assert sc.temporal_info() == (tp_bytes, 3) and sc.motion_info() == (mt_bytes, (n_meshes - 1, 1, 0))
    ids = sc.motion_ids()
    assert (N()[ids == SHORT_BOX] > 1).any() and N().max() == 3
    # kz_scene_set_vertices restarts kz_denoise_motion as well - even one that moves nothing
    mesh = sc.desc.meshes[0]
    sc.set_vertices({0: mesh["V"] if mesh["N"] is None else (mesh["V"], mesh["N"])})
    frame(sc.denoise_motion, 3)
    assert sc.temporal_info() == (tp_bytes, 1) and N().max() == 1 and sc.motion_info()[1] == (n_meshes, 0, 0)
    # a projective matrix: that mesh's pixels take no history, the others blend on; left alone it is static in the next frame
    proj = translate((-0.05, 0, 0.03))
    proj[3, 1] = 0.01
    sc.set_transforms({SHORT_BOX: proj})
    frame(sc.denoise_motion, 4)
    ids = sc.motion_ids()
    assert sc.temporal_info() == (tp_bytes, 2) and sc.motion_info() == (mt_bytes, (n_meshes - 1, 0, 1))
    assert (ids == SHORT_BOX).any() and (N()[ids == SHORT_BOX] == 1).all() and (N()[ids != SHORT_BOX] == 2).mean() > 0.5
    frame(sc.denoise_motion, 5)
    assert sc.motion_info()[1] == (n_meshes, 0, 0) and (N()[ids == SHORT_BOX] == 2).any()
    # a kz_denoise_temporal history is picked up by kz_denoise_motion after a transform; kz_denoise_temporal itself starts afresh after one
    sc.temporal_reset()
    assert sc.temporal_info() == (0, 0) and sc.motion_info() == (0, (0, 0, 0))      # kz_temporal_reset frees the id plane and the rows
    sc.set_transforms({SHORT_BOX: translate((0, 0, 0))})              # (affine again)
    frame(sc.denoise_temporal, 6)
    sc.set_transforms({SHORT_BOX: translate((0.04, 0, 0.0))})
    frame(sc.denoise_motion, 7)
    ids = sc.motion_ids()
    assert sc.temporal_info() == (tp_bytes, 2) and sc.motion_info() == (mt_bytes, (n_meshes - 1, 1, 0)) and (N()[ids == SHORT_BOX] == 2).any()
    sc.set_transforms({SHORT_BOX: translate((0.08, 0, 0.0))})
    frame(sc.denoise_temporal, 8)
    assert sc.temporal_info() == (tp_bytes, 1)
    frame(sc.denoise_motion, 9)                                       # ... and its history knows where the box was
    assert sc.temporal_info() == (tp_bytes, 2) and sc.motion_info()[1] == (n_meshes, 0, 0)
    # refusals with a device, under the call's own name
    with pytest.raises(kz.abi.KzError) as e:
        sc.denoise_motion(demodulate=False)
    assert e.value.code == kz.abi.KZ_ERR_STATE and "kz_denoise_motion" in str(e.value) and "kz_temporal_reset" in str(e.value)
    buf = np.zeros(W * H + 1, np.uint32)
    assert sc.lib.kz_motion_ids(sc.h, -1, buf.ctypes.data_as(kz.abi.u32p), W * H + 1) == kz.abi.KZ_ERR_INVALID_ARG
    assert sc.lib.kz_motion_info(sc.h, -1, None, None) == kz.abi.KZ_ERR_INVALID_ARG
    # a plain render's film has the bits it had before any of this
    sc.temporal_reset()
    sc.set_aovs(())
    sc.set_variance(False)
    V, Nrm = base[SHORT_BOX]
    sc.set_vertices({SHORT_BOX: V if Nrm is None else (V, Nrm)})
    sc.render()
    assert np.array_equal(sc.film(), plain)
    assert sc.motion_info() == (0, (0, 0, 0))
