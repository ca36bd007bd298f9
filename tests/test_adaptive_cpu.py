"""Adaptive sampling (include_ext/kazen_mi355x_adaptive.h) without a GPU: the header against the library's exports, the structs' layout, the refusals that need no
device, the two pure host functions - the round schedule and the tile list - against Python restatements, and the test-only CPU reference
(tests/cpu_ref/kz_adaptive_ref.cpp) the GPU tests compare against: its classification against a numpy restatement on crafted films, its films of a uniform plane of
counts against the canonical films."""
import ctypes as C
import re

import numpy as np
import pytest

import adaptive_refs as A
from checks import c_layout, header_surface, refused, same_bits_strict

FRAMES = [(40, 24), (72, 40), (1921, 1)]
BLOCKS = [8, 16, 32, 64]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return A.lib(tmp_path_factory.mktemp("kzad"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    _, src = header_surface(kz, "include_ext/kazen_mi355x_adaptive.h", a.ADAPTIVE_EXPORTS, 8,
                            [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS, a.VARIANCE_EXPORTS, a.TEMPORAL_EXPORTS, a.MOTION_EXPORTS, a.RESPONSIVE_EXPORTS,
                             a.MATTE_EXPORTS, a.DEV_ONLY_EXPORTS], ["include", "include_ext/kazen_mi355x_matte.h"], ["kz_adaptive", "kzadaptive"])
    consts = {n: int(re.search(r"#define %s\s+(\d+)u?" % n, src).group(1)) for n in ("KZ_ADAPTIVE_CONVERGED", "KZ_ADAPTIVE_AT_CAP")}
    assert consts == {"KZ_ADAPTIVE_CONVERGED": a.KZ_ADAPTIVE_CONVERGED, "KZ_ADAPTIVE_AT_CAP": a.KZ_ADAPTIVE_AT_CAP} == {"KZ_ADAPTIVE_CONVERGED": A.CONVERGED, "KZ_ADAPTIVE_AT_CAP": A.AT_CAP}


def test_structs_as_gcc_sees_them(kz, tmp_path):
    a = kz.abi
    opts = ["threshold", "floor", "minSamples", "maxSamples", "step", "block", "outlierPermille", "flags"]
    block = ["samples", "noisy", "valid", "flags"]
    info = ["rounds", "blocks", "converged", "atCap", "samples", "bytes"]
    got = c_layout(tmp_path, "kazen_mi355x_adaptive.h", ["sizeof(KzAdaptiveOpts)", "sizeof(KzAdaptiveBlock)", "sizeof(KzAdaptiveInfo)"] +
                   ["offsetof(KzAdaptiveOpts, %s)" % f for f in opts] + ["offsetof(KzAdaptiveBlock, %s)" % f for f in block] + ["offsetof(KzAdaptiveInfo, %s)" % f for f in info],
                   include="include_ext")
    want = [C.sizeof(a.KzAdaptiveOpts), C.sizeof(a.KzAdaptiveBlock), C.sizeof(a.KzAdaptiveInfo)] + [getattr(a.KzAdaptiveOpts, f).offset for f in opts] + \
           [getattr(a.KzAdaptiveBlock, f).offset for f in block] + [getattr(a.KzAdaptiveInfo, f).offset for f in info]
    assert got == [str(x) for x in want]
    assert got[:3] == ["32", "16", "32"]
    d = np.dtype(a.ADAPTIVE_BLOCK_DTYPE)
    assert d.itemsize == 16 and [d.fields[f][1] for f in block] == [0, 4, 8, 12] and d == np.dtype(A.BLOCK_DTYPE)


# ---------------------------------------------------------------- refusals
def test_refusals_without_a_device(kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 8))
    sc.set_variance(True)
    bad_fields = [("threshold", dict(threshold=0.0)), ("threshold", dict(threshold=-1.0)), ("threshold", dict(threshold=float("nan"))), ("threshold", dict(threshold=float("inf"))),
                  ("floor", dict(threshold=0.1, floor=-0.5)), ("floor", dict(threshold=0.1, floor=float("inf"))), ("maxSamples", dict(threshold=0.1, max_samples=9)),
                  ("block", dict(threshold=0.1, block=12)), ("block", dict(threshold=0.1, block=128)), ("outlierPermille", dict(threshold=0.1, outlier_permille=1000)),
                  ("flags", dict(threshold=0.1, aflags=1))]
    for field, kw in bad_fields:
        refused(kz, lambda: sc.render_adaptive(**kw), a.KZ_ERR_INVALID_ARG, "kz_render_adaptive", "KzAdaptiveOpts." + field)
    refused(kz, lambda: sc.render_adaptive(0.1, sample_begin=2), a.KZ_ERR_INVALID_ARG, "sampleBegin")
    refused(kz, lambda: sc.render_adaptive(0.1, sample_end=4), a.KZ_ERR_INVALID_ARG, "sampleEnd")
    refused(kz, lambda: sc.render_adaptive(0.1, tiles=[(0, 0, 8, 8)]), a.KZ_ERR_INVALID_ARG, "tiles")
    refused(kz, lambda: sc.render_adaptive(0.1, accumulate=True), a.KZ_ERR_INVALID_ARG, "accumulate")
    refused(kz, lambda: sc.render_adaptive(0.1, pipeline=1), a.KZ_ERR_UNSUPPORTED, "pipeline")
    # NULL options, a dealer and packedOutput: through the C entry itself
    lib = sc.lib
    o, ad = a.KzRenderOpts(), kz.adaptive_opts(0.1)

    def call(opts, aopts):
        a.check(lib, lib.kz_render_adaptive(sc.h, opts, aopts, None))

    refused(kz, lambda: call(None, C.byref(ad)), a.KZ_ERR_INVALID_ARG, "KzRenderOpts")
    refused(kz, lambda: call(C.byref(o), None), a.KZ_ERR_INVALID_ARG, "KzAdaptiveOpts")
    counter = (C.c_uint32 * 1)()
    dealer = a.KzTileDealer(counter, 1, 1, None, 0, None, None)
    o.dealer = C.pointer(dealer)
    refused(kz, lambda: call(C.byref(o), C.byref(ad)), a.KZ_ERR_UNSUPPORTED, "dealer")
    o = a.KzRenderOpts()
    o.packedOutput = 1
    refused(kz, lambda: call(C.byref(o), C.byref(ad)), a.KZ_ERR_UNSUPPORTED, "packedOutput")
    # a bad field is named before the switch is looked at; the switch before any replica
    sc.set_variance(False)
    refused(kz, lambda: sc.render_adaptive(0.0), a.KZ_ERR_INVALID_ARG, "threshold")
    refused(kz, lambda: sc.render_adaptive(0.1), a.KZ_ERR_STATE, "kz_scene_set_variance(scene, 1) first")
    sc.set_variance(True)
    # well formed: the scene is on no device
    refused(kz, lambda: sc.render_adaptive(0.1), a.KZ_ERR_STATE, "kz_scene_upload")
    for read in (sc.adaptive_info, sc.adaptive_blocks, sc.adaptive_counts, sc.adaptive_stage_ms):
        refused(kz, read, a.KZ_ERR_STATE)
    # the test surface: bad options by name, then no device (or, where there is one, records)
    film = np.zeros((16, 16, 4), np.float32)
    refused(kz, lambda: kz.adaptive_classify_films(film, film, [1], 0.0), a.KZ_ERR_INVALID_ARG, "kz_adaptive_classify_films", "threshold")
    refused(kz, lambda: kz.adaptive_classify_films(film, film, [1], 0.1, block=9), a.KZ_ERR_INVALID_ARG, "block")
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.adaptive_classify_films(film, film, [1], 0.1), a.KZ_ERR_NO_DEVICE)


# ---------------------------------------------------------------- the schedule
SCHEDULES = [dict(), dict(min_samples=1), dict(min_samples=4, step=5), dict(min_samples=3, step=1), dict(min_samples=100, max_samples=7), dict(max_samples=1),
             dict(max_samples=1, step=3), dict(max_samples=100), dict(min_samples=7, max_samples=100), dict(max_samples=33, step=16), dict(min_samples=16, max_samples=16),
             dict(min_samples=1, step=0xFFFFFFFF), dict(step=1000)]


@pytest.mark.parametrize("scene_samples", [1, 7, 16, 64, 100, 4096, 0xFFFFFFFF])
def test_schedule_equals_the_restatement(kz, scene_samples):
    for kw in SCHEDULES:
        if kw.get("max_samples", 0) > scene_samples:
            refused(kz, lambda: kz.adaptive_schedule(scene_samples, **kw), kz.abi.KZ_ERR_INVALID_ARG, "maxSamples")
            continue
        if scene_samples == 0xFFFFFFFF and kw.get("step") in (1, 5, 1000) and not kw.get("max_samples"):
            continue                                                   # (billions of rounds)
        got = kz.adaptive_schedule(scene_samples, **kw)
        assert got == A.py_schedule(scene_samples, kw.get("min_samples", 0), kw.get("max_samples", 0), kw.get("step", 0)), (scene_samples, kw)
        assert got[-1] == (kw.get("max_samples") or scene_samples) and all(x < y for x, y in zip(got, got[1:]))
    assert kz.adaptive_schedule(64) == [16, 32, 64] and kz.adaptive_schedule(100, min_samples=3, step=40) == [3, 43, 83, 100]
    assert kz.adaptive_schedule(100) == [16, 32, 64, 100] and kz.adaptive_schedule(1) == [1] and kz.adaptive_schedule(64, min_samples=80, max_samples=20) == [20]
    refused(kz, lambda: kz.adaptive_schedule(0), kz.abi.KZ_ERR_INVALID_ARG, "sceneSamples")
    refused(kz, lambda: kz.adaptive_schedule(64, threshold=0.0), kz.abi.KZ_ERR_INVALID_ARG, "threshold")


@pytest.mark.parametrize("sampler", ["stratified", "correlated"])
def test_schedule_ends_at_the_samplers_rounded_count(kz, sampler):
    """The stratified and the correlated sampler round the sample count they are asked for: the cap is what kz_scene_sample_count says, and a cap beyond it is refused."""
    for asked in (10, 50, 64):
        sc = kz.Scene(kz.scenes.cornell_box(16, 16, asked, sampler=sampler))
        n = sc.sample_count
        got = kz.adaptive_schedule(n)
        assert got == A.py_schedule(n) and got[-1] == n
        sc.set_variance(True)
        refused(kz, lambda: sc.render_adaptive(0.1, max_samples=n + 1), kz.abi.KZ_ERR_INVALID_ARG, "maxSamples", str(n))
        refused(kz, lambda: sc.render_adaptive(0.1, max_samples=n), kz.abi.KZ_ERR_STATE, "kz_scene_upload")


# ---------------------------------------------------------------- the tile list
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("block", BLOCKS)
def test_tiles_equal_the_restatement(kz, frame, block):
    w, h = frame
    nbx, nby = (w + block - 1) // block, (h + block - 1) // block
    rng = np.random.default_rng(1000 * block + w)
    masks = [np.zeros(nbx * nby, np.uint8), np.ones(nbx * nby, np.uint8)] + [(rng.random(nbx * nby) < p).astype(np.uint8) for p in (0.2, 0.5, 0.8)]
    masks.append((rng.random(nbx * nby) < 0.5).astype(np.uint8) * 200)          # (any non-zero byte is active)
    for mask in masks:
        tiles = kz.adaptive_tiles(w, h, block, mask)
        assert tiles == A.py_tiles(w, h, block, mask)
        cover = np.zeros((h, w), np.int32)
        for x0, y0, tw, th in tiles:
            assert 0 <= x0 and 0 <= y0 and tw > 0 and th > 0 and x0 + tw <= w and y0 + th <= h                      # inside the frame
            assert x0 % 8 == 0 and y0 % 8 == 0 and (tw % 8 == 0 or x0 + tw == w) and (th % 8 == 0 or y0 + th == h)    # on the 8-pixel grid
            cover[y0:y0 + th, x0:x0 + tw] += 1
        want = np.repeat(np.repeat(mask.reshape(nby, nbx) != 0, block, 0), block, 1)[:h, :w]
        assert cover.max(initial=0) <= 1 and np.array_equal(cover == 1, want)                                        # disjoint, exactly the active blocks
        assert tiles == sorted(tiles, key=lambda t: (t[1], t[0]))                                                    # rows top to bottom, runs left to right
        for (x0, y0, tw, th), (x1, y1, _, _) in zip(tiles, tiles[1:]):
            assert y0 != y1 or x0 + tw < x1                                                                          # runs are maximal
    refused(kz, lambda: kz.adaptive_tiles(w, h, 12, np.ones(((w + 11) // 12) * ((h + 11) // 12))), kz.abi.KZ_ERR_INVALID_ARG, "block")


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("frame", FRAMES[:2])
@pytest.mark.parametrize("block", BLOCKS)
def test_reference_classification_equals_numpy(kz, ref, frame, block):
    w, h = frame
    seen = set()
    for border in (0, 2):
        for threshold in (0.05, 1e-18):
            film, moment, ns = A.crafted_films(w, h, border, block, threshold, seed=block + border)
            for permille in (0, 500):
                for cap in (0, 16):
                    o = kz.adaptive_opts(threshold, block=block, outlier_permille=permille, max_samples=cap)
                    got = A.ref_classify(ref, film, moment, ns, o, border)
                    want = A.np_classify(film, moment, ns, threshold, 0.0, cap, block, permille, border)
                    assert np.array_equal(got, want), (border, threshold, permille, cap, got[got != want], want[got != want])
                    assert (got[ns == 0] == np.zeros(1, A.BLOCK_DTYPE)).all() and (got["samples"] == ns).all()
                    seen |= set(got["flags"].tolist())
            if threshold == 1e-18:                                     # the bound is subnormal: flushed to zero it would make every pixel with a variance noisy
                fl = np.float32(0.01)
                assert 0 < float((np.float32(threshold) * np.float32(threshold)) * (fl * fl)) < np.finfo(np.float32).tiny
    if block <= 16:
        assert seen == {0, A.CONVERGED, A.AT_CAP}


def test_reference_films_of_a_uniform_plane_are_the_canonical_films(kz, ref):
    desc = kz.scenes.cornell_box(24, 16, 6, sampler="pmj02bn")
    r = A.AdaptiveRef(ref, desc)
    for n in (6, 4):
        plane = np.full((16, 24), n, np.uint32)
        assert same_bits_strict(r.film_counts(0, plane), r.film(0, n))
        assert same_bits_strict(r.film_counts(1, plane), r.moment_film(0, n))
    # ... and a plane that is not uniform differs from both, where the counts differ
    plane = np.full((16, 24), 6, np.uint32)
    plane[:, 12:] = 4
    f = r.film_counts(0, plane)
    assert not same_bits_strict(f, r.film(0, 6)) and not same_bits_strict(f, r.film(0, 4))
