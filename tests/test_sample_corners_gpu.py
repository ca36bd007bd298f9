"""-m gpu: both pipelines of kz_render and the per-sample entry, sample by sample, at the corners of the samplers' domain (cases and instrument: tests/sample_corners.py;
the instrument on the oracle alone: tests/test_sample_corners_cpu.py).

Every check runs three ways - kz_render with pipeline 0 (the wavefront kernels, the default), with pipeline 1 (the megakernel), and kz_render_samples - except the
pass schedules and camera-ray kernels, which are options of pipeline 0 alone and are held there. Every assertion is equality of bits with the oracle: whole
films against OracleScene.render_canonical of the same range (and tiles), per-sample rows against OracleScene.render_samples. Two NaNs count as equal, +0 and -0 do not; there is no tolerance in this module. Under the box filter of radius 0.5 a one-sample film
is that sample of every pixel, so a failure names the pixel, the sample index, the sampler, its count and the seed (sample_corners.report)."""
import pytest

import sample_corners as SC
from checks import same_bits

pytestmark = pytest.mark.gpu
PIPELINES = ((0, "kz_render pipeline 0 (wavefront)"), (1, "kz_render pipeline 1 (megakernel)"))


def _ids(cases):
    return [c.id for c in cases]


def _pair(kz, O, case):
    desc = SC.scene_of(kz.scenes, case)
    sc, ora = kz.Scene(desc, device=0), O.OracleScene(desc)
    assert sc.border == ora.border == 0
    assert sc.sample_count == ora.sample_count == case.count, (case.id, sc.sample_count, ora.sample_count)
    return sc, ora


def _hold_films(case, sc, ora, ranges, tiles=None, wave_shaped=False, **render_kw):
    """Every range's film from both pipelines against the oracle's; the oracle's film is computed once per range."""
    for b, e in ranges:
        want = SC.range_film(ora, b, e, tiles=tiles)
        for pipeline, name in PIPELINES:
            got = SC.range_film(sc, b, e, tiles=tiles, pipeline=pipeline, **render_kw)
            assert same_bits(got, want), SC.report(case, ora, b, e, got, want, name + (" %r" % (render_kw,) if render_kw else ""))
            if wave_shaped and pipeline == 0:
                assert sc.last_pass_info()["sppPerPass"] % 64 == 0, sc.last_pass_info()      # a wave of kz_wf_generate is one pixel: its (S & 63) == 0 branch


def _hold_samples(case, sc, ora, ks, tiles=None, w=SC.W, h=SC.H):
    """kz_render_samples (the megakernel, per sample) of every pixel at every k against the oracle's render_samples: position and radiance."""
    pxy = SC.pixel_grid(w, h, tiles)
    for k in ks:
        got, want = SC.samples_of(sc, pxy, k), SC.samples_of(ora, pxy, k)
        assert same_bits(got, want), SC.report_samples(case, ora, pxy, k, got, want, "kz_render_samples")


@pytest.mark.parametrize("case", SC.COUNT_CASES, ids=_ids(SC.COUNT_CASES))
def test_single_samples_across_counts_and_seeds(gpu_lib, kz, O, case):
    """All four samplers x the counts {1, 100, 1000, 2048, 4097, 65536} after rounding - a power of 4, a power of 2 only, neither: permuteIdx with and without its
    modulo, next1D with and without invSpp, the jump table, the pmj pixel table and index %= 65536 at their last entries - at k in {0, 1, 63, 64, n/2, n-2, n-1},
    under seeds up to 64 bits wide (the tail bytes of Hash(p, dim, seed))."""
    sc, ora = _pair(kz, O, case)
    ks = SC.sample_indices(case.count)
    _hold_films(case, sc, ora, [(k, k + 1) for k in ks])
    _hold_samples(case, sc, ora, ks)
    sc.close()


@pytest.mark.parametrize("case", SC.WAVE_CASES, ids=_ids(SC.WAVE_CASES))
def test_wave_shaped_ranges(gpu_lib, kz, O, case):
    """[0, 64), [n - 64, n) and [n - 128, n) at 4096 and 65536 samples: every wave of kz_wf_generate is one pixel (the pass's samples per pixel are asserted to be a
    multiple of 64), and the film is the tap sums in sample order."""
    sc, ora = _pair(kz, O, case)
    _hold_films(case, sc, ora, SC.wave_ranges(case.count), wave_shaped=True)
    _hold_samples(case, sc, ora, [case.count - 64, case.count - 1])
    sc.close()


@pytest.mark.parametrize("case", SC.DIM_CASES, ids=_ids(SC.DIM_CASES))
def test_dimension_bookkeeping_of_deep_paths(gpu_lib, kz, O, case):
    """maxDepth 12 at count 100: pmj02bn instances >= 5 and the roulette dimension of bounces > 3 (wfPmjDim against the megakernel's and the oracle's running counter; the
    first-lane counter of wfLoadSampler), with and without regularization, through a thin lens, without lights under a background (a lone sphere; the open cornell
    box), and with the light invisible to camera rays (the walk-through continuation) and visible."""
    sc, ora = _pair(kz, O, case)
    _hold_films(case, sc, ora, [(k, k + 1) for k in SC.DIM_KS] + [SC.DIM_RANGE])
    _hold_samples(case, sc, ora, SC.DIM_KS)
    sc.close()


@pytest.mark.parametrize("case", SC.BIG_CASES, ids=_ids(SC.BIG_CASES))
def test_pixels_far_from_the_origin(gpu_lib, kz, O, case):
    """A 2048 x 1536 frame rendered over tiles at its last row and column, past the 128-texel blue-noise period and past the pmj pixel tile, at k = 999 of 1000."""
    sc, ora = _pair(kz, O, case)
    _hold_films(case, sc, ora, [(SC.BIG_K, SC.BIG_K + 1)], tiles=SC.BIG_TILES)
    _hold_samples(case, sc, ora, [SC.BIG_K], tiles=SC.BIG_TILES, w=SC.BIG_W, h=SC.BIG_H)
    sc.close()


@pytest.mark.parametrize("case", SC.SCHEDULE_CASES, ids=_ids(SC.SCHEDULE_CASES))
def test_schedules_leave_the_samples_alone(gpu_lib, kz, O, case):
    """Sample 65535 of 65536 and the range [n - 64, n) under passes of 64 items, passes of 4096 items three in flight, and each of the three camera-ray kernels: the same
    film, the oracle's. (Pipeline 0 only: passes of items and the camera-ray kernels are the wavefront pipeline's; the same cases go three ways in
    test_single_samples_across_counts_and_seeds and test_wave_shaped_ranges.)"""
    sc, ora = _pair(kz, O, case)
    n = case.count
    wants = {r: SC.range_film(ora, *r) for r in ((n - 1, n), (n - 64, n))}
    for kw in SC.SCHEDULES:
        for (b, e), want in wants.items():
            got = SC.range_film(sc, b, e, **kw)
            assert same_bits(got, want), SC.report(case, ora, b, e, got, want, "kz_render %r" % (kw,))
    sc.close()
