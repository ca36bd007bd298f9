"""The instrument of tests/test_sample_corners_gpu.py, held to what it claims on the oracle alone (no GPU): under the box filter of radius 0.5 the film of a
one-sample range IS that sample of every pixel, and the film of a longer range is the float32 sum of its samples in sample order. With this established a
device film that differs from OracleScene.render_canonical is a sample that differs, not an artefact of the film. The module also asserts the facts the case
table of tests/sample_corners.py relies on: the counts after each sampler's rounding, and that bits 32 .. 63 of the seed reach every case's stream."""
import numpy as np
import pytest

import sample_corners as SC

EDGE_SHARE = 0.01                # samples not strictly inside their pixel: at most 1 % of a case (0 in every case so far); beyond that the case gets another seed


def _ids(cases):
    return [c.id for c in cases]


def _identity(kz, O, case, ks, ranges, tiles=None, w=SC.W, h=SC.H):
    """Every one-sample film of `ks` is the oracle's own render_samples of that index; every film of `ranges` is the sequential float32 sum."""
    ora = O.OracleScene(SC.scene_of(kz.scenes, case))
    assert ora.border == 0 and ora.sample_count == case.count
    assert (ora.width, ora.height) == (w, h)
    pxy = SC.pixel_grid(w, h, tiles)
    n_edge = n_all = 0
    for k, film in SC.one_sample_films(ora, ks, tiles=tiles).items():
        rows = SC.samples_of(ora, pxy, k)
        edge, ok = SC.on_edge(rows, pxy), SC.valid(rows)
        n_edge, n_all = n_edge + int(edge.sum()), n_all + len(rows)
        x, y = pxy[~edge, 0], pxy[~edge, 1]
        want = np.concatenate([np.float32(0) + rows[:, 2:5], np.ones((len(rows), 1), np.float32)], 1)       # (0 + -0 = +0: the tap sum starts at +0)
        want[~ok] = 0                                                                                       # Color3f::isValid drops the sample and its weight
        bad = SC.differing_words(film[y, x], want[~edge]).any(axis=1)
        assert not bad.any(), (case.id, k, int(bad.sum()), pxy[~edge][bad][:4].tolist())
        assert (film[y, x, 3] == ok[~edge]).all()
        if not edge.any():                                                                                  # nothing anywhere else (untouched tiles included)
            assert not SC.differing_words(film, SC.film_of_samples([rows], pxy, w, h)).any(), (case.id, k)
    assert n_edge <= EDGE_SHARE * n_all, (case.id, n_edge, n_all)
    for b, e in ranges:
        per_sample = [SC.samples_of(ora, pxy, k) for k in range(b, e)]
        # an on-edge sample may feed a neighbouring texel too: the texels it can reach (its pixel and the eight around it) leave the identity - the film comparison
        # on the device still covers them -, every other texel of the range stays in, so no range goes unchecked; such samples count against the same 1 % as the
        # single samples do. (Three ranges of the tables hold one such sample each: independent-65536-seedffffffff [0, 64), and [36, 100) of correlated-100-seed7
        # under thinlens and under box_env: at most 9 texels of 960 leave each.)
        n_range_edge = sum(int(SC.on_edge(r, pxy).sum()) for r in per_sample)
        assert n_range_edge <= EDGE_SHARE * len(pxy) * (e - b), (case.id, b, e, n_range_edge)
        out = SC.edge_texels(per_sample, pxy, w, h)
        assert out.sum() <= 9 * n_range_edge and out.sum() <= EDGE_SHARE * 9 * out.size, (case.id, b, e, int(out.sum()))
        film = SC.range_film(ora, b, e, tiles=tiles)
        bad = SC.differing_words(film, SC.film_of_samples(per_sample, pxy, w, h)).any(axis=2) & ~out
        assert not bad.any(), (case.id, b, e, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return ora


def test_the_rounded_counts_are_the_constructors(kz, O):
    """Stratified rounds up to a square from resolution 4 on, Correlated to ceil(n / floor(sqrt n)) * floor(sqrt n): the table's counts are the oracle's, and they are
    a power of 4, a power of 2 only, and neither."""
    got = {}
    for s in SC.SAMPLERS:
        got[s] = tuple(O.OracleScene(SC.scene_of(kz.scenes, SC._case(s, n, 7))).sample_count for n in SC.REQUESTED)
    assert got == SC.ROUNDED
    assert (got["stratified"][0], got["stratified"][4], got["correlated"][2], got["correlated"][4]) == (16, 4225, 1023, 4160)
    pow2 = lambda n: n & (n - 1) == 0
    pow4 = lambda n: pow2(n) and n.bit_length() % 2 == 1
    for s in SC.SAMPLERS:
        counts = got[s]
        assert any(pow4(n) and n > 1 for n in counts) and any(not pow2(n) for n in counts), (s, counts)
        assert any(pow2(n) and not pow4(n) for n in counts) == (s in ("independent", "pmj02bn")), (s, counts)      # (no square, and no r0 * r1 of Correlated, is 2^odd)
    for c in SC.WAVE_CASES:
        assert O.OracleScene(SC.scene_of(kz.scenes, c)).sample_count == c.requested == c.count and c.count % 64 == 0


@pytest.mark.parametrize("case", SC.COUNT_CASES, ids=_ids(SC.COUNT_CASES))
def test_a_one_sample_box_film_is_that_sample(kz, O, case):
    _identity(kz, O, case, SC.sample_indices(case.count), [])


@pytest.mark.parametrize("case", SC.WAVE_CASES, ids=_ids(SC.WAVE_CASES))
def test_a_wave_shaped_range_is_the_sequential_float_sum(kz, O, case):
    _identity(kz, O, case, [case.count - 1], SC.wave_ranges(case.count))


@pytest.mark.parametrize("case", SC.DIM_CASES, ids=_ids(SC.DIM_CASES))
def test_deep_paths_keep_the_identity(kz, O, case):
    """maxDepth 12 under regularization, a thin lens, a scene without lights and a light camera rays walk through: the instrument does not depend on the path."""
    ora = _identity(kz, O, case, SC.DIM_KS, [SC.DIM_RANGE])
    rows = SC.samples_of(ora, SC.pixel_grid(), SC.DIM_KS[-1])
    assert np.abs(rows[:, 2:5]).max() > 0


@pytest.mark.parametrize("case", SC.BIG_CASES, ids=_ids(SC.BIG_CASES))
def test_corner_tiles_of_a_large_frame_keep_the_identity(kz, O, case):
    """2048 x 1536, tiles at the last row and column, past the 128-texel blue-noise period and the pmj pixel tile: texels outside the tiles stay zero."""
    _identity(kz, O, case, [SC.BIG_K], [], tiles=SC.BIG_TILES, w=SC.BIG_W, h=SC.BIG_H)


@pytest.mark.parametrize("case", SC.SCHEDULE_CASES, ids=_ids(SC.SCHEDULE_CASES))
def test_the_schedule_cases_keep_the_identity(kz, O, case):
    _identity(kz, O, case, [case.count - 1], [(case.count - 64, case.count)])


ALL_CASES = SC.COUNT_CASES + SC.WAVE_CASES + SC.DIM_CASES + SC.SCHEDULE_CASES + SC.BIG_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_the_high_word_of_the_seed_reaches_every_case(kz, O, case):
    """hashDimSeed / hashPixelDimSeed mix seed >> 32 in as the key's 4 tail bytes, Hash(p, seed) takes the whole word: a seed that differs only above bit 31 changes at
    least 64 of the case's 960 samples (of the 350 in the corner tiles of the large frame) - so a device that dropped those bits cannot pass the case. Two exceptions, by the reference's own definition: pmj02bn
    draws its pixel sample from the table and takes the index itself for instances below 5, so the seed reaches it through next1D and the later instances only. At ONE
    sample per pixel those permute one element - 0 whatever the key -, and sphere_env's paths (a convex sphere alone, no lights) end before either is drawn. Both
    cases stay for what else they reach, and are asserted to be seed-free."""
    pxy = SC.pixel_grid(SC.BIG_W, SC.BIG_H, SC.BIG_TILES) if case.setting == "big" else SC.pixel_grid()      # (big: the 350 pixels of its corner tiles)
    k = case.count - 1
    a = SC.samples_of(O.OracleScene(SC.scene_of(kz.scenes, case)), pxy, k)
    b = SC.samples_of(O.OracleScene(SC.with_seed(SC.scene_of(kz.scenes, case), case.seed ^ SC.HIGH_WORD)), pxy, k)
    assert (case.seed ^ SC.HIGH_WORD) & 0xffffffff == case.seed & 0xffffffff
    changed = int(SC.differing_words(a, b).any(axis=1).sum())
    if case.sampler == "pmj02bn" and (case.count == 1 or case.setting == "sphere_env"):
        assert changed == 0
    else:
        assert changed >= 64, (case.id, changed)
