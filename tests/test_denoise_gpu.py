"""-m gpu: the a-trous denoiser of include/kazen_mi355x_denoise.h on the MI355X. Its result has the bits of the CPU restatement (tests/cpu_ref/kz_denoise_ref.cpp) on
synthetic films - frames smaller than the filter's reach, every guide subset - and on the films a render leaves on the device; the result is a snapshot beside the
picture, which does not notice it; the raster is the oracle's; bad options are refused. Comparisons are same_bits, never a tolerance."""
import copy

import numpy as np
import pytest

from checks import differing, same_bits_strict
from cpu_refs import lib, ref_denoise
from film_cases import BAD_OPTS, GUIDES, synthetic_films

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 72, 8
FILTERS = {"gaussian r=2": {"type": "gaussian", "radius": 2.0, "stddev": 0.5, "B": 1 / 3.0, "C": 1 / 3.0},
           "box r=0.5": {"type": "box", "radius": 0.5, "stddev": 0.5, "B": 1 / 3.0, "C": 1 / 3.0}}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("denoise", tmp_path_factory.mktemp("kzd"))


# ---------------------------------------------------------------- the device code on host films
# not multiples of any tile and smaller than the filter's 62-pixel reach at 5 iterations: taps fall off every side; at 8 iterations the step is 128, wider than every frame
@pytest.mark.parametrize("frame", [(1, 1), (5, 3), (17, 33), (70, 45), (130, 20)])
def test_films_entry_has_the_references_bits(gpu_lib, kz, ref, frame):
    w, h = frame
    for b in (0, 2):
        films = synthetic_films(w, h, b, seed=100 * w + h + b)
        for it in (1, 5, 8):
            got = kz.denoise_films(*films, border=b, iterations=it)
            want = ref_denoise(ref, kz, *films, border=b, iterations=it)
            assert same_bits_strict(got, want), (frame, b, it, differing(got, want, per_pixel=True))
            assert np.isfinite(got).all() and (w * h < 20 or (0 < (got[..., 3] == 1).sum() < w * h))      # some pixels are out, and stay out
        assert same_bits_strict(kz.denoise_films(*films, border=b), ref_denoise(ref, kz, *films, border=b, iterations=5))      # the default


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("subset", range(8))
def test_every_guide_subset(gpu_lib, kz, ref, subset, demodulate):
    b = 2
    colour, albedo, normal, depth = synthetic_films(70, 45, b, seed=9)
    given = [f if subset & (1 << k) else None for k, f in enumerate((albedo, normal, depth))]
    got = kz.denoise_films(colour, *given, border=b, demodulate=demodulate)
    want = ref_denoise(ref, kz, colour, *given, border=b, demodulate=demodulate)
    assert same_bits_strict(got, want), (subset, demodulate, differing(got, want, per_pixel=True))
    if subset:
        # the same subset named by `guides` with every film given, and colour weights alone with the subset's demodulation
        assert same_bits_strict(kz.denoise_films(colour, albedo, normal, depth, border=b, demodulate=demodulate, guides=subset), want)
        flat = kz.denoise_films(colour, *given, border=b, demodulate=demodulate, use_guides=False)
        assert same_bits_strict(flat, ref_denoise(ref, kz, colour, *given, border=b, demodulate=demodulate, use_guides=False))
        assert not same_bits_strict(flat, want)
    # other sigmas than the defaults
    sig = dict(sigma_color=0.4, sigma_normal=0.7, sigma_depth=0.25, sigma_albedo=0.05, iterations=3)
    assert same_bits_strict(kz.denoise_films(colour, *given, border=b, demodulate=demodulate, **sig), ref_denoise(ref, kz, colour, *given, border=b, demodulate=demodulate, **sig))


# ---------------------------------------------------------------- a scene's own films
def _scene(kz, name, filt):
    d = kz.scenes.cornell_box(W, H, SPP) if name == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    d = copy.deepcopy(d)
    d.camera["rfilter"] = dict(FILTERS[filt])
    return d


def _four_films(sc):
    return [sc.film()] + [sc.aov_film(a) for a in GUIDES]


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_scene_denoise_equals_the_reference(gpu_lib, kz, ref, scene, filt):
    sc = kz.Scene(_scene(kz, scene, filt), device=0)
    sc.set_aovs(GUIDES)
    sc.render()
    films = _four_films(sc)
    sc.denoise()
    got = sc.denoised_film()
    want = ref_denoise(ref, kz, *films, border=sc.border)
    assert same_bits_strict(got, want), (scene, filt, differing(got, want, per_pixel=True))
    assert same_bits_strict(kz.denoise_films(*films, border=sc.border), want)
    b = sc.border
    inner = got[b:got.shape[0] - b, b:got.shape[1] - b] if b else got
    assert (inner[..., 3] == 1).all() and inner[..., :3].max() > 0.1 and np.isfinite(got).all()
    if b:
        assert not got[:b].any() and not got[:, :b].any() and not got[-b:].any() and not got[:, -b:].any()
    assert not same_bits_strict(got[..., :3], sc.film()[..., :3] / np.where(films[0][..., 3:] == 0, 1, films[0][..., 3:]))      # it filtered
    # a subset of the mask, and options
    sc.denoise(guides=["normal", "depth"], iterations=3, sigma_color=0.5)
    assert same_bits_strict(sc.denoised_film(), ref_denoise(ref, kz, films[0], None, films[2], films[3], border=b, iterations=3, sigma_color=0.5))


# ---------------------------------------------------------------- lifecycle
def test_lifecycle(gpu_lib, kz, ref):
    a = kz.abi
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(GUIDES)
    b = sc.border
    assert sc.denoise_info() == 0
    for early in (sc.denoised_film, sc.denoised_srgb8):
        with pytest.raises(a.KzError) as e:
            early()
        assert e.value.code == a.KZ_ERR_STATE and "kz_denoise" in str(e.value)
    # enabled guides that were never rendered count as zeros (and an empty film has no valid pixel)
    sc.denoise()
    assert not sc.denoised_film().any()
    sc.render()
    before = _four_films(sc)
    sc.denoise()
    snap = sc.denoised_film()
    assert sc.denoise_info() == 4 * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16      # the documented count
    # the picture's film and the AOV films do not notice
    for x, y in zip(before, _four_films(sc)):
        assert same_bits_strict(x, y)
    # a render after a denoise gives the film it gives without one; the snapshot is left alone by it, by a clear and by an edit
    sc.render(sample_begin=0, sample_end=4)
    fresh = kz.Scene(d, device=0)
    fresh.set_aovs(GUIDES)
    fresh.render(sample_begin=0, sample_end=4)
    for x, y in zip(_four_films(sc), _four_films(fresh)):
        assert same_bits_strict(x, y)
    assert same_bits_strict(sc.denoised_film(), snap)
    sc.film_clear()
    sc.sync()
    assert not sc.film().any() and same_bits_strict(sc.denoised_film(), snap)
    sc.set_camera({"fov": 45.0})
    assert same_bits_strict(sc.denoised_film(), snap)
    assert same_bits_strict(snap, ref_denoise(ref, kz, *before, border=b))
    # the next denoise replaces it: of the cleared film, nothing
    sc.denoise()
    assert not sc.denoised_film().any()
    sc.denoise_release()
    assert sc.denoise_info() == 0
    with pytest.raises(a.KzError) as e:
        sc.denoised_film()
    assert e.value.code == a.KZ_ERR_STATE
    sc.render()                                                       # (the moved camera's picture)
    sc.denoise(iterations=2)
    assert same_bits_strict(sc.denoised_film(), ref_denoise(ref, kz, *_four_films(sc), border=b, iterations=2))
    # a scene without AOVs: colour weights alone
    plain = kz.Scene(d, device=0)
    plain.render()
    plain.denoise()
    assert same_bits_strict(plain.denoised_film(), ref_denoise(ref, kz, plain.film(), border=b))


def test_static_tiles_over_half_the_frame(gpu_lib, kz, ref):
    """A static kz_render_tiles over the left half: the replica's own film has samples there and, through the reconstruction filter, in a strip of `border` pixels
    beside it; every pixel further right has weight 0 and stays (0, 0, 0, 0)."""
    sc = kz.Scene(kz.scenes.cornell_box(W, H, SPP), device=0)
    sc.set_aovs(GUIDES)
    sc.render_tiles([(0, 0, W // 2, H)], download=False)
    films = _four_films(sc)
    b = sc.border
    assert (films[0][b:b + H, b:b + W // 2, 3] > 0).all() and not films[0][:, b + W // 2 + b:].any()
    sc.denoise()
    got = sc.denoised_film()
    want = ref_denoise(ref, kz, *films, border=b)
    assert same_bits_strict(got, want), differing(got, want, per_pixel=True)
    assert (got[b:b + H, b:b + W // 2, 3] == 1).all() and got[b:b + H, b:b + W // 2, :3].max() > 0.1      # inside the tiles
    assert not got[:, b + W // 2 + b:].any()                                                               # outside, past the filter's strip
    assert same_bits_strict(got[..., 3], (films[0][..., 3] != 0) & (want[..., 3] == 1))


# ---------------------------------------------------------------- the raster
def test_srgb8_is_the_oracles(gpu_lib, kz, O):
    d = kz.scenes.textured_scene(W, H, SPP)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(GUIDES)
    sc.render()
    sc.denoise()
    got = sc.denoised_srgb8()
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, O.OracleScene(d).srgb8(sc.denoised_film()))
    assert not np.array_equal(got, sc.srgb8()) and got.max() > 100


# ---------------------------------------------------------------- refusals
def test_refusals_with_a_device(gpu_lib, kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(32, 32, 2), device=0)
    sc.set_aovs(["albedo", "depth"])
    sc.render()
    sc.denoise()
    snap = sc.denoised_film()

    def refused(fn, *words):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == a.KZ_ERR_INVALID_ARG, str(e.value)
        for w in ("kz_denoise",) + words:
            assert w in str(e.value), (w, str(e.value))

    for bad in BAD_OPTS:
        refused(lambda: sc.denoise(**bad))
        refused(lambda: sc.denoise(device=0, **bad))
    for g in ("normal", 2, 7, 8, 1 << 31):
        refused(lambda: sc.denoise(guides=g), "guides")
    film = sc.film()
    for bad in BAD_OPTS:
        refused(lambda: kz.denoise_films(film, border=sc.border, **bad), "kz_denoise_films")
    refused(lambda: kz.denoise_films(film, border=sc.border, guides="albedo"), "kz_denoise_films", "guides")
    assert same_bits_strict(sc.denoised_film(), snap)                        # a refused call leaves the last result alone
    with pytest.raises(a.KzError) as e:
        sc.denoise(device=3)
    assert e.value.code == a.KZ_ERR_STATE
    # the buffers' sizes are checked
    n = snap.size
    buf = np.zeros(n + 4, np.float32)
    assert sc.lib.kz_denoise_download(sc.h, -1, buf.ctypes.data_as(a.f32p), n + 4) == a.KZ_ERR_INVALID_ARG
    # what AOVs refuse stays refused
    with pytest.raises(a.KzError) as e:
        sc.render_multi([0])
    assert e.value.code == a.KZ_ERR_UNSUPPORTED
