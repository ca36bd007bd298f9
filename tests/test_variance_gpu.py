"""-m gpu: the second-moment film and the variance-guided denoiser of include/kazen_mi355x_variance.h on the MI355X. The film is the CPU reference's canonical film
(tests/cpu_ref/kz_variance_ref.cpp) texel for texel under every filter, schedule and way of feeding it, and its w channel is the picture's; the picture does not notice
it; it follows the picture through clears, accumulation and the switch; the filter's result - colours and v_last - has the bits of the C++ restatement on synthetic
films and on the films a render leaves on the device. Comparisons are same_bits / array_equal, never a tolerance."""
import numpy as np
import pytest

from checks import differing, same_bits_strict
from cpu_refs import lib, ref_denoise, ref_denoise_variance, ref_moment
from film_cases import BAD_OPTS, BAD_VOPTS, FILTERS, GUIDES, H, SCHEDULES, SPP, W, _visible, _with_filter, synthetic_films, synthetic_moment, with_integrator

pytestmark = pytest.mark.gpu

TAPS = 5                                                              # gaussian r = 2 (the scenes' default filter): tapLo = -2, tapHi = 2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("variance", tmp_path_factory.mktemp("kzv"))


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return lib("denoise", tmp_path_factory.mktemp("kzd"))


# ---------------------------------------------------------------- the film
@pytest.mark.parametrize("scene", ["cornell", "textured"])
@pytest.mark.parametrize("filt", list(FILTERS))
def test_moment_film_equals_the_reference(gpu_lib, kz, ref, scene, filt):
    """Every filter of film_cases.FILTERS, the feature films' (7 taps: the 4-group kernel, which the one-pass form leaves to two launches), and each way of feeding the film."""
    a = kz.abi
    base = kz.scenes.cornell_box(W, H, SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    d = _with_filter(base, FILTERS[filt])
    want = ref_moment(ref, (scene, filt), d)
    sc = kz.Scene(d, device=0)
    for mode in (a.KZ_VARIANCE_ON, a.KZ_VARIANCE_TWO_LAUNCHES, a.KZ_VARIANCE_ONE_PASS):
        sc.set_variance(mode)
        sc.render()
        m, f = sc.moment_film(), sc.film()
        assert np.array_equal(m, want), (mode, differing(m, want))
        assert same_bits_strict(m[..., 3], f[..., 3]), mode                  # the w channel is the picture's, bit for bit
        assert m[..., 3].max() > 0 and m[..., :3].max() > 0 and not np.array_equal(m[..., :3], f[..., :3])
    assert sc.variance_info()[1] == SPP


@pytest.mark.parametrize("integ", ["path_mis", "ao"])
def test_the_film_does_not_depend_on_the_schedule(gpu_lib, kz, ref, integ):
    """One film whatever the pass size, the sample chunking, passes in flight, halves, shadow rays beside and the split of the sample range over calls, for both ways of
    feeding it; the picture beside it stays the switch-off picture under each."""
    a = kz.abi
    base = with_integrator(_visible(kz.scenes.cornell_box(W, H, SPP)), integ)
    want = ref_moment(ref, ("cornell/visible", integ), base)
    off = kz.Scene(base, device=0)
    off.render()
    plain = off.film()
    sc = kz.Scene(base, device=0)
    for mode in (a.KZ_VARIANCE_TWO_LAUNCHES, a.KZ_VARIANCE_ONE_PASS):
        sc.set_variance(mode)
        for kw in SCHEDULES:
            sc.render(**kw)
            info = sc.last_pass_info()
            if "passes_in_flight" in kw:
                assert info["passesInFlight"] == 2 and info["passes"] >= 6, info
            if "tune" in kw:
                assert info["sppPerPass"] == 4 and info["passes"] >= 2, info
            if "pass_halves" in kw and integ == "path_mis":
                assert info["shadowBeside"] == 2, info
            assert np.array_equal(sc.moment_film(), want), (integ, mode, kw)
            assert np.array_equal(sc.film(), plain), (integ, mode, kw)
        sc.render(sample_begin=0, sample_end=4)
        assert sc.variance_info()[1] == 4
        sc.render(sample_begin=4, sample_end=8, accumulate=True)
        assert sc.variance_info()[1] == 8
        assert np.array_equal(sc.moment_film(), want), (integ, mode, "two calls")
        assert np.array_equal(sc.film(), plain), (integ, mode, "two calls")


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_picture_untouched_and_memory(gpu_lib, kz, scene):
    d = kz.scenes.cornell_box(W, H, SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    sc = kz.Scene(d, device=0)
    assert sc.variance_info() == (0, 0)
    sc.render()
    plain = sc.film()
    b = sc.border
    one_film = TAPS * TAPS * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16
    for mode in (1, 2, 3):
        sc.set_variance(mode)
        if mode == 1:
            assert sc.variance_info() == (0, 0)                       # allocated by the first render that needs it
        sc.render()
        assert np.array_equal(sc.film(), plain), mode
        assert sc.variance_info() == (one_film, SPP)
    assert sc.aov_info() == 0 and sc.denoise_info() == 0
    sc.set_variance(False)
    assert sc.variance_info() == (0, 0)                               # freed
    sc.render()
    assert np.array_equal(sc.film(), plain)
    assert sc.variance_info() == (0, 0)


# ---------------------------------------------------------------- lifecycle
def test_lifecycle(gpu_lib, kz, ref, dref):
    a = kz.abi
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    b = sc.border
    sc.set_variance(True)
    assert not sc.moment_film().any()                                 # switched on, nothing rendered: zeros
    sc.render(sample_begin=0, sample_end=4)
    first = ref_moment(ref, "cornell", d, 0, 4)
    assert np.array_equal(sc.moment_film(), first) and sc.variance_info()[1] == 4
    # accumulated with the picture
    sc.render(sample_begin=4, sample_end=8, accumulate=True)
    whole = ref_moment(ref, ("cornell", "gaussian r=2"), _with_filter(kz.scenes.cornell_box(W, H, SPP), FILTERS["gaussian r=2"]))
    assert np.array_equal(sc.moment_film(), whole) and sc.variance_info()[1] == 8
    # the edits leave it alone
    sc.set_camera({"fov": 41.0})
    assert np.array_equal(sc.moment_film(), whole) and sc.variance_info()[1] == 8
    sc.set_camera({"fov": d.camera["fov"]})
    # cleared with the picture
    sc.film_clear()
    sc.sync()
    assert not sc.moment_film().any() and not sc.film().any() and sc.variance_info()[1] == 0
    # a render that does not accumulate clears it too
    sc.render(sample_begin=0, sample_end=4)
    sc.render(sample_begin=4, sample_end=8)
    assert np.array_equal(sc.moment_film(), ref_moment(ref, "cornell", d, 4, 8)) and sc.variance_info()[1] == 4
    # off and on again: freed, then zero, then the samples rendered from then on
    sc.set_variance(False)
    with pytest.raises(a.KzError) as e:
        sc.moment_film()
    assert e.value.code == a.KZ_ERR_STATE
    sc.render(sample_begin=0, sample_end=4)                           # the picture alone: 4 samples
    sc.set_variance(True)
    assert not sc.moment_film().any() and sc.variance_info() == (0, 0)
    sc.render(sample_begin=4, sample_end=8, accumulate=True)          # a late enable without a clear: the picture holds 8, the moment film 4
    assert np.array_equal(sc.moment_film(), ref_moment(ref, "cornell", d, 4, 8)) and sc.variance_info()[1] == 4
    for kw in ({}, {"samples": 4}, {"samples": 8}):
        with pytest.raises(a.KzError) as e:
            sc.denoise_variance(**kw)
        assert e.value.code == a.KZ_ERR_STATE and "kz_denoise_variance" in str(e.value) and " 8 " in str(e.value) and " 4 " in str(e.value), str(e.value)
    # kz_denoise alone allocates and reports what it did before this call existed
    sc.denoise()
    assert sc.denoise_info() == 4 * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16
    # ... a clear and a render of both make the pair good, and the variance call needs no buffer beyond kz_denoise's
    sc.film_clear()
    with pytest.raises(a.KzError) as e:
        sc.denoise_variance()                                         # samples resolves to 0
    assert e.value.code == a.KZ_ERR_STATE and "samples = 0" in str(e.value)
    sc.render(accumulate=True)
    sc.denoise_variance()
    assert sc.denoise_info() == 4 * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16
    want, _ = ref_denoise_variance(ref, kz, sc.film(), sc.moment_film(), border=b, samples=SPP)
    assert same_bits_strict(sc.denoised_film(), want)
    sc.denoise_release()
    assert sc.denoise_info() == 0
    fresh = kz.Scene(d, device=0)
    fresh.set_variance(True)
    fresh.render()
    fresh.denoise_variance()                                          # allocated by the variance call's first call, counted from then on, freed by the release
    assert fresh.denoise_info() == 4 * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16 and same_bits_strict(fresh.denoised_film(), want)
    fresh.denoise_release()
    assert fresh.denoise_info() == 0


def test_static_tiles_over_half_the_frame(gpu_lib, kz, ref):
    """A static kz_render_tiles over the left half: both films have samples there and in the filter's strip beside it; every pixel further right has weight 0, is not
    valid and stays (0, 0, 0, 0) with variance 0. The moment film of the tiles equals the whole frame's wherever the right half's pixels do not reach."""
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    sc.set_variance(True)
    sc.set_aovs(GUIDES)
    sc.render_tiles([(0, 0, W // 2, H)], download=False)
    b = sc.border
    m, f = sc.moment_film(), sc.film()
    whole = ref_moment(ref, ("cornell", "gaussian r=2"), _with_filter(kz.scenes.cornell_box(W, H, SPP), FILTERS["gaussian r=2"]))
    assert same_bits_strict(m[..., 3], f[..., 3]) and sc.variance_info()[1] == SPP
    reach = W // 2 + b - 2                                            # the first film column a pixel of the right half reaches (5 taps: 2 to its left)
    assert np.array_equal(m[:, :reach], whole[:, :reach]) and not m[:, b + W // 2 + b:].any() and (m[b:b + H, b:b + W // 2, 3] > 0).all()
    films = [f, m] + [sc.aov_film(g) for g in GUIDES]
    sc.denoise_variance()
    got = sc.denoised_film()
    want, _ = ref_denoise_variance(ref, kz, *films, border=b, samples=SPP)
    assert same_bits_strict(got, want), differing(got, want)
    assert (got[b:b + H, b:b + W // 2, 3] == 1).all() and got[b:b + H, b:b + W // 2, :3].max() > 0.1 and not got[:, b + W // 2 + b:].any()


def test_refusals_with_a_device(gpu_lib, kz):
    a = kz.abi
    d = kz.scenes.cornell_box(64, 64, 4)
    sc = kz.Scene(d, device=0)
    tiles = kz.shard.deal_tiles(64, 64, 1, 0, 32)

    def refused(fn, code, *words):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == code, str(e.value)
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
    refused(sc.denoise_variance, a.KZ_ERR_STATE, "kz_denoise_variance", "switched off")
    sc.set_variance(True)
    U = a.KZ_ERR_UNSUPPORTED
    refused(lambda: sc.render(pipeline=1), U, "kz_render", "pipeline = 1")
    refused(lambda: sc.render_multi([0]), U, "kz_render_multi")
    refused(lambda: sc.render_dealt(tiles, np.zeros(1, np.uint32), takers=1, batch_tiles=2), U, "kz_render_tiles", "KzTileDealer")
    refused(lambda: sc.render_tiles(tiles, packed=True), U, "kz_render_tiles", "packedOutput")
    refused(lambda: sc.film_tiles(tiles), U, "kz_film_download_tiles")
    # a plain render and a static kz_render_tiles on one replica work
    sc.render()
    whole = sc.moment_film()
    sc.render_tiles(tiles)
    assert np.array_equal(sc.moment_film(), whole) and whole[..., 3].max() > 0
    # bad options, with a replica behind the scene
    for bad in BAD_OPTS + BAD_VOPTS:
        refused(lambda: sc.denoise_variance(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance")
        refused(lambda: kz.denoise_variance_films(whole, whole, border=sc.border, samples=4, **bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance_films")
    refused(lambda: sc.denoise_variance(guides="normal"), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance", "guides")
    refused(lambda: kz.denoise_variance_films(whole, whole, border=sc.border), a.KZ_ERR_STATE, "samples = 0")
    refused(lambda: sc.denoise_variance(device=3), a.KZ_ERR_STATE)
    n = whole.size
    buf = np.zeros(n + 4, np.float32)
    assert sc.lib.kz_variance_download(sc.h, -1, buf.ctypes.data_as(a.f32p), n + 4) == a.KZ_ERR_INVALID_ARG
    sc.set_variance(False)
    all_work()


# ---------------------------------------------------------------- the filter on host films
# test_denoise_gpu's frames: not multiples of any tile, smaller than the filter's 62-pixel reach, across the 16 x 16 LDS tile and its halo
@pytest.mark.parametrize("frame", [(1, 1), (5, 3), (17, 33), (70, 45), (130, 20)])
def test_films_entry_has_the_references_bits(gpu_lib, kz, ref, frame):
    w, h = frame
    for b in (0, 2):
        films = synthetic_films(w, h, b, seed=100 * w + h + b)
        moment = synthetic_moment(films[0], seed=7 * w + h + b)
        for it in (1, 5, 8):
            got, gv = kz.denoise_variance_films(films[0], moment, *films[1:], border=b, iterations=it, samples=4, return_variance=True)
            want, wv = ref_denoise_variance(ref, kz, films[0], moment, *films[1:], border=b, iterations=it, samples=4)
            assert same_bits_strict(got, want), (frame, b, it, differing(got, want))
            assert same_bits_strict(gv, wv), (frame, b, it, differing(gv, wv))
            assert np.isfinite(got).all() and np.isfinite(gv).all() and (w * h < 20 or (0 < (got[..., 3] == 1).sum() < w * h))
        assert same_bits_strict(kz.denoise_variance_films(films[0], moment, *films[1:], border=b, samples=4),
                         ref_denoise_variance(ref, kz, films[0], moment, *films[1:], border=b, iterations=5, samples=4)[0])      # the defaults; outVariance NULL


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("subset", range(8))
def test_every_guide_subset(gpu_lib, kz, ref, dref, subset, demodulate):
    b = 2
    colour, albedo, normal, depth = synthetic_films(70, 45, b, seed=9)
    moment = synthetic_moment(colour, seed=10)
    given = [f if subset & (1 << k) else None for k, f in enumerate((albedo, normal, depth))]
    got, gv = kz.denoise_variance_films(colour, moment, *given, border=b, demodulate=demodulate, samples=8, return_variance=True)
    want, wv = ref_denoise_variance(ref, kz, colour, moment, *given, border=b, demodulate=demodulate, samples=8)
    assert same_bits_strict(got, want) and same_bits_strict(gv, wv), (subset, demodulate, differing(got, want), differing(gv, wv))
    if subset:
        # the same subset named by `guides` with every film given, and colour weights alone with the subset's demodulation
        assert same_bits_strict(kz.denoise_variance_films(colour, moment, albedo, normal, depth, border=b, demodulate=demodulate, guides=subset, samples=8), want)
        flat, fv = kz.denoise_variance_films(colour, moment, *given, border=b, demodulate=demodulate, use_guides=False, samples=8, return_variance=True)
        wflat, wfv = ref_denoise_variance(ref, kz, colour, moment, *given, border=b, demodulate=demodulate, use_guides=False, samples=8)
        assert same_bits_strict(flat, wflat) and same_bits_strict(fv, wfv) and not same_bits_strict(flat, want)
    # other sigmas and sample counts than the defaults
    sig = dict(sigma_color=0.8, sigma_normal=0.7, sigma_depth=0.25, sigma_albedo=0.05, iterations=3, sigma_variance=1.5, samples=3)
    got, gv = kz.denoise_variance_films(colour, moment, *given, border=b, demodulate=demodulate, return_variance=True, **sig)
    want2, wv2 = ref_denoise_variance(ref, kz, colour, moment, *given, border=b, demodulate=demodulate, **sig)
    assert same_bits_strict(got, want2) and same_bits_strict(gv, wv2)
    # the degenerate identity on the device: a moment film of 1e30 x w leaves kz_denoise_films' colours at the same KzDenoiseOpts, and the reference's
    huge = synthetic_moment(colour, 0, degenerate=True)
    for kw in (dict(sigma_color=2.0), dict(sigma_color=1.0, iterations=8)):
        deg = kz.denoise_variance_films(colour, huge, *given, border=b, demodulate=demodulate, samples=4, **kw)
        plain = kz.denoise_films(colour, *given, border=b, demodulate=demodulate, **kw)
        assert same_bits_strict(deg, plain), (subset, demodulate, kw, differing(deg, plain))
        assert same_bits_strict(plain, ref_denoise(dref, kz, colour, *given, border=b, demodulate=demodulate, **kw))
    assert not same_bits_strict(kz.denoise_films(colour, *given, border=b, demodulate=demodulate, sigma_color=2.0), want)      # the variance's tolerance did something


# ---------------------------------------------------------------- a scene's own films
@pytest.mark.parametrize("filt", ["gaussian r=2", "box r=0.5"])
@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_scene_denoise_variance_equals_the_reference(gpu_lib, kz, ref, dref, scene, filt):
    base = kz.scenes.cornell_box(W, H, SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, SPP)
    sc = kz.Scene(_with_filter(base, FILTERS[filt]), device=0)
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    sc.render()
    b = sc.border
    films = [sc.film(), sc.moment_film()] + [sc.aov_film(g) for g in GUIDES]
    sc.denoise_variance()
    got = sc.denoised_film()
    want, _ = ref_denoise_variance(ref, kz, *films, border=b, samples=SPP)
    assert same_bits_strict(got, want), (scene, filt, differing(got, want))
    assert same_bits_strict(kz.denoise_variance_films(*films, border=b, samples=SPP), want)
    inner = got[b:got.shape[0] - b, b:got.shape[1] - b] if b else got
    assert (inner[..., 3] == 1).all() and inner[..., :3].max() > 0.1 and np.isfinite(got).all()
    # the picture's film, the moment film and the AOV films do not notice
    for x, y in zip(films, [sc.film(), sc.moment_film()] + [sc.aov_film(g) for g in GUIDES]):
        assert same_bits_strict(x, y)
    # the raster serves both calls
    assert sc.denoised_srgb8().shape == (H, W, 3)
    # a stated sample count, a subset of the mask, and options
    sc.denoise_variance(guides=["normal", "depth"], iterations=3, sigma_color=1.0, sigma_variance=2.0, samples=16)
    want2, _ = ref_denoise_variance(ref, kz, films[0], films[1], None, films[3], films[4], border=b, iterations=3, sigma_color=1.0, sigma_variance=2.0, samples=16)
    assert same_bits_strict(sc.denoised_film(), want2) and not same_bits_strict(want2, want)
    # afterwards kz_denoise on the same replica still gives its own reference's bits
    sc.denoise()
    plain = ref_denoise(dref, kz, films[0], *films[2:], border=b)
    assert same_bits_strict(sc.denoised_film(), plain) and not same_bits_strict(plain, want)
