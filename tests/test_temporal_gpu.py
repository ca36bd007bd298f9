"""-m gpu: the temporal stage of include/kazen_mi355x_temporal.h on the MI355X. kz_denoise_temporal_films - the result, the new history and v_last - has the bits of
the C++ restatement (tests/cpu_ref/kz_temporal_ref.cpp) over frames, borders, guide subsets, histories and pairs of views; a replica's chain of calls across camera
edits has the bits of the reference chain on the films it downloads; the history's life follows the header. Comparisons are same_bits / array_equal, never a
tolerance."""
import copy

import numpy as np
import pytest

from checks import differing, same_bits_strict
from cpu_refs import lib, ref_denoise_temporal, ref_denoise_variance
from film_cases import GUIDES, H, SPP, W, _orbit, random_history, synthetic_films, synthetic_moment, view_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("temporal", tmp_path_factory.mktemp("kzt"))


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return lib("variance", tmp_path_factory.mktemp("kzv"))


def check(kz, ref, films, b, cur, prev, history, tag, **kw):
    got, gh, gv = kz.denoise_temporal_films(*films, border=b, samples=4, current=cur, previous=prev, history=history, return_variance=True, **kw)
    want, wh, wv = ref_denoise_temporal(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=history, **kw)
    assert same_bits_strict(got, want), (tag, kw, "film", differing(got, want))
    assert same_bits_strict(gh, wh), (tag, kw, "history", differing(gh, wh))
    assert same_bits_strict(gv, wv), (tag, kw, "variance", differing(gv, wv))
    return wh


# frames: one pixel; smaller than the 2 x 2 gather's reach; not multiples of a wave or a block; more than one block; a row of 65 (one pixel into the second wave); test_denoise_gpu's widest
@pytest.mark.parametrize("frame", [(1, 1), (2, 2), (7, 5), (64, 33), (65, 3), (130, 20)])
def test_films_entry_has_the_references_bits(gpu_lib, kz, ref, frame):
    w, h = frame
    blended = 0
    for b in (0, 2):
        colour, albedo, normal, depth = synthetic_films(w, h, b, seed=200 * w + h + b)      # (with z = 0 pixels and pixels that are not valid)
        moment = synthetic_moment(colour, seed=3 * w + h + b)
        full = (colour, moment, albedo, normal, depth)
        views = view_pairs(kz, w, h)
        junk = random_history(w, h, seed=w + h + b)
        # no history, at 1 and 5 iterations; its own output is the third kind of history
        own = check(kz, ref, full, b, views["same"][0], None, None, (frame, b, "none"), iterations=1)
        check(kz, ref, full, b, views["same"][0], None, None, (frame, b, "none"), iterations=5)
        for vname, (cur, prev) in views.items():
            for hname, hist in (("random", junk), ("own", own)):
                # default tolerances, and tolerances that let most taps through so that the blend is exercised on random depths too
                for kw in (dict(iterations=1), dict(iterations=5 if vname == "fraction" else 1, depth_tolerance=20.0, normal_tolerance=3.0, max_history=7)):
                    out = check(kz, ref, full, b, cur, prev, hist, (frame, b, vname, hname), **kw)
                    blended += int((out[..., 8] > 1).sum())
        # every guide subset that holds depth, with and without demodulation
        for al in (False, True):
            for no in (False, True):
                films = (colour, moment, albedo if al else None, normal if no else None, depth)
                for demodulate in (True, False):
                    cur, prev = views["fraction"]
                    check(kz, ref, films, b, cur, prev, own, (frame, b, al, no), iterations=1, demodulate=demodulate, depth_tolerance=20.0)
                    check(kz, ref, films, b, cur, prev, junk, (frame, b, al, no), iterations=1, demodulate=demodulate, use_guides=False, normal_tolerance=3.0)
        # the same subset named by `guides` with every film given
        check(kz, ref, full, b, *views["fraction"], own, (frame, b, "guides"), iterations=1, guides=["normal", "depth"])
    assert blended > 0 or w * h < 4


def test_identities_on_the_device(gpu_lib, kz):
    """Without a history, and with maxHistory = 1 over a random one, the device's result has kz_denoise_variance_films' bits."""
    b = 2
    colour, albedo, normal, depth = synthetic_films(70, 45, b, seed=9)
    moment = synthetic_moment(colour, seed=10)
    cur, prev = view_pairs(kz, 70, 45)["fraction"]
    for kw in (dict(), dict(iterations=3, demodulate=False, sigma_variance=1.5)):
        want, wv = kz.denoise_variance_films(colour, moment, albedo, normal, depth, border=b, samples=8, return_variance=True, **kw)
        got, hist, gv = kz.denoise_temporal_films(colour, moment, albedo, normal, depth, border=b, samples=8, current=cur, return_variance=True, **kw)
        assert same_bits_strict(got, want) and same_bits_strict(gv, wv)
        got, hist1, gv = kz.denoise_temporal_films(colour, moment, albedo, normal, depth, border=b, samples=8, current=cur, previous=prev, history=random_history(70, 45, 1),
                                                   max_history=1, return_variance=True, **kw)
        assert same_bits_strict(got, want) and same_bits_strict(gv, wv) and same_bits_strict(hist1, hist)
        assert set(np.unique(hist[..., 8])) == {0.0, 1.0}


# ---------------------------------------------------------------- a replica across camera edits
def _films(sc):
    return [sc.film(), sc.moment_film()] + [sc.aov_film(g) for g in GUIDES]


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_replica_chain_equals_the_reference_chain(gpu_lib, kz, ref, scene):
    d = kz.scenes.cornell_box(W, H, 3 * SPP) if scene == "cornell" else kz.scenes.textured_scene(W, H, 3 * SPP)      # (three frames of SPP samples each)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    b = sc.border
    assert sc.temporal_info() == (0, 0)
    history, prev = None, None
    start = copy.copy(d)
    start.camera = dict(d.camera)                                     # (Scene.desc.camera follows the edits)
    for f in range(3):
        if f:
            sc.set_camera({"toWorld": _orbit(kz, start, 1.5 * f).camera["toWorld"]})
        sc.render(sample_begin=SPP * f, sample_end=SPP * (f + 1), accumulate=False)
        films = _films(sc)
        sc.denoise_temporal()
        view = kz.temporal_view(sc.desc.camera)
        want, history, _ = ref_denoise_temporal(ref, kz, *films, border=b, samples=SPP, current=view, previous=prev, history=history)
        prev = view
        got, gh = sc.denoised_film(), sc.temporal_history()
        assert same_bits_strict(got, want), (scene, f, differing(got, want))
        assert same_bits_strict(gh, history), (scene, f, differing(gh, history))
        assert sc.temporal_info() == (2 * W * H * 36, f + 1)
        for x, y in zip(films, _films(sc)):                           # the films do not notice
            assert same_bits_strict(x, y)
        if f:                                                         # most of the frame found its history
            found = float((history[..., 8] > 1).mean())
            print("temporal chain %s frame %d: %.1f %% of the pixels found a history" % (scene, f + 1, 100 * found))
            assert found > 0.1, (scene, f, found)
    assert sc.denoised_srgb8().shape == (H, W, 3)


# ---------------------------------------------------------------- lifecycle
def test_lifecycle(gpu_lib, kz, ref, vref):
    a = kz.abi
    d = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(d, device=0)
    b = sc.border
    dn_bytes, tp_bytes = 4 * W * H * 16 + (H + 2 * b) * (W + 2 * b) * 16, 2 * W * H * 36

    def refused(fn, code, *words):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    sc.render()
    plain = sc.film()
    refused(sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "KZ_AOV_DEPTH")
    sc.set_aovs(["albedo", "normal"])
    refused(sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "KZ_AOV_DEPTH", "mask 3")
    sc.set_aovs(GUIDES)
    refused(sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "switched off")
    sc.set_variance(True)
    refused(sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "samples = 0")
    refused(sc.temporal_history, a.KZ_ERR_STATE, "kz_temporal_download")
    sc.denoise()
    assert sc.denoise_info() == dn_bytes and sc.temporal_info() == (0, 0)
    sc.render()
    films = _films(sc)
    view = kz.temporal_view(sc.desc.camera)
    sc.denoise_temporal()
    assert sc.denoise_info() == dn_bytes and sc.temporal_info() == (tp_bytes, 1)      # no buffer beyond kz_denoise's but the history
    first, _ = ref_denoise_variance(vref, kz, *films, border=b, samples=SPP)
    assert same_bits_strict(sc.denoised_film(), first)                      # no history yet: kz_denoise_variance's bits
    sc.denoise_temporal()
    assert sc.temporal_info() == (tp_bytes, 2)
    _, h1, _ = ref_denoise_temporal(ref, kz, *films, border=b, samples=SPP, current=view)
    want2, h2, _ = ref_denoise_temporal(ref, kz, *films, border=b, samples=SPP, current=view, previous=view, history=h1)
    assert same_bits_strict(sc.denoised_film(), want2) and same_bits_strict(sc.temporal_history(), h2) and not same_bits_strict(want2, first)
    # kz_denoise_release leaves the history; the next call finds it
    sc.denoise_release()
    assert sc.denoise_info() == 0 and sc.temporal_info() == (tp_bytes, 2) and same_bits_strict(sc.temporal_history(), h2)
    sc.denoise_temporal()
    assert sc.temporal_info() == (tp_bytes, 3) and sc.denoise_info() == dn_bytes
    # a material edit keeps it, an edit of the geometry - even one that moves nothing - makes it stale: the next call starts at 1 in the buffers it has
    m = next(i for i, mesh in enumerate(sc.desc.meshes) if mesh["bsdf"] and mesh["bsdf"]["type"] == "diffuse" and mesh["light"] is None)
    original = dict(sc.desc.meshes[m]["bsdf"])
    sc.set_bsdfs({m: dict(original, albedo=(0.5, 0.4, 0.3))})
    sc.denoise_temporal()
    assert sc.temporal_info() == (tp_bytes, 4)
    mesh = sc.desc.meshes[m]
    sc.set_vertices({m: mesh["V"] if mesh["N"] is None else (mesh["V"], mesh["N"])})
    assert sc.temporal_info() == (tp_bytes, 4)                       # (a host flag: nothing happens until the next call)
    sc.denoise_temporal()
    assert sc.temporal_info() == (tp_bytes, 1)
    assert same_bits_strict(sc.denoised_film(), first) and same_bits_strict(sc.temporal_history(), h1)      # (the films are still the ones rendered above)
    # a call that demodulates differently from the history is refused and changes nothing
    refused(lambda: sc.denoise_temporal(demodulate=False), a.KZ_ERR_STATE, "kz_denoise_temporal", "kz_temporal_reset")
    refused(lambda: sc.denoise_temporal(guides=["normal", "depth"]), a.KZ_ERR_STATE, "kz_denoise_temporal", "kz_temporal_reset")
    refused(lambda: sc.denoise_temporal(guides=["albedo", "normal"]), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal", "KZ_AOV_DEPTH")
    assert sc.temporal_info() == (tp_bytes, 1) and same_bits_strict(sc.temporal_history(), h1)
    # kz_temporal_reset: the info is zero, the next result is kz_denoise_variance's, and the other demodulation is welcome
    sc.temporal_reset()
    assert sc.temporal_info() == (0, 0) and sc.denoise_info() == dn_bytes
    refused(sc.temporal_history, a.KZ_ERR_STATE, "kz_temporal_download")
    sc.denoise_temporal(demodulate=False)
    want, _ = ref_denoise_variance(vref, kz, *films, border=b, samples=SPP, demodulate=False)
    assert same_bits_strict(sc.denoised_film(), want) and sc.temporal_info() == (tp_bytes, 1)
    sc.denoise_variance()
    assert same_bits_strict(sc.denoised_film(), first) and sc.temporal_info() == (tp_bytes, 1)      # the other calls leave the history alone
    # the variance switch off: refused; the history stays until it is reset
    sc.set_variance(False)
    refused(sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "switched off")
    assert sc.temporal_info() == (tp_bytes, 1)
    # a plain render's film has the bits it had before any temporal call
    sc.set_aovs(())
    sc.temporal_reset()
    sc.set_bsdfs({m: original})
    sc.render()
    assert np.array_equal(sc.film(), plain)
    n = W * H * 12
    buf = np.zeros(n + 4, np.float32)
    sc.set_aovs(GUIDES)
    sc.set_variance(True)
    sc.render()
    sc.denoise_temporal()
    assert sc.lib.kz_temporal_download(sc.h, -1, buf.ctypes.data_as(a.f32p), n + 4) == a.KZ_ERR_INVALID_ARG
    assert sc.lib.kz_temporal_info(sc.h, -1, None, None) == a.KZ_ERR_INVALID_ARG
