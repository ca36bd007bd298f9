"""The second-moment film and the variance-guided denoiser (include/kazen_mi355x_variance.h) without a GPU: the header against the library's exports, the refusals
that need no device, the test-only CPU reference (tests/cpu_ref/kz_variance_ref.cpp) the GPU tests compare against - checked here against a float64 numpy
restatement, against the existing denoiser's reference where the two must agree to the bit, and on inputs whose answer is known - and what the variance guidance is
worth on the oracle's own films."""
import ctypes as C
import re

import numpy as np
import pytest

from checks import c_layout, header_surface, refused
from cpu_refs import MomentRef, lib, ref_denoise, ref_denoise_variance
from film_cases import BAD_OPTS, BAD_VOPTS, frame_rgb, quality_inputs, synthetic_films, synthetic_moment


def np_denoise_variance(film, moment, albedo=None, normal=None, depth=None, border=0, samples=4, sigma_variance=3.0, iterations=5, demodulate=True, use_guides=True,
                        sigmas=(2.0, 0.3, 0.1, 0.1)):
    """The header's definition in float64 numpy, one shifted frame per tap. Returns (film, v_last). One step is taken in fp32 as the definition words it: s - c * c cancels
    where the variance is small against the mean's square, and its value is then set by the fp32 roundings of s, c and c * c, not by anything a float64 restatement could
    reproduce from the films."""
    b = border
    rows, cols = film.shape[:2]
    h, w = rows - 2 * b, cols - 2 * b

    def values(f):
        if f is None:
            return np.zeros((h, w, 3)), np.zeros((h, w))
        f = f[b:rows - b, b:cols - b].astype(np.float64)
        wgt = f[..., 3]
        return np.where(wgt[..., None] != 0, f[..., :3] / np.where(wgt == 0, 1.0, wgt)[..., None], 0.0), wgt

    (c, wc), (s, _), (a, _), (n, _), (z3, _) = values(film), values(moment), values(albedo), values(normal), values(depth)
    z, valid = z3[..., 0], wc != 0
    demodulate = demodulate and albedo is not None
    guided = use_guides and any(g is not None for g in (albedo, normal, depth))
    am = np.maximum(a, np.float32(1e-3))
    e = c / am if demodulate else c.copy()
    def values32(f):
        f = f[b:rows - b, b:cols - b]
        wgt = f[..., 3:]
        return np.where(wgt != 0, f[..., :3] / np.where(wgt == 0, np.float32(1), wgt), np.float32(0))

    c32, s32 = values32(np.asarray(film, np.float32)), values32(np.asarray(moment, np.float32))
    assert c32.dtype == np.float32 and s32.dtype == np.float32
    var = np.maximum(s32 - c32 * c32, np.float32(0)).astype(np.float64) / float(samples)
    v = (var / (am * am)).sum(axis=2) if demodulate else var.sum(axis=2)
    hk = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    k3 = np.array([1 / 4, 1 / 2, 1 / 4])
    kn, kz, ka = (1.0 / (np.float64(np.float32(x)) ** 2) for x in sigmas[1:])
    sv2 = np.float64(np.float32(sigma_variance)) ** 2
    yy, xx = np.mgrid[0:h, 0:w]

    def shifted(dy, dx):
        qy, qx = yy + dy, xx + dx
        inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
        qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
        return qy, qx, inside & valid[qy, qx] & valid

    for i in range(iterations):
        st = 1 << i
        kc = 1.0 / (np.float64(np.float32(sigmas[0])) * 2.0 ** -i) ** 2
        gn, gd = np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx, use = shifted(dy, dx)
                gn += np.where(use, k3[dy + 1] * k3[dx + 1] * v[qy, qx], 0.0)
                gd += np.where(use, k3[dy + 1] * k3[dx + 1], 0.0)
        g = gn / np.where(gd == 0, 1.0, gd)
        kcv = np.maximum(kc, 1.0 / (sv2 * g + np.float64(np.float32(1e-12))))
        num, den, nv = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx, use = shifted(st * dy, st * dx)
                arg = ((e[qy, qx] - e) ** 2).sum(axis=2) * kcv
                if guided:
                    m = np.maximum(np.maximum(z, z[qy, qx]), np.float64(np.float32(1e-20)))
                    arg = arg + ((n[qy, qx] - n) ** 2).sum(axis=2) * kn + ((z[qy, qx] - z) / m) ** 2 * kz + ((a[qy, qx] - a) ** 2).sum(axis=2) * ka
                wgt = np.where(use, hk[dy + 2] * hk[dx + 2] * np.exp(-arg), 0.0)
                num += wgt[..., None] * e[qy, qx]
                den += wgt
                nv += wgt * wgt * v[qy, qx]
        safe = np.where(den == 0, 1.0, den)
        e = np.where(valid[..., None], num / safe[..., None], e)
        v = np.where(valid, nv / (safe * safe), v)
    out = np.zeros((rows, cols, 4))
    out[b:rows - b, b:cols - b, :3] = np.where(valid[..., None], e * am if demodulate else e, 0.0)
    out[b:rows - b, b:cols - b, 3] = valid
    return out, np.where(valid, v, 0.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("variance", tmp_path_factory.mktemp("kzv"))


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return lib("denoise", tmp_path_factory.mktemp("kzd"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: disjoint from the five other lists, and nothing added to the existing headers
    _, src = header_surface(kz, "include/kazen_mi355x_variance.h", a.VARIANCE_EXPORTS, 6, [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS],
                            ["include/kazen_mi355x.h", "include/kazen_mi355x_dev.h", "include/kazen_mi355x_edit.h", "include/kazen_mi355x_aov.h", "include/kazen_mi355x_denoise.h"],
                            ["kz_variance", "kz_denoise_variance", "kz_scene_set_variance", "kz_scene_variance", "kzvarianceopts"])
    for n, v in (("KZ_VARIANCE_OFF", a.KZ_VARIANCE_OFF), ("KZ_VARIANCE_ON", a.KZ_VARIANCE_ON), ("KZ_VARIANCE_TWO_LAUNCHES", a.KZ_VARIANCE_TWO_LAUNCHES),
                 ("KZ_VARIANCE_ONE_PASS", a.KZ_VARIANCE_ONE_PASS)):
        assert int(re.search(r"#define %s\s+(\d+)" % n, src).group(1)) == v


def test_opts_struct_is_16_bytes(kz, tmp_path):
    assert c_layout(tmp_path, "kazen_mi355x_variance.h", ["sizeof(KzVarianceOpts)", "offsetof(KzVarianceOpts, samples)", "offsetof(KzVarianceOpts, flags)",
                                                          "offsetof(KzVarianceOpts, reserved)"]) == ["16", "4", "8", "12"]
    o = kz.abi.KzVarianceOpts
    assert C.sizeof(o) == 16 and (o.sigmaVariance.offset, o.samples.offset, o.flags.offset, o.reserved.offset) == (0, 4, 8, 12)


def test_refusals_without_a_device(kz):
    a = kz.abi
    lib = a.load_library()
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert sc.variance() == 0
    for bad in (-1, 4, 1 << 20):
        refused(kz, lambda: sc.set_variance(bad), a.KZ_ERR_INVALID_ARG, "kz_scene_set_variance")
    assert sc.variance() == 0
    assert lib.kz_scene_set_variance(None, 1) == a.KZ_ERR_INVALID_ARG and lib.kz_denoise_variance(None, -1, None, None) == a.KZ_ERR_INVALID_ARG
    # the switch off: bad options first, then the state - all before a replica is looked for
    for bad in BAD_OPTS:
        refused(kz, lambda: sc.denoise_variance(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance")
    for bad in BAD_VOPTS:
        refused(kz, lambda: sc.denoise_variance(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance", "KzVarianceOpts")
    refused(kz, lambda: sc.denoise_variance(guides="albedo"), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance", "guides")      # the scene's mask is 0
    refused(kz, sc.denoise_variance, a.KZ_ERR_STATE, "kz_denoise_variance", "switched off", "0")
    refused(kz, sc.moment_film, a.KZ_ERR_STATE, "kz_variance_download", "switched off")
    refused(kz, sc.variance_info, a.KZ_ERR_STATE)
    tiles = [(0, 0, 16, 16)]
    counter = np.zeros(2, np.uint32)
    for mode in (True, a.KZ_VARIANCE_TWO_LAUNCHES, a.KZ_VARIANCE_ONE_PASS):
        sc.set_variance(mode)                                         # (a scene on no device: the switch alone)
        assert sc.variance() == int(mode)
        # what AOVs refuse, naming the call
        refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "pipeline = 1", "second-moment")
        refused(kz, lambda: sc.render_multi([0]), a.KZ_ERR_UNSUPPORTED, "kz_render_multi", "second-moment")
        refused(kz, lambda: sc.render_dealt(tiles, counter, device=0), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "KzTileDealer")
        refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "packedOutput")
        refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_UNSUPPORTED, "kz_film_download_tiles", "second-moment")
        # bad options are still refused first; good ones get as far as the missing device
        for bad in BAD_OPTS + BAD_VOPTS:
            refused(kz, lambda: sc.denoise_variance(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance")
        for good in ({}, {"samples": 4, "sigma_variance": 2.0, "iterations": 8, "sigma_color": 1.0, "flags": 2}):
            refused(kz, lambda: sc.denoise_variance(**good), a.KZ_ERR_STATE, "kz_scene_upload")
        refused(kz, sc.moment_film, a.KZ_ERR_STATE, "kz_scene_upload")
    # with AOVs on as well, the AOVs' refusal comes first, as before
    sc.set_aovs(["depth"])
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "AOVs")
    sc.set_aovs(())
    # switched off, the same calls get as far as they got before: the scene is on no device
    sc.set_variance(False)
    assert sc.variance() == 0
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_STATE)
    # the test surface checks its arguments and options first, then the sample count, then asks for the device
    film = np.ones((5, 7, 4), np.float32)
    for bad in BAD_OPTS + BAD_VOPTS:
        refused(kz, lambda: kz.denoise_variance_films(film, film, samples=4, **bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance_films")
    refused(kz, lambda: kz.denoise_variance_films(film, film, samples=4, guides="normal"), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance_films", "guides")
    refused(kz, lambda: kz.denoise_variance_films(film, film, samples=4, border=3), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance_films")
    refused(kz, lambda: kz.denoise_variance_films(film, None, samples=4), a.KZ_ERR_INVALID_ARG, "kz_denoise_variance_films")
    refused(kz, lambda: kz.denoise_variance_films(film, film), a.KZ_ERR_STATE, "kz_denoise_variance_films", "samples = 0")
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.denoise_variance_films(film, film, samples=4), a.KZ_ERR_NO_DEVICE)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", [dict(), dict(iterations=2, demodulate=False), dict(iterations=8, use_guides=False, sigma_variance=1.0),
                                  dict(iterations=3, sigmas=(1.5, 0.6, 0.3, 0.4), samples=16, sigma_variance=1.0)])
def test_reference_agrees_with_numpy(kz, ref, case):
    """The colours to 1e-5 relative, by the argument of test_denoise_cpu.test_reference_agrees_with_numpy: the new terms - the nine-tap prefilter, one division, one
    maximum, and per tap one square and one product - add a handful of roundings of 2^-24 per pixel and iteration to the ~26 the sums already see, and the tolerance kcv
    enters a weight only through arg x 2^-23. v_last to 1e-4: v is no normalised mean - a tap's share of nv is wgt^2 v(q), and v(q) spans eight decades on these films
    (demodulation by am = 1e-3 multiplies a variance by 1e6), so taps count down to wgt^2 ~ 1e-8, arg ~ 9, where the relative error of wgt^2, 2 arg x (the ~8 roundings
    of 2^-24 behind arg), is ten times that of the taps of arg ~ 1 that make a colour."""
    b = 2
    colour, albedo, normal, depth = synthetic_films(37, 29, b, seed=11)
    moment = synthetic_moment(colour, seed=12)
    sig = case.get("sigmas", (2.0, 0.3, 0.1, 0.1))
    sv, n = case.get("sigma_variance", 3.0), case.get("samples", 4)
    opts = {k: v for k, v in case.items() if k not in ("sigmas", "sigma_variance", "samples")}
    got, gv = ref_denoise_variance(ref, kz, colour, moment, albedo, normal, depth, border=b, samples=n, sigma_variance=sv,
                                   sigma_color=sig[0], sigma_normal=sig[1], sigma_depth=sig[2], sigma_albedo=sig[3], **opts)
    want, wv = np_denoise_variance(colour, moment, albedo, normal, depth, border=b, samples=n, sigma_variance=sv, sigmas=sig, **opts)
    assert np.isfinite(got).all() and np.isfinite(gv).all()
    assert np.array_equal(got[..., 3], want[..., 3]) and 0.9 < got[b:-b, b:-b, 3].mean() < 0.99
    assert not got[:b].any() and not got[-b:].any() and not got[:, :b].any() and not got[:, -b:].any()      # the apron
    err = np.abs(got[..., :3] - want[..., :3]) / np.maximum(np.abs(want[..., :3]), 1e-30)
    assert err[want[..., :3] != 0].max() < 1e-5, float(err[want[..., :3] != 0].max())
    verr = np.abs(gv - wv) / np.maximum(np.abs(wv), 1e-30)
    assert (wv != 0).sum() > 800 and verr[wv != 0].max() < 1e-4, float(verr[wv != 0].max())
    assert not gv[want[b:-b, b:-b, 3] == 0].any()                     # 0 where the pixel is not valid (elsewhere an fp32 v may underflow where the float64 one does not)
    # it did filter, the variance fell, and the variance's tolerance did something: the result is not the fixed-tolerance filter's
    assert np.abs(frame_rgb(got, b) - frame_rgb(colour, b)).max() > 0.01
    fixed, _ = ref_denoise_variance(ref, kz, colour, synthetic_moment(colour, 0, degenerate=True), albedo, normal, depth, border=b, samples=n, sigma_variance=sv,
                                    sigma_color=sig[0], sigma_normal=sig[1], sigma_depth=sig[2], sigma_albedo=sig[3], **opts)
    assert not np.array_equal(fixed, got)


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("subset", range(8))
def test_degenerate_identity(kz, ref, dref, subset, demodulate):
    """A moment film of 1e30 x w: var = 1e30 / n per channel (c^2 is far below half an ulp of it), v_0 between 7.5e29 and - demodulated by am = 1e-3 - 7.5e35, finite;
    every later v is a convex-like mean nv / den^2 <= max v; so kv = 1 / (9 g) stays below 1e-29, under every kc_i >= 1 / sigmaColor^2, and kcv = kc_i: the colours
    have the bits of the existing reference at the same KzDenoiseOpts."""
    b = 2
    colour, albedo, normal, depth = synthetic_films(45, 31, b, seed=21)
    moment = synthetic_moment(colour, 0, degenerate=True)
    given = [f if subset & (1 << k) else None for k, f in enumerate((albedo, normal, depth))]
    for kw in (dict(sigma_color=2.0), dict(sigma_color=1.0), dict(sigma_color=0.4, sigma_normal=0.7, iterations=8), dict(sigma_color=2.0, use_guides=False, iterations=3)):
        got, v = ref_denoise_variance(ref, kz, colour, moment, *given, border=b, samples=4, demodulate=demodulate, **kw)
        want = ref_denoise(dref, kz, colour, *given, border=b, demodulate=demodulate, **kw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (subset, demodulate, kw)
        assert np.isfinite(v).all() and v.max() > 1e28
    # the default sigmaColor of this call is 2.0, not kz_denoise's 1.0
    got, _ = ref_denoise_variance(ref, kz, colour, moment, *given, border=b, samples=4, demodulate=demodulate)
    assert np.array_equal(got.view(np.uint32), ref_denoise(dref, kz, colour, *given, border=b, demodulate=demodulate, sigma_color=2.0).view(np.uint32))
    assert not np.array_equal(got, ref_denoise(dref, kz, colour, *given, border=b, demodulate=demodulate))


@pytest.mark.parametrize("subset", range(8))
def test_a_constant_colour_comes_back(kz, ref, subset):
    """A weighted mean of equal values is that value whatever the tolerance makes of the weights: below 1e-5 relative over 5 iterations, as for kz_denoise."""
    b = 1
    colour, albedo, normal, depth = synthetic_films(41, 23, b, seed=3)
    value = np.array([0.37, 1.9, 0.004], np.float32)
    colour[..., :3] = value * colour[..., 3:]
    moment = synthetic_moment(colour, seed=4)
    films = [f if subset & (1 << k) else None for k, f in enumerate((albedo, normal, depth))]
    out, v = ref_denoise_variance(ref, kz, colour, moment, *films, border=b, demodulate=False)
    ok = out[..., 3] == 1
    assert ok.sum() > 800 and np.array_equal(ok[b:-b, b:-b], colour[b:-b, b:-b, 3] != 0)
    assert (np.abs(out[ok][:, :3] / value - 1).max()) < 1e-5
    assert (v >= 0).all() and v.max() > 0
    if subset & 1:
        flat = albedo.copy()
        flat[..., :3] = np.array([0.3, 0.0, 0.7], np.float32) * flat[..., 3:]
        out, _ = ref_denoise_variance(ref, kz, colour, moment, flat, films[1], films[2], border=b)
        assert (np.abs(out[ok][:, :3] / value - 1).max()) < 1e-5


def test_zero_weight_pixels_neither_give_nor_receive(kz, ref):
    b = 2
    colour, albedo, normal, depth = synthetic_films(33, 27, b, seed=7)
    moment = synthetic_moment(colour, seed=8)
    dead = colour[..., 3] == 0
    assert dead[b:-b, b:-b].sum() > 20
    out, v = ref_denoise_variance(ref, kz, colour, moment, albedo, normal, depth, border=b)
    assert not out[dead].any() and not out[:b].any() and not out[:, :b].any()
    assert not v[dead[b:-b, b:-b]].any() and (v[~dead[b:-b, b:-b]] > 0).any()
    # what a dead texel holds - in the picture, the moment film and the guides - and what the apron holds changes neither e nor v of anybody
    c2, m2, a2, n2, d2 = (f.copy() for f in (colour, moment, albedo, normal, depth))
    inner = np.zeros_like(dead)
    inner[b:-b, b:-b] = True
    for f in (c2, m2, a2, n2, d2):
        f[dead, :3] = 1e6
        f[~inner] = 123.0
    a2[dead] = 77.0
    m2[dead] = 1e9                                                    # (its weight too: validity is the picture's alone)
    c2[~inner, 3] = 5.0
    c2[dead, 3] = 0.0
    again, v2 = ref_denoise_variance(ref, kz, c2, m2, a2, n2, d2, border=b)
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)) and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    # ... and a live pixel does count: reviving one changes its neighbours' colour and variance
    c3 = colour.copy()
    y, x = np.argwhere(dead & inner)[0]
    c3[y, x, 3] = 1.0
    m3 = moment.copy()
    m3[y, x, 3] = 1.0
    out3, v3 = ref_denoise_variance(ref, kz, c3, m3, albedo, normal, depth, border=b)
    assert not np.array_equal(out3, out) and not np.array_equal(v3, v)


def test_out_variance_of_one_flat_iteration(kz, ref):
    """A flat frame (every pixel the same colour, moment and weight) without guides, one iteration: dc = 0 at every tap, so wgt = h h' exp(-0) = h h' exactly, and at an
    interior pixel all 25 taps count: sum wgt = 1 and sum wgt^2 = (sum h^2)^2 = (70 / 256)^2 - v_1 = v_0 x 4900 / 65536, to the few roundings of 25 additions."""
    w, h, n = 16, 12, 8
    colour = np.ones((h, w, 4), np.float32) * np.array([0.5, 0.25, 2.0, 1.0], np.float32)
    moment = np.ones((h, w, 4), np.float32) * np.array([0.5 ** 2 + 0.8, 0.25 ** 2 + 0.4, 2.0 ** 2 + 1.6, 1.0], np.float32)
    v0 = (np.float32(0.8) + np.float32(0.4) + np.float32(1.6)) / n
    out, v = ref_denoise_variance(ref, kz, colour, moment, iterations=1, samples=n)
    assert np.array_equal(out, colour)                                # (a mean of equal values over weights that sum to exactly 1)
    assert abs(v[2:-2, 2:-2] / (v0 * 4900.0 / 65536.0) - 1).max() < 1e-6
    # at the corner 3 x 3 taps count: sum wgt = (3/8 + 1/4 + 1/16)^2, sum wgt^2 = ((3/8)^2 + (1/4)^2 + (1/16)^2)^2
    s1, s2 = 0.375 + 0.25 + 0.0625, 0.375 ** 2 + 0.25 ** 2 + 0.0625 ** 2
    assert abs(v[0, 0] / (v0 * s2 ** 2 / s1 ** 4) - 1) < 1e-6
    # a moment below the mean's square clamps to zero variance
    out, v = ref_denoise_variance(ref, kz, colour, colour * np.array([0.1, 0.1, 0.1, 1], np.float32), iterations=1, samples=n)
    assert not v.any() and np.array_equal(out, colour)


def test_moment_reference_sanity(kz, ref):
    """The canonical moment film of a scene whose every sample is one constant - the `normals` integrator in front of a single quad - is the picture's film with the
    values squared, and its w channel is the picture's bit for bit on any scene."""
    one = kz.scenes.SceneDescription()
    q = kz.scenes.quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    one.add_mesh(q[0], q[3], N=q[1], UV=q[2], bsdf=kz.scenes.diffuse((0.25, 0.5, 0.125)))
    one.camera.update(width=40, height=36, fov=40.0, nearClip=0.1, farClip=100.0, toWorld=kz.scenes.look_at((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    one.sampler = {"type": "independent", "sampleCount": 4, "seed": 0}
    one.integrator = dict(one.integrator, type="normals")
    r = MomentRef(ref, one)
    f, m = r.film(), r.moment_film()
    assert np.array_equal(m[..., 3], f[..., 3]) and f[..., 3].max() > 0
    assert np.array_equal(m[..., :3], f[..., :3]) and np.array_equal(f[..., 2], f[..., 3]) and not f[..., :2].any()      # |n| = (0, 0, 1): 1^2 = 1
    d = kz.scenes.cornell_box(40, 36, 4)
    r = MomentRef(ref, d)
    f, m = r.film(), r.moment_film()
    assert np.array_equal(m[..., 3].view(np.uint32), f[..., 3].view(np.uint32)) and not np.array_equal(m[..., :3], f[..., :3])
    b = r.border
    c, s = frame_rgb(f, b).astype(np.float64), frame_rgb(m, b).astype(np.float64)
    assert (s - c * c > -1e-4 * np.maximum(s, 1e-6)).all() and (s - c * c).max() > 0.01      # E[x^2] >= E[x]^2 under the film's weights, up to rounding
    assert np.array_equal(r.moment_film(0, 2) [..., 3], r.film(0, 2)[..., 3])


# ---------------------------------------------------------------- what it is worth
@pytest.mark.parametrize("scene", ["cornell", "materials", "textured"])
def test_quality_on_the_oracles_films(kz, O, ref, dref, tmp_path_factory, scene):
    """The setting and the metric of test_denoise_cpu.test_quality_on_the_oracles_films - 4 spp against 1024 spp at 96 x 72, the oracle's canonical film, the AOV
    reference's feature films, MSE after the filter over MSE before it - with the second-moment film of tests/cpu_ref/kz_variance_ref.cpp and samples = 4. At default
    options (sigmaVariance 3, sigmaColor 2) the ratio is strictly below the existing filter's at its defaults on each scene; both are computed here. The relative-MSE
    pair (x - ref)^2 / (ref^2 + 0.01) and the 16-spp figures are printed, not asserted. Recorded in DESIGN.md 4f."""
    clean, per = quality_inputs(kz, O, ref, tmp_path_factory, scene)
    b = (clean.shape[0] - 72) // 2
    want = frame_rgb(clean, b).astype(np.float64)
    mse = lambda f: float(((frame_rgb(f, b).astype(np.float64) - want) ** 2).mean())
    rel = lambda f: float((((frame_rgb(f, b).astype(np.float64) - want) ** 2) / (want ** 2 + 0.01)).mean())
    figures = {}
    for spp in (4, 16):
        noisy, moment, films = per[spp]
        assert np.array_equal(moment[..., 3].view(np.uint32), noisy[..., 3].view(np.uint32))      # the moment film's w is the oracle's film's
        new, _ = ref_denoise_variance(ref, kz, noisy, moment, *films, border=b, samples=spp)
        old = ref_denoise(dref, kz, noisy, *films, border=b)
        figures[spp] = (mse(new) / mse(noisy), mse(old) / mse(noisy), rel(new) / rel(noisy), rel(old) / rel(noisy))
        print("variance quality %s %2d spp: MSE ratio new %.4f (existing %.4f), relative MSE ratio new %.4f (existing %.4f)" % ((scene, spp) + figures[spp]))
        if spp == 16:                                                 # the other pair the issue measured at 16 spp
            alt, _ = ref_denoise_variance(ref, kz, noisy, moment, *films, border=b, samples=spp, sigma_color=1.0, sigma_variance=2.0)
            print("variance quality %s 16 spp, sigmaColor 1 / sigmaVariance 2: MSE ratio %.4f, relative %.4f" % (scene, mse(alt) / mse(noisy), rel(alt) / rel(noisy)))
    new4, old4 = figures[4][0], figures[4][1]
    assert new4 < old4, (scene, new4, old4)
