"""The a-trous denoiser (include/kazen_mi355x_denoise.h) without a GPU: the header against the library's exports, the refusals that need no device, the test-only
CPU restatement (tests/cpu_ref/kz_denoise_ref.cpp) the GPU tests compare against - checked here against a float64 numpy restatement and on inputs whose answer
is known - and what the filter is worth on the oracle's own films."""
import ctypes as C
import re

import numpy as np
import pytest

from checks import c_layout, header_surface, refused
from cpu_refs import AovRef, lib, ref_denoise
from film_cases import BAD_OPTS, GUIDES, frame_rgb, synthetic_films


def np_denoise(film, albedo=None, normal=None, depth=None, border=0, iterations=5, demodulate=True, use_guides=True, sigmas=(1.0, 0.3, 0.1, 0.1)):
    """The header's definition in float64 numpy, one shifted frame per tap."""
    b = border
    rows, cols = film.shape[:2]
    h, w = rows - 2 * b, cols - 2 * b

    def values(f):
        if f is None:
            return np.zeros((h, w, 3)), np.zeros((h, w))
        f = f[b:rows - b, b:cols - b].astype(np.float64)
        wgt = f[..., 3]
        return np.where(wgt[..., None] != 0, f[..., :3] / np.where(wgt == 0, 1.0, wgt)[..., None], 0.0), wgt

    (c, wc), (a, _), (n, _), (z3, _) = values(film), values(albedo), values(normal), values(depth)
    z, valid = z3[..., 0], wc != 0
    demodulate = demodulate and albedo is not None
    guided = use_guides and any(g is not None for g in (albedo, normal, depth))
    am = np.maximum(a, np.float32(1e-3))
    e = c / am if demodulate else c.copy()
    hk = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    kn, kz, ka = (1.0 / (np.float64(np.float32(s)) ** 2) for s in sigmas[1:])
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(iterations):
        s = 1 << i
        kc = 1.0 / (np.float64(np.float32(sigmas[0])) * 2.0 ** -i) ** 2
        num, den = np.zeros((h, w, 3)), np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = yy + s * dy, xx + s * dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                use = inside & valid[qy, qx] & valid
                arg = ((e[qy, qx] - e) ** 2).sum(axis=2) * kc
                if guided:
                    m = np.maximum(np.maximum(z, z[qy, qx]), np.float64(np.float32(1e-20)))
                    arg = arg + ((n[qy, qx] - n) ** 2).sum(axis=2) * kn + ((z[qy, qx] - z) / m) ** 2 * kz + ((a[qy, qx] - a) ** 2).sum(axis=2) * ka
                wgt = np.where(use, hk[dy + 2] * hk[dx + 2] * np.exp(-arg), 0.0)
                num += wgt[..., None] * e[qy, qx]
                den += wgt
        e = np.where(valid[..., None], num / np.where(den == 0, 1.0, den)[..., None], e)
    out = np.zeros((rows, cols, 4))
    out[b:rows - b, b:cols - b, :3] = np.where(valid[..., None], e * am if demodulate else e, 0.0)
    out[b:rows - b, b:cols - b, 3] = valid
    return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("denoise", tmp_path_factory.mktemp("kzd"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: disjoint from the other lists, and nothing added to the existing headers
    _, src = header_surface(kz, "include/kazen_mi355x_denoise.h", a.DENOISE_EXPORTS, 7, [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS],
                            ["include/kazen_mi355x.h", "include/kazen_mi355x_dev.h", "include/kazen_mi355x_edit.h", "include/kazen_mi355x_aov.h"], ["kz_denoise"])
    for n, v in (("KZ_DENOISE_NO_DEMODULATE", a.KZ_DENOISE_NO_DEMODULATE), ("KZ_DENOISE_NO_GUIDES", a.KZ_DENOISE_NO_GUIDES), ("KZ_DENOISE_MAX_ITERATIONS", a.KZ_DENOISE_MAX_ITERATIONS)):
        assert int(re.search(r"#define %s\s+(\d+)u" % n, src).group(1)) == v


def test_opts_struct_is_32_bytes(kz, tmp_path):
    assert c_layout(tmp_path, "kazen_mi355x_denoise.h", ["sizeof(KzDenoiseOpts)", "offsetof(KzDenoiseOpts, flags)", "offsetof(KzDenoiseOpts, sigmaDepth)"]) == ["32", "8", "24"]
    o = kz.abi.KzDenoiseOpts
    assert C.sizeof(o) == 32 and o.flags.offset == 8 and o.sigmaDepth.offset == 24


def test_refusals_without_a_device(kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    # bad options are refused before a replica is looked for, and the message names the call
    for bad in BAD_OPTS:
        refused(kz, lambda: sc.denoise(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise")
    for g in ("albedo", 7, 8):
        refused(kz, lambda: sc.denoise(guides=g), a.KZ_ERR_INVALID_ARG, "kz_denoise", "guides")      # the scene's mask is 0
    sc.set_aovs(["albedo", "depth"])
    refused(kz, lambda: sc.denoise(guides="normal"), a.KZ_ERR_INVALID_ARG, "kz_denoise", "guides")
    # good options: the scene is on no device, the existing error
    for good in ({}, {"guides": "albedo"}, {"iterations": 8, "sigma_color": 2.0, "flags": 3}):
        refused(kz, lambda: sc.denoise(**good), a.KZ_ERR_STATE, "kz_scene_upload")
    refused(kz, lambda: sc.denoise(device=0), a.KZ_ERR_STATE)
    refused(kz, sc.denoised_film, a.KZ_ERR_STATE)
    refused(kz, sc.denoised_srgb8, a.KZ_ERR_STATE)
    refused(kz, sc.denoise_info, a.KZ_ERR_STATE)
    refused(kz, sc.denoise_release, a.KZ_ERR_STATE)
    lib = a.load_library()
    assert lib.kz_denoise(None, None) == a.KZ_ERR_INVALID_ARG
    # the test surface checks its arguments and options first, then asks for the device
    film = np.ones((5, 7, 4), np.float32)
    for bad in BAD_OPTS:
        refused(kz, lambda: kz.denoise_films(film, **bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_films")
    refused(kz, lambda: kz.denoise_films(film, guides="normal"), a.KZ_ERR_INVALID_ARG, "kz_denoise_films", "guides")      # no normal film given
    refused(kz, lambda: kz.denoise_films(film, border=3), a.KZ_ERR_INVALID_ARG, "kz_denoise_films")                     # nothing left of the frame
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.denoise_films(film), a.KZ_ERR_NO_DEVICE)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", [dict(), dict(iterations=2, demodulate=False), dict(iterations=8, use_guides=False), dict(iterations=3, sigmas=(0.5, 0.6, 0.3, 0.4))])
def test_reference_agrees_with_numpy(kz, ref, case):
    """To 1e-5 relative: the float64 restatement differs from the fp32 one by the ~26 roundings of 2^-24 a pixel's sums see per iteration, and by the relative error of
    a tap weight, arg x 2^-23, which matters only where the weight does (arg of a few units)."""
    b = 2
    colour, albedo, normal, depth = synthetic_films(37, 29, b, seed=11)
    sig = case.get("sigmas", (1.0, 0.3, 0.1, 0.1))
    opts = {k: v for k, v in case.items() if k != "sigmas"}
    got = ref_denoise(ref, kz, colour, albedo, normal, depth, border=b, sigma_color=sig[0], sigma_normal=sig[1], sigma_depth=sig[2], sigma_albedo=sig[3], **opts)
    want = np_denoise(colour, albedo, normal, depth, border=b, sigmas=sig, **opts)
    assert np.isfinite(got).all()
    assert np.array_equal(got[..., 3], want[..., 3]) and 0.9 < got[b:-b, b:-b, 3].mean() < 0.99
    assert not got[:b].any() and not got[-b:].any() and not got[:, :b].any() and not got[:, -b:].any()      # the apron
    err = np.abs(got[..., :3] - want[..., :3]) / np.maximum(np.abs(want[..., :3]), 1e-30)
    assert err[want[..., :3] != 0].max() < 1e-5, float(err[want[..., :3] != 0].max())
    # it did filter: the result is not the input, and with guides it is not the unguided result
    assert np.abs(frame_rgb(got, b) - frame_rgb(colour, b)).max() > 0.01


@pytest.mark.parametrize("subset", range(8))
def test_a_constant_colour_comes_back(kz, ref, subset):
    """Whatever the guides make of the weights, a weighted mean of equal values is that value: 25 products, 24 additions and one division per iteration round it,
    26 roundings of 2^-24 in the worst case and far fewer in the mean - over 5 iterations below 1e-5 relative. With demodulation the filtered signal is c / max(a, 1e-3),
    constant only where the albedo is: checked with a constant albedo (two more roundings)."""
    b = 1
    colour, albedo, normal, depth = synthetic_films(41, 23, b, seed=3)
    value = np.array([0.37, 1.9, 0.004], np.float32)
    colour[..., :3] = value * colour[..., 3:]
    films = [f if subset & (1 << k) else None for k, f in enumerate((albedo, normal, depth))]
    out = ref_denoise(ref, kz, colour, *films, border=b, demodulate=False)
    ok = out[..., 3] == 1
    assert ok.sum() > 800 and np.array_equal(ok[b:-b, b:-b], colour[b:-b, b:-b, 3] != 0)
    assert (np.abs(out[ok][:, :3] / value - 1).max()) < 1e-5
    if subset & 1:
        flat = albedo.copy()
        flat[..., :3] = np.array([0.3, 0.0, 0.7], np.float32) * flat[..., 3:]
        out = ref_denoise(ref, kz, colour, flat, films[1], films[2], border=b)
        assert (np.abs(out[ok][:, :3] / value - 1).max()) < 1e-5


def test_an_edge_in_the_normals_holds_and_blurs_without_guides(kz, ref):
    """Two half-planes of colour 0 and 1 whose normals are perpendicular, default sigmas: |n_q - n_p|^2 = 2, so a tap across the edge weighs at most
    exp(-2 / 0.09) = 2.2e-10 of the centre's - each side keeps its colour to 1e-6. Colour weights alone let the edge blur: after iteration 0 the last pixel of
    the 0 side is R / (L + R) = 0.0221 with L = 3/8 + 1/4 + 1/16 (its own side) and R = (1/4 + 1/16) exp(-3) (three channels differ by 1); every later iteration
    is a weighted mean in which the pixel itself holds at least 9/64 of the weight (its centre tap, of a total below 1), so five iterations leave it above
    0.0221 (9/64)^4 = 8.6e-6 - eight times the bound the guided filter keeps."""
    w, h = 48, 20
    colour = np.ones((h, w, 4), np.float32)
    colour[:, :w // 2, :3] = 0
    normal = np.ones((h, w, 4), np.float32)
    normal[:, :w // 2, :3] = (1, 0, 0)
    normal[:, w // 2:, :3] = (0, 1, 0)
    out = ref_denoise(ref, kz, colour, None, normal, None)
    assert np.abs(out[:, :w // 2, :3]).max() < 1e-6 and np.abs(out[:, w // 2:, :3] - 1).max() < 1e-6
    assert (out[..., 3] == 1).all()
    r = 0.3125 * np.exp(-3.0)
    for kw in (dict(normal=normal, use_guides=False), dict()):
        once = ref_denoise(ref, kz, colour, iterations=1, **kw)
        assert np.abs(once[:, w // 2 - 1, :3] - r / (0.6875 + r)).max() < 1e-6
        blurred = ref_denoise(ref, kz, colour, **kw)
        assert blurred[:, w // 2 - 1, 0].min() > 8e-6 and blurred[:, w // 2, 0].max() < 1 - 8e-6


def test_zero_weight_pixels_neither_give_nor_receive(kz, ref):
    b = 2
    colour, albedo, normal, depth = synthetic_films(33, 27, b, seed=7)
    dead = colour[..., 3] == 0
    assert dead[b:-b, b:-b].sum() > 20
    out = ref_denoise(ref, kz, colour, albedo, normal, depth, border=b)
    assert not out[dead].any() and not out[:b].any() and not out[:, :b].any()
    # what a dead texel holds - in the picture and in the guides - and what the apron holds changes nothing
    c2, a2, n2, d2 = (f.copy() for f in (colour, albedo, normal, depth))
    inner = np.zeros_like(dead)
    inner[b:-b, b:-b] = True
    for f in (c2, a2, n2, d2):
        f[dead, :3] = 1e6
        f[~inner] = 123.0
    a2[dead] = 77.0
    c2[~inner, 3] = 5.0
    c2[dead, 3] = 0.0
    again = ref_denoise(ref, kz, c2, a2, n2, d2, border=b)
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32))
    # ... and a live pixel does count: reviving one changes its neighbours
    c3 = colour.copy()
    y, x = np.argwhere(dead & inner)[0]
    c3[y, x, 3] = 1.0
    assert not np.array_equal(ref_denoise(ref, kz, c3, albedo, normal, depth, border=b), out)


# ---------------------------------------------------------------- what it is worth
QUALITY = {"cornell": 0.5, "materials": 1.0, "textured": 1.0}


@pytest.mark.parametrize("scene", list(QUALITY))
def test_quality_on_the_oracles_films(kz, O, ref, tmp_path_factory, scene):
    """4 spp against 1024 spp at 96 x 72, default options, the oracle's canonical film and the AOV reference's feature films: the mean squared error of the
    frame's rgb values after the filter over the one before it. Deterministic; the ratios are recorded in DESIGN.md 4e."""
    make = {"cornell": kz.scenes.cornell_box, "materials": kz.scenes.materials_scene, "textured": kz.scenes.textured_scene}[scene]
    noisy_desc, clean_desc = make(96, 72, 4), make(96, 72, 1024)
    ora = O.OracleScene(noisy_desc)
    noisy = ora.render_canonical(threads=0)
    clean = O.OracleScene(clean_desc).render_canonical(threads=0)
    b = (noisy.shape[0] - 72) // 2
    aov = AovRef(lib("aov", tmp_path_factory.mktemp("kza")), noisy_desc)
    films = [aov.film(a) for a in GUIDES]
    out = ref_denoise(ref, kz, noisy, *films, border=b)
    want = frame_rgb(clean, b).astype(np.float64)
    mse = lambda f: float(((frame_rgb(f, b).astype(np.float64) - want) ** 2).mean())
    ratio = mse(out) / mse(noisy)
    print("denoise quality %s: mse noisy %.6g, denoised %.6g, ratio %.4f" % (scene, mse(noisy), mse(out), ratio))
    assert ratio < QUALITY[scene], ratio
