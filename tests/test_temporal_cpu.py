"""The temporal stage of the denoiser (include/kazen_mi355x_temporal.h) without a GPU: the header against the library's exports, kz_temporal_view against the
oracle's camera rays and against itself, the refusals that need no device, the test-only CPU reference (tests/cpu_ref/kz_temporal_ref.cpp) the GPU tests compare
against - checked here against the variance-guided reference where the two must agree to the bit, on a two-view case whose answer is known, and against a float64
numpy restatement - and what the history is worth on the oracle's own films."""
import ctypes as C

import numpy as np
import pytest

from checks import c_layout, header_surface, refused, same_bits_strict
from cpu_refs import AovRef, MomentRef, lib, ref_denoise_temporal, ref_denoise_variance
from film_cases import BAD_OPTS, BAD_TOPTS, BAD_VOPTS, GUIDES, _orbit, camera_of, frame_rgb, quality_inputs, random_history, synthetic_films, synthetic_moment, view_arrays


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("temporal", tmp_path_factory.mktemp("kzt"))


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return lib("variance", tmp_path_factory.mktemp("kzv"))


# ---------------------------------------------------------------- 1. ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: disjoint from every other list, and nothing added to the existing headers
    header_surface(kz, "include/kazen_mi355x_temporal.h", a.TEMPORAL_EXPORTS, 6, [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS, a.VARIANCE_EXPORTS],
                   ["include/kazen_mi355x.h", "include/kazen_mi355x_dev.h", "include/kazen_mi355x_edit.h", "include/kazen_mi355x_aov.h", "include/kazen_mi355x_denoise.h",
                    "include/kazen_mi355x_variance.h"], ["kz_temporal", "kz_denoise_temporal", "kztemporal"])


def test_struct_sizes(kz, tmp_path):
    assert c_layout(tmp_path, "kazen_mi355x_temporal.h", ["sizeof(KzTemporalView)", "offsetof(KzTemporalView, a)", "offsetof(KzTemporalView, inv)", "offsetof(KzTemporalView, reserved)",
                                                          "sizeof(KzTemporalOpts)", "offsetof(KzTemporalOpts, normalTolerance)", "offsetof(KzTemporalOpts, maxHistory)",
                                                          "offsetof(KzTemporalOpts, flags)", "offsetof(KzTemporalOpts, reserved)"]) == ["96", "12", "48", "84", "32", "4", "8", "12", "16"]
    v, o = kz.abi.KzTemporalView, kz.abi.KzTemporalOpts
    assert C.sizeof(v) == 96 and (v.o.offset, v.a.offset, v.u.offset, v.v.offset, v.inv.offset, v.reserved.offset) == (0, 12, 24, 36, 48, 84)
    assert C.sizeof(o) == 32 and (o.depthTolerance.offset, o.normalTolerance.offset, o.maxHistory.offset, o.flags.offset, o.reserved.offset) == (0, 4, 8, 12, 16)


# ---------------------------------------------------------------- 2. / 3. the view
def _view_cameras(kz):
    rng = np.random.default_rng(5)
    cams = {"cornell": kz.scenes.cornell_box(96, 72, 4).camera, "textured": kz.scenes.textured_scene(160, 96, 4).camera,
            "thinlens": dict(kz.scenes.cornell_box(96, 72, 4).camera, type="thinlens", apertureRadius=0.05, focusDistance=3.0)}
    for k in range(3):
        o = rng.uniform(-5, 5, 3)
        cams["random%d" % k] = camera_of(kz, 200 + 37 * k, 120 + 11 * k, o, o + rng.normal(size=3), fov=float(rng.uniform(20, 90)))
    return cams


@pytest.mark.parametrize("name", ["cornell", "textured", "thinlens", "random0", "random1", "random2"])
def test_view_agrees_with_the_oracles_camera_rays(kz, O, name):
    """(a + sx u + sy v) normalised against the oracle's Camera::sampleRay direction at pixel centres, 1e-5 per component: the words are formed in double and narrowed
    once, cameraRay is an fp32 chain - a few ulp of a unit vector. The thin-lens camera with the lens sample that lands on the lens centre, (0, 0): radius sqrt(0)."""
    cam = _view_cameras(kz)[name]
    d = kz.scenes.cornell_box(cam["width"], cam["height"], 1)
    d.camera = cam
    ora = O.OracleScene(d)
    view = kz.temporal_view(cam)
    o, a, u, v, inv = view_arrays(view)
    assert not any(view.reserved)
    W, H = cam["width"], cam["height"]
    worst = 0.0
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 3, 2 * H // 3), (5, H - 7)]:
        sx, sy = x + 0.5, y + 0.5
        ray = ora.camera_ray(sx, sy, 0.0, 0.0)[0] if name == "thinlens" else ora.camera_ray(sx, sy)[0]
        d3 = a + sx * u + sy * v
        d3 /= np.linalg.norm(d3)
        worst = max(worst, float(np.abs(d3 - ray[3:6].astype(np.float64)).max()))
        assert np.abs(o - ray[:3].astype(np.float64)).max() < 1e-5
    assert worst < 1e-5, worst
    # inv is the inverse of (u | v | a)
    assert np.abs(inv @ np.stack([u, v, a], axis=1) - np.eye(3)).max() < 1e-5


def test_view_round_trip(kz):
    """inv (o + t d - o) = l (sx, sy, 1) gives back (sx, sy) within 0.01 pixel, in fp32 as the stage computes it, at frames up to 4096 wide: fp32 rounding at that
    coordinate is 4096 x 2^-23 ~ 5e-4, 0.01 is twenty times that and two orders below anything the bilinear weights can show. t is the distance along the
    normalised direction (the view's a is a point of the near plane, 1e-4 from the origin). The cameras stand within 0.05 of the world's origin: X = o + t d is
    rounded to half an ulp of |X|, and a pixel of a 4096-wide frame at distance 0.1 is 4e-6 to 4e-5 wide - a camera 20 units out would know X to 1e-6, a quarter
    of such a pixel, whatever the view's arithmetic; that is the scale of fp32 world coordinates, which the caller chooses, not a property of the view."""
    rng = np.random.default_rng(9)
    f = np.float32
    for W, H, fov in ((64, 48, 40.0), (1920, 1080, 30.0), (4096, 2160, 75.0), (4096, 1716, 12.0)):
        o0 = rng.uniform(-0.05, 0.05, 3)
        view = kz.temporal_view(camera_of(kz, W, H, o0, o0 + rng.normal(size=3), fov=fov))
        o, a, u, v, inv = (x.astype(f) for x in view_arrays(view))
        sxy = np.concatenate([rng.uniform(0, 1, (200, 2)) * (W, H), [[0.5, 0.5], [W - 0.5, H - 0.5], [W - 0.5, 0.5], [0.5, H - 0.5]]]).astype(f)
        d = a + sxy[:, :1] * u + sxy[:, 1:] * v
        d = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
        assert d.dtype == f
        for t in (0.1, 1.0, 100.0):
            q = (o + d * f(t)) - o
            P = q @ inv.T
            assert P.dtype == f and (P[:, 2] > 0).all()
            back = P[:, :2] / P[:, 2:]
            assert np.abs(back.astype(np.float64) - sxy).max() < 0.01, (W, H, t, float(np.abs(back - sxy).max()))


# ---------------------------------------------------------------- 4. refusals
def test_refusals_without_a_device(kz):
    a = kz.abi
    lib = a.load_library()
    # kz_temporal_view: a singular matrix (a toWorld that flattens the camera's x axis), a toWorld that is not affine, an unsupported type, null pointers
    cam = camera_of(kz, 64, 48, (0, 0, 0), (0, 0, 1))
    flat = np.array(cam["toWorld"], np.float32).reshape(4, 4).copy()
    flat[:3, 0] = 0.0
    refused(kz, lambda: kz.temporal_view(dict(cam, toWorld=flat)), a.KZ_ERR_UNSUPPORTED, "kz_temporal_view", "singular")
    persp = np.array(cam["toWorld"], np.float32).reshape(4, 4).copy()
    persp[3, 0] = 0.25
    refused(kz, lambda: kz.temporal_view(dict(cam, toWorld=persp)), a.KZ_ERR_UNSUPPORTED, "kz_temporal_view", "not affine")
    refused(kz, lambda: kz.temporal_view(dict(cam, type="orthographic")), a.KZ_ERR_UNSUPPORTED)
    assert lib.kz_temporal_view(None, None) == a.KZ_ERR_INVALID_ARG
    assert not any(kz.temporal_view(cam).reserved)
    # kz_denoise_temporal: bad options of each of the three structs first, then the state, all before a replica is looked for
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert lib.kz_denoise_temporal(None, -1, None, None, None) == a.KZ_ERR_INVALID_ARG
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: sc.denoise_temporal(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal")
    for bad in BAD_TOPTS:
        refused(kz, lambda: sc.denoise_temporal(**bad), a.KZ_ERR_INVALID_ARG, "KzTemporalOpts")
    refused(kz, sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "KZ_AOV_DEPTH", "mask 0")
    sc.set_aovs(["albedo", "normal"])
    refused(kz, sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "KZ_AOV_DEPTH", "mask 3")
    sc.set_aovs(GUIDES)
    refused(kz, sc.denoise_temporal, a.KZ_ERR_STATE, "kz_denoise_temporal", "switched off")
    refused(kz, lambda: sc.denoise_temporal(guides=["albedo", "normal"]), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal", "KZ_AOV_DEPTH")
    sc.set_variance(True)
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: sc.denoise_temporal(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal")
    for good in ({}, {"samples": 4, "max_history": 65535, "depth_tolerance": 0.5, "normal_tolerance": 2.0, "iterations": 8}):
        refused(kz, lambda: sc.denoise_temporal(**good), a.KZ_ERR_STATE, "kz_scene_upload")      # the scene is on no device
    for fn in (sc.temporal_info, sc.temporal_reset, sc.temporal_history):
        refused(kz, fn, a.KZ_ERR_STATE, "kz_scene_upload")
    # the test surface checks its arguments and options first, then the sample count, then asks for the device
    film = np.ones((5, 7, 4), np.float32)
    view = kz.temporal_view(camera_of(kz, 7, 5, (0, 0, 0), (0, 0, 1)))
    ok = dict(depth=film, samples=4, current=view)
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: kz.denoise_temporal_films(film, film, **ok, **bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, samples=4, current=view), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films", "depth")
    refused(kz, lambda: kz.denoise_temporal_films(film, None, **ok), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, depth=film, samples=4), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films", "view")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, **ok, history=np.zeros((5, 7, 12), np.float32)), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films", "view")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, film, **ok, guides="albedo"), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films", "KZ_AOV_DEPTH")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, **ok, border=3), a.KZ_ERR_INVALID_ARG, "kz_denoise_temporal_films")
    refused(kz, lambda: kz.denoise_temporal_films(film, film, depth=film, current=view), a.KZ_ERR_STATE, "kz_denoise_temporal_films", "samples = 0")
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.denoise_temporal_films(film, film, **ok), a.KZ_ERR_NO_DEVICE)


# ---------------------------------------------------------------- 5. identities
def _guide_subsets():
    """(albedo?, normal?) - depth is always among the guides."""
    return [(al, no) for al in (False, True) for no in (False, True)]


@pytest.mark.parametrize("frame", [(1, 1), (7, 5), (64, 33)])
@pytest.mark.parametrize("border", [0, 2])
def test_identities(kz, ref, vref, frame, border):
    """Without a history, and with maxHistory = 1 whatever the history holds, the result has the variance-guided reference's bits; a frame's own history fed back with
    the same view counts 2 in every valid pixel with z > 0 (the reprojection of a pixel centre lands on the pixel: |s - x| far below 1, and whichever of the four
    taps carry the weight, each of them that is valid and passes agrees; the pixel's own record always passes) and 1 where z == 0."""
    w, h = frame
    b = border
    colour, albedo, normal, depth = synthetic_films(w, h, b, seed=31 * w + h + b)
    moment = synthetic_moment(colour, seed=w + 7 * h + b)
    view = kz.temporal_view(camera_of(kz, w, h, (0.3, -0.2, 1.0), (0.1, 0.4, 9.0), fov=47.0))
    other = kz.temporal_view(camera_of(kz, w, h, (0.35, -0.2, 1.0), (0.1, 0.4, 9.0), fov=47.0))
    inner = (slice(b, b + h), slice(b, b + w))
    for al, no in _guide_subsets():
        given = [albedo if al else None, normal if no else None, depth]
        for demodulate in (True, False):
            kw = dict(border=b, samples=4, demodulate=demodulate, iterations=2)
            want, wv = ref_denoise_variance(vref, kz, colour, moment, *given, **kw)
            got, hist, gv = ref_denoise_temporal(ref, kz, colour, moment, *given, current=view, **kw)
            assert same_bits_strict(got, want) and same_bits_strict(gv, wv), (frame, b, al, no, demodulate)
            valid = colour[inner][..., 3] != 0
            assert np.array_equal(hist[..., 8], valid.astype(np.float32)) and not hist[..., 9:].any() and not hist[~valid].any()
            junk = random_history(w, h, seed=5)
            got, hist1, gv = ref_denoise_temporal(ref, kz, colour, moment, *given, current=view, previous=other, history=junk, max_history=1, **kw)
            assert same_bits_strict(got, want) and same_bits_strict(gv, wv) and same_bits_strict(hist1, hist)
            # the frame's own history, the same view
            _, hist2, _ = ref_denoise_temporal(ref, kz, colour, moment, *given, current=view, previous=view, history=hist, max_history=32, **kw)
            z = np.where(depth[inner][..., 3] != 0, depth[inner][..., 0] / np.where(depth[inner][..., 3] == 0, 1, depth[inner][..., 3]), 0)
            assert np.array_equal(hist2[..., 8], np.where(valid, np.where(z > 0, 2.0, 1.0), 0.0).astype(np.float32)), (frame, b, al, no, demodulate)
            assert same_bits_strict(hist2[..., 4:8], hist[..., 4:8])


# ---------------------------------------------------------------- 6. two views of a plane
def np_temporal(film, moment, albedo, normal, depth, border, samples, current, previous, history, demodulate=True, depth_tolerance=0.05, normal_tolerance=0.5, max_history=32):
    """The stage of the header in float64 numpy, s - c * c in fp32 as np_denoise_variance takes it: (e, v, N) per frame pixel, before the spatial filter."""
    b = border
    rows, cols = film.shape[:2]
    h, w = rows - 2 * b, cols - 2 * b

    def values(f):
        if f is None:
            return np.zeros((h, w, 3), np.float32)
        f = np.asarray(f, np.float32)[b:rows - b, b:cols - b]
        wgt = f[..., 3:]
        return np.where(wgt != 0, f[..., :3] / np.where(wgt == 0, np.float32(1), wgt), np.float32(0))

    c32, s32 = values(film), values(moment)
    c, a, n, z = c32.astype(np.float64), values(albedo).astype(np.float64), values(normal).astype(np.float64), values(depth)[..., 0].astype(np.float64)
    valid = np.asarray(film)[b:rows - b, b:cols - b, 3] != 0
    demodulate = demodulate and albedo is not None
    am = np.maximum(a, np.float32(1e-3))
    var = np.maximum(s32 - c32 * c32, np.float32(0)).astype(np.float64) / float(samples)
    e = c / am if demodulate else c.copy()
    v = (var / (am * am)).sum(axis=2) if demodulate else var.sum(axis=2)
    N = valid.astype(np.float64)
    if history is None or max_history == 1:
        return e, v, N
    o, va, vu, vv, _ = view_arrays(current)
    po, _, _, _, pinv = view_arrays(previous)
    yy, xx = np.mgrid[0:h, 0:w]
    d = va + (xx[..., None] + 0.5) * vu + (yy[..., None] + 0.5) * vv
    X = o + d * (z / np.linalg.norm(d, axis=2))[..., None]
    q = X - po
    P = q @ pinv.T
    with np.errstate(divide="ignore", invalid="ignore"):
        sx, sy = P[..., 0] / P[..., 2] - 0.5, P[..., 1] / P[..., 2] - 0.5
    ok = valid & (z > 0) & (P[..., 2] > 0) & (sx >= -1) & (sx < w) & (sy >= -1) & (sy < h)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    tx, ty = sx - x0, sy - y0
    zp = np.linalg.norm(q, axis=2)
    hist = np.asarray(history, np.float64).reshape(h, w, 12)
    Wb, E, V, M = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    for j in (0, 1):
        for i in (0, 1):
            hx, hy = x0 + i, y0 + j
            inside = (hx >= 0) & (hx < w) & (hy >= 0) & (hy < h)
            rec = hist[np.clip(hy, 0, h - 1), np.clip(hx, 0, w - 1)]
            use = ok & inside & (rec[..., 8] != 0) & (np.abs(rec[..., 7] - zp) <= depth_tolerance * np.maximum(zp, 1e-20)) & \
                (((rec[..., 4:7] - n) ** 2).sum(axis=2) <= np.float64(np.float32(normal_tolerance)) ** 2)
            bw = np.where(use, (tx if i else 1 - tx) * (ty if j else 1 - ty), 0.0)
            Wb += bw
            E += bw[..., None] * rec[..., :3]
            V += bw * rec[..., 3]
            M += bw * rec[..., 8]
    has = ok & (Wb > 1e-3)
    safe = np.where(has, Wb, 1.0)
    Nn = np.minimum(M / safe + 1.0, float(max_history))
    al = 1.0 / np.where(has, Nn, 1.0)
    om = 1.0 - al
    e = np.where(has[..., None], om[..., None] * (E / safe[..., None]) + al[..., None] * e, e)
    v = np.where(has, om * om * (V / safe) + al * al * v, v)
    N = np.where(has, Nn, N)
    return e, v, N


def _plane_case(kz, view, w, h, D, grad):
    """Films of the plane z = D (the cameras look along +z) seen through `view`: depth is the distance along each pixel's ray, the normal (0, 0, -1), the colour a
    linear ramp in world x and y, albedo 1, moment c^2, weight 1 everywhere. Returns (films, the ramp per pixel in float64)."""
    o, a, u, v, _ = view_arrays(view)
    yy, xx = np.mgrid[0:h, 0:w]
    d = a + (xx[..., None] + 0.5) * u + (yy[..., None] + 0.5) * v
    X = o + d * ((D - o[2]) / d[..., 2])[..., None]
    ramp = 0.5 + X[..., :1] * grad[0] + X[..., 1:2] * grad[1]                     # (h, w, 3)
    assert ramp.min() >= 0.0 and ramp.max() <= 1.0
    one = np.ones((h, w, 1), np.float32)
    film = lambda val: np.concatenate([np.broadcast_to(np.asarray(val, np.float32), (h, w, 3)), one], axis=2).astype(np.float32)
    colour = film(ramp)
    depth = film(np.repeat(np.linalg.norm(X - o, axis=2)[..., None], 3, axis=2))
    c32 = colour[..., :3]
    return (colour, film(c32 * c32), film(1.0), film((0.0, 0.0, -1.0)), depth), ramp


def test_two_views_of_a_plane(kz, ref):
    w, h, D = 64, 48, 4.0
    cam1 = camera_of(kz, w, h, (0, 0, 0), (0, 0, 1), fov=40.0)
    v1 = kz.temporal_view(cam1)
    o, a, u, v, inv = view_arrays(v1)
    pix = D * np.linalg.norm(u) / a[2]                                # a pixel's footprint on the plane
    shift = np.array([2.37 * pix, -1.6 * pix, 0.0])
    v2 = kz.temporal_view(camera_of(kz, w, h, shift, shift + (0, 0, 1), fov=40.0))
    extent = D * np.tan(np.radians(20.0)) + 3 * pix                   # |x| of the plane the two frames see
    grad = (np.array([0.45, -0.3, 0.2]) / extent, np.array([0.04, 0.15, -0.25]) / extent)      # |ramp - 0.5| <= 0.49 over both frames, ~1/64 per pixel at most
    films1, _ = _plane_case(kz, v1, w, h, D, grad)
    films2, ramp2 = _plane_case(kz, v2, w, h, D, grad)
    kw = dict(border=0, samples=4, iterations=1)
    _, hist1, _ = ref_denoise_temporal(ref, kz, *films1, current=v1, **kw)
    assert (hist1[..., 8] == 1).all()
    _, hist2, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=hist1, **kw)
    # where frame 2's pixels land in frame 1, in float64
    o2, a2, u2, vv2, _ = view_arrays(v2)
    yy, xx = np.mgrid[0:h, 0:w]
    d = a2 + (xx[..., None] + 0.5) * u2 + (yy[..., None] + 0.5) * vv2
    X = o2 + d * (D / d[..., 2])[..., None]
    P = (X - o) @ inv.T
    px, py = P[..., 0] / P[..., 2], P[..., 1] / P[..., 2]             # continuous pixel coordinates of frame 1 (a pixel centre at + 0.5)
    assert abs(abs(np.median(px - (xx + 0.5))) - 2.37) < 1e-3 and abs(abs(np.median(py - (yy + 0.5))) - 1.6) < 1e-3      # the cameras are 2.37 and 1.6 pixels apart
    inside = (px >= 1.5) & (px <= w - 1.5) & (py >= 1.5) & (py <= h - 1.5)      # all four taps at least one pixel inside: the reprojection a pixel inside the frame
    outside = (px - 0.5 < -1) | (px - 0.5 >= w) | (py - 0.5 < -1) | (py - 0.5 >= h)
    assert inside.sum() > 0.8 * w * h and (~inside).sum() > 100
    N, e = hist2[..., 8], hist2[..., :3].astype(np.float64)
    assert (N[inside] == 2).all(), int((N[inside] != 2).sum())
    assert (N[outside] == 1).all()
    err = np.abs(e - ramp2)[inside]
    print("two views of a plane: %d pixels with history, max |e - ramp| = %.3g" % (int(inside.sum()), float(err.max())))
    assert err.max() < 1e-4, float(err.max())
    assert np.array_equal(hist2[..., 7], films2[4][..., 0]) and (hist2[..., 6] == -1).all()
    # the variance of a two-frame mean: (v_h + v_cur) / 4 - zero here up to the rounding of s - c c
    assert (hist2[..., 3] >= 0).all()
    # turned round: every point is behind the history's camera
    back = kz.temporal_view(camera_of(kz, w, h, shift, shift - (0, 0, 1), fov=40.0))
    filmsb, _ = _plane_case(kz, back, w, h, -D, grad)
    _, histb, _ = ref_denoise_temporal(ref, kz, *filmsb, current=back, previous=v1, history=hist1, **kw)
    assert (histb[..., 8] == 1).all()
    # the history's depth off by a fifth: every tap is rejected
    far = hist1.copy()
    far[..., 7] *= 1.2
    _, histf, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=far, **kw)
    assert (histf[..., 8] == 1).all()
    # ... and a tolerance that admits it finds the history again; a normal that differs by more than the tolerance is rejected like the depth
    _, histw, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=far, depth_tolerance=0.25, **kw)
    assert (histw[..., 8][inside] == 2).all()
    tilted = hist1.copy()
    tilted[..., 4:7] = (0.6, 0.0, -0.8)                               # |n_h - n| = 0.632 > 0.5
    _, histn, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=tilted, **kw)
    assert (histn[..., 8] == 1).all()
    _, histn, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=tilted, normal_tolerance=0.7, **kw)
    assert (histn[..., 8][inside] == 2).all()
    # a longer history: counts follow min(N_h + 1, maxHistory)
    old = hist1.copy()
    old[..., 8] = 7.0
    _, histo, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=old, max_history=5, **kw)
    assert (histo[..., 8][inside] == 5).all()
    _, histo, _ = ref_denoise_temporal(ref, kz, *films2, current=v2, previous=v1, history=old, **kw)
    assert (histo[..., 8][inside] == 8).all()


@pytest.mark.parametrize("case", ["plane", "synthetic"])
def test_reference_agrees_with_numpy(kz, ref, case):
    """The stage against its float64 restatement, rtol 1e-4 wherever the two make the same tap decisions (they then have the same count N): the sums are four
    products, the blend three - a handful of roundings of 2^-24 each on values of one sign. A decision can flip where a tap sits at a threshold (depth, normal,
    Wb > 1e-3, the frame's edge): at most 1 % of the pixels are excused, and the reference must stay within that cap on these inputs."""
    if case == "plane":
        w, h, D = 64, 48, 4.0
        v1 = kz.temporal_view(camera_of(kz, w, h, (0, 0, 0), (0, 0, 1), fov=40.0))
        v2 = kz.temporal_view(camera_of(kz, w, h, (0.09, -0.06, 0.0), (0.09, -0.06, 1.0), fov=40.0))
        grad = (np.array([0.2, -0.15, 0.1]), np.array([0.02, 0.07, -0.12]))
        films, _ = _plane_case(kz, v2, w, h, D, grad)
        films1, _ = _plane_case(kz, v1, w, h, D, grad)
        _, history, _ = ref_denoise_temporal(ref, kz, *films1, current=v1, border=0, samples=4, iterations=1)
        history[..., 8] = np.random.default_rng(1).integers(1, 9, (h, w))
        history[..., 3] = np.random.default_rng(2).lognormal(-3, 1, (h, w))
        b = 0
    else:
        w, h, b = 70, 45, 2
        colour, albedo, normal, depth = synthetic_films(w, h, b, seed=77)
        films = (colour, synthetic_moment(colour, seed=78), albedo, normal, depth)
        v1 = kz.temporal_view(camera_of(kz, w, h, (0, 0, 0), (0, 0, 1), fov=40.0))
        v2 = kz.temporal_view(camera_of(kz, w, h, (0.02, 0.01, 0.0), (0.02, 0.01, 1.0), fov=40.0))
        # a history that fits: the frame's own, so that depth and normal tests pass in many taps, with random counts and a fifth of holes
        _, history, _ = ref_denoise_temporal(ref, kz, *films, current=v1, border=b, samples=4, iterations=1)
        rng = np.random.default_rng(3)
        history[..., 8] = np.where(history[..., 8] != 0, rng.integers(1, 40, (h, w)), 0)
        history[rng.random((h, w)) < 0.2] = 0.0
    _, got, _ = ref_denoise_temporal(ref, kz, *films, current=v2, previous=v1, history=history, border=b, samples=4, iterations=1)
    e, v, N = np_temporal(*films, border=b, samples=4, current=v2, previous=v1, history=history)
    same = got[..., 8].astype(np.float64) == N
    close_n = np.abs(got[..., 8] - N) <= 1e-4 * np.maximum(N, 1)      # (the count itself is a rounded mean)
    agree = same | close_n
    excused = 1.0 - agree.mean()
    blended = (got[..., 8] > 1).sum()
    print("temporal reference against numpy (%s): %d pixels blended, %.2f %% excused for a decision at a threshold" % (case, int(blended), 100 * excused))
    assert blended > 0.3 * w * h and excused <= 0.01, (int(blended), excused)
    ge, gv = got[..., :3].astype(np.float64), got[..., 3].astype(np.float64)
    valid = got[..., 8] != 0
    m = agree & valid
    assert np.abs(ge - e)[m].max() <= 1e-4 * np.abs(e)[m].max() and (np.abs(ge - e)[m] <= 1e-4 * np.maximum(np.abs(e)[m], 1e-3)).all()
    assert (np.abs(gv - v)[m] <= 1e-4 * np.maximum(np.abs(v)[m], 1e-12)).all()


# ---------------------------------------------------------------- 7. what it is worth
def _sequence(kz, ref, aov_lib, make, frames, step_degrees):
    """The reference chain over `frames` frames of 4 spp from the sample ranges [4f, 4f + 4), the camera turned by step_degrees per frame. Returns the last
    frame's description, its temporal result, its variance-guided result on the frame alone, and its noisy film."""
    history, prev, last = None, None, None
    for f in range(frames):
        d = _orbit(kz, make(96, 72, 4), f * step_degrees) if step_degrees else make(96, 72, 4)
        mr = MomentRef(ref, d)
        b = mr.border
        noisy, moment = mr.film(4 * f, 4 * f + 4), mr.moment_film(4 * f, 4 * f + 4)
        aov = AovRef(aov_lib, d)
        films = [aov.film(g, 4 * f, 4 * f + 4) for g in GUIDES]
        view = kz.temporal_view(d.camera)
        out, history, _ = ref_denoise_temporal(ref, kz, noisy, moment, *films, border=b, samples=4, current=view, previous=prev, history=history)
        prev, last = view, (d, out, noisy, moment, films, b)
    d, out, noisy, moment, films, b = last
    alone, _, _ = ref_denoise_temporal(ref, kz, noisy, moment, *films, border=b, samples=4, current=prev)
    return d, out, alone, noisy, int(history[..., 8].max())


@pytest.mark.parametrize("scene", ["cornell", "materials", "textured"])
def test_quality_on_the_oracles_films(kz, O, ref, vref, tmp_path_factory, scene):
    """The setting of test_variance_cpu.test_quality_on_the_oracles_films - 96 x 72, 4 spp frames against 1024 spp, default options - with eight frames folded into
    the history: the MSE of frame 8's result is strictly below that of the variance-guided filter on frame 8 alone (asserted on Cornell, static camera; printed for
    the other scenes and for a camera that orbits by 2 degrees per frame; recorded in DESIGN.md 4g)."""
    make = {"cornell": kz.scenes.cornell_box, "materials": kz.scenes.materials_scene, "textured": kz.scenes.textured_scene}[scene]
    aov_lib = lib("aov", tmp_path_factory.mktemp("kza"))
    clean, _ = quality_inputs(kz, O, vref, tmp_path_factory, scene)      # (shared with test_variance_cpu when both run: the 1024 spp film is the expensive one)
    b = (clean.shape[0] - 72) // 2
    mse = lambda f, want: float(((frame_rgb(f, b).astype(np.float64) - want) ** 2).mean())
    want = frame_rgb(clean, b).astype(np.float64)
    d, out, alone, noisy, longest = _sequence(kz, ref, aov_lib, make, 8, 0.0)
    static = (mse(out, want) / mse(noisy, want), mse(alone, want) / mse(noisy, want))
    print("temporal quality %s static, frame 8 of 4 spp: MSE ratio temporal %.4f, frame alone %.4f (temporal / alone %.3f), longest history %d" % (scene, static[0], static[1], static[0] / static[1], longest))
    assert longest == 8
    if scene == "cornell":
        assert static[0] < static[1], static
    # a camera that orbits by 2 degrees per frame: against 1024 spp from the last camera
    d, out, alone, noisy, longest = _sequence(kz, ref, aov_lib, make, 8, 2.0)
    moved = O.OracleScene(_orbit(kz, make(96, 72, 256), 14.0)).render_canonical(threads=0)
    want = frame_rgb(moved, b).astype(np.float64)
    orbit = (mse(out, want) / mse(noisy, want), mse(alone, want) / mse(noisy, want))
    print("temporal quality %s orbit 2 deg / frame, frame 8 of 4 spp (against 256 spp): MSE ratio temporal %.4f, frame alone %.4f (temporal / alone %.3f), longest history %d" % (scene, orbit[0], orbit[1], orbit[0] / orbit[1], longest))
