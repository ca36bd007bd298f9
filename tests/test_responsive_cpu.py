"""The fast history and the clamp of include/kazen_mi355x_responsive.h without a GPU: the header against the library's exports, the refusals that need no device, and
the test-only CPU reference (tests/cpu_ref/kz_responsive_ref.cpp) the GPU tests compare against - checked here against the motion reference where the header's three
identities say the two agree to the bit, on a case whose every figure is a dyadic fraction, on a step edge against numpy in float64, and for what it is worth on the
oracle's films: a lamp that changes colour under a camera at rest (scripts/responsive_quality.py runs the same sequences at length)."""
import ctypes as C
import os

import numpy as np
import pytest

from checks import c_layout, header_surface, refused, same_bits_strict
from cpu_refs import lib, ref_denoise_motion, ref_denoise_responsive
from film_cases import (BAD_OPTS, BAD_ROPTS, BAD_TOPTS, BAD_VOPTS, FRAMES, camera_of, chains, light_step, mse_ratio, plane_films, plane_history, quality_inputs, random_fast,
                        random_history, random_ids, reference_frames, row_tables, static_rows, synthetic_films, synthetic_moment)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("responsive", tmp_path_factory.mktemp("kzr"))


# ---------------------------------------------------------------- 1. ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: disjoint from every other list, and nothing added to the older headers
    older = sorted(n for n in os.listdir(os.path.join(ROOT, "include")) if n != "kazen_mi355x_responsive.h")
    assert len(older) == 8, older
    header_surface(kz, "include/kazen_mi355x_responsive.h", a.RESPONSIVE_EXPORTS, 4,
                   [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS, a.VARIANCE_EXPORTS, a.TEMPORAL_EXPORTS, a.MOTION_EXPORTS, a.DEV_ONLY_EXPORTS],
                   ["include/" + n for n in older], ["kz_responsive", "kz_denoise_responsive", "kzresponsive"], dev_required=True)
    assert a.KZ_RESPONSIVE_CLAMP_OFF == 1


def test_opts_struct_is_32_bytes(kz, tmp_path):
    assert c_layout(tmp_path, "kazen_mi355x_responsive.h", ["sizeof(KzResponsiveOpts)", "offsetof(KzResponsiveOpts, clampSigma)", "offsetof(KzResponsiveOpts, radius)",
                                                            "offsetof(KzResponsiveOpts, flags)", "offsetof(KzResponsiveOpts, reserved)", "KZ_RESPONSIVE_CLAMP_OFF"]) == ["32", "4", "8", "12", "16", "1"]
    r = kz.abi.KzResponsiveOpts
    assert C.sizeof(r) == 32 and (r.fastHistory.offset, r.clampSigma.offset, r.radius.offset, r.flags.offset, r.reserved.offset) == (0, 4, 8, 12, 16)


# ---------------------------------------------------------------- 2. refusals
def test_refusals_without_a_device(kz):
    a = kz.abi
    lib = a.load_library()
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert lib.kz_denoise_responsive(None, -1, None, None, None, None) == a.KZ_ERR_INVALID_ARG
    assert lib.kz_responsive_info(sc.h, -1, None) == a.KZ_ERR_INVALID_ARG
    # kz_denoise_responsive: kz_denoise_motion's refusals under its own name, and its own options', one bad field at a time - before the replica is looked up
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: sc.denoise_responsive(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_responsive")
    for bad in BAD_ROPTS:
        refused(kz, lambda: sc.denoise_responsive(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_responsive", "KzResponsiveOpts")
    refused(kz, sc.denoise_responsive, a.KZ_ERR_STATE, "kz_denoise_responsive", "KZ_AOV_DEPTH", "mask 0")
    sc.set_aovs(["albedo", "normal", "depth"])
    refused(kz, sc.denoise_responsive, a.KZ_ERR_STATE, "kz_denoise_responsive", "switched off")
    refused(kz, lambda: sc.denoise_responsive(guides=["albedo", "normal"]), a.KZ_ERR_INVALID_ARG, "kz_denoise_responsive", "KZ_AOV_DEPTH")
    sc.set_variance(True)
    for bad in BAD_ROPTS:                                             # (still before the replica)
        refused(kz, lambda: sc.denoise_responsive(**bad), a.KZ_ERR_INVALID_ARG, "KzResponsiveOpts")
    refused(kz, sc.denoise_responsive, a.KZ_ERR_STATE, "kz_scene_upload")      # the scene is on no device
    for fn in (sc.responsive_fast, sc.responsive_info):
        refused(kz, fn, a.KZ_ERR_STATE, "kz_scene_upload")
    # the test surface: arguments, options, ids and rows first, then the device
    film = np.ones((5, 7, 4), np.float32)
    view = kz.temporal_view(camera_of(kz, 7, 5, (0, 0, 0), (0, 0, 1)))
    rows, ids = static_rows(kz, 4), random_ids(7, 5, 4, seed=1)
    ok = dict(depth=film, samples=4, current=view, ids=ids, rows=rows)
    name = "kz_denoise_responsive_films"
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS + BAD_ROPTS:
        refused(kz, lambda: kz.denoise_responsive_films(film, film, **ok, **bad), a.KZ_ERR_INVALID_ARG, name)
    refused(kz, lambda: kz.denoise_responsive_films(film, film, samples=4, current=view, ids=ids, rows=rows), a.KZ_ERR_INVALID_ARG, name, "depth")
    refused(kz, lambda: kz.denoise_responsive_films(film, film, depth=film, samples=4, ids=ids, rows=rows), a.KZ_ERR_INVALID_ARG, name, "view")
    refused(kz, lambda: kz.denoise_responsive_films(film, film, depth=film, samples=4, current=view, rows=rows), a.KZ_ERR_INVALID_ARG, name, "ids")
    out_of_range = ids.copy()
    out_of_range[3, 2] = 4
    refused(kz, lambda: kz.denoise_responsive_films(film, film, **dict(ok, ids=out_of_range)), a.KZ_ERR_INVALID_ARG, name, "pixel (2, 3)", "mesh 4", "4 rows")
    both = static_rows(kz, 4)
    both[2].flags = 3
    refused(kz, lambda: kz.denoise_responsive_films(film, film, **dict(ok, rows=both)), a.KZ_ERR_INVALID_ARG, name, "row 2")
    negative = random_history(7, 5, seed=2, holes=0.0)
    negative[1, 4, 3] = -0.5
    refused(kz, lambda: kz.denoise_responsive_films(film, film, **ok, previous=view, history=negative), a.KZ_ERR_INVALID_ARG, name, "pixel (4, 1)", "negative variance")
    refused(kz, lambda: kz.denoise_responsive_films(film, film, depth=film, current=view, ids=ids, rows=rows), a.KZ_ERR_STATE, name, "samples = 0")
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.denoise_responsive_films(film, film, **ok), a.KZ_ERR_NO_DEVICE)


# ---------------------------------------------------------------- 3. the identities
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("border", [0, 2])
def test_identities_on_the_reference(kz, ref, frame, border):
    """The header's three identities, bit for bit, over the five row tables, a view that moved, random ids (misses among them), a random history and fast plane:
    1. CLAMP_OFF gives kz_motion_ref's picture, history and v_last; 2. so does a call without a history, and one in which no N_l exceeds fastHistory;
    3. with the fast plane absent and fastHistory >= maxHistory the fast plane is (e_l, v_l) - the history of the CLAMP_OFF call."""
    w, h = frame
    b = border
    colour, albedo, normal, depth = synthetic_films(w, h, b, seed=23 * w + h + b)
    films = (colour, synthetic_moment(colour, seed=w + 7 * h + b), albedo, normal, depth)
    at = lambda o: kz.temporal_view(camera_of(kz, w, h, o, (o[0], o[1], o[2] + 1), fov=50.0))
    pix = 2.0 * np.tan(np.radians(25.0)) / w
    cur, prev = at((1.5 * pix, -0.9 * pix, 0)), at((0, 0, 0))
    ids = random_ids(w, h, 4, seed=w + h + b, misses=0.15 if w * h >= 64 else 0.0)
    junk = random_history(w, h, seed=5 + w)
    fast = random_fast(junk, seed=6 + w)
    lenient = dict(depth_tolerance=20.0, normal_tolerance=3.0)
    clamped = 0
    for tname, rows in row_tables(kz, w).items():
        kw = dict(border=b, samples=4, current=cur, previous=prev, ids=ids, rows=rows, iterations=1, **lenient)
        want = ref_denoise_motion(ref, kz, *films, history=junk, **kw)
        # 1. CLAMP_OFF, whatever the other options and the fast plane
        for f, more in ((fast, dict(fast_history=2, clamp_sigma=0.5, radius=1)), (None, dict()), (fast, dict(fast_history=40))):
            got = ref_denoise_responsive(ref, kz, *films, history=junk, fast=f, clamp=False, **more, **kw)
            assert same_bits_strict(got[0], want[0]) and same_bits_strict(got[1], want[1]) and same_bits_strict(got[3], want[2]), (frame, b, tname, more)
        # ... and the clamp itself does something on this input (the random history's counts reach 40)
        on = ref_denoise_responsive(ref, kz, *films, history=junk, fast=fast, fast_history=2, clamp_sigma=0.5, radius=1, **kw)
        clamped += int((on[1][..., 8] != want[1][..., 8]).sum())
        # 2. no history: kz_motion_ref's bits (which are kz_variance_ref's there), a fast plane given is ignored; and no N_l above fastHistory
        first = ref_denoise_motion(ref, kz, *films, **dict(kw, previous=None))
        got = ref_denoise_responsive(ref, kz, *films, fast=fast, **dict(kw, previous=None))
        assert same_bits_strict(got[0], first[0]) and same_bits_strict(got[1], first[1]) and same_bits_strict(got[3], first[2]), (frame, b, tname)
        valid = first[1][..., 8] > 0
        assert same_bits_strict(got[2][..., :3][valid], first[1][..., :3][valid]) and same_bits_strict(got[2][..., 3][valid], first[1][..., 3][valid]) and not got[2][~valid].any()
        got = ref_denoise_responsive(ref, kz, *films, history=junk, fast=fast, fast_history=40, clamp_sigma=0.01, **kw)      # (N_l <= maxHistory = 32 < 40)
        assert same_bits_strict(got[0], want[0]) and same_bits_strict(got[1], want[1]) and same_bits_strict(got[3], want[2]), (frame, b, tname)
        got = ref_denoise_responsive(ref, kz, *films, history=junk, fast=fast, max_history=1, clamp_sigma=0.01, **kw)         # (maxHistory = 1: without history)
        one = ref_denoise_motion(ref, kz, *films, history=junk, max_history=1, **kw)
        assert same_bits_strict(got[0], one[0]) and same_bits_strict(got[1], one[1])
        # 3. the fast plane absent, fastHistory >= maxHistory: f == e_l, vf == v_l
        for fh, mh in ((32, 0), (7, 7), (65535, 32)):
            long_ = ref_denoise_motion(ref, kz, *films, history=junk, max_history=mh, **kw)
            got = ref_denoise_responsive(ref, kz, *films, history=junk, fast=None, fast_history=fh, max_history=mh, **kw)
            valid = long_[1][..., 8] > 0
            assert same_bits_strict(got[2][valid], long_[1][..., :4][valid]) and not got[2][~valid].any(), (frame, b, tname, fh)
            assert same_bits_strict(got[1], long_[1])
    assert clamped > 0 or w * h < 4, frame


# ---------------------------------------------------------------- 4. a case in dyadic fractions
@pytest.mark.parametrize("radius", [1, 2])
def test_exact_dyadic_case(kz, ref, radius):
    """One valid surface; the history holds colour 0.5, v = 0, N = 32 everywhere, the fast plane is absent, this frame's colour is 1.0 with zero variance, the views
    are identical, fastHistory = 4. Then at every pixel - the frame's corners, whose windows hold 4 or 9 texels, included - f = 3/4 * 1/2 + 1/4 = 0.625 exactly,
    the window's deviation is 0, and the long history's 31/32 * 1/2 + 1/32 = 0.515625 (which kz_motion_ref stores) is clamped to 0.625 with N = 4 and v = vf = 0."""
    w, h = 9, 7
    view, films, z = plane_films(kz, w, h, 1.0)
    hist = plane_history(z, 0.5, 32.0)
    kw = dict(border=0, samples=4, current=view, previous=view, history=hist, ids=np.zeros((h, w), np.uint32), rows=static_rows(kz, 1), iterations=1)
    _, mh, _ = ref_denoise_motion(ref, kz, *films, **kw)
    assert (mh[..., :3] == np.float32(0.515625)).all() and (mh[..., 8] == 32).all() and (mh[..., 3] == 0).all()
    _, rh, fast, _ = ref_denoise_responsive(ref, kz, *films, fast=None, fast_history=4, radius=radius, **kw)
    assert (fast[..., :3] == np.float32(0.625)).all() and (fast[..., 3] == 0).all()
    assert (rh[..., :3] == np.float32(0.625)).all() and (rh[..., 8] == 4).all() and (rh[..., 3] == 0).all()
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):    # the corners by name: cnt = (radius + 1)^2
        assert rh[y, x, 0] == np.float32(0.625) and rh[y, x, 8] == 4
    assert same_bits_strict(rh[..., 4:8], mh[..., 4:8])                           # (n, z) as the film has them
    # with the clamp off the same call stores kz_motion_ref's history and the same fast plane
    _, oh, ofast, _ = ref_denoise_responsive(ref, kz, *films, fast=None, fast_history=4, radius=radius, clamp=False, **kw)
    assert same_bits_strict(oh, mh) and same_bits_strict(ofast, fast)
    # fastHistory = 32 = N_l: the condition N_l > fastHistory fails, nothing is clamped
    _, eh, efast, _ = ref_denoise_responsive(ref, kz, *films, fast=None, fast_history=32, radius=radius, **kw)
    assert same_bits_strict(eh, mh) and same_bits_strict(efast[..., :3], mh[..., :3])


# ---------------------------------------------------------------- 5. a step edge in the fast plane
@pytest.mark.parametrize("radius", [1, 2])
def test_a_step_edge_widens_the_bounds(kz, ref, radius):
    """The fast plane holds 0.2 left of column 20 and 0.8 from it on, the long history and this frame 0.5 everywhere: e_l = 0.5 lies between the two sides. A window
    that holds both sides has a deviation near 0.2, so with clampSigma = 2 the pixels at the edge keep e_l and N = 32; a window of one side has deviation 0, so the
    pixels two windows away are clamped to that side's fast colour with N = 4. Every pixel's result equals clip(e_l, m - k sd, m + k sd) from the reference's own fast
    plane in float64 to 1e-6 relative (the window's sums are 9 or 25 fp32 additions: a few units of 2^-24)."""
    w, h, edge = 40, 11, 20
    view, films, z = plane_films(kz, w, h, 0.5)
    hist = plane_history(z, 0.5, 32.0)
    fin = np.zeros((h, w, 4), np.float32)
    fin[:, :edge, :3], fin[:, edge:, :3] = 0.2, 0.8
    kw = dict(border=0, samples=4, current=view, previous=view, history=hist, ids=np.zeros((h, w), np.uint32), rows=static_rows(kz, 1), iterations=1)
    _, mh, _ = ref_denoise_motion(ref, kz, *films, **kw)
    assert (mh[..., :3] == np.float32(0.5)).all()
    _, rh, fast, _ = ref_denoise_responsive(ref, kz, *films, fast=fin, fast_history=4, clamp_sigma=2.0, radius=radius, **kw)
    f = fast[..., :3].astype(np.float64)
    assert np.abs(f[:, :edge - 1] - 0.275).max() < 1e-5 and np.abs(f[:, edge + 1:] - 0.725).max() < 1e-5      # 3/4 of the fast plane + 1/4 of 0.5
    want = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            win = f[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].reshape(-1, 3)
            m, sd = win.mean(axis=0), win.std(axis=0)
            want[y, x] = np.clip(0.5, m - 2.0 * sd, m + 2.0 * sd)
    got = rh[..., :3].astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print("step edge, radius %d: max relative |e - clip| = %.3g" % (radius, float(rel.max())))
    assert rel.max() < 1e-6, float(rel.max())
    N = rh[..., 8]
    at_edge = slice(edge - 1, edge + 1)
    assert (N[:, at_edge] == 32).all() and same_bits_strict(rh[:, at_edge, :4], mh[:, at_edge, :4])      # the bounds widened: e_l kept
    away = 2 * (2 * radius + 1)
    far = np.ones(w, bool)
    far[edge - away:edge + away] = False
    assert far.sum() >= 10 and (N[:, far] == 4).all()
    assert np.abs(got[:, far] - f[:, far]).max() < 1e-6 and (rh[..., 3][:, far] == fast[..., 3][:, far]).all()      # clamped onto the fast colour, with its variance


# ---------------------------------------------------------------- 6. what it is worth
def test_quality_on_the_light_step(kz, O, ref, tmp_path_factory):
    """scripts/responsive_quality.py's light step at the defaults: Cornell, 96 x 72, a camera at rest, eight frames of 4 spp, then the lamp turns from white 15 to orange
    12 and eight more frames follow; MSE over the noisy frame's against 1024 spp of the new lighting. At frame 12 the responsive chain is strictly below the
    kz_motion_ref chain; and on the static sequence (no edit, frame 8) strictly below the frame alone. Every other figure is printed.

    Measured at the defaults (fastHistory 2, clampSigma 2, radius 1; this test's print): frame 9: responsive 5.9576, motion chain 10.7178, frame alone 0.1269; frame 12:
    0.2524, 5.3180, 0.0965; frame 16: 0.0790, 4.9172, 0.1686; static Cornell, frame 8: 0.0708, 0.0707, 0.1471."""
    aov_lib = lib("aov", tmp_path_factory.mktemp("kza"))
    frames = reference_frames(kz, ref, aov_lib, [light_step(kz, 4, f) for f in range(16)])
    clean = O.OracleScene(light_step(kz, 1024, 8)).render_canonical(threads=0)
    pics, hists, _ = chains(kz, ref, frames)
    b = frames[0][3]
    at = {}
    for f in (9, 12, 16):
        at[f] = {k: mse_ratio(v[f - 1], frames[f - 1][0], clean, b) for k, v in pics.items()}
        print("light step, frame %2d: MSE ratio responsive %.4f, motion chain %.4f, frame alone %.4f; longest history %d" % (
            f, at[f]["responsive"], at[f]["motion"], at[f]["alone"], int(hists[f - 1][..., 8].max())))
    # the static sequence: the first eight frames are it
    still, _ = quality_inputs(kz, O, ref, tmp_path_factory, "cornell")
    static = {k: mse_ratio(v[7], frames[7][0], still, b) for k, v in pics.items()}
    print("static cornell, frame 8: MSE ratio responsive %.4f, motion chain %.4f, frame alone %.4f" % (static["responsive"], static["motion"], static["alone"]))
    assert at[12]["responsive"] < at[12]["motion"], at[12]
    assert static["responsive"] < static["alone"], static
