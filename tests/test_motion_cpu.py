"""Motion vectors for the denoiser's history (include/kazen_mi355x_motion.h) without a GPU: the header against the library's exports, kz_motion_rows against numpy
in double, the refusals that need no device, and the test-only CPU reference (tests/cpu_ref/kz_motion_ref.cpp) the GPU tests compare against - checked here against
the temporal reference where the two must agree to the bit, on a plane that slides by a known number of pixels, and, for the ids, against a brute-force loop over the
scene's triangles."""
import ctypes as C

import numpy as np
import pytest

from checks import c_layout, header_surface, refused, same_bits_strict
from cpu_refs import lib, ref_denoise_motion, ref_denoise_temporal, ref_ids
from film_cases import (BAD_OPTS, BAD_TOPTS, BAD_VOPTS, MISS, camera_of, random_history, random_ids, rotate, sliding_plane, static_rows, synthetic_films, synthetic_moment,
                        translate, view_arrays)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("motion", tmp_path_factory.mktemp("kzm"))


# ---------------------------------------------------------------- 1. ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: disjoint from every other list, and nothing added to the existing headers
    header_surface(kz, "include/kazen_mi355x_motion.h", a.MOTION_EXPORTS, 5,
                   [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS, a.VARIANCE_EXPORTS, a.TEMPORAL_EXPORTS],
                   ["include/kazen_mi355x.h", "include/kazen_mi355x_dev.h", "include/kazen_mi355x_edit.h", "include/kazen_mi355x_aov.h", "include/kazen_mi355x_denoise.h",
                    "include/kazen_mi355x_variance.h", "include/kazen_mi355x_temporal.h"], ["kz_motion", "kz_denoise_motion", "kzmotion"])
    assert (a.KZ_MOTION_STATIC, a.KZ_MOTION_UNTRACKED, a.KZ_MOTION_MISS) == (1, 2, MISS)


def test_struct_sizes(kz, tmp_path):
    assert c_layout(tmp_path, "kazen_mi355x_motion.h", ["sizeof(KzMotionRow)", "offsetof(KzMotionRow, n)", "offsetof(KzMotionRow, flags)", "offsetof(KzMotionRow, reserved)",
                                                        "KZ_MOTION_STATIC", "KZ_MOTION_UNTRACKED", "KZ_MOTION_MISS"]) == ["96", "48", "84", "88", "1", "2", str(MISS)]
    r = kz.abi.KzMotionRow
    assert C.sizeof(r) == 96 and (r.d.offset, r.n.offset, r.flags.offset, r.reserved.offset) == (0, 48, 84, 88)


# ---------------------------------------------------------------- 2. the rows
def _row(rows, m):
    return np.array(list(rows[m].d), np.float32).reshape(3, 4), np.array(list(rows[m].n), np.float32).reshape(3, 3), int(rows[m].flags), list(rows[m].reserved)


def test_rows_against_numpy(kz):
    """d = H C^-1 and n = the inverse transpose of d's linear part, against numpy in double narrowed once. The library inverts 3 x 3 blocks by their adjugate, numpy
    a 4 x 4 by LU: ANOTHER ROUTE, so the two doubles differ by a few units of 2^-53 times the condition number (below 100 in these cases) times the largest entry,
    and after narrowing the floats are equal or neighbours. The bound per entry is therefore 1 ulp of the fp32 value plus 1e-13 of the matrix's largest entry (the
    second term for entries that are zero but for cancellation, whose own ulp is next to nothing); most entries come out bit for bit, which is printed."""
    sc, sh = np.diag([2.0, 0.5, 1.25, 1.0]), np.eye(4)
    sh[0, 1], sh[2, 0] = 0.3, -0.2
    R = rotate((1, 2, 3), 0.7)
    cases = {"translation": (translate((0.3, -1.0, 2.5)), np.eye(4)), "translation both": (translate((0.3, -1.0, 2.5)), translate((-0.1, 0.2, 0.05))),
             "rotation": (translate((1, 0, -2)) @ R, translate((1, 0.1, -2)) @ rotate((1, 2, 3), 0.4)), "non-uniform scale": (translate((0, 1, 0)) @ sc, R),
             "shear": (sh @ translate((0.5, 0.5, 0.5)), translate((0.1, 0, 0)) @ sh @ sc)}
    names = list(cases)
    cur = np.stack([cases[k][0] for k in names]).astype(np.float32)
    prev = np.stack([cases[k][1] for k in names]).astype(np.float32)
    rows = kz.motion_rows(cur, prev)
    exact = total = 0
    for m, name in enumerate(names):
        d, n, flags, reserved = _row(rows, m)
        assert flags == 0 and reserved == [0, 0], (name, flags)
        Cm, Hm = cur[m].astype(np.float64), prev[m].astype(np.float64)
        assert np.linalg.cond(Cm[:3, :3]) < 100 and np.linalg.cond(Hm[:3, :3]) < 100
        M = Hm @ np.linalg.inv(Cm)
        Nn = np.linalg.inv(M[:3, :3]).T
        for got, want in ((d, M[:3]), (n, Nn)):
            w32 = want.astype(np.float32)
            bound = np.spacing(np.abs(w32)).astype(np.float64) + 1e-13 * np.abs(want).max()
            assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= bound).all(), (name, got, w32)
            exact += int((got == w32).sum())                          # (as values: the two routes may disagree about the sign of a zero)
            total += got.size
    print("kz_motion_rows against numpy: %d of %d entries bit for bit, the others within 1 ulp" % (exact, total))
    assert exact >= 0.8 * total
    # identity by NULL on either side and both: STATIC, and so are any two matrices that are bitwise equal - a singular or projective one included
    one = np.eye(4, dtype=np.float32)[None]
    for c, p in ((one, None), (None, one), (one, one)):
        d, n, flags, _ = _row(kz.motion_rows(c, p), 0)
        assert flags == kz.abi.KZ_MOTION_STATIC and np.array_equal(d, np.eye(4, dtype=np.float32)[:3]) and np.array_equal(n, np.eye(3, dtype=np.float32))
    assert [rows_flags for rows_flags in (r.flags for r in kz.motion_rows(cur, cur))] == [kz.abi.KZ_MOTION_STATIC] * len(names)
    flat = np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32)[None]
    assert kz.motion_rows(flat, flat)[0].flags == kz.abi.KZ_MOTION_STATIC
    # not affine, singular, not finite: UNTRACKED, with the identity in d and n
    persp = np.eye(4, dtype=np.float32)
    persp[3, 0] = 0.25
    inf = np.eye(4, dtype=np.float32)
    inf[1, 3] = np.inf
    nan = np.eye(4, dtype=np.float32)
    nan[0, 0] = np.nan
    huge = (np.eye(4) * 1e30).astype(np.float32)
    huge[3, 3] = 1
    tiny = (np.eye(4) * 1e-30).astype(np.float32)
    tiny[3, 3] = 1
    moved = translate((1, 2, 3)).astype(np.float32)
    for name, c, p in (("projective C", persp, moved), ("projective H", moved, persp), ("singular C", flat[0], moved), ("singular H", moved, flat[0]), ("infinite", inf, moved),
                       ("infinite H", moved, inf), ("nan both", nan, nan), ("overflow", tiny, huge)):
        d, n, flags, _ = _row(kz.motion_rows(c[None], p[None]), 0)
        assert flags == kz.abi.KZ_MOTION_UNTRACKED, (name, flags)
        assert np.array_equal(d, np.eye(4, dtype=np.float32)[:3]) and np.array_equal(n, np.eye(3, dtype=np.float32)), name
    lib = kz.abi.load_library()
    assert lib.kz_motion_rows(None, None, 3, None) == kz.abi.KZ_ERR_INVALID_ARG and lib.kz_motion_rows(None, None, 0, None) == kz.abi.KZ_OK


# ---------------------------------------------------------------- 3. refusals
def test_refusals_without_a_device(kz):
    a = kz.abi
    lib = a.load_library()
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert lib.kz_denoise_motion(None, -1, None, None, None) == a.KZ_ERR_INVALID_ARG
    assert lib.kz_motion_ids(None, -1, None, 0) == a.KZ_ERR_INVALID_ARG
    # kz_denoise_motion: kz_denoise_temporal's refusals in its order, under its own name
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: sc.denoise_motion(**bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion")
    refused(kz, sc.denoise_motion, a.KZ_ERR_STATE, "kz_denoise_motion", "KZ_AOV_DEPTH", "mask 0")
    sc.set_aovs(["albedo", "normal", "depth"])
    refused(kz, sc.denoise_motion, a.KZ_ERR_STATE, "kz_denoise_motion", "switched off")
    refused(kz, lambda: sc.denoise_motion(guides=["albedo", "normal"]), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion", "KZ_AOV_DEPTH")
    sc.set_variance(True)
    refused(kz, sc.denoise_motion, a.KZ_ERR_STATE, "kz_scene_upload")      # the scene is on no device
    for fn in (sc.motion_ids, sc.motion_info):
        refused(kz, fn, a.KZ_ERR_STATE, "kz_scene_upload")
    # the test surface: arguments, options, ids and rows first, then the device
    film = np.ones((5, 7, 4), np.float32)
    view = kz.temporal_view(camera_of(kz, 7, 5, (0, 0, 0), (0, 0, 1)))
    rows = static_rows(kz, 4)
    ids = random_ids(7, 5, 4, seed=1)
    ok = dict(depth=film, samples=4, current=view, ids=ids, rows=rows)
    for bad in BAD_OPTS + BAD_VOPTS + BAD_TOPTS:
        refused(kz, lambda: kz.denoise_motion_films(film, film, **ok, **bad), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films")
    refused(kz, lambda: kz.denoise_motion_films(film, film, samples=4, current=view, ids=ids, rows=rows), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "depth")
    refused(kz, lambda: kz.denoise_motion_films(film, film, depth=film, samples=4, ids=ids, rows=rows), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "view")
    refused(kz, lambda: kz.denoise_motion_films(film, film, depth=film, samples=4, current=view, rows=rows), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "ids")
    refused(kz, lambda: kz.denoise_motion_films(film, film, depth=film, samples=4, current=view, ids=ids, n_rows=4), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "rows")
    out_of_range = ids.copy()
    out_of_range[3, 2] = 4
    refused(kz, lambda: kz.denoise_motion_films(film, film, **dict(ok, ids=out_of_range)), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "pixel (2, 3)", "mesh 4", "4 rows")
    refused(kz, lambda: kz.denoise_motion_films(film, film, **dict(ok, ids=ids), n_rows=3), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "3 rows")
    both = static_rows(kz, 4)
    both[2].flags = 3
    refused(kz, lambda: kz.denoise_motion_films(film, film, **dict(ok, rows=both)), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "row 2")
    both[2].flags = 4
    refused(kz, lambda: kz.denoise_motion_films(film, film, **dict(ok, rows=both)), a.KZ_ERR_INVALID_ARG, "kz_denoise_motion_films", "row 2")
    refused(kz, lambda: kz.denoise_motion_films(film, film, depth=film, current=view, ids=ids, rows=rows), a.KZ_ERR_STATE, "kz_denoise_motion_films", "samples = 0")
    if lib.kz_device_count() == 0:
        refused(kz, lambda: kz.denoise_motion_films(film, film, **ok), a.KZ_ERR_NO_DEVICE)
        refused(kz, lambda: kz.denoise_motion_films(film, film, **dict(ok, ids=np.full((5, 7), MISS, np.uint32)), n_rows=0), a.KZ_ERR_NO_DEVICE)      # only misses: no row is needed


# ---------------------------------------------------------------- 4. identity
@pytest.mark.parametrize("frame", [(1, 1), (7, 5), (65, 3)])
@pytest.mark.parametrize("border", [0, 2])
def test_static_rows_give_the_temporal_references_bits(kz, ref, frame, border):
    """With every row STATIC and any ids - misses among them - the result, the new history and v_last are kz_temporal_ref's, bit for bit: without a history, with a
    random one and with the call's own, through a view that moved."""
    w, h = frame
    b = border
    colour, albedo, normal, depth = synthetic_films(w, h, b, seed=17 * w + h + b)
    films = (colour, synthetic_moment(colour, seed=w + 5 * h + b), albedo, normal, depth)
    at = lambda o: kz.temporal_view(camera_of(kz, w, h, o, (o[0], o[1], o[2] + 1), fov=50.0))
    pix = 2.0 * np.tan(np.radians(25.0)) / w
    cur, prev = at((1.5 * pix, -0.9 * pix, 0)), at((0, 0, 0))
    rows, ids = static_rows(kz, 4), random_ids(w, h, 4, seed=w + h + b)
    own = None
    for history in (None, random_history(w, h, seed=3 + w), "own"):
        history = own if isinstance(history, str) else history
        for kw in (dict(iterations=1), dict(iterations=2, depth_tolerance=20.0, normal_tolerance=3.0, max_history=7)):
            want = ref_denoise_temporal(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=history, **kw)
            got = ref_denoise_motion(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=history, ids=ids, rows=rows, **kw)
            for g, x, what in zip(got, want, ("film", "history", "variance")):
                assert same_bits_strict(g, x), (frame, b, what, kw)
        own = want[1]
    # only misses and no row at all: the same
    got = ref_denoise_motion(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=own, ids=np.full((h, w), MISS, np.uint32), rows=rows, n_rows=0, iterations=1)
    want = ref_denoise_temporal(ref, kz, *films, border=b, samples=4, current=cur, previous=prev, history=own, iterations=1)
    assert all(same_bits_strict(g, x) for g, x in zip(got, want))


# ---------------------------------------------------------------- 5. a plane that slides
def test_a_plane_that_slides(kz, ref):
    w, h, k = 64, 48, 3
    view, films1, ids1, films2, ids2, rows, shift = sliding_plane(kz, w, h, shift_pixels=k)
    assert rows[0].flags == 0
    kw = dict(border=0, samples=4, iterations=1)
    _, hist1, _ = ref_denoise_motion(ref, kz, *films1, current=view, ids=ids1, rows=static_rows(kz, 1), **kw)
    assert set(np.unique(hist1[..., 8])) == {0.0, 1.0}
    _, hist2, _ = ref_denoise_motion(ref, kz, *films2, current=view, previous=view, history=hist1, ids=ids2, rows=rows, **kw)
    # where frame 2's pixels were in frame 1, in float64: k columns to the left, to a thousandth of a pixel
    o, a, u, v, inv = view_arrays(view)
    yy, xx = np.mgrid[0:h, 0:w]
    d = a + (xx[..., None] + 0.5) * u + (yy[..., None] + 0.5) * v
    X = o + d * (4.0 / d[..., 2])[..., None]
    P = (X - shift - o) @ inv.T
    px, py = P[..., 0] / P[..., 2] - 0.5, P[..., 1] / P[..., 2] - 0.5
    assert np.abs(px - (xx - k)).max() < 1e-3 and np.abs(py - yy).max() < 1e-3
    # the pixels whose reprojection lies at least 2 pixels inside the frame and the quad's silhouette of frame 1 (columns 10 .. 49, rows 8 .. 39)
    sx, sy = xx - k, yy
    inside = (sx >= 12) & (sx <= 47) & (sy >= 10) & (sy <= 37)        # (the silhouette lies more than 2 pixels inside the frame)
    assert inside.sum() == 36 * 28
    N, e = hist2[..., 8], hist2[..., :3].astype(np.float64)
    assert (N[inside] == 2).all(), int((N[inside] != 2).sum())
    want = 0.5 * np.roll(hist1[..., :3].astype(np.float64), k, axis=1) + 0.5 * films2[0][..., :3].astype(np.float64)      # om = al = 1/2; the history k columns over
    rel = np.abs(e - want)[inside] / np.abs(want)[inside]
    print("a plane that slides: %d pixels, max relative |e - blend| = %.3g" % (int(inside.sum()), float(rel.max())))
    assert rel.max() < 1e-6, float(rel.max())
    assert (N[ids2 == MISS] == 0).all()                               # nothing there: not valid
    # the same films through the temporal reference, and with the row STATIC: those pixels blend with the wrong neighbour - the quad's point k pixels away
    _, histt, _ = ref_denoise_temporal(ref, kz, *films2, current=view, previous=view, history=hist1, **kw)
    _, hists, _ = ref_denoise_motion(ref, kz, *films2, current=view, previous=view, history=hist1, ids=ids2, rows=static_rows(kz, 1), **kw)
    assert same_bits_strict(histt, hists)
    wrong = 0.5 * hist1[..., :3].astype(np.float64) + 0.5 * films2[0][..., :3].astype(np.float64)
    both = inside & (xx >= 12) & (xx <= 47)                           # ... where the pixel itself lies inside frame 1's silhouette too
    assert (histt[..., 8][both] == 2).all() and np.abs(histt[..., :3] - wrong)[both].max() < 1e-6
    assert np.abs(histt[..., :3].astype(np.float64) - e)[both].min() > 1e-4      # (the ramp changes by more than that over 3 pixels in every channel)
    assert not same_bits_strict(histt, hist2)
    # an UNTRACKED row: no history anywhere on the quad
    lost = static_rows(kz, 1)
    lost[0].flags = kz.abi.KZ_MOTION_UNTRACKED
    _, histu, _ = ref_denoise_motion(ref, kz, *films2, current=view, previous=view, history=hist1, ids=ids2, rows=lost, **kw)
    assert (histu[..., 8][ids2 == 0] == 1).all()
    # a revealed background: a far wall behind everything in both frames, static; where the quad was and no longer is, the history's depth is the quad's - rejected
    wall_depth = 2.0 * films1[4][10, 20, 0]
    def with_wall(films, ids):
        out = [f.copy() for f in films]
        bg = ids == MISS
        out[0][bg] = (0.2, 0.2, 0.2, 1.0)
        out[1][bg] = (0.04, 0.04, 0.04, 1.0)
        out[2][bg] = (1.0, 1.0, 1.0, 1.0)
        out[3][bg] = (0.0, 0.0, -1.0, 1.0)
        out[4][bg] = (wall_depth, wall_depth, wall_depth, 1.0)
        return out, np.where(bg, 1, ids).astype(np.uint32)
    f1, i1 = with_wall(films1, ids1)
    f2, i2 = with_wall(films2, ids2)
    two = kz.motion_rows(np.stack([translate(shift), np.eye(4)]).astype(np.float32), None)
    _, h1, _ = ref_denoise_motion(ref, kz, *f1, current=view, ids=i1, rows=static_rows(kz, 2), **kw)
    _, h2, _ = ref_denoise_motion(ref, kz, *f2, current=view, previous=view, history=h1, ids=i2, rows=two, **kw)
    revealed = (ids1 == 0) & (ids2 == MISS)
    assert revealed.sum() == 32 * k and (h2[..., 8][revealed] == 1).all()
    still = (ids1 == MISS) & (ids2 == MISS)
    still[:, :1] = still[:, -1:] = still[:1] = still[-1:] = False
    assert (h2[..., 8][still] == 2).all() and (h2[..., 8][inside] == 2).all()


# ---------------------------------------------------------------- 6. the ids
def test_ids_reference_against_brute_force(kz, O, ref):
    """The reference's ids of the Cornell box at 24 x 18 against a Moeller-Trumbore loop in float64 over every triangle, on the oracle's own camera rays; a first hit on
    the invisible ceiling light is walked through (path_mis). Pixels where the two nearest hits of the ray that decides are within 1e-4 of each other are left out:
    there the order depends on fp32 rounding. At most 2 % of the frame may be left out."""
    d = kz.scenes.cornell_box(24, 18, 1)
    W, H = 24, 18
    got = ref_ids(ref, d)
    assert got.shape == (H, W)
    tris, mesh_of = [], []
    for m, mesh in enumerate(d.meshes):
        V, F = np.asarray(mesh["V"], np.float64), np.asarray(mesh["F"])
        for f in F.reshape(-1, 3):
            tris.append(V[f])
            mesh_of.append(m)
    tris, mesh_of = np.array(tris), np.array(mesh_of)
    assert len(tris) == 36
    invisible = np.array([d.meshes[m]["light"] is not None and not d.meshes[m]["light"]["lightPrimaryVisibility"] for m in mesh_of])
    ora = O.OracleScene(d)
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]

    def hits(o, dr, lo, hi):
        """(t, triangle) of every hit in (lo, hi), nearest first."""
        pv = np.cross(dr, e2)
        det = (e1 * pv).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - p0
            uu = (tv * pv).sum(axis=1) * inv
            qv = np.cross(tv, e1)
            vv = (qv * dr).sum(axis=1) * inv
            t = (e2 * qv).sum(axis=1) * inv
        ok = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > lo) & (t < hi)
        order = np.argsort(np.where(ok, t, np.inf))
        return [(t[i], i) for i in order if ok[i]]

    left_out = walked = 0
    for y in range(H):
        for x in range(W):
            ray, mint, maxt = ora.camera_ray(x + 0.5, y + 0.5)
            o, dr = ray[:3].astype(np.float64), ray[3:6].astype(np.float64)
            hs = hits(o, dr, mint, maxt)
            want = MISS
            ambiguous = len(hs) > 1 and hs[1][0] - hs[0][0] < 1e-4
            if hs:
                want = mesh_of[hs[0][1]]
                if invisible[hs[0][1]]:
                    walked += 1
                    behind = [q for q in hs[1:] if q[0] > hs[0][0] + 1e-4]      # (the continuation starts traceBias behind the light: anything nearer than that is ambiguous)
                    ambiguous = ambiguous or len(behind) != len(hs) - 1 or (len(behind) > 1 and behind[1][0] - behind[0][0] < 1e-4)
                    if behind:
                        want = mesh_of[behind[0][1]]
            if ambiguous:
                left_out += 1
                continue
            assert got[y, x] == want, (x, y, int(got[y, x]), int(want))
    print("ids against brute force: %d of %d pixels left out, %d first hits on the invisible light" % (left_out, W * H, walked))
    assert left_out <= 0.02 * W * H, left_out
    assert len(np.unique(got)) >= 5
