"""Inputs nobody rendered, and the scene helpers, that more than one test module (or a script under scripts/) uses: synthetic films, moments, histories, ids and
row tables; views and planes; the frame sequences of the quality figures; variations of a scene description; the tables of options every entry refuses. Every
generator is a function of its arguments alone - its seed, its draw order and its defaults are part of what the tests pin. A support module beside the tests,
like sample_corners.py: imported, never collected."""
import copy

import numpy as np

from cpu_refs import AovRef, MomentRef, lib, ref_denoise_motion, ref_denoise_responsive, ref_ids

W, H, SPP = 96, 72, 8          # wider and taller than one 64-px resolve cell and than two 32-px reference blocks; 55 296 items
AOVS = ("albedo", "normal", "depth")
GUIDES = ("albedo", "normal", "depth")
INTEGRATORS = ("normals", "ao", "path_mats")                          # the integrators beside path_mis
KEYS = ("mesh", "bsdf")
NONE = 0xFFFFFFFF                                                     # KZ_MATTE_NONE
MISS = 0xFFFFFFFF                                                     # KZ_MOTION_MISS
FRAMES = [(1, 1), (7, 5), (65, 3), (130, 9)]                          # one pixel; more rows than a block; more columns than a block; several blocks on both axes
SHORT_BOX = 6                                                         # the short box of scenes.cornell_box: floor, ceiling, back, left, right, tall box, SHORT BOX, light
LAMP = 7                                                              # scenes.cornell_box: the ceiling light
NEW_LIGHT = dict(color=(1.0, 0.45, 0.2), intensity=12.0)              # the light step: from white 15 to a dimmer orange - a change of colour, not only of level
FILTERS = {"gaussian r=2": {"type": "gaussian", "radius": 2.0, "stddev": 0.5, "B": 1 / 3.0, "C": 1 / 3.0},
           "box r=0.5": {"type": "box", "radius": 0.5, "stddev": 0.5, "B": 1 / 3.0, "C": 1 / 3.0},
           "mitchell r=2": {"type": "mitchell", "radius": 2.0, "stddev": 0.5, "B": 1 / 3.0, "C": 1 / 3.0},
           "gaussian r=3": {"type": "gaussian", "radius": 3.0, "stddev": 0.75, "B": 1 / 3.0, "C": 1 / 3.0}}      # 7 taps: the 4-group tap kernel
SCHEDULES = [{}, {"tune": {"sppPerPass": 4}}, {"passes_in_flight": 2, "pass_items": 1024 * SPP}, {"pass_halves": 2}, {"shadow_beside": 2}]

# ---------------------------------------------------------------- what every entry of a family refuses
BAD_OPTS = [{"iterations": 9}, {"iterations": 1 << 31}, {"sigma_color": -1.0}, {"sigma_normal": float("nan")}, {"sigma_depth": float("inf")}, {"sigma_albedo": -1e-30},
            {"flags": 4}, {"flags": 1 << 31}, {"reserved": 1}]
BAD_VOPTS = [{"sigma_variance": -1.0}, {"sigma_variance": float("nan")}, {"sigma_variance": float("inf")}, {"sigma_variance": -1e-30}, {"vflags": 1}, {"vflags": 1 << 31},
             {"vreserved": 1}]
BAD_TOPTS = [{"depth_tolerance": -1.0}, {"depth_tolerance": float("nan")}, {"depth_tolerance": float("inf")}, {"normal_tolerance": -1e-30}, {"normal_tolerance": float("nan")},
             {"normal_tolerance": float("-inf")}, {"max_history": 65536}, {"max_history": 1 << 31}, {"tflags": 1}, {"tflags": 1 << 31}, {"treserved": (1, 0, 0, 0)},
             {"treserved": (0, 2, 0, 0)}, {"treserved": (0, 0, 3, 0)}, {"treserved": (0, 0, 0, 4)}]
BAD_ROPTS = [{"fast_history": 65536}, {"clamp_sigma": -1.0}, {"clamp_sigma": float("nan")}, {"clamp_sigma": float("inf")}, {"radius": 3}, {"rflags": 2}, {"rflags": 1 << 31},
             {"rreserved": (0, 0, 1, 0)}, {"rreserved": (7, 0, 0, 0)}]


# ---------------------------------------------------------------- variations of a scene description
def with_integrator(desc, name):
    d = copy.copy(desc)
    d.integrator = dict(desc.integrator, type=name)
    return d


def grid_of(desc, S=None):
    """Every (pixel, sample) of the frame."""
    w, h = desc.camera["width"], desc.camera["height"]
    S = S or desc.sampler["sampleCount"]
    yy, xx, ii = np.meshgrid(np.arange(h), np.arange(w), np.arange(S), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)


def octant_scene(kz, width=W, height=H, spp=SPP, n_tris=200, seed=5):
    """The cross-check scene: `n_tris` triangles WITHOUT vertex normals, each built in a plane whose unit normal has all components >= 0.2 and wound so that
    cross(e1, e2) points along it; the camera looks down (-1, -1, -1), so it sees their front sides. The shading normal of such a triangle is its geometric one
    (accel.cpp:231-233) with no negative component, so |n_geo| - what `normals` renders - and the signed NORMAL feature are the same numbers."""
    S = kz.scenes
    rng = np.random.default_rng(seed)
    s = S.SceneDescription()
    V, F = [], []
    for k in range(n_tris):
        n = rng.uniform(0.2, 1.0, 3)
        n /= np.linalg.norm(n)
        while n.min() < 0.25:                                         # (margin: the float32 normal the renderers form stays >= 0.2)
            n = rng.uniform(0.2, 1.0, 3)
            n /= np.linalg.norm(n)
        a = np.cross(n, [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(n, a)                                            # (a, b, n) right-handed: cross(a, b) = n
        c = rng.uniform(-1.0, 1.0, 3)
        r = rng.uniform(0.25, 0.6)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        V += [c + r * (np.cos(t) * a + np.sin(t) * b) for t in ang]   # counter-clockwise about n
        F.append([3 * k, 3 * k + 1, 3 * k + 2])
    s.add_mesh(np.array(V, np.float32), np.array(F, np.uint32), bsdf=S.diffuse((0.6, 0.5, 0.4)))
    q = S.quad((-0.5, 3.0, -0.5), (-0.5, 3.0, 0.5), (0.5, 3.0, 0.5), (0.5, 3.0, -0.5), flip=True)
    s.add_mesh(q[0], q[3], N=None, UV=None, bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 1, 1), 10.0, True))      # (behind the camera's view: n = -y)
    s.camera.update(width=width, height=height, fov=45.0, nearClip=0.1, farClip=100.0, toWorld=S.look_at((3.2, 3.2, 3.2), (0, 0, 0), (0, 1, 0)))
    s.sampler = {"type": "independent", "sampleCount": spp, "seed": 3}
    s.integrator["maxDepth"] = 3
    return s


def looks_at_the_light(kz, w=24, h=18, spp=16):
    """The Cornell box seen from below its ceiling light, which is invisible to camera rays: path_mis walks through it to the ceiling 0.01 behind it. The defaults are
    the matte tests' frame."""
    d = kz.scenes.cornell_box(w, h, spp)
    d.camera.update(fov=50.0, toWorld=kz.scenes.look_at((0.05, -0.2, 0.7), (0, 0.99, 0), (0, 0, -1)))
    return d


def _looks_at_the_light(kz):
    """looks_at_the_light at W x H, SPP samples: the feature films' frame."""
    return looks_at_the_light(kz, W, H, SPP)


def _visible(desc):
    d = copy.deepcopy(desc)
    for m in d.meshes:
        if m["light"] is not None:
            m["light"] = dict(m["light"], lightPrimaryVisibility=True)
    return d


def _thinlens(desc):
    d = copy.deepcopy(desc)
    d.camera.update(type="thinlens", apertureRadius=0.1, focusDistance=3.5)
    return d


def _with_filter(desc, rf):
    d = copy.deepcopy(desc)
    d.camera["rfilter"] = dict(rf)
    return d


def _orbit(kz, desc, degrees):
    """`desc` with its camera turned by `degrees` about the world's y axis through the point it looks at (taken 4 units along its axis)."""
    d = copy.copy(desc)
    m = np.array(desc.camera["toWorld"], np.float64).reshape(4, 4)
    centre = m[:3, 3] + 4.0 * m[:3, 2]
    t = np.radians(degrees)
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    out = m.copy()
    out[:3, :3] = R @ m[:3, :3]
    out[:3, 3] = centre + R @ (m[:3, 3] - centre)
    d.camera = dict(desc.camera, toWorld=out.astype(np.float32))
    return d


def fresh_film(kz, desc, **kw):
    """The film a scene created from `desc` on device 0 renders."""
    sc = kz.Scene(desc, device=0)
    sc.render(**kw)
    f = sc.film()
    sc.close()
    return f


def _fuzz_scene(S, seed, rich=False):
    """A random small scene: triangle soup + room, random BSDF plugins on every mesh, random visible / invisible lights (some stacked so
    shadow rays cross them), random camera / sampler / filter / integrator settings. rich: the same scene with (from a second generator, so the plain scene
    of a seed does not change) bicubic image lookups and an environment image, colour ramp or constant behind the background (scripts/dev/fuzz_sweep.py --rich)."""
    rng = np.random.default_rng(seed)
    d = S.random_triangles(int(rng.integers(50, 3000)), int(rng.integers(24, 72)), int(rng.integers(24, 56)), 4, sampler="independent", s_edge=float(rng.uniform(0.05, 0.4)))
    makers = [lambda: S.diffuse(tuple(rng.uniform(0.1, 0.9, 3))),
              lambda: S.kazenstandard(tuple(rng.uniform(0.1, 0.9, 3)), float(rng.uniform(0, 1)), float(rng.integers(0, 2)), float(rng.uniform(0, 0.8)),
                                      float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1))),
              lambda: S.mirror(), lambda: S.dielectric(float(rng.uniform(1.2, 1.8)), 1.0), lambda: S.ggx(tuple(rng.uniform(0.2, 0.9, 3)), float(rng.uniform(0.05, 0.9)), float(rng.uniform(0, 0.5))),
              lambda: S.roughconductor(float(rng.uniform(0.05, 0.6)), str(rng.choice(["Au", "Cu", "Cr"]))), lambda: S.roughplastic(float(rng.uniform(0.05, 0.6)), kd=tuple(rng.uniform(0.1, 0.6, 3))),
              lambda: S.roughdielectric(float(rng.uniform(0.05, 0.6)))]
    if seed % 3 == 0:                                                            # every third scene: texture trees and normal maps too (8f rank 4)
        chk, noise, gray, nrm = S._test_images()
        t_noise, t_gray = S.imagetexture(noise, float(rng.uniform(0.5, 4)), "srgb"), S.imagetexture(gray, float(rng.uniform(0.5, 4)), "linear")
        t_nrm = S.imagetexture(nrm, float(rng.uniform(0.5, 3)), "linear")
        makers += [lambda: S.lambertian(S.blend(t_gray, S.constanttexture(tuple(rng.uniform(0, 1, 3))), t_noise)),
                   lambda: S.kazenstandard(t_noise, S.colorramp(t_gray, 0.1, 0.9), t_gray, clearcoat=float(rng.uniform(0, 1))),
                   lambda: S.normalmap(t_nrm, makers[int(rng.integers(0, 8))]()), lambda: S.ggx(S.imagetexture(chk, 3.0, "srgb"), float(rng.uniform(0.1, 0.8)))]
    for m in d.meshes:
        if m["light"]:
            m["light"]["lightPrimaryVisibility"] = bool(rng.integers(0, 2))
            m["light"]["intensity"] = float(rng.uniform(5, 40))
        elif rng.random() < 0.85:
            m["bsdf"] = makers[int(rng.integers(0, len(makers)))]()
        else:
            m["bsdf"] = None                                                    # default diffuse (mesh.cpp:25-28)
        if rng.random() < 0.2:
            m["N"] = None                                                       # no vertex normals (H4)
    # an extra light hanging in the room below the ceiling lights: shadow rays to the ceiling cross it
    q = S.quad((-0.5, 0.6, 1.2), (-0.5, 0.6, 2.2), (0.5, 0.6, 2.2), (0.5, 0.6, 1.2), flip=True)
    d.add_mesh(q[0], q[3], q[1], q[2], bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 0.8, 0.6), float(rng.uniform(2, 10)), bool(rng.integers(0, 2))))
    d.sampler = {"type": str(rng.choice(["independent", "pmj02bn", "stratified", "correlated"])), "sampleCount": int(rng.integers(1, 12)), "seed": int(rng.integers(0, 100))}
    d.integrator.update(maxDepth=int(rng.integers(1, 9)), traceBias=float(rng.choice([1e-3, 1e-4, 5e-3])), regularization=bool(rng.integers(0, 2)),
                        accumulatedRoughness=float(rng.uniform(0.1, 0.9)))
    d.camera["rfilter"] = [{"type": "gaussian", "radius": 2.0, "stddev": 0.5}, {"type": "tent"}, {"type": "box"}, {"type": "mitchell", "radius": 2.0, "B": 1 / 3, "C": 1 / 3},
                           {"type": "gaussian", "radius": 3.5, "stddev": 1.0}][int(rng.integers(0, 5))]
    if rng.random() < 0.4:
        d.camera.update(type="thinlens", apertureRadius=float(rng.uniform(0, 0.2)), focusDistance=float(rng.uniform(1, 4)))
    if rng.random() < 0.5:
        d.background = {"color": tuple(rng.uniform(0, 1, 3)), "intensity": float(rng.uniform(0, 2))}
    if rich:
        r2 = np.random.default_rng(1_000_003 * (seed + 1))

        def walk(node):
            if isinstance(node, dict):
                if node.get("type") == "imagetexture" and r2.random() < 0.5:
                    node["filter"] = "bicubic"
                for v in node.values():
                    walk(v)
        for m in d.meshes:
            walk(m["bsdf"])
        k = r2.random()
        if k < 0.6:
            env = r2.random((int(r2.integers(2, 9)), int(r2.integers(3, 17)), 3)).astype(np.float32) * float(r2.uniform(0.2, 3))
            tex = S.imagetexture(env, 1.0, "linear", "bicubic" if r2.random() < 0.3 else "bilinear")
            d.background = {"texture": tex if k < 0.45 else S.colorramp(tex, 0.1, 0.9), "intensity": float(r2.uniform(0.2, 2))}
    return d


# ---------------------------------------------------------------- films, moments, histories, ids nobody rendered
def synthetic_films(w, h, b, seed):
    """Films a renderer could have made, with every awkward texel the definition names: lognormal colour times a filter weight, about 5 % of the frame's pixels
    with weight 0 (their rgb left non-zero: it must not count), normals constant on pieces of the frame (unit, signed), a depth with zeros, an albedo with channels
    that are exactly 0 (demodulation divides by max(a, 1e-3)), and a non-zero apron in every film (it must not count either)."""
    rng = np.random.default_rng(seed)
    rows, cols = h + 2 * b, w + 2 * b

    def film_of(values):
        wgt = rng.uniform(0.5, 4.0, (rows, cols, 1)).astype(np.float32)
        return np.concatenate([values.astype(np.float32) * wgt, wgt], axis=2)

    yy, xx = np.mgrid[0:rows, 0:cols]
    piece = ((yy // 7) * 3 + (xx // 9)) % 5
    normals = rng.normal(size=(5, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    colour = film_of(rng.lognormal(-1.0, 1.0, (rows, cols, 3)))
    colour[rng.random((rows, cols)) < 0.05, 3] = 0.0
    normal = film_of(normals[piece])
    z = rng.uniform(1.0, 9.0, (rows, cols, 1)) * (rng.random((rows, cols, 1)) > 0.1)
    depth = film_of(np.repeat(z, 3, axis=2))
    alb = rng.uniform(0.05, 0.95, (5, 3))[(piece + xx // 4) % 5] * (rng.random((rows, cols, 3)) > 0.15)
    albedo = film_of(alb)
    return colour, albedo, normal, depth


def synthetic_moment(colour, seed, degenerate=False):
    """A second-moment film for a synthetic picture: the picture's own weights (zeros included), values c^2 (1 + t) with t = lognormal(-3, 2) - 0.01 - relative variances
    from 1e-3 to 10, so that the variance's tolerance is the tighter one in some pixels and iterations and the fixed one in others; a fifth of the channels below c^2,
    where the variance clamps to 0 - and the apron left non-zero. degenerate: 1e30 x w in every channel, which takes the variance's tolerance out of the filter."""
    rng = np.random.default_rng(seed)
    w = colour[..., 3:]
    c = np.where(w != 0, colour[..., :3] / np.where(w == 0, 1, w), 0)
    s = np.full(c.shape, 1e30, np.float32) if degenerate else (c * c * (0.99 + rng.lognormal(-3.0, 2.0, c.shape))).astype(np.float32)
    m = np.concatenate([s * w, w], axis=2).astype(np.float32)
    dead = w[..., 0] == 0
    m[dead, :3] = 5.0                                                 # (what a texel of weight 0 holds must not count)
    return m


def frame_rgb(film, b):
    f = film[b:film.shape[0] - b, b:film.shape[1] - b] if b else film
    return np.where(f[..., 3:] != 0, f[..., :3] / np.where(f[..., 3:] == 0, 1, f[..., 3:]), 0)


def mse_ratio(pic, noisy, clean, b):
    want = frame_rgb(clean, b).astype(np.float64)
    mse = lambda x: float(((frame_rgb(x, b).astype(np.float64) - want) ** 2).mean())
    return mse(pic) / mse(noisy)


def random_history(w, h, seed, holes=0.2):
    """A history nobody rendered: lognormal colours and variances, unit normals, distances 1 .. 9, counts 1 .. 40, and `holes` of the pixels empty (N = 0, all zeros)."""
    rng = np.random.default_rng(seed)
    hist = np.zeros((h, w, 12), np.float32)
    hist[..., :3] = rng.lognormal(-1.0, 1.0, (h, w, 3))
    hist[..., 3] = rng.lognormal(-3.0, 2.0, (h, w))
    n = rng.normal(size=(h, w, 3))
    hist[..., 4:7] = n / np.linalg.norm(n, axis=2, keepdims=True)
    hist[..., 7] = rng.uniform(1.0, 9.0, (h, w))
    hist[..., 8] = rng.integers(1, 41, (h, w))
    hist[rng.random((h, w)) < holes] = 0.0
    return hist


def random_fast(history, seed):
    """A fast plane nobody rendered, to go with `history` (h, w, 12): lognormal colours and variances, zeros where the history is empty."""
    rng = np.random.default_rng(seed)
    h, w = history.shape[:2]
    fast = np.zeros((h, w, 4), np.float32)
    fast[..., :3] = rng.lognormal(-1.0, 1.0, (h, w, 3))
    fast[..., 3] = rng.lognormal(-3.0, 2.0, (h, w))
    fast[history[..., 8] == 0] = 0.0
    return fast


def record(dtype, ids=(), counts=(), other=0, miss=0):
    """One matte record (dtype: kz.abi.MATTE_DTYPE) with the first slots, `other` and `miss` as given."""
    r = np.zeros((), dtype)
    r["id"][:len(ids)] = ids
    r["count"][:len(counts)] = counts
    r["other"], r["miss"] = other, miss
    return r


def random_ids(w, h, n_meshes, seed, misses=0.15):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_meshes, (h, w)).astype(np.uint32)
    ids[rng.random((h, w)) < misses] = MISS
    return ids


# ---------------------------------------------------------------- views, motions, row tables
def camera_of(kz, width, height, origin, target, up=(0, 1, 0), fov=40.0, **more):
    """A SceneDescription.camera: a perspective look-at camera."""
    cam = dict(kz.scenes.SceneDescription().camera)
    cam.update(width=width, height=height, fov=fov, toWorld=kz.scenes.look_at(origin, target, up), **more)
    return cam


def view_arrays(view):
    """(o, a, u, v, inv 3 x 3) of a KzTemporalView as float64 arrays of the fp32 words."""
    f = lambda x: np.array(list(x), np.float32).astype(np.float64)
    return f(view.o), f(view.a), f(view.u), f(view.v), f(view.inv).reshape(3, 3)


def view_pairs(kz, w, h):
    """(current, previous) over a frame whose synthetic depths are 1 .. 9: the same view; the camera moved by 0.3 of a pixel's footprint at distance 5; turned by the
    angle of 40 pixels, so that part of a wide frame leaves (and all of a narrow one); turned round."""
    at = lambda o, t: kz.temporal_view(camera_of(kz, w, h, o, t, fov=50.0))
    base = at((0, 0, 0), (0, 0, 1))
    pix = 2.0 * np.tan(np.radians(25.0)) / w
    yaw = 40 * pix
    return {"same": (base, base), "fraction": (at((1.5 * pix, -0.9 * pix, 0), (1.5 * pix, -0.9 * pix, 1)), base),
            "forty": (at((0, 0, 0), (np.sin(yaw), 0, np.cos(yaw))), base), "round": (at((0, 0, 0), (0, 0, -1)), base)}


def translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def rotate(axis, angle):
    """Rodrigues: the 4 x 4 of a turn by `angle` about `axis` through the origin."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return m


def static_rows(kz, n):
    return kz.motion_rows(np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), None)


def row_tables(kz, w):
    """Tables of 4 rows over a frame whose synthetic depths are 1 .. 9 (view_pairs' cameras: fov 50 at the origin, looking down +z): all STATIC; every mesh translated
    by 0.3 of a pixel's footprint at distance 5; every mesh turned about the camera by the angle of 40 pixels; all UNTRACKED; one of each."""
    pix = 2.0 * np.tan(np.radians(25.0)) / w
    I = np.eye(4)
    T, R = translate((0.3 * pix * 5.0, -0.2 * pix * 5.0, 0.0)), rotate((0, 1, 0), 40 * pix)
    f32 = lambda ms: np.stack(ms).astype(np.float32)
    tables = {"static": kz.motion_rows(f32([I] * 4), None), "translated": kz.motion_rows(f32([T] * 4), None), "rotated": kz.motion_rows(f32([R] * 4), None),
              "untracked": kz.motion_rows(f32([T] * 4), None), "mixed": kz.motion_rows(f32([I, T, R, T]), None)}
    for r in tables["untracked"]:
        r.flags = kz.abi.KZ_MOTION_UNTRACKED
    tables["mixed"][3].flags = kz.abi.KZ_MOTION_UNTRACKED
    assert [r.flags for r in tables["mixed"]] == [1, 0, 0, 2] and [r.flags for r in tables["rotated"]] == [0] * 4
    return tables


# ---------------------------------------------------------------- planes
def plane_films(kz, w, h, colour, D=4.0):
    """A frame of ONE valid surface: the plane z = D seen by a camera at the origin, every pixel valid with the colour given (a scalar or (h, w, 3)), a second
    moment of exactly colour^2 - zero variance -, albedo 1, normal (0, 0, -1). Returns (view, (film, moment, albedo, normal, depth), the depth per pixel)."""
    view = kz.temporal_view(camera_of(kz, w, h, (0, 0, 0), (0, 0, 1), fov=40.0))
    o, a, u, v, _ = view_arrays(view)
    yy, xx = np.mgrid[0:h, 0:w]
    d = a + (xx[..., None] + 0.5) * u + (yy[..., None] + 0.5) * v
    X = o + d * ((D - o[2]) / d[..., 2])[..., None]
    z = np.linalg.norm(X - o, axis=2).astype(np.float32)
    one = np.ones((h, w, 1), np.float32)
    film = lambda val: np.concatenate([np.broadcast_to(np.asarray(val, np.float32), (h, w, 3)), one], axis=2).astype(np.float32)
    c = film(colour)
    return view, (c, film(c[..., :3] * c[..., :3]), film(1.0), film((0.0, 0.0, -1.0)), film(z[..., None])), z


def plane_history(z, colour, count, v=0.0):
    """The history of plane_films' surface: colour (a scalar or (h, w, 3)), variance v and count N everywhere."""
    h, w = z.shape
    hist = np.zeros((h, w, 12), np.float32)
    hist[..., :3] = np.broadcast_to(np.asarray(colour, np.float32), (h, w, 3))
    hist[..., 3], hist[..., 6], hist[..., 7], hist[..., 8] = v, -1.0, z, count
    return hist


def sliding_plane(kz, w=64, h=48, D=4.0, shift_pixels=3):
    """The setting of test_temporal_cpu's two views of a plane with the camera at rest: a quad (mesh 0) in the plane z = D, its silhouette the pixel columns 10 .. 49 and
    rows 8 .. 39 of frame 1, painted with a linear ramp in ITS OWN coordinates, albedo 1, normal (0, 0, -1), nothing around it (pixels that are not valid, ids a miss).
    Frame 2: the quad translated along x in its plane by the footprint of `shift_pixels` pixels and lit 0.8 times as brightly. Returns (view, films1, ids1, films2,
    ids2, rows of frame 2, the world shift)."""
    view = kz.temporal_view(camera_of(kz, w, h, (0, 0, 0), (0, 0, 1), fov=40.0))
    o, a, u, v, _ = view_arrays(view)
    pix = D * np.linalg.norm(u) / a[2]                                # a pixel's footprint on the plane
    shift = shift_pixels * pix * u / np.linalg.norm(u)                # along the image's x axis: + shift_pixels columns
    yy, xx = np.mgrid[0:h, 0:w]
    d = a + (xx[..., None] + 0.5) * u + (yy[..., None] + 0.5) * v
    X = o + d * ((D - o[2]) / d[..., 2])[..., None]
    extent = D * np.tan(np.radians(20.0)) + (shift_pixels + 1) * pix
    gx, gy = np.array([0.45, -0.3, 0.2]) / extent, np.array([0.04, 0.15, -0.25]) / extent
    one = np.ones((h, w, 1), np.float32)
    film = lambda val, mask: np.where(mask[..., None], np.concatenate([np.broadcast_to(np.asarray(val, np.float32), (h, w, 3)), one], axis=2), np.float32(0)).astype(np.float32)
    depth = np.repeat(np.linalg.norm(X - o, axis=2)[..., None], 3, axis=2)

    def frame(offset, gain, mask):
        obj = X - offset                                              # the quad's own coordinates of what each pixel shows
        ramp = gain * (0.5 + obj[..., :1] * gx + obj[..., 1:2] * gy)
        assert ramp.min() >= 0.0 and ramp.max() <= 1.0
        colour = film(ramp, mask)
        c32 = colour[..., :3]
        return (colour, film(c32 * c32, mask), film(1.0, mask), film((0.0, 0.0, -1.0), mask), film(depth, mask)), np.where(mask, 0, MISS).astype(np.uint32)

    mask1 = np.zeros((h, w), bool)
    mask1[8:40, 10:50] = True
    mask2 = np.zeros((h, w), bool)
    mask2[8:40, 10 + shift_pixels:50 + shift_pixels] = True
    films1, ids1 = frame(np.zeros(3), 1.0, mask1)
    films2, ids2 = frame(shift, 0.8, mask2)
    rows = kz.motion_rows(translate(shift).astype(np.float32)[None], None)
    return view, films1, ids1, films2, ids2, rows, shift


# ---------------------------------------------------------------- the sequences of the quality figures
_quality = {}


def quality_inputs(kz, O, ref, tmp_path_factory, scene):
    """The oracle's canonical films of `scene` at 96 x 72: 4 and 16 spp noisy, 1024 spp clean, the AOV reference's feature films and the moment film of `ref`
    (lib("variance") or a library that inherits it). Computed once per scene and shared by the modules that ask: the 1024 spp film is the expensive one."""
    if scene not in _quality:
        make = {"cornell": kz.scenes.cornell_box, "materials": kz.scenes.materials_scene, "textured": kz.scenes.textured_scene}[scene]
        clean = O.OracleScene(make(96, 72, 1024)).render_canonical(threads=0)
        per = {}
        for spp in (4, 16):
            desc = make(96, 72, spp)
            noisy = O.OracleScene(desc).render_canonical(threads=0)
            aov = AovRef(lib("aov", tmp_path_factory.mktemp("kza")), desc)
            per[spp] = (noisy, MomentRef(ref, desc).moment_film(), [aov.film(a) for a in GUIDES])
        _quality[scene] = (clean, per)
    return _quality[scene]


def reference_frames(kz, L, aov_lib, descs):
    """Per frame f the reference's inputs of descs[f] (96 x 72), 4 spp from the sample range [4f, 4f + 4): (noisy, moment, [guides], border, view, ids)."""
    out = []
    for f, d in enumerate(descs):
        mr = MomentRef(L, d)
        out.append((mr.film(4 * f, 4 * f + 4), mr.moment_film(4 * f, 4 * f + 4), [AovRef(aov_lib, d).film(g, 4 * f, 4 * f + 4) for g in GUIDES], mr.border,
                    kz.temporal_view(d.camera), ref_ids(L, d)))
    return out


def light_step(kz, spp, f, at=8):
    """Cornell at 96 x 72 as frame f of the light step sees it: from frame `at` on the lamp is NEW_LIGHT."""
    d = kz.scenes.cornell_box(96, 72, spp)
    if f >= at:
        d.meshes[LAMP] = dict(d.meshes[LAMP], light=kz.scenes.area(NEW_LIGHT["color"], NEW_LIGHT["intensity"], False))
    return d


def chains(kz, L, frames, rows_of=None, which=("responsive", "motion", "alone"), **ropts):
    """The chains over `frames` (reference_frames' tuples): per frame the pictures of "responsive", "motion" (the kz_motion_ref chain) and "alone" (the frame
    without a history); the responsive chain's histories; and per frame (eligible, clamped): the pixels of the responsive call with N_l > fastHistory and those of
    them the clamp changed, from the same call with CLAMP_OFF. rows_of(f): the frame's row table (default: Cornell's eight meshes, static)."""
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    pics, hists, counts = {k: [] for k in which}, [], []
    hr = hm = fast = prev = None
    for f, (noisy, moment, guides, b, view, ids) in enumerate(frames):
        rows = rows_of(f) if rows_of else static_rows(kz, 8)
        kw = dict(border=b, samples=4, current=view, previous=prev, ids=ids, rows=rows)
        if "responsive" in which:
            off = ref_denoise_responsive(L, kz, noisy, moment, *guides, history=hr, fast=fast, **dict(ropts, clamp=False), **kw)[1]
            out, hr, fast, _ = ref_denoise_responsive(L, kz, noisy, moment, *guides, history=hr, fast=fast, **ropts, **kw)
            pics["responsive"].append(out)
            hists.append(hr)
            counts.append((int((off[..., 8] > (ropts.get("fast_history") or 2)).sum()), int((bits(off[..., :4]) != bits(hr[..., :4])).any(axis=2).sum())))
        if "motion" in which:
            out, hm, _ = ref_denoise_motion(L, kz, noisy, moment, *guides, history=hm, **kw)
            pics["motion"].append(out)
        if "alone" in which:
            pics["alone"].append(ref_denoise_motion(L, kz, noisy, moment, *guides, **dict(kw, previous=None))[0])
        prev = view
    return pics, hists, counts
