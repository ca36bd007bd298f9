"""Scenes and seeded ray sets of the ray-level tests of the BVH4 traversal kernels (tests/test_trace_wf_cpu.py, tests/test_trace_wf_gpu.py).

The kernels a render launches - kz_wf_trace<0|1|2|4>, kz_wf_trace_packet - are run on these rays through Scene.trace_rays_wf and compared ray by ray with the
brute-force oracle. The sets aim at what a render rarely or never sends: direction components that are exactly zero or next to the 1e-20 stand-in, origins
that lie bit for bit on the planes of the quantised BVH4 packets with tmin = 0, rays through vertices and edge midpoints, tmax one ulp around the hit, dead
rays (NaN / inf / zero direction) between live ones, and - for the shadow kernels - segments that end on, stop short of and pass through a light of
lightPrimaryVisibility == false. test_trace_wf_cpu.py holds every set to what it claims, on the oracle alone.

With deform=..., a case is the scene AFTER an edit (Scene.set_vertices, `deformation` below): the build's topology under refit boxes that no longer form a good
tree. Scene, oracle, ray sets and reference are then those of the deformed description, and two aimed sets (h), (i) follow the others
(tests/test_trace_refit_cpu.py, tests/test_trace_refit_gpu.py). Last: a launch of kz_trace_rays_wf on a case and the checks of its result, which the two GPU modules share."""
import numpy as np

from checks import same_bits

NODE4 = np.dtype([("p", "<f4", 3), ("scaleX", "<f4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("scaleY", "<f4"), ("scaleZ", "<f4"), ("child", "<u4", 4)])
EPS = np.float32(1e-3)                 # the scenes' traceBias (SceneDescription's default)
SCENES = ("cornell", "soup", "coincident", "cornell_il", "panel")
CLOSEST_SCENES = ("cornell", "soup", "coincident")
SHADOW_SCENES = ("cornell_il", "soup", "panel")
ROOM = {"cornell": ((-1, -1, -1), (1, 1, 1)), "cornell_il": ((-1, -1, -1), (1, 1, 1)), "panel": ((-1, -1, -1), (1, 1, 1)),
        "soup": ((-1.2, -1.2, -1.2), (1.2, 1.2, 3.6)), "coincident": ((0, 0, -1), (1, 1, 1))}


def scene(S, name):
    """cornell: 36 triangles, a shallow tree, its light invisible to camera rays (the packet kernel's FIX variant). soup: 5000 random triangles in a closed room
    with eight invisible lights (16 triangles: shadowFast = 1), deep enough that an LDS stack of 2 entries spills. coincident: three identical triangles.
    cornell_il: the cornell box with lightPrimaryVisibility stated false (shadowFast = 1, 2 invisible-light triangles). panel: the cornell box whose light is a
    6 x 6 grid of quads hanging at y = 0.5 - 72 invisible-light triangles, more than the any-hit shadow kernel takes: shadowFast = 0."""
    if name == "cornell":
        return S.cornell_box(32, 32, 1)
    if name == "soup":
        return S.random_triangles(5000, 32, 32, 1, sampler="independent", s_edge=0.08)
    if name == "coincident":
        s = S.SceneDescription()
        V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
        N = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
        for _ in range(3):
            s.add_mesh(V, np.array([[0, 1, 2]], np.uint32), N)
        s.camera.update(width=32, height=32)
        return s
    if name == "cornell_il":
        s = S.cornell_box(32, 32, 1)
        s.meshes[-1] = dict(s.meshes[-1], light=S.area((1, 1, 1), 15.0, False))
        return s
    if name == "panel":
        s = S.cornell_box(32, 32, 1)
        xs = np.linspace(-0.5, 0.5, 7)
        parts = [S.quad((xs[i], 0.5, xs[k]), (xs[i], 0.5, xs[k + 1]), (xs[i + 1], 0.5, xs[k + 1]), (xs[i + 1], 0.5, xs[k]), flip=True) for i in range(6) for k in range(6)]
        P, N, UV, F = S.merge(parts)
        s.meshes[-1] = dict(s.meshes[-1], V=P, N=N, UV=UV, F=F, light=S.area((1, 1, 1), 15.0, False))
        return s
    raise KeyError(name)


def invisible_meshes(desc):
    return [i for i, m in enumerate(desc.meshes) if m["light"] is not None and not m["light"]["lightPrimaryVisibility"]]


def only_meshes(S, desc, keep):
    """The scene with nothing but the meshes `keep` (no lights): brute force on it says whether a segment crosses one of THEIR triangles, whatever lies in front."""
    s = S.SceneDescription()
    for i in keep:
        m = desc.meshes[i]
        s.add_mesh(m["V"], m["F"], m["N"], m["UV"])
    s.camera.update(width=32, height=32)
    return s


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _inside(rng, name, n, shrink=0.9):
    lo, hi = (np.array(x, np.float64) for x in ROOM[name])
    c, h = (lo + hi) / 2, (hi - lo) / 2 * shrink
    return (c + rng.uniform(-1, 1, (n, 3)) * h).astype(np.float32)


def _triangles(desc):
    """(nTris, 3, 3) float32: every triangle's vertices, mesh after mesh."""
    return np.concatenate([np.asarray(m["V"], np.float32)[np.asarray(m["F"], np.int64)] for m in desc.meshes])


# ------------------------------------------------------------------------------------------------ closest-hit sets
def set_random(name, n, seed):
    """(a) random origins in the room, random unit directions; the first 64 axis-aligned."""
    rng = np.random.default_rng(seed)
    o = _inside(rng, name, n)
    d = _unit(rng.normal(size=(n, 3)))
    k = min(64, n)
    d[:k] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.choice([-1, 1], k)[:, None].astype(np.float32)
    return o, d, np.full(n, EPS, np.float32), np.full(n, np.inf, np.float32)


TINY = (1e-21, 1e-20, 1e-19)


def set_zero_components(name, per, seed):
    """(b) directions with one, two and three components exactly zero - as +0 and as -0 - and every sign combination of the others, and directions with a component of
    +-1e-21, +-1e-20, +-1e-19 (below, at and above the kernels' stand-in threshold) alone and beside an exact zero. Returns the rays and, per ray, how many
    components are exactly zero."""
    rng = np.random.default_rng(seed)
    rows = []
    for zero in (0.0, -0.0):
        for mask in range(1, 8):                                   # bit a set: component a is zero
            free = [a for a in range(3) if not mask >> a & 1]
            for signs in range(1 << len(free)):
                for _ in range(per):
                    v = np.full(3, zero)
                    for j, a in enumerate(free):
                        v[a] = (1 if signs >> j & 1 else -1) * rng.uniform(0.2, 1.0)
                    rows.append(v)
    for t in TINY:
        for sg in (1, -1):
            for a in range(3):
                for _ in range(per):
                    v = rng.normal(size=3)
                    v[a] = sg * t
                    rows.append(v)                                 # a tiny component beside two ordinary ones
                    w = v.copy()
                    w[(a + 1) % 3] = 0.0
                    rows.append(w)                                 # ... and beside an exact zero
    d = np.array(rows, np.float64)
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    ln[ln == 0] = 1
    d64 = d / ln
    d = d64.astype(np.float32)
    d[np.abs(np.array(rows)) < 1e-18] = np.array(rows, np.float32)[np.abs(np.array(rows)) < 1e-18]      # the zeros (signed) and the tiny values stay what they are
    n = len(d)
    o = _inside(rng, name, n)
    return (o, d, np.full(n, EPS, np.float32), np.full(n, np.inf, np.float32)), (d == 0).sum(axis=1)


def packet_planes(nodes4):
    """Per axis, the float32 values that ARE a plane of a BVH4 packet: the packet origins p and the dequantised p + q * scale that are exact in fp32 (q = a
    quantised bound of a non-empty child slot). Returns a list of (axis, value, node index, q)."""
    out = []
    for i, nd in enumerate(nodes4):
        scale = (nd["scaleX"], nd["scaleY"], nd["scaleZ"])
        for a in range(3):
            qs = {0}
            for k in range(4):
                lo, hi = int(nd["qlo"][a]) >> (8 * k) & 255, int(nd["qhi"][a]) >> (8 * k) & 255
                if hi >= lo:
                    qs |= {lo, hi}
            for q in sorted(qs):
                exact = float(nd["p"][a]) + q * float(scale[a])
                if float(np.float32(exact)) == exact:
                    out.append((a, np.float32(exact), i, q))
    return out


def node_box(nd):
    """The union of a packet's child boxes (float64 lo, hi)."""
    scale = np.array([nd["scaleX"], nd["scaleY"], nd["scaleZ"]], np.float64)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for a in range(3):
        for k in range(4):
            l, h = int(nd["qlo"][a]) >> (8 * k) & 255, int(nd["qhi"][a]) >> (8 * k) & 255
            if h >= l:
                lo[a], hi[a] = min(lo[a], nd["p"][a] + l * scale[a]), max(hi[a], nd["p"][a] + h * scale[a])
    return lo, hi


def set_on_planes(name, nodes4, n, seed):
    """(c) origins with one component equal, bit for bit, to a plane of a BVH4 packet (half of them a packet origin p itself: q = 0, where the kernels' q * a + b comes
    out as -0.0 for a negative direction), the other two inside that packet's boxes; tmin = 0; directions of both signs, a third of them axis-aligned and a third
    aligned with the plane's own axis. Returns the rays and the plane (axis, value) of each."""
    rng = np.random.default_rng(seed)
    planes = packet_planes(nodes4)
    origins = [p for p in planes if p[3] == 0]
    o, d, ax, val = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int64), np.zeros(n, np.float32)
    for i in range(n):
        a, v, node, q = (origins if i % 2 == 0 else planes)[rng.integers(0, len(origins if i % 2 == 0 else planes))]
        lo, hi = node_box(nodes4[node])
        lo, hi = np.maximum(lo, np.array(ROOM[name][0], np.float64)), np.minimum(hi, np.array(ROOM[name][1], np.float64))
        p = (lo + rng.uniform(0.02, 0.98, 3) * (hi - lo)).astype(np.float32)
        p[a] = v
        o[i], ax[i], val[i] = p, a, v
        kind = i // 2 % 3
        if kind == 0:
            d[i] = _unit(rng.normal(size=3))
        elif kind == 1:
            d[i, rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
        else:
            d[i, a] = rng.choice([-1.0, 1.0])
    return (o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)), (ax, val)


def set_vertices_and_edges(name, desc, n, seed):
    """(d) rays from inside the room at mesh vertices and edge midpoints: the hits lie on shared edges and corners, where neighbours tie."""
    rng = np.random.default_rng(seed)
    T = _triangles(desc)
    t = T[rng.integers(0, len(T), n)]
    k = rng.integers(0, 3, n)
    vert = t[np.arange(n), k]
    mid = ((t[np.arange(n), k].astype(np.float64) + t[np.arange(n), (k + 1) % 3]) / 2).astype(np.float32)
    target = np.where((np.arange(n) % 2 == 0)[:, None], vert, mid)
    o = _inside(rng, name, n, 0.85)
    d = _unit(target.astype(np.float64) - o)
    return o, d, np.full(n, EPS, np.float32), np.full(n, np.inf, np.float32)


def set_tmax_around_hit(ora, name, n, seed, pinched=192):
    """(e) tmax one ulp below, at and one ulp above a hit distance the brute force reports: of the ray's closest hit t1 (rows 0-2 of a ray: clipped away, kept, kept) and
    of its second hit t2 - the closest hit behind t1 - (rows 3-5: the ray then returns t1 in every position). Behind them `pinched` rays with tmin = tmax = t1: the
    interval is closed at both ends (mesh.cpp:91), the hit stays. Every box that holds such a hit is entered at max(tnear, tmin) = tmax; the pinched rays are
    those whose t1 has its two low bits clear - the bits the packet kernel's child keys give to the slot number - so that key and tmax compare EQUAL, and they
    fill whole waves, so that no other lane keeps a stack entry alive. Returns the rays and each row's position (-1, 0, +1; 2 = pinched)."""
    o, d, tmin, _ = set_random(name, 4 * n, seed)
    h1 = ora.trace_rays(o, d, tmin, np.inf)
    t1 = h1["t"]
    h2 = ora.trace_rays(o, d, np.nextafter(t1, np.float32(np.inf)), np.inf)
    keep = np.flatnonzero(np.isfinite(t1) & np.isfinite(h2["t"]))[:n]
    rows_o, rows_d, rows_tmin, rows_tmax, pos = [], [], [], [], []
    for t in (t1[keep], h2["t"][keep]):
        for p, tm in ((-1, np.nextafter(t, np.float32(-np.inf))), (0, t), (1, np.nextafter(t, np.float32(np.inf)))):
            rows_o.append(o[keep]); rows_d.append(d[keep]); rows_tmin.append(tmin[keep]); rows_tmax.append(tm.astype(np.float32)); pos.append(np.full(len(keep), p))
    po, pd, ptmin, _ = set_random(name, 8 * pinched, seed + 50)
    pt = ora.trace_rays(po, pd, ptmin, np.inf)["t"]
    pk = np.flatnonzero(np.isfinite(pt) & (pt.view(np.uint32) & 3 == 0))[:pinched]
    rows_o.append(po[pk]); rows_d.append(pd[pk]); rows_tmin.append(pt[pk]); rows_tmax.append(pt[pk]); pos.append(np.full(len(pk), 2))
    return (np.concatenate(rows_o), np.concatenate(rows_d), np.concatenate(rows_tmin), np.concatenate(rows_tmax)), np.concatenate(pos)


def dead_rows():
    """The NaN / zero / infinite rays of test_ray_edge_cases: (o, d) that must miss at once, not walk the tree."""
    o = np.array([[np.nan, 0, 0], [0.2, 0.2, 1], [0.2, 0.2, 1], [0.2, 0.2, 1], [0.2, np.inf, 0.1], [0.1, 0.2, -np.inf]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, 0], [np.inf, 0, -1], [0, np.nan, -1], [0, 0, -1], [0, 1, 0]], np.float32)
    return o, d


def set_dead_between_live(name, n, seed):
    """(f) those rows between live rays - every fourth ray is dead, so every wave mixes dead and live lanes. Returns the rays and the mask of the dead rows."""
    o, d, tmin, tmax = set_random(name, n, seed)
    do, dd = dead_rows()
    dead = np.arange(n) % 4 == 1
    idx = np.flatnonzero(dead)
    o[idx], d[idx] = do[np.arange(len(idx)) % len(do)], dd[np.arange(len(idx)) % len(dd)]
    return (o, d, tmin, tmax), dead


def set_outside(name, n, seed):
    """(g) origins outside the room: half of the rays point away from it and miss, the others have random directions (many enter through a wall)."""
    rng = np.random.default_rng(seed)
    lo, hi = (np.array(x, np.float64) for x in ROOM[name])
    c, h = (lo + hi) / 2, (hi - lo) / 2
    u = _unit(rng.normal(size=(n, 3))).astype(np.float64)
    o = (c + u * np.linalg.norm(h) * rng.uniform(1.1, 2.0, (n, 1))).astype(np.float32)
    d = np.where((np.arange(n) % 2 == 0)[:, None], _unit(u + 0.3 * rng.normal(size=(n, 3))), _unit(c - o + np.linalg.norm(h) * 0.7 * rng.normal(size=(n, 3))))
    return o, d.astype(np.float32), np.full(n, EPS, np.float32), np.full(n, np.inf, np.float32)


def set_aimed(name, desc, meshes, n, seed):
    """Rays from inside the room at uniform points of the triangles of `meshes` as `desc` places them (degenerate triangles included: their points lie on a segment
    or are one point)."""
    rng = np.random.default_rng(seed)
    target = _light_points(rng, desc, meshes, n)
    o = _inside(rng, name, n, 0.85)
    return o, _unit(target - o), np.full(n, EPS, np.float32), np.full(n, np.inf, np.float32)


def closest_sets(S, name, host_scene, ora, seed=5):
    """{set name: (o, d, tmin, tmax)} of scene `name`, with {set name: extra} beside it. host_scene: a kz.Scene of it (its host copy of the BVH4); ora: its brute-force oracle.
    The sizes are the smallest that fill several waves per set and, together, more rays than one static batch per wave of a one-workgroup launch."""
    desc = host_scene.desc
    extra = {}
    if name == "coincident":
        rng = np.random.default_rng(seed)
        n = 192
        o = np.stack([rng.uniform(-0.2, 1.0, n), rng.uniform(-0.2, 1.0, n), np.ones(n)], 1).astype(np.float32)
        d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
        d[1::3] = _unit(np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), -np.ones(n)], 1))[1::3]
        tmax = np.full(n, np.inf, np.float32)
        tmax[2::8] = 0.5                                                # clipped in front of the triangles
        d[5::16] = np.array([0, 0, 1], np.float32)                     # pointing away
        sets = {"a": (o, d, np.zeros(n, np.float32), tmax)}
        (fo, fd, ft0, ft1), dead = set_dead_between_live(name, 128, seed + 5)
        fo[~dead], fd[~dead] = o[:128][~dead], d[:128][~dead]
        sets["f"], extra["f"] = (fo, fd, np.zeros(128, np.float32), ft1), dead
        return sets, extra
    big = name == "cornell"
    nodes4 = host_scene.table(1).view(NODE4)                           # KZ_TABLE_NODES4
    sets = {"a": set_random(name, 4096 if big else 2048, seed)}
    sets["b"], extra["b"] = set_zero_components(name, 12 if big else 6, seed + 1)
    sets["c"], extra["c"] = set_on_planes(name, nodes4, 1536 if big else 1024, seed + 2)
    sets["d"] = set_vertices_and_edges(name, desc, 1024 if big else 768, seed + 3)
    sets["e"], extra["e"] = set_tmax_around_hit(ora, name, 128, seed + 4)
    sets["f"], extra["f"] = set_dead_between_live(name, 512, seed + 5)
    sets["g"] = set_outside(name, 512, seed + 6)
    return sets, extra


def concat(sets):
    """All sets of a scene as one ray array (o, d, tmin, tmax), with the [begin, end) of each."""
    spans, at = {}, 0
    for k, s in sets.items():
        spans[k] = (at, at + len(s[0]))
        at += len(s[0])
    return tuple(np.ascontiguousarray(np.concatenate([s[j] for s in sets.values()])) for j in range(4)), spans


# ------------------------------------------------------------------------------------------------ shadow sets
def _light_points(rng, desc, meshes, n):
    """n uniform points on the triangles of `meshes` (float64) and the triangle of each."""
    T = np.concatenate([np.asarray(desc.meshes[m]["V"], np.float32)[np.asarray(desc.meshes[m]["F"], np.int64)] for m in meshes]).astype(np.float64)
    t = T[rng.integers(0, len(T), n)]
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    f = u + v > 1
    u[f], v[f] = 1 - u[f], 1 - v[f]
    return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])


def _segment(a, b, cut):
    """The shadow ray from a towards b: unit direction, tmin = eps, tmax = |b - a| - cut (float32 arithmetic, as the integrator forms it)."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    v = b - a
    dist = np.sqrt((v * v).sum(axis=1, dtype=np.float32)).astype(np.float32)
    d = (v / dist[:, None]).astype(np.float32)
    return a, d, np.full(len(a), EPS, np.float32), (dist - np.float32(cut)).astype(np.float32)


def shadow_pairs(name, n, seed):
    """Segments between random point pairs of the room: tmin = 1e-3, tmax = |b - a| - 1e-3."""
    rng = np.random.default_rng(seed)
    return _segment(_inside(rng, name, n, 0.97), _inside(rng, name, n, 0.97), EPS)


def shadow_to_lights(name, desc, ora, n, seed):
    """Segments from surface points to points on the lights - the invisible ones included - with tmax = dist - eps, as the integrator forms them. The surface points
    are the brute-force hits of rays that start in the lower half of the room and do not point upwards: the floor, the lower walls and the sides of what stands
    on the floor, a good part of which the objects hide from the lights."""
    rng = np.random.default_rng(seed)
    o, d, tmin, tmax = set_random(name, 3 * n, seed + 100)
    lo, hi = (np.array(x, np.float32) for x in ROOM[name])
    o[:, 1] = lo[1] + (o[:, 1] - lo[1]) * np.float32(0.45)
    d[:, 1] = -np.abs(d[:, 1])
    h = ora.trace_rays(o, d, tmin, tmax)
    ok = np.flatnonzero(h["mesh"] >= 0)[:n]
    lights = [i for i, m in enumerate(desc.meshes) if m["light"] is not None]
    return _segment(h["p"][ok], _light_points(rng, desc, lights, len(ok)), EPS)


def shadow_through_invisible(name, desc, n, seed):
    """Segments aimed from below at points of the invisible lights that go on behind them: half end between the light and the ceiling, the others behind the ceiling."""
    rng = np.random.default_rng(seed)
    L = _light_points(rng, desc, invisible_meshes(desc), n)
    lo, hi = (np.array(x, np.float64) for x in ROOM[name])
    v = rng.normal(size=(n, 3))
    v[:, 1] = -np.abs(v[:, 1]) - 0.3
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.1, 0.7, (n, 1))
    a = np.clip(L + v, lo + 0.02, hi - 0.02)
    u = (L - a) / np.linalg.norm(L - a, axis=1, keepdims=True)
    reach = (hi[1] - L[:, 1]) / u[:, 1]                                    # from the light to the ceiling along the segment
    ext = np.where(np.arange(n) % 2 == 0, rng.uniform(0.2, 0.8, n) * reach, reach + rng.uniform(0.01, 0.3, n))
    return _segment(a, L + u * ext[:, None], 0.0)


def shadow_sets(S, name, desc, ora, seed=5):
    n = 768 if name == "soup" else 1024
    return {"pairs": shadow_pairs(name, n, seed + 10), "lights": shadow_to_lights(name, desc, ora, n, seed + 11), "through": shadow_through_invisible(name, desc, n, seed + 12)}


def shadow_reference(ora, ora_il, desc, o, d, tmin, tmax, eps=EPS):
    """The occlusion test of integrator.cpp:257-278, composed from brute-force closest hits in float32: a miss is free; a hit on anything but a light with
    lightPrimaryVisibility == false is occluded; else o = o + d * (t + eps), tmin = eps, tmax = tmax - t, again. ora_il: the brute-force oracle of the invisible
    lights alone (None: the scene has none). Returns (occluded, walk-throughs per ray, whether the ORIGINAL segment crosses an invisible-light triangle at all -
    in front of or behind whatever else it hits)."""
    inv = np.zeros(len(desc.meshes) + 1, bool)
    inv[invisible_meshes(desc)] = True
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    tmin, tmax = np.array(tmin, np.float32), np.array(tmax, np.float32)
    n = len(o)
    crosses = np.zeros(n, bool) if ora_il is None else ora_il.trace_rays(o, d, tmin, tmax)["mesh"] >= 0
    occluded, walks = np.zeros(n, bool), np.zeros(n, np.int64)
    live = np.arange(n)
    while len(live):
        h = ora.trace_rays(o[live], d[live], tmin[live], tmax[live])
        hit = h["mesh"] >= 0
        through = hit & inv[h["mesh"]]
        occluded[live[hit & ~through]] = True
        go = live[through]
        t = h["t"][through]
        o[go] = o[go] + d[go] * (t + np.float32(eps))[:, None]
        tmin[go] = np.float32(eps)
        tmax[go] = tmax[go] - t
        walks[go] += 1
        live = go
    return occluded, walks, crosses


# ------------------------------------------------------------------------------------------------ deformations: the same topology under boxes that stopped forming a good tree
DEFORMS = {"soup": ("scatter", "slivers", "stacked", "nested"), "cornell": ("flattened",), "cornell_il": ("flattened",)}
SOUP_MESHES, SOUP_LIGHTS = tuple(range(8)), tuple(range(9, 17))       # random_triangles(5000): eight meshes of 625 unshared triangles, the room, eight light quads
STACKED = (0, 1, 2, 3)                                                # `stacked`: the meshes that end up coincident
NESTED_FACTORS = (1.0, 0.85, 0.7, 0.55, 0.4, 0.25, 0.1, 0.05)         # `nested`: steps of 0.15 down to 0.1; the eighth mesh keeps a positive factor
FLAT_POINT = (0.35, -0.6, 0.3)                                        # `flattened`: where mesh 6 collapses to
REFIT_CLOSEST = (("soup", "scatter"), ("soup", "slivers"), ("soup", "stacked"), ("soup", "nested"), ("cornell", "flattened"))
REFIT_SHADOW = (("soup", "scatter"), ("cornell_il", "flattened"))


def deformation(name, desc, deform, seed=71):
    """{mesh: (V, N)} of deformation `deform` of scene `name` (Scene.set_vertices' argument): seeded, inside ROOM[name], every mesh named once, N as it is.
    soup - scatter: inside each soup mesh every triangle moves rigidly so that its centroid lands on the centroid of triangle pi(i), pi a seeded permutation, and
    the light quads change places along a seeded 8-cycle: a leaf then holds triangles from anywhere in the room and every inner box is about the room's size.
    slivers: V' = V[perm] inside each soup mesh - triangles whose corners are three random points of the mesh. stacked: meshes 1, 2, 3 take mesh 0's vertices bit
    for bit - four coincident copies in four subtrees. nested: soup mesh k is scaled about the room's centre by NESTED_FACTORS[k].
    cornell, cornell_il - flattened: the tall box (mesh 5) gets the floor's y in every vertex, the short box (mesh 6) collapses to FLAT_POINT, the light drops by 0.3."""
    rng = np.random.default_rng(seed)
    M = desc.meshes
    upd = {}
    if deform == "scatter":
        for m in SOUP_MESHES:
            T = np.asarray(M[m]["V"], np.float32).reshape(-1, 3, 3).astype(np.float64)
            c = T.mean(axis=1)
            upd[m] = (T + (c[rng.permutation(len(T))] - c)[:, None, :]).astype(np.float32).reshape(-1, 3)
        order = rng.permutation(len(SOUP_LIGHTS))
        cent = {m: np.asarray(M[m]["V"], np.float64).mean(axis=0) for m in SOUP_LIGHTS}
        for i, k in enumerate(order):
            a, b = SOUP_LIGHTS[k], SOUP_LIGHTS[order[(i + 1) % len(order)]]
            upd[a] = (np.asarray(M[a]["V"], np.float64) + (cent[b] - cent[a])).astype(np.float32)
    elif deform == "slivers":
        for m in SOUP_MESHES:
            V = np.asarray(M[m]["V"], np.float32)
            upd[m] = V[rng.permutation(len(V))]
    elif deform == "stacked":
        for m in STACKED[1:]:
            upd[m] = np.asarray(M[STACKED[0]]["V"], np.float32).copy()
    elif deform == "nested":
        lo, hi = (np.array(x, np.float64) for x in ROOM[name])
        c = (lo + hi) / 2
        for m, f in zip(SOUP_MESHES[1:], NESTED_FACTORS[1:]):              # (factor 1.0 leaves mesh 0 where it is: not named)
            upd[m] = (c + (np.asarray(M[m]["V"], np.float64) - c) * f).astype(np.float32)
    elif deform == "flattened":
        V5 = np.asarray(M[5]["V"], np.float32).copy()
        V5[:, 1] = np.asarray(M[0]["V"], np.float32)[0, 1]
        V7 = np.asarray(M[7]["V"], np.float32).copy()
        V7[:, 1] -= np.float32(0.3)
        upd = {5: V5, 6: np.tile(np.array(FLAT_POINT, np.float32), (len(M[6]["V"]), 1)), 7: V7}
    else:
        raise KeyError(deform)
    return {m: (np.ascontiguousarray(V, np.float32), M[m]["N"]) if M[m]["N"] is not None else np.ascontiguousarray(V, np.float32) for m, V in upd.items()}


# ------------------------------------------------------------------------------------------------ a scene's rays with their reference, made once per process
_cases = {}


def edited_scene(kz, name, deform, device, lib=None):
    """The scene built from its description and then, with a deformation, edited in place: the tree keeps the build's topology under refit boxes, desc follows."""
    desc = scene(kz.scenes, name)
    sc = kz.Scene(desc, device=device, lib=lib)
    if deform is not None:
        sc.set_vertices(deformation(name, sc.desc, deform))
    return sc


def closest_case(kz, O, name, device=None, deform=None):
    """{"desc", "scene" (kz.Scene, on `device` if given), "rays" (o, d, tmin, tmax of all sets), "spans", "extra", "ref" (the brute-force hits)} of a closest-hit scene.
    deform: a name of DEFORMS[name] - the scene is built, then deformed with set_vertices; the oracle, the ray sets (set (c) from the REFIT packets) and the
    reference are those of the deformed description."""
    key = ("closest", name, device, deform)
    if key not in _cases:
        sc = edited_scene(kz, name, deform, device)
        desc = sc.desc
        ora = O.OracleScene(desc, brute=True)
        sets, extra = closest_sets(kz.scenes, name, sc, ora)
        if deform is not None:
            # the room is large and the soup thin - of the 2 048 rays of set (a) 66 end on the coincident copies of `stacked`, and the boxes of `flattened` are a small
            # part of their room - so two AIMED sets follow: (h) at the meshes the deformation names where they are now, (i) at where they were before the edit
            before = scene(kz.scenes, name)
            moved = sorted(deformation(name, before, deform))
            sets["h"], sets["i"] = set_aimed(name, desc, moved, 2048, 12), set_aimed(name, before, moved, 1024, 13)
        rays, spans = concat(sets)
        _cases[key] = {"desc": desc, "scene": sc, "ora": ora, "rays": rays, "spans": spans, "extra": extra, "ref": ora.trace_rays(*rays)}
    return _cases[key]


def shadow_case(kz, O, name, device=None, deform=None):
    """The same for a shadow scene: "ref" = (occluded, walk-throughs, crosses an invisible-light triangle) per segment (shadow_reference)."""
    key = ("shadow", name, device, deform)
    if key not in _cases:
        sc = edited_scene(kz, name, deform, device)
        desc = sc.desc
        ora = O.OracleScene(desc, brute=True)
        ora_il = O.OracleScene(only_meshes(kz.scenes, desc, invisible_meshes(desc)), brute=True)
        rays, spans = concat(shadow_sets(kz.scenes, name, desc, ora))
        _cases[key] = {"desc": desc, "scene": sc, "ora": ora, "ora_il": ora_il, "rays": rays, "spans": spans, "ref": shadow_reference(ora, ora_il, desc, *rays)}
    return _cases[key]


def flattened_ties(kz, O, case):
    """The rays of a flattened case whose closest hit lies on the squashed box's footprint with the floor's triangle and the box's triangle at the SAME t, bit for bit
    (the floor alone and the box alone answer with the bits of the scene's closest hit): a tie between mesh 0 and mesh 5."""
    floor = O.OracleScene(only_meshes(kz.scenes, case["desc"], [0]), brute=True).trace_rays(*case["rays"])
    box = O.OracleScene(only_meshes(kz.scenes, case["desc"], [5]), brute=True).trace_rays(*case["rays"])
    t = case["ref"]["t"].view(np.uint32)
    return (floor["mesh"] >= 0) & (box["mesh"] >= 0) & (floor["t"].view(np.uint32) == t) & (box["t"].view(np.uint32) == t)


# ------------------------------------------------------------------------------------------------ a launch of kz_trace_rays_wf on a case, and its checks
LDS_ENTRIES = 16                              # stack entries per lane the default launch keeps in LDS
KINDS = {0: "per-lane", 1: "packet", 2: "walk-through"}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sentinel_hits(n):
    """A hit record per slot that no kernel writes: t = 2^20 + slot, u, v, and a gid the scene does not have."""
    h = np.zeros((n, 4), np.float32)
    h[:, 0] = np.float32(1 << 20) + np.arange(n, dtype=np.float32)
    h[:, 1], h[:, 2] = 0.125, 0.375
    h[:, 3] = (np.uint32(0xF0000000) | np.arange(n, dtype=np.uint32)).view(np.float32)
    return h


def sums_before(n):
    return ((np.arange(3 * n, dtype=np.float32) + 1) * np.float32(0.03125)).reshape(n, 3)


def pending_of(n):
    return ((np.arange(3 * n, dtype=np.float32) + 1) * np.float32(0.001)).reshape(n, 3)


def run(case, kernel, queue=None, **opts):
    o, d, tmin, tmax = case["rays"]
    n = len(o)
    return case["scene"].trace_rays_wf(o, d, tmin, tmax, kernel=kernel, queue=queue, hits=sentinel_hits(n), sums=sums_before(n), pending=pending_of(n), **opts)


def report(case, bad, got, want, what):
    o, d, tmin, tmax = case["rays"]
    lines = ["%s: %d of %d rays differ; the first:" % (what, len(bad), len(o))]
    for i in bad[:6]:
        lines.append("  ray %d o=%r d=%r tmin=%r tmax=%r\n    kernel: %s\n    oracle: %s" % (i, o[i].tolist(), d[i].tolist(), float(tmin[i]), float(tmax[i]),
                     {k: got[k][i].tolist() for k in ("t", "u", "v", "mesh", "prim")}, {k: want[k][i].tolist() for k in ("t", "u", "v", "mesh", "prim")}))
    return "\n".join(lines)


def check_closest(case, kernel, res, queue=None):
    """`res` against the brute-force hits for the slots of `queue` (None: all), the sentinel for the others; the sums untouched everywhere."""
    ref, n = case["ref"], len(case["rays"][0])
    queued = np.ones(n, bool) if queue is None else np.isin(np.arange(n), queue)
    sent = sentinel_hits(n)
    hit = ref["mesh"] >= 0
    want = {"t": np.where(hit, ref["t"], np.float32(np.inf)), "u": np.where(hit, ref["u"], np.float32(0)), "v": np.where(hit, ref["v"], np.float32(0)),
            "mesh": ref["mesh"].copy(), "prim": ref["prim"].copy()}
    if kernel == 2:                      # the walk-through ray keeps the slot's previous hit on a miss
        for j, k in enumerate(("t", "u", "v")):
            want[k] = np.where(hit, want[k], sent[:, j])
    keep = ~queued | ((kernel == 2) & ~hit)
    for j, k in enumerate(("t", "u", "v")):
        want[k] = np.where(queued, want[k], sent[:, j]).astype(np.float32)
    want["mesh"][keep], want["prim"][keep] = -1, -1
    wrong = (res["mesh"] != want["mesh"]) | (res["prim"] != want["prim"])
    for k in ("t", "u", "v"):
        wrong |= u32(res[k]) != u32(want[k])
    wrong |= keep & (res["gid"] != u32(sent[:, 3]))                 # what a kernel must not write keeps its gid too
    wrong |= queued & ~hit & (kernel != 2) & (res["gid"] != 0)      # the miss record is (+inf, 0, 0, 0)
    bad = np.flatnonzero(wrong)
    assert len(bad) == 0, report(case, bad, res, want, "%s kernel" % KINDS[kernel])
    assert same_bits(res["sums"], sums_before(n)), "a closest-hit launch wrote sample sums"
    assert same_bits(res["t"][hit & queued], ref["t"][hit & queued])


SHAPES = [dict(grid_blocks=1, batch=64), dict(lds_stack=2), dict(refill=1), dict(refill=64), dict(postpone=1), dict(postpone=64), dict(stats=True),
          dict(stats=True, grid_blocks=1, batch=64, lds_stack=2, refill=64, postpone=1)]
PACKET_SHAPES = [dict(grid_blocks=1, packet_batch=1), dict(grid_blocks=2, packet_batch=3), dict(stats=True), dict(stats=True, grid_blocks=1, packet_batch=1)]
OUT = ("t", "u", "v", "gid", "mesh", "prim", "sums")


def same_result(a, b):
    return all(np.array_equal(u32(a[k]) if a[k].dtype == np.float32 else a[k], u32(b[k]) if b[k].dtype == np.float32 else b[k]) for k in OUT)


def check_shadow(case, res, queue=None, stats=False):
    occluded, walks, crosses = case["ref"]
    n = len(occluded)
    queued = np.ones(n, bool) if queue is None else np.isin(np.arange(n), queue)
    before, pend = sums_before(n), pending_of(n)
    want = np.where((queued & ~occluded)[:, None], before + pend, before).astype(np.float32)
    wrong = (u32(res["sums"]) != u32(want)).any(axis=1)
    bad = np.flatnonzero(wrong)
    o, d, tmin, tmax = case["rays"]
    msg = "\n".join("  segment %d o=%r d=%r tmin=%r tmax=%r queued=%s reference: occluded=%s walk-throughs=%d crosses=%s\n    sums before %r pending %r after %r" %
                    (i, o[i].tolist(), d[i].tolist(), float(tmin[i]), float(tmax[i]), queued[i], occluded[i], walks[i], crosses[i], before[i].tolist(), pend[i].tolist(), res["sums"][i].tolist()) for i in bad[:6])
    assert len(bad) == 0, "shadow kernels: %d of %d segments differ; the first:\n%s" % (len(bad), n, msg)
    sent = sentinel_hits(n)
    assert all(same_bits(res[k], sent[:, j]) for j, k in enumerate(("t", "u", "v"))) and np.array_equal(res["gid"], u32(sent[:, 3])), "a shadow launch wrote hit records"
    info = res["info"]
    if info["shadowFast"]:
        assert info["nQueueB"] == int((crosses & queued).sum()), (info, int((crosses & queued).sum()))
    else:
        assert info["nQueueB"] == 0
    if stats:
        assert info["rays"] == int(queued.sum()) + int(walks[queued].sum()), (info, int(queued.sum()), int(walks[queued].sum()))
