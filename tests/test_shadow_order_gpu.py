"""-m gpu: the any-hit shadow kernel (kz_wf_trace<4>) descends first into the child whose box holds the longest part of the segment (kz_devfn.h node4KeysOf<true>).
Which occluder an any-hit ray meets first does not change its answer, so nothing a render computes may move. Here: the shadow launches of a render on
4 096 rays per scene through Scene.trace_rays_wf (kz_trace_rays_wf, kernel 3), every answer against brute force over all triangles - the occlusion loop of
the integrator composed from brute-force closest hits (trace_ray_sets.shadow_reference) - with no tolerance; the same with the order switched off
(kz_debug_shadow_order, development library); and one film of the C1 job both ways.

Scenes: a 2 000-triangle soup in the closed room with its eight invisible lights, one triangle (the root IS a leaf), no triangle at all, and three leaves under a
root packet with empty slots (two triangles and an invisible light that hangs inside their box).

Rays (those a scene can have; shuffled, so that every wave mixes the kinds):
  tied      origins inside two child boxes of one packet at once: both children are entered at tmin, only the overlap tells them apart
  pairs     segments between random points of the room, tmax = distance - eps: most end inside a box of the tree
  lights    from surface points to points on the lights, as the integrator forms them
  through   across an invisible light: the any-hit kernel must hand them to the general kernel (info.nQueueB counts them)
  pinched   tmax == tmin at a brute-force hit distance (a closed interval: the hit stays) and away from one, and tmax < tmin
  zeros     direction components that are +-0, +-1e-45, +-1e-40 (denormal), +-1.2e-38 or next to the kernels' 1e-20 stand-in
  dead      NaN / infinite / zero-direction rays: nothing on them, they add their radiance
  long      long free segments: through the empty half of the room, or to infinity where there is no room"""
import os

import numpy as np
import pytest

import trace_ray_sets as R

pytestmark = pytest.mark.gpu
NRAYS = 4096
EPS = R.EPS
Q1 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q1_default_m0_r0.5.npz")
SHAPES = ("soup", "one_triangle", "empty", "small_root")
ROOM_OF = {"soup": "soup", "one_triangle": "cornell", "empty": "cornell", "small_root": "cornell"}


def scene(S, name):
    if name == "soup":
        return S.random_triangles(2000, 32, 32, 1, sampler="independent", s_edge=0.08)
    s = S.SceneDescription()
    N = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
    F = np.array([[0, 1, 2]], np.uint32)
    if name == "one_triangle":
        s.add_mesh(np.array([[-0.6, -0.5, 0.1], [0.7, -0.4, -0.2], [0.0, 0.8, 0.3]], np.float32), F, N)
    if name == "small_root":
        s.add_mesh(np.array([[-0.7, -0.6, -0.3], [0.1, -0.5, 0.3], [-0.3, 0.5, 0.0]], np.float32), F, N)          # boxes that share the slab -0.1 <= x <= 0.1
        s.add_mesh(np.array([[-0.1, -0.6, 0.3], [0.7, -0.4, -0.3], [0.3, 0.5, 0.1]], np.float32), F, N)
        P, Nn, UV, Fq = S.merge([S.quad((-0.4, 0.2, -0.4), (-0.4, 0.2, 0.4), (0.4, 0.2, 0.4), (0.4, 0.2, -0.4), flip=True)])
        s.add_mesh(P, Fq, Nn, UV, bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 1, 1), 10.0, False))
    s.camera.update(width=32, height=32)
    return s


def child_boxes(nd):
    """[(slot, lo, hi)] of the non-empty slots of a BVH4 packet (float64)."""
    scale = np.array([nd["scaleX"], nd["scaleY"], nd["scaleZ"]], np.float64)
    out = []
    for k in range(4):
        lo = np.array([int(nd["qlo"][a]) >> (8 * k) & 255 for a in range(3)], np.float64)
        hi = np.array([int(nd["qhi"][a]) >> (8 * k) & 255 for a in range(3)], np.float64)
        if (hi >= lo).all():
            out.append((k, nd["p"].astype(np.float64) + lo * scale, nd["p"].astype(np.float64) + hi * scale))
    return out


def tied_origins(nodes4, room, n, rng):
    """n points that lie inside two child boxes of one packet (and inside the room), or None if no two children of a packet overlap."""
    lo_r, hi_r = (np.array(x, np.float64) for x in R.ROOM[room])
    regions = []
    for nd in nodes4:
        b = child_boxes(nd)
        for i in range(len(b)):
            for j in range(i + 1, len(b)):
                lo, hi = np.maximum(np.maximum(b[i][1], b[j][1]), lo_r), np.minimum(np.minimum(b[i][2], b[j][2]), hi_r)
                if (hi - lo > 1e-4).all():
                    regions.append((lo, hi))
    if not regions:
        return None
    pick = rng.integers(0, len(regions), n)
    return np.array([regions[k][0] + rng.uniform(0.05, 0.95, 3) * (regions[k][1] - regions[k][0]) for k in pick]).astype(np.float32)


def tiny_directions(n, rng):
    d = R._unit(rng.normal(size=(n, 3)))
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.2e-38, -1.2e-38, 1e-20, -1e-20, 9e-21, 2e-20], np.float32)
    k = np.arange(n)
    d[k, k % 3] = vals[k // 3 % len(vals)]
    two = k % 5 == 0                                                   # a second small component beside it
    d[two, (k[two] + 1) % 3] = vals[(k[two] // 5 + 3) % len(vals)]
    return d


def ray_sets(S, name, desc, nodes4, ora, seed=41):
    room = ROOM_OF[name]
    rng = np.random.default_rng(seed)
    sets = {}
    tied = tied_origins(nodes4, room, 768, rng)
    if tied is not None:
        sets["tied"] = R._segment(tied, R._inside(rng, room, len(tied), 0.97), EPS)
    sets["pairs"] = R.shadow_pairs(room, 1024, seed + 1)
    if name == "soup":
        sets["lights"] = R.shadow_to_lights(room, desc, ora, 384, seed + 2)
    if R.invisible_meshes(desc):
        sets["through"] = R.shadow_through_invisible(room, desc, 384, seed + 3)
    # pinched: rays that hit something, with tmin = tmax = t (192), tmin = tmax = 0.37 * t (32), tmax one ulp below tmin (32) and far below it (32)
    po, pd, ptmin, _ = R.set_random(room, 2048, seed + 4)
    if name != "soup":                                                 # aim at the few triangles there are
        T = R._triangles(desc) if desc.meshes else np.zeros((0, 3, 3), np.float32)
        if len(T):
            pd = R._unit(T[rng.integers(0, len(T), len(po))].mean(axis=1).astype(np.float64) + rng.normal(size=(len(po), 3)) * 0.1 - po)
    t = ora.trace_rays(po, pd, ptmin, np.inf)["t"]
    hit = np.flatnonzero(np.isfinite(t))[:288]
    if len(hit) == 288:
        a, b, c, e = hit[:192], hit[192:224], hit[224:256], hit[256:288]
        tm = np.concatenate([t[a], np.float32(0.37) * t[b], t[c], t[e]]).astype(np.float32)
        tx = np.concatenate([t[a], np.float32(0.37) * t[b], np.nextafter(t[c], np.float32(-np.inf)), np.float32(0.25) * t[e]]).astype(np.float32)
        sets["pinched"] = (po[hit], pd[hit], tm, tx)
    else:                                                              # nothing to hit: any distance serves
        k = np.arange(288)
        tm = rng.uniform(0.1, 2.0, 288).astype(np.float32)
        sets["pinched"] = (po[:288], pd[:288], tm, np.where(k % 2 == 0, tm, np.nextafter(tm, np.float32(-np.inf))).astype(np.float32))
    zd = tiny_directions(384, rng)
    sets["zeros"] = (R._inside(rng, room, 384), zd, np.full(384, EPS, np.float32), rng.uniform(0.05, 3.0, 384).astype(np.float32))
    do, dd = R.dead_rows()
    k = np.arange(96)
    sets["dead"] = (do[k % len(do)], dd[k % len(dd)], np.full(96, EPS, np.float32), np.where(k % 2 == 0, np.float32(np.inf), np.float32(1.5)).astype(np.float32))
    if name == "soup":                                                 # the half of the room the soup leaves empty, below the lights
        a = np.stack([rng.uniform(-1.1, 1.1, 256), rng.uniform(-1.1, 1.0, 256), rng.uniform(1.15, 3.5, 256)], 1)
        b = np.stack([rng.uniform(-1.1, 1.1, 256), rng.uniform(-1.1, 1.0, 256), rng.uniform(1.15, 3.5, 256)], 1)
        sets["long"] = R._segment(a, b, EPS)
    else:                                                              # no room: free rays run to infinity
        o, d, tmin, _ = R.set_outside(room, 512, seed + 5)              # (its even rows point away from the room)
        sets["long"] = (o[::2], d[::2], tmin[::2], np.full(256, np.inf, np.float32))
    have = sum(len(s[0]) for s in sets.values())
    assert have <= NRAYS, have
    sets["fill"] = R.shadow_pairs(room, NRAYS - have, seed + 6)
    return sets


_cases = {}


def case(kz, O, dev_lib, name):
    """A scene on the development library, its 4 096 shuffled rays with the span each kind came from, and the brute-force reference - made once per process."""
    if name not in _cases:
        desc = scene(kz.scenes, name)
        sc = kz.Scene(desc, device=0, lib=dev_lib)
        ora = O.OracleScene(desc, brute=True)
        inv = R.invisible_meshes(desc)
        ora_il = O.OracleScene(R.only_meshes(kz.scenes, desc, inv), brute=True) if inv else None
        nodes4 = sc.table(1).view(R.NODE4)
        sets = ray_sets(kz.scenes, name, desc, nodes4, ora)
        rays, spans = R.concat(sets)
        kind = np.zeros(NRAYS, np.int64)
        for i, k in enumerate(spans):
            kind[spans[k][0]:spans[k][1]] = i
        perm = np.random.default_rng(43).permutation(NRAYS)
        rays = tuple(np.ascontiguousarray(x[perm]) for x in rays)
        _cases[name] = {"desc": desc, "scene": sc, "rays": rays, "kinds": list(spans), "kind": kind[perm], "nodes4": nodes4,
                        "ref": R.shadow_reference(ora, ora_il, desc, *rays)}
    return _cases[name]


def sums_before(n):
    return ((np.arange(3 * n, dtype=np.float32) + 1) * np.float32(0.03125)).reshape(n, 3)


def pending_of(n):
    return ((np.arange(3 * n, dtype=np.float32) + 1) * np.float32(0.001)).reshape(n, 3)


def sentinel_hits(n):
    h = np.zeros((n, 4), np.float32)
    h[:, 0] = np.float32(1 << 20) + np.arange(n, dtype=np.float32)
    h[:, 1], h[:, 2] = 0.125, 0.375
    h[:, 3] = (np.uint32(0xF0000000) | np.arange(n, dtype=np.uint32)).view(np.float32)
    return h


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(c, scene=None, **opts):
    o, d, tmin, tmax = c["rays"]
    n = len(o)
    return (scene or c["scene"]).trace_rays_wf(o, d, tmin, tmax, kernel=3, hits=sentinel_hits(n), sums=sums_before(n), pending=pending_of(n), **opts)


def check(c, res, what):
    """Every slot's sums against the reference: + pending exactly where the segment is free, untouched where it is occluded; no hit record written; the rays handed
    to the general kernel are those that cross an invisible-light triangle."""
    occluded, walks, crosses = c["ref"]
    n = len(occluded)
    want = np.where(~occluded[:, None], sums_before(n) + pending_of(n), sums_before(n)).astype(np.float32)
    bad = np.flatnonzero((u32(res["sums"]) != u32(want)).any(axis=1))
    o, d, tmin, tmax = c["rays"]
    msg = "\n".join("  ray %d (%s) o=%r d=%r tmin=%r tmax=%r: brute force says occluded=%s (walk-throughs %d, crosses an invisible light %s), the kernel %s" %
                    (i, c["kinds"][c["kind"][i]], o[i].tolist(), d[i].tolist(), float(tmin[i]), float(tmax[i]), occluded[i], walks[i], crosses[i],
                     "added nothing" if np.array_equal(u32(res["sums"][i]), u32(sums_before(n)[i])) else "added %r" % (res["sums"][i] - sums_before(n)[i]).tolist()) for i in bad[:8])
    assert len(bad) == 0, "%s: %d of %d answers differ from brute force; the first:\n%s" % (what, len(bad), n, msg)
    sent = sentinel_hits(n)
    assert all(np.array_equal(u32(res[k]), u32(sent[:, j])) for j, k in enumerate(("t", "u", "v"))) and np.array_equal(res["gid"], u32(sent[:, 3])), what + ": a shadow launch wrote hit records"
    assert res["info"]["shadowFast"] == 1, res["info"]
    assert res["info"]["nQueueB"] == int(crosses.sum()), (what, res["info"], int(crosses.sum()))


@pytest.fixture
def order(dev_lib):
    """order(False): the any-hit launches in closest-hit order (kz_wf_trace<5>); order(True): largest overlap first, the default."""
    yield lambda on: dev_lib.kz_debug_shadow_order(int(on))
    dev_lib.kz_debug_shadow_order(1)


def test_the_ray_sets_hold_what_they_claim(gpu_lib, dev_lib, kz, O):
    """On the reference alone: 4 096 rays per scene; occluded and free rays both occur where there is something to hit; the scenes with an invisible light have rays
    across it; tied origins lie in two child boxes; the small tree is one packet with an empty slot, the one-triangle and the empty scene have no packet."""
    for name in SHAPES:
        c = case(kz, O, dev_lib, name)
        o, d, tmin, tmax = c["rays"]
        occluded, walks, crosses = c["ref"]
        kind = lambda k: c["kind"] == c["kinds"].index(k)
        assert len(o) == NRAYS
        assert (~occluded[kind("dead")]).all() and (~occluded[kind("long")]).all()
        assert (tmax[kind("pinched")] <= tmin[kind("pinched")]).all() and (tmax[kind("pinched")] < tmin[kind("pinched")]).any()
        zd = d[kind("zeros")]
        assert (zd == 0).any() and ((zd != 0) & (np.abs(zd) < 1.17e-38)).any()
        if name == "empty":
            assert not occluded.any() and len(c["nodes4"]) == 0
            continue
        assert occluded.any() and (~occluded).any()
        assert occluded[kind("pinched")].any() and (~occluded[kind("pinched")]).any()          # the closed interval keeps its hit; an empty one has none
        if name == "one_triangle":
            assert len(c["nodes4"]) == 0
            continue
        assert crosses.sum() >= 64 and walks.sum() >= 64
        assert "tied" in c["kinds"] and kind("tied").sum() == 768
        if name == "small_root":
            assert len(c["nodes4"]) == 1 and 2 <= len(child_boxes(c["nodes4"][0])) < 4
        if name == "soup":
            assert len(c["nodes4"]) > 100
            assert (tmax[kind("long")] > 1.0).sum() >= 64


@pytest.mark.parametrize("name", SHAPES)
def test_every_answer_equals_brute_force(gpu_lib, dev_lib, kz, O, order, name):
    """The shadow launches with the overlap order (the default), the counting instantiation, a one-workgroup launch whose lanes take ray after ray on stacks that
    occluded rays abandon, a two-entry LDS stack - and the closest-hit order: every boolean is brute force's in each, and the orders visit different nodes on the soup."""
    c = case(kz, O, dev_lib, name)
    order(True)
    check(c, launch(c), name + ", overlap order")
    on = launch(c, stats=True)
    check(c, on, name + ", overlap order, counted")
    check(c, launch(c, grid_blocks=1, batch=64), name + ", overlap order, one workgroup")
    check(c, launch(c, lds_stack=2, refill=64, postpone=1), name + ", overlap order, two LDS entries")
    order(False)
    check(c, launch(c), name + ", closest-hit order")
    off = launch(c, stats=True)
    check(c, off, name + ", closest-hit order, counted")
    order(True)
    print("%s: node visits / triangle tests of the %d rays: %d / %d overlap order, %d / %d closest-hit order" %
          (name, NRAYS, on["info"]["nodeVisits"], on["info"]["triTests"], off["info"]["nodeVisits"], off["info"]["triTests"]))
    assert on["info"]["rays"] == off["info"]["rays"]
    if name == "soup":          # the switch switches: tied entries are everywhere in a soup, and the two rules break them differently
        assert on["info"]["nodeVisits"] != off["info"]["nodeVisits"]


def test_product_library_gives_the_same_answers(gpu_lib, dev_lib, kz, O):
    c = case(kz, O, dev_lib, "soup")
    sc = kz.Scene(c["desc"], device=0)
    check(c, launch(c, scene=sc), "soup, product library")
    sc.close()


def test_c1_film_is_the_same_bits_with_the_order_off(gpu_lib, dev_lib, kz, order):
    """The C1 job (the q1 asset, 256 x 256 x 16) in one process: the film with the overlap order equals the film with the closest-hit order, and the product library's."""
    d = kz.scenes.load_npz(Q1, {"camera": {"width": 256, "height": 256}, "sampler": {"sampleCount": 16}})
    sc = kz.Scene(d, device=0, lib=dev_lib)
    order(True)
    sc.render()
    on = sc.film()
    order(False)
    sc.render()
    off = sc.film()
    order(True)
    sc.close()
    assert np.abs(on[..., :3]).max() > 0
    assert np.array_equal(on, off)
    p = kz.Scene(d, device=0)
    p.render()
    assert np.array_equal(p.film(), on)
    p.close()
