"""-m gpu: the traversal kernels a render launches - kz_wf_trace<0|1|2|4> and kz_wf_trace_packet, in the instantiations and launch shapes of a pass - ray by ray
against brute force, through Scene.trace_rays_wf (kz_trace_rays_wf). The rays are those of tests/trace_ray_sets.py, which tests/test_trace_wf_cpu.py holds to
what they claim; the reference of a scene is computed once and shared by the cases.

Closest-hit kinds: (mesh, prim) of every ray equal the oracle's, t / u / v of a hit have the oracle's BITS (the triangle test is Mesh::rayIntersect operation
for operation on both sides), a miss is (+inf, 0, 0). Shadow kind: a free ray adds its pending radiance to its slot's sums once, an occluded one nothing - exact
float equality. Every kind leaves the slots outside its queue alone, and every launch shape gives the bits of the default one.

A mismatch prints the first offending rays with their inputs and both answers."""
import ctypes as C

import numpy as np
import pytest

import trace_ray_sets as R
from checks import same_bits
from trace_ray_sets import KINDS, PACKET_SHAPES, SHAPES, check_closest, check_shadow, pending_of, report, run, same_result, sums_before, u32

pytestmark = pytest.mark.gpu
# ------------------------------------------------------------------------------------------------ closest-hit kinds
@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("name", R.CLOSEST_SCENES)
def test_closest_hit_kernels_equal_brute_force_ray_by_ray(gpu_lib, kz, O, name, kernel):
    """Sets (a) - (g) of a scene in one launch of the default shape, identity queue. The coincident scene returns the lowest id (what brute force reports). On the
    cornell box the packet kernel also queues its first hits on the invisible light for the walk-through: as many as the oracle finds."""
    case = R.closest_case(kz, O, name, device=0)
    res = run(case, kernel)
    check_closest(case, kernel, res)
    if name == "coincident":
        assert (res["mesh"][case["ref"]["mesh"] >= 0] == 0).all()
    if kernel == 1:
        inv = R.invisible_meshes(case["desc"])
        assert res["info"]["nFirstHitsOnInvisibleLight"] == int(np.isin(case["ref"]["mesh"], inv).sum())


@pytest.mark.parametrize("name", R.CLOSEST_SCENES)
def test_bvh2_and_both_bvh4_kernels_agree(gpu_lib, kz, O, name):
    """kz_trace_rays (the reference-shaped BVH2 walk) on the same rays: the same triangle and the same bits of t, u, v as the per-lane and the packet kernel."""
    case = R.closest_case(kz, O, name, device=0)
    b2 = case["scene"].trace_rays(*case["rays"])
    for kernel in (0, 1):
        res = run(case, kernel)
        hit = b2["mesh"] >= 0
        wrong = (res["mesh"] != b2["mesh"]) | (res["prim"] != b2["prim"])
        for k in ("t", "u", "v"):
            wrong |= hit & (u32(res[k]) != u32(b2[k]))
        bad = np.flatnonzero(wrong)
        assert len(bad) == 0, report(case, bad, res, b2, "%s kernel against the BVH2 kernel" % KINDS[kernel])


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_queues_of_every_length_write_their_slots_and_no_other(gpu_lib, kz, O, name, kernel):
    """Queues with indirection: a seeded permutation of all slots, and its first 1, 63, 64, 65 and 4113 entries (a lane, a wave less one, a wave, a wave and a lane, a
    partial last packet behind 64 full ones) - strict subsets. The queued slots hold the oracle's answer, the others their sentinel hit and their sums bit for bit."""
    case = R.closest_case(kz, O, name, device=0)
    n = len(case["rays"][0])
    perm = np.random.default_rng(17).permutation(n).astype(np.uint32)
    for nq in (1, 63, 64, 65, 4113, n):
        q = perm[:nq]
        check_closest(case, kernel, run(case, kernel, queue=q), queue=q)


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_launch_shapes_give_the_bits_of_the_default_launch(gpu_lib, kz, O, name, kernel):
    """4113 queued rays. Per-lane kernels: one workgroup with batches of 64 (4 waves x 64 static entries, then dynamic reservations, the guided reservation size and the
    clipped last one), an LDS stack of 2 entries (everything deeper in the global overflow area), refill and postpone thresholds of 1 and 64, the counting
    instantiations - alone and with all of the former. Packet kernel: one workgroup claiming one packet at a time (dynamic batches, the partial last packet), and
    the counting instantiation. Every result equals the default launch's bit for bit (which the cases above hold to the oracle); a counting launch reports one ray
    per queue entry."""
    case = R.closest_case(kz, O, name, device=0)
    n = len(case["rays"][0])
    q = np.random.default_rng(23).permutation(n).astype(np.uint32)[:4113]
    base = run(case, kernel, queue=q)
    check_closest(case, kernel, base, queue=q)
    counted = []
    for shape in (PACKET_SHAPES if kernel == 1 else SHAPES):
        res = run(case, kernel, queue=q, **shape)
        assert same_result(res, base), (name, KINDS[kernel], shape, report(case, np.flatnonzero(u32(res["t"]) != u32(base["t"])), res, base, "launch shape"))
        if shape.get("stats"):
            assert res["info"]["rays"] == len(q), (shape, res["info"])
            counted.append((shape, res["info"]["nodeVisits"], res["info"]["triTests"]))
        if "grid_blocks" in shape:
            assert res["info"]["gridBlocks"] == shape["grid_blocks"]
    # The walk of a ray - the nodes it visits, the triangles it tests - is a function of the ray alone (of its packet's 64 rays, in the packet kernel): the same
    # counts whether a lane traces one ray, as in the default launch (more lanes than rays), or one after another on a stack it must find empty (one workgroup)
    assert len({c[1:] for c in counted}) == 1 and counted[0][1] > 0 and counted[0][2] > 0, counted


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_exactly_zero_direction_components_do_not_switch_a_slab_off(gpu_lib, kz, O, name, kernel):
    """The box test's FMA form q * (s / d) + (p - o) / d is inf - inf = NaN for d = 0, which fminf / fmaxf drop: the axis would stop constraining, the hits would
    stay right (test_closest_hit_kernels_equal_brute_force_ray_by_ray passes either way) and the ray would walk a slab of the tree. The kernels stand 1e-20 in
    for such a component. Measured here by the counting instantiations: the rays of set (b) with one or two exactly-zero components visit no more nodes than the
    same rays with those zeros replaced by +-1e-19 - a value the kernels take as it is. Bound: for an origin off a box's planes, (plane - o) / 1e-19 and
    (plane - o) * 1e20 both lie beyond +-1e11 with the same sign, far outside any [tmin, tmax] of these rays, so every box is classified alike and the child
    keys, max(tnear, tmin), are the same numbers: the walks are the same. 1 % is left for triangle tests that the 1e-19 decides differently on an edge
    (a closer or farther tmax). Without the stand-in one or two of three slabs are off: several times the visits."""
    case = R.closest_case(kz, O, name, device=0)
    i, j = case["spans"]["b"]
    zeros = case["extra"]["b"]
    pick = np.flatnonzero((zeros == 1) | (zeros == 2)) + i
    o, d, tmin, tmax = (x[pick].copy() for x in case["rays"])
    tilted = np.where(d == 0, np.copysign(np.float32(1e-19), d), d).astype(np.float32)
    sc = case["scene"]
    a = sc.trace_rays_wf(o, d, tmin, tmax, kernel=kernel, stats=True)
    b = sc.trace_rays_wf(o, tilted, tmin, tmax, kernel=kernel, stats=True)
    print("%s %s: %d rays, node visits %d with exact zeros, %d with 1e-19" % (name, KINDS[kernel], len(o), a["info"]["nodeVisits"], b["info"]["nodeVisits"]))
    assert 0 < a["info"]["nodeVisits"] <= 1.01 * b["info"]["nodeVisits"], (a["info"], b["info"])


def test_a_two_entry_lds_stack_spills_into_the_overflow_area_and_stays_inside_it(gpu_lib, kz, O):
    """On the soup an LDS stack of 2 entries sends the deeper entries of most rays to the global overflow area: rows of it are written, none beyond the rows the launch
    owns (the entry keeps a guard row behind them and fails the call if a stack reaches it), and the launch owns at least the builder's bound less the LDS entries."""
    case = R.closest_case(kz, O, "soup", device=0)
    for kernel in (0, 2):
        info = run(case, kernel, lds_stack=2)["info"]
        assert info["ldsStack"] == 2 and info["stackBound"] > 4, info
        assert 1 <= info["ovfRowsTouched"] <= info["ovfRows"], info
        assert info["ovfRows"] >= info["stackBound"] - info["ldsStack"], info
        dflt = run(case, kernel)["info"]
        assert dflt["ldsStack"] == min(16, max(2, dflt["stackBound"])) and dflt["ovfRows"] >= max(1, dflt["stackBound"] - dflt["ldsStack"]), dflt


# ------------------------------------------------------------------------------------------------ the shadow kind
@pytest.mark.parametrize("name", R.SHADOW_SCENES)
def test_shadow_kernels_add_each_pending_radiance_once_to_its_own_slot(gpu_lib, kz, O, name):
    """The shadow launches of a bounce on segments between random points, from surfaces to the lights and through the invisible lights, against the occlusion loop of
    integrator.cpp:257-278 composed from brute-force closest hits: sums_after == sums_before + pending exactly for the free segments, == sums_before for the
    occluded ones, every slot with its own distinct values. Identity queue, a permutation, strict subsets of 1 .. 65 entries. On the scenes with the any-hit kernel
    (shadowFast: cornell_il with 2 invisible-light triangles, soup with 16) the rays diverted to the second queue are those whose segment crosses an
    invisible-light triangle; the panel scene (72 such triangles) sends everything through the general kernel."""
    case = R.shadow_case(kz, O, name, device=0)
    n = len(case["rays"][0])
    assert run(case, 3)["info"]["shadowFast"] == (0 if name == "panel" else 1)
    check_shadow(case, run(case, 3))
    perm = np.random.default_rng(29).permutation(n).astype(np.uint32)
    for nq in (n, 1, 63, 64, 65, n // 2 + 1):
        check_shadow(case, run(case, 3, queue=perm[:nq]), queue=perm[:nq])


@pytest.mark.parametrize("name", R.SHADOW_SCENES)
def test_shadow_launch_shapes_give_the_bits_of_the_default_launch(gpu_lib, kz, O, name):
    """The shapes of the closest-hit case for the shadow launches (one workgroup with batches of 64 reaches the dynamic reservations on these ~3000 segments). The counting
    instantiations report one ray per queue entry and one per walk-through of the reference loop, and the same node visits and triangle tests in every shape."""
    case = R.shadow_case(kz, O, name, device=0)
    n = len(case["rays"][0])
    q = np.random.default_rng(31).permutation(n).astype(np.uint32)[:n - 7]
    base = run(case, 3, queue=q)
    check_shadow(case, base, queue=q)
    counted = []
    for shape in SHAPES:
        res = run(case, 3, queue=q, **shape)
        assert same_result(res, base) and res["info"]["nQueueB"] == base["info"]["nQueueB"], (name, shape)
        check_shadow(case, res, queue=q, stats=bool(shape.get("stats")))
        if shape.get("stats"):
            counted.append((shape, res["info"]["nodeVisits"], res["info"]["triTests"]))
    # (an occluded shadow ray abandons its stack where it stands: the lane's next ray must not walk what is left on it - in a launch of one workgroup every
    # lane takes a dozen rays, in the default launch one)
    assert len({c[1:] for c in counted}) == 1 and counted[0][1] > 0 and counted[0][2] > 0, counted


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_anything_is_launched(gpu_lib, kz, O):
    """A null buffer, a queue index beyond the slots, a repeated one, a negative (-0.0 included) or NaN tmin, an unknown kernel: KZ_ERR_INVALID_ARG, and the caller's hit records and
    sums are as they were. An empty queue is KZ_OK without a launch. (The packet kernel on a tree that may need more than 128 stack entries is refused too; the
    builder caps the tree depth at 32, so no scene reaches that bound.)"""
    case = R.closest_case(kz, O, "cornell", device=0)
    sc, a = case["scene"], kz.abi
    o, d, tmin, tmax = (x[:200].copy() for x in case["rays"])
    n = len(o)
    Hit = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("gid", "<u4"), ("mesh", "<i4"), ("prim", "<i4")])

    def call(kernel=0, o=o, d=d, tmin=tmin, tmax=tmax, queue=None, nq=0, pending=True, hits=True, sums=True, opts=True):
        h = np.zeros(n, Hit)
        h["t"], h["gid"], h["mesh"] = 7.0, 99, 5
        s = sums_before(n)
        p = pending_of(n)
        fp = lambda x: None if x is None else np.ascontiguousarray(x, np.float32).ctypes.data_as(a.f32p)
        op = a.KzTraceWfOpts(kernel, 0, 0, 0, 0, 0, 0, 0)
        qq = None if queue is None else np.ascontiguousarray(queue, np.uint32)
        rc = sc.lib.kz_trace_rays_wf(sc.h, C.byref(op) if opts else None, n, fp(o), fp(d), fp(tmin), fp(tmax), None if qq is None else qq.ctypes.data_as(a.u32p), nq,
                                     fp(p) if pending else None, h.ctypes.data_as(C.POINTER(a.KzTraceWfHit)) if hits else None, fp(s) if sums else None, None)
        untouched = (h["t"] == 7.0).all() and (h["gid"] == 99).all() and (h["mesh"] == 5).all() and same_bits(s, sums_before(n))
        return rc, untouched

    assert call() == (a.KZ_OK, False)                                           # the call as such is fine
    bad_tmin, nan_tmin = tmin.copy(), tmin.copy()
    bad_tmin[150], nan_tmin[3] = -1e-3, np.nan
    negzero = tmin.copy()
    negzero[10] = -0.0                                                           # its sign bit would order a child key behind every positive tmax: negative
    for kw in (dict(o=None), dict(d=None), dict(tmin=None), dict(tmax=None), dict(hits=False), dict(sums=False), dict(opts=False), dict(kernel=3, pending=False),
               dict(queue=[0, 1, n], nq=3), dict(queue=[0, 0xFFFFFFFF], nq=2), dict(queue=[4, 9, 4], nq=3), dict(queue=np.arange(n + 1) % n, nq=n + 1),
               dict(tmin=bad_tmin), dict(tmin=nan_tmin), dict(tmin=negzero), dict(kernel=4), dict(kernel=-1)):
        assert call(**kw) == (a.KZ_ERR_INVALID_ARG, True), kw
    assert call(queue=[0], nq=0) == (a.KZ_OK, True)                              # an empty queue: nothing to do
