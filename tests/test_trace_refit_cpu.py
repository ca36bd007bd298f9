"""The deformed cases of tests/trace_ray_sets.py (closest_case / shadow_case with deform=...) on the host tables and the brute-force oracle alone (no GPU): each
deformation does what it claims to a tree that keeps the build's topology. tests/test_trace_refit_gpu.py runs the traversal kernels on the same cases.

These tests run before the GPU tests and establish the stack bound first: the bound recomputed from the refit KZ_TABLE_NODES4 equals KzParams.stackBound4 and
the fresh tree's, so the overflow area a launch sizes from it covers the deformed tree before any kernel walks it.

A walk model (numpy, all rays stepped together) gives the stack depth the per-lane closest-hit kernels reach on a tree: the nearest hit child first, the other hit
children pushed in slot order, leaves taken as misses so that tmax never shrinks - an upper bound of what a ray with hits does."""
import os
import subprocess

import numpy as np
import pytest

import trace_ray_sets as R
from scene_tables import check_refit
from trace_ray_sets import LDS_ENTRIES, flattened_ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_STACKBOUND4, P_SHADOWFAST = 292, 296        # offsets into KzParams (nano-kazen_amd/csrc/kz_internal.h), pinned by test_stack_bound_offset
CASES = sorted(set(R.REFIT_CLOSEST) | set(R.REFIT_SHADOW))


def fresh_case(kz, O, name):
    return R.shadow_case(kz, O, name) if name == "cornell_il" else R.closest_case(kz, O, name)


def deformed_case(kz, O, name, deform):
    return R.shadow_case(kz, O, name, deform=deform) if name == "cornell_il" else R.closest_case(kz, O, name, deform=deform)


def stack_bound(nodes4):
    """kz_collapse_bvh4's bound from the table alone: need[h] = (children - 1) + max(need[inner child]) over the non-empty slots, bound = need[0] + 1."""
    need = np.zeros(len(nodes4), np.int64)
    for h in range(len(nodes4) - 1, -1, -1):
        nd = nodes4[h]
        kids = [int(nd["child"][k]) for k in range(4) if (int(nd["qlo"][0]) >> (8 * k) & 255) <= (int(nd["qhi"][0]) >> (8 * k) & 255)]
        inner = [c for c in kids if not c & 0x80000000]
        assert all(c > h for c in inner)
        need[h] = len(kids) - 1 + max([need[c] for c in inner] or [0])
    return int(need[0]) + 1 if len(nodes4) else 1


def param_word(sc, kz, offset):
    return int(sc.table(kz.abi.KZ_TABLE_PARAMS)[offset:offset + 4].view(np.int32)[0])


def walk_model(nodes4, o, d, tmin, cap):
    """The closest-hit walk of kz_wf_trace on the dequantised packets, every ray stepped at once: per visit the four child keys (bits of max(tnear, tmin), the slot in
    the two low bits; a miss where tnear > tfar * 1.0000004), the smallest taken, the other hit children pushed in slot order; a leaf is a miss and pops.
    Returns (deepest stack, node visits) per ray. cap: entries the model's stack holds (the tree's bound)."""
    p = np.ascontiguousarray(nodes4["p"], np.float32)
    s = np.stack([nodes4["scaleX"], nodes4["scaleY"], nodes4["scaleZ"]], 1).astype(np.float32)
    sh = (8 * np.arange(4)).astype(np.uint32)
    qlo = ((nodes4["qlo"][:, :, None] >> sh) & 255).astype(np.float32)                       # (packets, axis, slot)
    qhi = ((nodes4["qhi"][:, :, None] >> sh) & 255).astype(np.float32)
    child = nodes4["child"].astype(np.int64)
    n = len(o)
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        r = (np.float32(1) / np.where(np.abs(d) < 1e-20, np.copysign(np.float32(1e-20), d), d)).astype(np.float32)
    tmin = np.asarray(tmin, np.float32)
    MISS = np.int64(0xFFFFFFFF)
    cur, top, active = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, bool)
    stack = np.zeros((n, cap + 4), np.int64)
    deepest, visits = np.zeros(n, np.int64), np.zeros(n, np.int64)
    while active.any():
        idx = np.flatnonzero(active)
        leaf = (cur[idx] & 0x80000000) != 0
        ii, h = idx[~leaf], cur[idx][~leaf]
        pop = idx[leaf]
        if len(ii):
            visits[ii] += 1
            with np.errstate(all="ignore"):
                a, b = (s[h] * r[ii])[:, :, None], ((p[h] - o[ii]) * r[ii])[:, :, None]
                tlo, thi = qlo[h] * a + b, qhi[h] * a + b
                pos = (r[ii] >= 0)[:, :, None]
                near = np.fmax(np.where(pos, tlo, thi).max(axis=1), tmin[ii][:, None]).astype(np.float32)
                far = (np.where(pos, thi, tlo).min(axis=1) * np.float32(1.0000004)).astype(np.float32)
            key = np.where(near <= far, (near.view(np.uint32).astype(np.int64) & ~np.int64(3)) | np.arange(4), MISS)
            kmin = key.min(axis=1)
            for k in range(4):
                push = (key[:, k] != MISS) & (key[:, k] != kmin)
                stack[ii[push], top[ii[push]]] = child[h[push], k]
                top[ii[push]] += 1
            deepest[ii] = np.maximum(deepest[ii], top[ii])
            hit = kmin != MISS
            cur[ii[hit]] = child[h[hit], kmin[hit] & 3]
            pop = np.concatenate([pop, ii[~hit]])
        done = pop[top[pop] == 0]
        active[done] = False
        go = pop[top[pop] > 0]
        top[go] -= 1
        cur[go] = stack[go, top[go]]
    return deepest, visits


def same_hits(a, b):
    s = (a["mesh"] == b["mesh"]) & (a["prim"] == b["prim"])
    for k in ("t", "u", "v"):
        s &= a[k].view(np.uint32) == b[k].view(np.uint32)
    return s


def test_stack_bound_offset(kz, tmp_path):
    src = tmp_path / "off.cpp"
    src.write_text('#include "kz_internal.h"\n#include <cstddef>\n#include <cstdio>\nint main(){printf("%zu %zu\\n", offsetof(KzParams, stackBound4), '
                   'offsetof(KzParams, shadowFast));}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "nano-kazen_amd", "csrc"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [P_STACKBOUND4, P_SHADOWFAST]


def test_soup_layout_is_what_the_deformations_assume(kz):
    """Meshes 0 - 7: 625 triangles each on unshared vertices (F is arange); mesh 8 the room; meshes 9 - 16 the eight light quads, invisible to camera rays."""
    d = R.scene(kz.scenes, "soup")
    assert len(d.meshes) == 17
    for m in R.SOUP_MESHES:
        x = d.meshes[m]
        assert x["F"].shape == (625, 3) and np.array_equal(x["F"].ravel(), np.arange(1875)) and x["V"].shape == (1875, 3) and x["N"] is not None and x["light"] is None
    assert d.meshes[8]["light"] is None and d.meshes[8]["F"].shape == (12, 3)
    assert tuple(R.invisible_meshes(d)) == R.SOUP_LIGHTS and all(d.meshes[m]["F"].shape == (2, 3) and d.meshes[m]["V"].shape == (4, 3) for m in R.SOUP_LIGHTS)
    c = R.scene(kz.scenes, "cornell")
    assert len(c.meshes) == 8 and (c.meshes[0]["V"][:, 1] == c.meshes[0]["V"][0, 1]).all() and c.meshes[5]["F"].shape == (12, 3) and c.meshes[6]["F"].shape == (12, 3)
    assert R.invisible_meshes(c) == [7] and R.invisible_meshes(R.scene(kz.scenes, "cornell_il")) == [7]


@pytest.mark.parametrize("name,deform", CASES)
def test_deformations_are_seeded_stay_in_the_room_and_name_each_mesh_once(kz, name, deform):
    assert deform in R.DEFORMS[name]
    d = R.scene(kz.scenes, name)
    a, b = R.deformation(name, d, deform), R.deformation(name, d, deform)
    lo, hi = (np.array(x, np.float32) for x in R.ROOM[name])
    assert sorted(a) == sorted(b) and len(a) >= 3
    for m in a:
        Va, Na = a[m] if isinstance(a[m], tuple) else (a[m], None)
        Vb = b[m][0] if isinstance(b[m], tuple) else b[m]
        assert np.array_equal(Va, Vb) and Va.shape == d.meshes[m]["V"].shape and Va.dtype == np.float32
        assert (Va >= lo).all() and (Va <= hi).all()
        assert (Na is None) == (d.meshes[m]["N"] is None) and (Na is None or Na is d.meshes[m]["N"])
    moved = [m for m in a if not np.array_equal(a[m][0] if isinstance(a[m], tuple) else a[m], d.meshes[m]["V"])]
    assert len(moved) == len(a)
    if deform == "stacked":
        assert all(np.array_equal(a[m][0], d.meshes[0]["V"]) for m in (1, 2, 3)) and 0 not in a
    if deform == "flattened":
        assert (a[5][0][:, 1] == d.meshes[0]["V"][0, 1]).all() and np.array_equal(a[5][0][:, [0, 2]], d.meshes[5]["V"][:, [0, 2]])
        assert (a[6][0] == a[6][0][0]).all() and (np.abs(a[6][0][0]) < 1).all()


@pytest.mark.parametrize("name,deform", CASES)
def test_refit_is_conservative_and_keeps_the_stack_bound(kz, O, name, deform):
    """check_refit of tests/scene_tables.py on the deformed host scene; the stack bound recomputed from the child words and empty-slot marks of
    KZ_TABLE_NODES4 equals KzParams.stackBound4, before and after the edit - the same number: the overflow area a launch owns covers the deformed tree."""
    fresh, case = fresh_case(kz, O, name), deformed_case(kz, O, name, deform)
    sc = case["scene"]
    check_refit(kz, sc)
    n4f, n4 = fresh["scene"].table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4), sc.table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4)
    assert np.array_equal(n4f["child"], n4["child"]) and not np.array_equal(n4f["qlo"], n4["qlo"])
    bound = stack_bound(n4)
    print("%s/%s: %d packets, stack bound %d (fresh %d), KzParams.stackBound4 %d" % (name, deform, len(n4), bound, stack_bound(n4f), param_word(sc, kz, P_STACKBOUND4)))
    assert bound == stack_bound(n4f) == param_word(sc, kz, P_STACKBOUND4) == param_word(fresh["scene"], kz, P_STACKBOUND4)
    assert bound <= 128                                             # the packet kernel's VGPR stack
    if name == "soup":
        assert bound == 28 and len(n4) == 2091
    assert param_word(sc, kz, P_SHADOWFAST) == 1


@pytest.mark.parametrize("deform", ["scatter", "slivers"])
def test_overlapping_boxes_drive_the_stack_past_the_lds_entries(kz, O, deform):
    """The walk model on the first 256 rays of set (a), fresh tree and deformed tree: the deepest stack on the deformed tree is greater than on the fresh one and
    greater than the 16 entries of the default LDS stack, and stays within the bound of 28. Measured: fresh 12 (16 node visits per ray); scatter 18 (507 per ray),
    slivers 21 (817 per ray) - both reach 17, so tests/test_trace_refit_gpu.py asserts a spill at the default launch shape too, not only at lds_stack=2."""
    fresh, case = R.closest_case(kz, O, "soup"), R.closest_case(kz, O, "soup", deform=deform)
    i, j = case["spans"]["a"]
    assert (i, j) == fresh["spans"]["a"] and all(np.array_equal(x[i:j], y[i:j]) for x, y in zip(case["rays"], fresh["rays"]))
    o, d, tmin = (x[i:i + 256] for x in case["rays"][:3])
    bound = param_word(case["scene"], kz, P_STACKBOUND4)
    out = {}
    for what, c in (("fresh", fresh), (deform, case)):
        deepest, visits = walk_model(c["scene"].table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4), o, d, tmin, bound)
        out[what] = (int(deepest.max()), int(visits.sum()))
        print("soup %s: deepest stack %d of a bound of %d, %d node visits of %d rays (%.1f per ray, at most %d)" %
              (what, deepest.max(), bound, visits.sum(), len(o), visits.mean(), visits.max()))
    assert out[deform][0] <= bound and out["fresh"][0] <= bound
    assert out[deform][0] > out["fresh"][0] and out[deform][0] > LDS_ENTRIES, out
    assert out[deform][1] > out["fresh"][1]


def slots_under(n4, tri_count, packet):
    """Per triangle of the leaf table: the child slot of `packet` it lies under (-1: not under that packet)."""
    slot = np.full(tri_count, -1, np.int64)
    for k in range(4):
        todo = [int(n4[packet]["child"][k])] if (int(n4[packet]["qlo"][0]) >> (8 * k) & 255) <= (int(n4[packet]["qhi"][0]) >> (8 * k) & 255) else []
        while todo:
            ref = todo.pop()
            if ref & 0x80000000:
                s = (ref & 0x7fffffff) >> 3
                slot[s:s + (ref & 7) + 1] = k
            else:
                nd = n4[ref]
                todo += [int(nd["child"][q]) for q in range(4) if (int(nd["qlo"][0]) >> (8 * q) & 255) <= (int(nd["qhi"][0]) >> (8 * q) & 255)]
    return slot


def test_stacked_copies_tie_four_ways_across_subtrees(kz, O):
    """soup/stacked, sets (a) and (h): the oracle reports mesh 0 for every ray that ends on the coincident copies, and each of the other copies alone answers those
    rays with the same bits of t - a four-way tie. At least a quarter of the rays that hit anything end there; set (a) alone does not get there - 66 of its
    2 048 rays, the room is large and the soup thin - which is why the deformed cases carry set (h).
    The copies lie in different subtrees. Not under different children of the ROOT: its four children are the soup as a whole, the walls and the lights (the
    builder splits those off first). The packet below it, the soup's top packet, spreads the copies: for at least half of the 625 triangles the four copies lie
    under two or more of its children (copies placed independently would do so for 1 - 4^-3 = 98 %)."""
    c = R.closest_case(kz, O, "soup", deform="stacked")
    pick = np.concatenate([np.arange(*c["spans"]["a"]), np.arange(*c["spans"]["h"])])
    rays = tuple(x[pick] for x in c["rays"])
    mesh, t = c["ref"]["mesh"][pick], c["ref"]["t"][pick]
    hit = mesh >= 0
    on = np.isin(mesh, R.STACKED)
    print("soup/stacked: %d rays of sets (a) and (h), %d hit, %d on the coincident copies (set (a) alone: %d of %d)" %
          (len(pick), hit.sum(), on.sum(), np.isin(c["ref"]["mesh"][slice(*c["spans"]["a"])], R.STACKED).sum(), c["spans"]["a"][1] - c["spans"]["a"][0]))
    assert (mesh[on] == 0).all() and on.sum() >= 0.25 * hit.sum(), (on.sum(), hit.sum())
    for m in R.STACKED[1:]:
        alone = O.OracleScene(R.only_meshes(kz.scenes, c["desc"], [m]), brute=True).trace_rays(*rays)
        assert (alone["mesh"][on] == 0).all() and np.array_equal(alone["t"][on].view(np.uint32), t[on].view(np.uint32)), m
    sc = c["scene"]
    n4 = sc.table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4)
    tris = sc.table(kz.abi.KZ_TABLE_TRIS).view(np.dtype([("g", "<f4", 9), ("mesh", "<u4"), ("prim", "<u4"), ("gid", "<u4")]))
    copy = np.isin(tris["mesh"], R.STACKED)
    root = slots_under(n4, len(tris), 0)
    assert (root >= 0).all() and len(np.unique(root[copy])) == 1, "the soup is one child of the root"
    top = int(n4[0]["child"][int(root[copy][0])])
    assert not top & 0x80000000
    slot = slots_under(n4, len(tris), top)
    where = np.full((len(R.STACKED), 625), -1, np.int64)
    where[tris["mesh"][copy], tris["prim"][copy]] = slot[copy]
    assert (where >= 0).all()
    spread = sum(len(set(where[:, p])) >= 2 for p in range(625))
    print("soup/stacked: the four copies of %d of 625 triangles lie under two or more children of packet %d" % (spread, top))
    assert spread >= 313, spread


def test_flattened_box_ties_with_the_floor_and_the_collapsed_box_is_never_hit(kz, O):
    """cornell/flattened: at least 64 rays end on the squashed box's footprint with the floor and the box tied in t, and the oracle reports the floor (mesh 0, the lower
    index) on each; no hit is on mesh 6, whose triangles are one point."""
    c = R.closest_case(kz, O, "cornell", deform="flattened")
    tie = flattened_ties(kz, O, c)
    print("cornell/flattened: %d rays, %d hit, %d tied between the floor and the squashed box" % (len(tie), (c["ref"]["mesh"] >= 0).sum(), tie.sum()))
    assert tie.sum() >= 64 and (c["ref"]["mesh"][tie] == 0).all()
    assert not (c["ref"]["mesh"] == 6).any()
    assert (c["ref"]["mesh"] == 7).sum() >= 64                      # the light that dropped is hit where it hangs now
    # what the tree holds now: 20 triangles without area (the collapsed box's 12, the squashed box's 8 sides), and packets whose boxes are nothing but the leaf
    # pad - the smallest scale on all three axes, 2^-25 here, where the fresh tree's smallest is 2^-14 (a box without extent keeps the pad: none is empty)
    tris = c["scene"].table(kz.abi.KZ_TABLE_TRIS).view(np.dtype([("p0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("mesh", "<u4"), ("prim", "<u4"), ("gid", "<u4")]))
    flat = ~np.cross(tris["e1"].astype(np.float64), tris["e2"].astype(np.float64)).any(axis=1)
    assert flat.sum() == 20 and set(tris["mesh"][flat]) == {5, 6}
    scale = lambda sc: np.stack([sc.table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4)[k] for k in ("scaleX", "scaleY", "scaleZ")], 1)
    s, s0 = scale(c["scene"]), scale(R.closest_case(kz, O, "cornell")["scene"])
    print("cornell/flattened: smallest packet scale 2^%d (fresh 2^%d), %d of %d packets at it on every axis" % (np.log2(s.min()), np.log2(s0.min()), (s == s.min()).all(axis=1).sum(), len(s)))
    assert s.min() < s0.min() and (s == s.min()).all(axis=1).any()


@pytest.mark.parametrize("name,deform", R.REFIT_CLOSEST)
def test_plane_set_of_a_deformed_case_starts_on_the_refit_packets(kz, O, name, deform):
    """Set (c) of a deformed case: every origin equals, bit for bit, a plane of a packet of the REFIT KZ_TABLE_NODES4 - and at least 64 of them no plane of the fresh
    tree's packets on that axis; tmin is 0; at least 64 of the rays hit."""
    fresh, c = R.closest_case(kz, O, name), R.closest_case(kz, O, name, deform=deform)
    i, j = c["spans"]["c"]
    o, tmin = c["rays"][0][i:j], c["rays"][2][i:j]
    ax, val = c["extra"]["c"]
    planes = lambda case: {(a, np.float32(v).tobytes()) for a, v, _, _ in R.packet_planes(case["scene"].table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4))}
    now, was = planes(c), planes(fresh)
    on = np.array([(int(ax[k]), o[k, ax[k]].tobytes()) in now for k in range(j - i)])
    old = np.array([(int(ax[k]), o[k, ax[k]].tobytes()) in was for k in range(j - i)])
    assert on.all() and (~old).sum() >= 64 and (tmin == 0).all()
    assert (on & (c["ref"]["mesh"][i:j] >= 0)).sum() >= 64


@pytest.mark.parametrize("name,deform", R.REFIT_CLOSEST)
def test_the_edit_took_effect(kz, O, name, deform):
    """The deformed case's rays through the fresh scene's brute force and the deformed one's: the answers (mesh, prim, the bits of t, u, v) differ on at least half of
    the rays that hit anything - of the whole case, and of set (i), the rays aimed at where the moved meshes WERE.
    `stacked` is held to the second only: it moves three of the soup's eight meshes onto a fourth that was there before, so an answer changes only where those
    three were - 0.22 of the case's rays that hit, whatever the rays; 0.67 of set (i).
    Measured, whole case / set (i): scatter 0.69 / 1.00, slivers 0.77 / 1.00, stacked 0.22 / 0.67, nested 0.60 / 0.94, flattened 0.55 / 1.00."""
    fresh, c = R.closest_case(kz, O, name), R.closest_case(kz, O, name, deform=deform)
    before = fresh["ora"].trace_rays(*c["rays"])
    hit = (before["mesh"] >= 0) | (c["ref"]["mesh"] >= 0)
    differ = hit & ~same_hits(before, c["ref"])
    i, j = c["spans"]["i"]
    print("%s/%s: %d rays, %d hit, %d answers changed by the edit (%.2f); of the %d rays aimed at where the moved meshes were %d hit, %d changed (%.2f)" %
          (name, deform, len(hit), hit.sum(), differ.sum(), differ.sum() / hit.sum(), j - i, hit[i:j].sum(), differ[i:j].sum(), differ[i:j].sum() / hit[i:j].sum()))
    assert hit[i:j].sum() >= 512 and differ[i:j].sum() >= 0.5 * hit[i:j].sum(), (differ[i:j].sum(), hit[i:j].sum())
    if deform != "stacked":
        assert differ.sum() >= 0.5 * hit.sum(), (differ.sum(), hit.sum())


@pytest.mark.parametrize("name,deform", R.REFIT_SHADOW)
def test_deformed_shadow_sets_cross_the_moved_invisible_lights(kz, O, name, deform):
    """The shadow sets of a deformed scene: occluded and free segments both, at least 32 segments that walk through an invisible light where it is NOW, and a `crosses`
    that differs from what the fresh scene's invisible lights give for the same segments (they moved)."""
    fresh, c = R.shadow_case(kz, O, name), R.shadow_case(kz, O, name, deform=deform)
    occluded, walks, crosses = c["ref"]
    assert 0.1 <= occluded.mean() <= 0.9 and (walks > 0).sum() >= 32 and crosses.sum() >= 64
    o, d, tmin, tmax = c["rays"]
    was = fresh["ora_il"].trace_rays(o, d, tmin, tmax)["mesh"] >= 0
    now = c["ora_il"].trace_rays(o, d, tmin, tmax)
    assert np.array_equal(now["mesh"] >= 0, crosses)
    print("%s/%s: %d segments, %d occluded, %d cross an invisible light now, %d crossed one before the edit" % (name, deform, len(o), occluded.sum(), crosses.sum(), (was & crosses).sum()))
    if deform == "scatter":                                         # the quads changed places: the same places, another mesh's triangles
        assert (now["mesh"][crosses] >= 0).all() and len(np.unique(now["mesh"][crosses])) == 8
        inv = R.invisible_meshes(c["desc"])
        assert not any(np.array_equal(c["desc"].meshes[m]["V"], fresh["desc"].meshes[m]["V"]) for m in inv)
    else:
        assert (crosses & ~was).sum() >= 32
