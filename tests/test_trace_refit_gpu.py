"""-m gpu: the traversal kernels on REFIT trees - the build's topology under boxes that stopped forming a good tree - ray by ray against brute force.

A resident scene is deformed with Scene.set_vertices (tests/trace_ray_sets.py `deformation`: scatter, slivers, stacked, nested on the 5 000-triangle soup, flattened
on the cornell box) and the kernels a render launches walk what kz_refit.hip and the host refit left: inner boxes about the size of the room, children that all
contain the ray's origin (entry distances tie at tmin, overlaps tie at tmax - tmin), four coincident copies of 625 triangles in different subtrees, boxes
that are nothing but the leaf pad, triangles without area, invisible lights that moved. The checks are those of tests/test_trace_wf_gpu.py - the helpers of tests/trace_ray_sets.py - against the brute force of
the DEFORMED description: mesh and prim equal, t / u / v the oracle's bits; shadow sums exact; every launch shape the bits of the default one.

tests/test_trace_refit_cpu.py runs before these tests (no GPU) and establishes the stack bound first: the bound of the refit tree is the build's, so the overflow
area a launch owns covers the deformed tree - and its walk model says the default 16 LDS entries are passed on scatter (18) and slivers (21), which is asserted
here at the default launch shape, not only behind lds_stack=2. The references are computed once per case, in-process, and shared through the case cache."""
import numpy as np
import pytest

import trace_ray_sets as R
from checks import all_samples_equal_the_oracle, same_bits
from film_cases import fresh_film
from trace_ray_sets import KINDS, LDS_ENTRIES, PACKET_SHAPES, SHAPES, check_closest, check_shadow, flattened_ties, report, run, same_result, u32

pytestmark = pytest.mark.gpu
TABLES = range(7)           # KZ_TABLE_NODES .. KZ_TABLE_IL_TRIS
ids = lambda cases: ["%s/%s" % c for c in cases]


def tie_rays(kz, O, case, deform):
    """The rays of a case whose closest hit is a tie the lowest id must win, made once: on the coincident copies of `stacked`, on the footprint of `flattened`
    where the floor's and the squashed box's triangle answer with the same bits of t. None for the other deformations."""
    if "ties" not in case:
        case["ties"] = np.isin(case["ref"]["mesh"], R.STACKED) if deform == "stacked" else flattened_ties(kz, O, case) if deform == "flattened" else None
    return case["ties"]


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("name,deform", R.REFIT_CLOSEST, ids=ids(R.REFIT_CLOSEST))
def test_closest_hit_kernels_equal_brute_force_on_refit_trees(gpu_lib, kz, O, name, deform, kernel):
    """Sets (a) - (i) of a deformed scene in one launch of the default shape, identity queue: (mesh, prim) and the bits of t, u, v of every ray are brute force's.
    The ties go to the lowest id - mesh 0 on the four coincident copies of `stacked` and on the floor under the squashed box of `flattened` - although the tied
    triangles lie in other leaves, reached only because t <= tmax and tnear <= tfar admit equality. The packet kernel queues as many first hits on the invisible
    lights as the oracle finds where the lights are now."""
    case = R.closest_case(kz, O, name, device=0, deform=deform)
    res = run(case, kernel)
    check_closest(case, kernel, res)
    ref = case["ref"]
    ties = tie_rays(kz, O, case, deform)
    print("%s/%s %s: %d rays compared, %d hit, %s ties resolved" % (name, deform, KINDS[kernel], len(ref["mesh"]), (ref["mesh"] >= 0).sum(), "no" if ties is None else int(ties.sum())))
    if ties is not None:
        assert ties.sum() >= 64 and (ref["mesh"][ties] == 0).all()
        bad = np.flatnonzero(ties & (res["mesh"] != 0))
        assert len(bad) == 0, report(case, bad, res, ref, "%s kernel, tie winners" % KINDS[kernel])
    if kernel == 1:
        assert res["info"]["nFirstHitsOnInvisibleLight"] == int(np.isin(ref["mesh"], R.invisible_meshes(case["desc"])).sum())
        assert res["info"]["stackBound"] <= 128                     # (the packet kernel's stack; a tree beyond it is refused)


@pytest.mark.parametrize("name,deform", R.REFIT_CLOSEST, ids=ids(R.REFIT_CLOSEST))
def test_bvh2_walk_agrees_on_refit_trees(gpu_lib, kz, O, name, deform):
    """kz_trace_rays - the BVH2 walk of the megakernel path, on the refit BVH2 - on the same rays: brute force's triangle and bits, and so the BVH4 kernels'."""
    case = R.closest_case(kz, O, name, device=0, deform=deform)
    b2, ref = case["scene"].trace_rays(*case["rays"]), case["ref"]
    hit = ref["mesh"] >= 0
    wrong = (b2["mesh"] != ref["mesh"]) | (b2["prim"] != ref["prim"])
    for k in ("t", "u", "v"):
        wrong |= hit & (u32(b2[k]) != u32(ref[k]))
    bad = np.flatnonzero(wrong)
    assert len(bad) == 0, report(case, bad, b2, ref, "BVH2 kernel against brute force")
    for kernel in (0, 1):
        res = run(case, kernel)
        wrong = (res["mesh"] != b2["mesh"]) | (res["prim"] != b2["prim"])
        for k in ("t", "u", "v"):
            wrong |= hit & (u32(res[k]) != u32(b2[k]))
        bad = np.flatnonzero(wrong)
        assert len(bad) == 0, report(case, bad, res, b2, "%s kernel against the BVH2 kernel" % KINDS[kernel])


CASES = sorted(set(R.REFIT_CLOSEST) | set(R.REFIT_SHADOW))


@pytest.mark.parametrize("name,deform", CASES, ids=ids(CASES))
def test_device_tables_equal_the_host_tables_after_each_deformation(gpu_lib, kz, O, name, deform):
    """The replica's refit (kz_refit.hip) equals the host's (kz_edit.cpp) at these magnitudes: BVH2, BVH4, leaf triangles, shading records, light CDFs, light rows and
    the invisible-light triangle table, byte for byte."""
    case = R.shadow_case(kz, O, name, device=0, deform=deform) if name == "cornell_il" else R.closest_case(kz, O, name, device=0, deform=deform)
    sc = case["scene"]
    assert [t for t in TABLES if not np.array_equal(sc.table(t, 0), sc.table(t))] == []
    assert len(sc.table(kz.abi.KZ_TABLE_IL_TRIS)) > 0


@pytest.mark.parametrize("kernel", [0, 2])
@pytest.mark.parametrize("deform", ["scatter", "slivers"])
def test_overlapping_boxes_fill_the_stacks_and_stay_inside_the_overflow_area(gpu_lib, kz, O, deform, kernel):
    """The tree's bound is the build's (28): a launch owns bound - LDS entries overflow rows and a guard row behind them, and fails the call if a stack reaches it.
    With 2 LDS entries the deformed tree reaches more overflow rows than the fresh one; at the default shape (16 LDS entries) the fresh tree reaches none that it
    must, the deformed one at least one - the walk model of tests/test_trace_refit_cpu.py passes 16 entries on both deformations."""
    fresh, case = R.closest_case(kz, O, "soup", device=0), R.closest_case(kz, O, "soup", device=0, deform=deform)
    two, two_fresh = run(case, kernel, lds_stack=2)["info"], run(fresh, kernel, lds_stack=2)["info"]
    dflt, dflt_fresh = run(case, kernel)["info"], run(fresh, kernel)["info"]
    for what, i in (("fresh, 2 LDS entries", two_fresh), (deform + ", 2 LDS entries", two), ("fresh, default", dflt_fresh), (deform + ", default", dflt)):
        print("soup %s kernel, %s: stackBound %d, ldsStack %d, ovfRows %d, ovfRowsTouched %d" % (KINDS[kernel], what, i["stackBound"], i["ldsStack"], i["ovfRows"], i["ovfRowsTouched"]))
    assert two["stackBound"] == two_fresh["stackBound"] == dflt["stackBound"] == 28 and two["stackBound"] <= 128
    assert two["ldsStack"] == 2 and two["ovfRows"] == 26 and 1 <= two["ovfRowsTouched"] <= two["ovfRows"], two
    assert two["ovfRowsTouched"] > two_fresh["ovfRowsTouched"] >= 1, (two, two_fresh)
    assert dflt["ldsStack"] == LDS_ENTRIES and dflt["ovfRows"] == 12 and 1 <= dflt["ovfRowsTouched"] <= dflt["ovfRows"], dflt
    assert dflt_fresh["ovfRowsTouched"] <= dflt_fresh["ovfRows"], dflt_fresh


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_launch_shapes_give_the_bits_of_the_default_launch_on_a_refit_tree(gpu_lib, kz, O, kernel):
    """soup/scatter, a 4 113-entry permuted queue: every shape of SHAPES / PACKET_SHAPES (tests/trace_ray_sets.py) gives the bits of the default launch - one
    workgroup whose lanes take ray after ray on stacks that reach the overflow area, 2 LDS entries, the thresholds, the counting instantiations - and the counting
    shapes agree on node visits and triangle tests. The deformed tree costs many times the node visits of the fresh one (printed)."""
    fresh, case = R.closest_case(kz, O, "soup", device=0), R.closest_case(kz, O, "soup", device=0, deform="scatter")
    q = np.random.default_rng(23).permutation(len(case["rays"][0])).astype(np.uint32)[:4113]
    base = run(case, kernel, queue=q)
    check_closest(case, kernel, base, queue=q)
    counted = []
    for shape in (PACKET_SHAPES if kernel == 1 else SHAPES):
        res = run(case, kernel, queue=q, **shape)
        assert same_result(res, base), ("soup/scatter", KINDS[kernel], shape, report(case, np.flatnonzero(u32(res["t"]) != u32(base["t"])), res, base, "launch shape"))
        if shape.get("stats"):
            assert res["info"]["rays"] == len(q), (shape, res["info"])
            counted.append((shape, res["info"]["nodeVisits"], res["info"]["triTests"]))
        if "grid_blocks" in shape:
            assert res["info"]["gridBlocks"] == shape["grid_blocks"]
    assert len({c[1:] for c in counted}) == 1 and counted[0][1] > 0 and counted[0][2] > 0, counted
    qf = np.random.default_rng(23).permutation(len(fresh["rays"][0])).astype(np.uint32)[:4113]
    f = run(fresh, kernel, queue=qf, stats=True)["info"]
    print("soup %s kernel, 4113 rays: node visits / triangle tests %d / %d on the scattered tree, %d / %d on the fresh one" %
          (KINDS[kernel], counted[0][1], counted[0][2], f["nodeVisits"], f["triTests"]))
    assert counted[0][1] > f["nodeVisits"]


@pytest.mark.parametrize("name,deform", R.REFIT_SHADOW, ids=ids(R.REFIT_SHADOW))
def test_shadow_kernels_on_refit_trees_and_moved_invisible_lights(gpu_lib, kz, O, name, deform):
    """The shadow launches of a bounce on a deformed scene against the occlusion loop composed from brute-force closest hits: identity queue and a permuted subset. Both
    scenes take the any-hit kernel (shadowFast), whose diversion to the second queue reads the invisible-light box and triangle table the edit re-formed: nQueueB
    is the number of queued segments that cross an invisible-light triangle where it is NOW (check_shadow, from the deformed reference's `crosses`)."""
    case = R.shadow_case(kz, O, name, device=0, deform=deform)
    n = len(case["rays"][0])
    res = run(case, 3)
    assert res["info"]["shadowFast"] == 1
    check_shadow(case, res)
    perm = np.random.default_rng(29).permutation(n).astype(np.uint32)[:n // 2 + 1]
    sub = run(case, 3, queue=perm, stats=True)
    check_shadow(case, sub, queue=perm, stats=True)
    occluded, walks, crosses = case["ref"]
    print("%s/%s shadow: %d segments, %d occluded, %d diverted to the second queue" % (name, deform, n, occluded.sum(), res["info"]["nQueueB"]))
    assert res["info"]["nQueueB"] == int(crosses.sum()) >= 64


def test_child_order_of_the_any_hit_kernel_does_not_change_an_answer_on_a_refit_tree(gpu_lib, dev_lib, kz, O):
    """soup/scatter on the development library: the any-hit kernel with the overlap order (node4KeysOf<true>, the default) and with the closest-hit order
    (kz_debug_shadow_order(0)). Where nearly every child contains the origin the two orders walk different nodes; the answers are identical and brute force's."""
    case = R.shadow_case(kz, O, "soup", device=0, deform="scatter")
    sc = R.edited_scene(kz, "soup", "scatter", 0, lib=dev_lib)
    assert all(np.array_equal(sc.desc.meshes[m]["V"], case["desc"].meshes[m]["V"]) for m in range(len(sc.desc.meshes)))
    dev = dict(case, scene=sc)
    try:
        dev_lib.kz_debug_shadow_order(1)
        on = run(dev, 3, stats=True)
        check_shadow(dev, on, stats=True)
        dev_lib.kz_debug_shadow_order(0)
        off = run(dev, 3, stats=True)
        check_shadow(dev, off, stats=True)
    finally:
        dev_lib.kz_debug_shadow_order(1)
        sc.close()
    print("soup/scatter shadow: node visits / triangle tests %d / %d overlap order, %d / %d closest-hit order" %
          (on["info"]["nodeVisits"], on["info"]["triTests"], off["info"]["nodeVisits"], off["info"]["triTests"]))
    assert same_result(on, off) and on["info"]["nQueueB"] == off["info"]["nQueueB"] and on["info"]["rays"] == off["info"]["rays"]
    assert on["info"]["nodeVisits"] != off["info"]["nodeVisits"]      # the switch switches


def render_scene(kz, name):
    if name == "soup":
        return kz.scenes.random_triangles(5000, 48, 32, 4, sampler="independent", s_edge=0.08)
    return kz.scenes.cornell_box(32, 32, 4)


@pytest.mark.parametrize("name,deform", [("soup", "scatter"), ("cornell", "flattened")], ids=["soup/scatter", "cornell/flattened"])
def test_render_after_the_edit_equals_the_oracle_and_a_fresh_scene(gpu_lib, kz, O, name, deform):
    """A resident scene that has rendered once is deformed and rendered again: the films of the three primary-ray kernels (tune packetPrimary 0, 1, 2 - per lane,
    packets, pixel beams) and of the megakernel (pipeline=1, the refit BVH2) are the same bits; every sample equals the oracle's for the deformed description; the
    film equals a fresh scene's. The pixel-beam lists are rebuilt from the refit tree: on overlapping boxes nearly every list is cut short at its 32 leaves or 16
    open entries, and the rays continue from t_valid under the claim that nothing is hit in front of it."""
    d = render_scene(kz, name)
    sc = kz.Scene(d, device=0)
    sc.render()
    before = sc.film()
    sc.set_vertices(R.deformation(name, sc.desc, deform))
    films = []
    for k in (0, 1, 2):
        sc.render(tune={"packetPrimary": k})
        films.append(sc.film())
    sc.render(pipeline=1)
    films.append(sc.film())
    assert np.isfinite(films[0]).all() and np.abs(films[0][..., :3]).max() > 0 and not np.array_equal(films[0], before)
    for k, f in enumerate(films[1:], 1):
        assert same_bits(f, films[0]), ("packetPrimary 1", "packetPrimary 2", "pipeline 1")[k - 1]
    assert [t for t in TABLES if not np.array_equal(sc.table(t, 0), sc.table(t))] == []
    ok, bad = all_samples_equal_the_oracle(kz, O, sc, sc.desc)
    assert ok, bad
    sc.render()
    assert same_bits(sc.film(), films[0]) and same_bits(films[0], fresh_film(kz, sc.desc))
    sc.close()
