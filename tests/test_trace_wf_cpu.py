"""The ray sets of tests/trace_ray_sets.py against the brute-force oracle alone (no GPU): each set exercises what it claims. These are conditions on the
generators, not measurements of the kernels - tests/test_trace_wf_gpu.py runs the kernels on the same rays. A generator that misses a condition gets another
recipe or seed; the condition stays."""
import ctypes as C

import numpy as np
import pytest

import trace_ray_sets as R


@pytest.mark.parametrize("name", R.CLOSEST_SCENES)
def test_closest_hit_sets_hit_and_miss(kz, O, name):
    """Every closest-hit set has at least 10 % hits (the dead rows of (f) apart, which all miss), and a scene's sets together at least 5 % misses - the closed
    soup answers every ray from inside with a hit, which is why set (g) starts outside."""
    c = R.closest_case(kz, O, name)
    hit = c["ref"]["mesh"] >= 0
    for k, (i, j) in c["spans"].items():
        live = ~c["extra"]["f"] if k == "f" else np.ones(j - i, bool)
        assert hit[i:j][live].mean() >= 0.10, (name, k, hit[i:j][live].mean())
        if k == "f":
            assert not hit[i:j][~live].any() and (~live).sum() >= 32
            assert all(((~live)[w:w + 64].any() and live[w:w + 64].any()) for w in range(0, j - i, 64)), "every wave of (f) mixes dead and live lanes"
    assert (~hit).mean() >= 0.05, (name, (~hit).mean())
    assert np.isinf(c["ref"]["t"][~hit]).all()


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_zero_component_set_hits_for_every_count(kz, O, name):
    """Set (b): at least 64 hits among the directions with ONE and with TWO exactly-zero components, and at least 64 among those with none but a component of
    +-1e-21 / 1e-20 / 1e-19. Three zero components are the zero vector: Mesh::rayIntersect rejects every triangle for it (det = 0), so that count can hold no
    hit - its rows are there, and the oracle misses on all of them. Both signs of zero and of every tiny value occur."""
    c = R.closest_case(kz, O, name)
    i, j = c["spans"]["b"]
    d, zeros, hit = c["rays"][1][i:j], c["extra"]["b"], c["ref"]["mesh"][i:j] >= 0
    for count in (0, 1, 2):
        assert hit[zeros == count].sum() >= 64, (name, count, hit[zeros == count].sum())
    assert (zeros == 3).sum() >= 8 and not hit[zeros == 3].any()
    assert (d.view(np.uint32) == 0x80000000).any() and (d.view(np.uint32) == 0).any()
    for t in R.TINY:
        for sg in (1, -1):
            assert (d == np.float32(sg * t)).any(), sg * t


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_plane_set_starts_on_packet_planes(kz, O, name):
    """Set (c): at least 64 rays whose origin equals a plane of a BVH4 packet bit for bit - taken from the host copy of the packets - and which hit; tmin is 0; among
    them packet origins p themselves with a negative direction along that axis (where q * a + b is -0.0 in the kernels' box test) and axis-aligned directions."""
    c = R.closest_case(kz, O, name)
    i, j = c["spans"]["c"]
    o, d, tmin = c["rays"][0][i:j], c["rays"][1][i:j], c["rays"][2][i:j]
    ax, val = c["extra"]["c"]
    nodes4 = c["scene"].table(kz.abi.KZ_TABLE_NODES4).view(R.NODE4)
    assert R.NODE4.itemsize == 64
    planes = {(a, np.float32(v).tobytes()) for a, v, _, _ in R.packet_planes(nodes4)}
    origins = {(a, nodes4[k]["p"][a].tobytes()) for k in range(len(nodes4)) for a in range(3)}
    on = np.array([(int(ax[k]), o[k, ax[k]].tobytes()) in planes for k in range(j - i)])
    on_p = np.array([(int(ax[k]), o[k, ax[k]].tobytes()) in origins for k in range(j - i)])
    hit = c["ref"]["mesh"][i:j] >= 0
    assert on.all() and (on & hit).sum() >= 64 and (tmin == 0).all()
    neg = d[np.arange(j - i), ax] < 0
    assert (on_p & neg & hit).sum() >= 64 and (on_p & ~neg & hit).sum() >= 64
    assert (((d != 0).sum(axis=1) == 1) & hit).sum() >= 64


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_tmax_set_brackets_the_hit(kz, O, name):
    """Set (e): tmax one ulp below, at and one ulp above a brute-force hit distance. Around the CLOSEST hit the outcome follows from the position - below: clipped, a miss;
    at and above: kept (t <= tmax, mesh.cpp:91) - so a position cannot show both outcomes there. The rows around the SECOND hit of the same rays give `below` its other
    outcome (the ray still returns its closest hit); `at` and `above` a hit distance cannot miss, whatever the generator. Every position is present around both. Then the pinched rays (tmin = tmax = t)."""
    c = R.closest_case(kz, O, name)
    i, j = c["spans"]["e"]
    pos, hit, t, tmin, tmax = c["extra"]["e"], c["ref"]["mesh"][i:j] >= 0, c["ref"]["t"][i:j], c["rays"][2][i:j], c["rays"][3][i:j]
    n = (pos == 0).sum() // 2
    assert n >= 64
    for p in (-1, 0, 1):
        assert (pos[:3 * n] == p).sum() == n and (pos[3 * n:6 * n] == p).sum() == n
    first, second = np.arange(j - i) < 3 * n, (np.arange(j - i) >= 3 * n) & (pos != 2)
    assert not hit[first & (pos == -1)].any() and hit[first & (pos >= 0)].all() and hit[second].all()
    assert (t[first & (pos == 0)] == tmax[first & (pos == 0)]).all()                              # the hit AT tmax is the closest hit itself
    assert (t[first & (pos == 1)] == t[first & (pos == 0)]).all()
    assert (t[second] == np.tile(t[first & (pos == 0)], 3)).all()                                 # around the second hit: the closest hit, in every position
    assert hit[pos == -1].any() and (~hit[pos == -1]).any()
    # the pinched rays: tmin == tmax == t, the hit stays; two low bits of t clear; one unbroken run of at least three waves (so one whole wave, wherever the run begins)
    pin = pos == 2
    assert pin.sum() >= 192 and pin[-pin.sum():].all() and hit[pin].all()
    assert (t[pin] == tmin[pin]).all() and (t[pin] == tmax[pin]).all() and (t[pin].view(np.uint32) & 3 == 0).all()


def test_coincident_scene_yields_ties(kz, O):
    """Three identical triangles: every hit is a three-way tie in t, and brute force reports the lowest id (mesh 0)."""
    c = R.closest_case(kz, O, "coincident")
    single = O.OracleScene(R.only_meshes(kz.scenes, c["desc"], [2]), brute=True).trace_rays(*c["rays"])
    hit = c["ref"]["mesh"] >= 0
    assert hit.sum() >= 64 and np.array_equal(hit, single["mesh"] >= 0)
    assert np.array_equal(c["ref"]["t"][hit].view(np.uint32), single["t"][hit].view(np.uint32))  # the last copy alone answers with the same t: a tie
    assert (c["ref"]["mesh"][hit] == 0).all()


@pytest.mark.parametrize("name", R.SHADOW_SCENES)
def test_shadow_sets_are_mixed_and_cross_the_invisible_light(kz, O, name):
    """The occluded share of every shadow set lies between 25 % and 75 %; at least 32 segments cross an invisible-light triangle and continue behind it, at least 8 of
    them occluded beyond it and at least 8 free; the light-sampling segments end in front of their light (none of them walks through)."""
    c = R.shadow_case(kz, O, name)
    occluded, walks, crosses = c["ref"]
    for k, (i, j) in c["spans"].items():
        assert 0.25 <= occluded[i:j].mean() <= 0.75, (name, k, occluded[i:j].mean())
    went = walks > 0
    assert went.sum() >= 32 and (went & occluded).sum() >= 8 and (went & ~occluded).sum() >= 8
    assert (crosses | ~went).all()                           # whoever walks through a light crosses it; the converse fails where something stands in front
    assert (crosses & ~went).any() or name == "cornell_il"
    o, d, tmin, tmax = c["rays"]
    assert (tmin == R.EPS).all() and (tmax > tmin).all() and np.isfinite(o).all() and np.isfinite(d).all()


def test_entry_structures_match_the_header(kz, tmp_path):
    """sizeof of the structures of kz_trace_rays_wf as gcc sees the C header == sizeof of their ctypes mirrors; the entry refuses to run without a device."""
    import os
    import subprocess
    names = ["KzTraceWfOpts", "KzTraceWfHit", "KzTraceWfInfo"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "kazen_mi355x_dev.h"\nint main(void){' + "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "sizes")])
    sizes = dict(l.split() for l in subprocess.check_output([str(tmp_path / "sizes")], text=True).splitlines())
    for n in names:
        assert C.sizeof(getattr(kz.abi, n)) == int(sizes[n]), n
    assert C.sizeof(kz.abi.KzTraceWfHit) == 24
    sc = kz.Scene(R.scene(kz.scenes, "coincident"))
    with pytest.raises(kz.abi.KzError) as e:
        sc.trace_rays_wf(np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32), 0.0, 1.0)
    assert e.value.code == kz.abi.KZ_ERR_STATE
