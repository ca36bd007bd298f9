"""-m gpu: kz_scene_set_bsdfs / kz_scene_set_lights / kz_scene_set_transforms (include/kazen_mi355x_edit.h) on a resident scene. After every edit the GPU
renders exactly what a fresh kz_scene_create of the edited description renders - film for film, sample for sample against the unchanged oracle - and
every replica's tables equal the host's and a fresh scene's, bit for bit; a refused edit leaves the replica's tables and its film as they were. Nothing here
provokes a fault: a refusal is one on the host, or a flag read back from the device."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from checks import same_bits
from film_cases import fresh_film

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Q1 = os.path.join(HERE, "golden", "q1_default_m0_r0.5.npz")
DEVICE_TABLES = (1, 2, 3, 4, 5, 6, 8)       # KZ_TABLE_NODES4 .. KZ_TABLE_IL_TRIS and KZ_TABLE_BSDFS (0, the BVH2, once a refit has made it resident; 7 is a host table)


def _grid(desc, S=None, stride=1):
    W, H = desc.camera["width"], desc.camera["height"]
    S = S or desc.sampler["sampleCount"]
    yy, xx, ii = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), np.arange(S), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)


def samples_equal_the_oracle(O, sc, stride=1):
    pxy, idx = _grid(sc.desc, sc.sample_count, stride)
    g, c = sc.render_samples(pxy, idx), O.OracleScene(sc.desc).render_samples(pxy, idx)
    assert np.abs(c[:, 2:]).max() > 0
    return same_bits(g, c), int((g.view(np.uint32) != c.view(np.uint32)).any(axis=1).sum())


def device_differs(sc, device=0, tables=DEVICE_TABLES):
    return [t for t in tables if not np.array_equal(sc.table(t, device), sc.table(t))]


def fresh_differs(kz, sc, tables, lib=None):
    fresh = kz.Scene(sc.desc, lib=lib)
    return [t for t in tables if not np.array_equal(fresh.table(t), sc.table(t))]


def turn(ang, about=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """rotation by ang about the vertical axis through `about`, after a scale about the same point, then a shift"""
    c, s = np.cos(ang), np.sin(ang)
    T = lambda t: np.array([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1.0]])
    R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    a = np.asarray(about, np.float64)
    return (T(np.asarray(shift) + a) @ R @ np.diag([scale[0], scale[1], scale[2], 1.0]) @ T(-a)).astype(np.float32)


def centre(desc, m):
    return desc.meshes[m]["V"].astype(np.float64).mean(axis=0)


@pytest.mark.parametrize("integrator,pipeline", [("path_mis", 1), ("path_mis", 2), ("path_mats", 1), ("path_mats", 2), ("normals", 0), ("ao", 0)])
def test_film_after_each_kind_of_edit_equals_a_fresh_scenes(gpu_lib, kz, integrator, pipeline):
    S = kz.scenes
    d = S.cornell_box(40, 32, 8)
    d.integrator["type"] = integrator
    sc = kz.Scene(d, device=0)
    sc.render(pipeline=pipeline)
    f0 = sc.film()
    assert f0.max() > 0
    shaded = integrator in ("path_mis", "path_mats")
    sc.set_bsdfs({5: S.mirror(), 6: S.kazenstandard((0.2, 0.5, 0.9), 0.3, 0.6)})
    sc.render(pipeline=pipeline)
    f1 = sc.film()
    fresh1 = fresh_film(kz, sc.desc, pipeline=pipeline)
    sc.set_lights({7: S.area((1.0, 0.6, 0.4), 31.0, True)})
    sc.render(pipeline=pipeline)
    f2 = sc.film()
    if shaded:
        assert not np.array_equal(f1, f0) and f1.max() > 0 and same_bits(f1, fresh1)
        assert not np.array_equal(f2, f1) and f2.max() > 0 and same_bits(f2, fresh_film(kz, sc.desc, pipeline=pipeline))
    else:                                   # normals / ao read neither materials nor lights
        assert same_bits(f1, f0) and same_bits(f2, f0)
    sc.set_transforms({5: turn(0.5, centre(d, 5), (1.0, 0.8, 1.1)), 7: turn(0.2, centre(d, 7), (0.8, 1.0, 0.8), (0.05, -0.02, 0.0))})
    sc.render(pipeline=pipeline)
    f3 = sc.film()
    assert not np.array_equal(f3, f2) and f3.max() > 0
    assert same_bits(f3, fresh_film(kz, sc.desc, pipeline=pipeline))
    assert device_differs(sc, 0, (0,) + DEVICE_TABLES) == []


def test_q1_four_parameter_sets_on_one_resident_scene_equal_the_oracle(gpu_lib, kz, O):
    """The four sets of tests/test_gpu_parity.py's parameter-scene test, applied in sequence to ONE resident scene: every sample the oracle's, the replica's
    BSDF table the host's and a fresh scene's."""
    params = json.load(open(os.path.join(HERE, "golden", "q1_params.json")))["params"]
    sc = kz.Scene(kz.scenes.load_npz(Q1, {"camera": {"width": 48, "height": 27}, "sampler": {"sampleCount": 4}}), device=0)
    pxy, idx = _grid(sc.desc)
    last = sc.render_samples(pxy, idx)
    geometry = {t: sc.table(t, 0) for t in (1, 2, 3, 4, 5, 6)}
    for name in ["m1_r0", "m0_r0_spec1_st1", "r0.5_c1_cr0.5", "r0_s1_st0.5"]:
        sc.set_bsdfs({4: {k: v for k, v in params[name].items() if not k.startswith("_")}})
        ok, bad = samples_equal_the_oracle(O, sc)
        assert ok, (name, bad)
        now = sc.render_samples(pxy, idx)
        assert not same_bits(now, last), name
        last = now
        assert device_differs(sc) == [] and fresh_differs(kz, sc, range(9)) == [], name
        assert all(np.array_equal(sc.table(t, 0), v) for t, v in geometry.items()), name


def test_cornell_light_edit_and_ten_frame_turntable_equal_the_oracle(gpu_lib, kz, O):
    d = kz.scenes.cornell_box(48, 48, 8)
    sc = kz.Scene(d, device=0)
    sc.render()
    f0 = sc.film()
    sc.set_lights({7: kz.scenes.area((0.9, 1.0, 0.7), 24.0, True)})
    ok, bad = samples_equal_the_oracle(O, sc)
    assert ok, bad
    assert device_differs(sc) == [] and fresh_differs(kz, sc, range(9)) == []
    c5, c6, c7 = centre(d, 5), centre(d, 6), centre(d, 7)
    for frame in range(10):
        a = 0.15 * (frame + 1)
        sc.set_transforms({5: turn(a, c5), 6: turn(-a, c6, (1.0, 1.0 - 0.02 * frame, 1.0)), 7: turn(0.5 * a, c7, shift=(0.01 * frame, 0.0, 0.0))})
        if frame in (0, 9):
            assert device_differs(sc, 0, (0,) + DEVICE_TABLES) == [], frame
            assert fresh_differs(kz, sc, (3, 4, 5, 6, 8)) == [], frame
            ok, bad = samples_equal_the_oracle(O, sc)
            assert ok, (frame, bad)
    sc.render()
    film = sc.film()
    assert not np.array_equal(film, f0) and film.max() > 0
    assert same_bits(film, fresh_film(kz, sc.desc))
    assert np.array_equal(film, O.OracleScene(sc.desc).render_canonical(threads=0))          # the whole film, apron and weights included
    sc.render(pipeline=1)                                       # the BVH2 paths read the refit BVH2
    assert same_bits(sc.film(), fresh_film(kz, sc.desc, pipeline=1))


def test_soup_transforms_of_all_soup_meshes_and_two_lights(gpu_lib, kz, O):
    d = kz.scenes.random_triangles(20000, 64, 48, 4, sampler="independent")
    sc = kz.Scene(d, device=0)
    sc.render()
    f0 = sc.film()
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    soup = list(range(8))
    assert len(lights) == 8 and all(d.meshes[m]["light"] is None for m in soup)
    for frame in range(2):
        upd = {m: turn(0.03 * (frame + 1) * (1 + i % 3), centre(d, m), shift=(0.002 * i, 0.0, -0.001 * i)) for i, m in enumerate(soup)}
        upd.update({m: turn(0.1 * (frame + 1), centre(d, m), (1.1, 1.0, 0.9)) for m in lights[:2]})
        sc.set_transforms(upd)
    sc.render()
    assert device_differs(sc, 0, (0,) + DEVICE_TABLES) == []
    assert fresh_differs(kz, sc, (3, 4, 5, 6, 8)) == []
    ok, bad = samples_equal_the_oracle(O, sc, stride=3)
    assert ok, bad
    assert not np.array_equal(sc.film(), f0) and same_bits(sc.film(), fresh_film(kz, sc.desc))
    # lights of this scene are invisible: all visible, scaled, then as they were
    original = {m: dict(d.meshes[m]["light"]) for m in lights}      # (d is sc.desc: it follows the edits)
    sc.set_lights({m: dict(l, lightPrimaryVisibility=True, intensity=l["intensity"] * 0.5) for m, l in original.items()})
    assert sc.table(6, 0).size == 0 and device_differs(sc) == [] and fresh_differs(kz, sc, (3, 4, 5, 6, 8)) == []      # (the trees differ: a refit keeps the build's)
    assert np.array_equal(kz.Scene(sc.desc).table(7)[296:332], sc.table(7)[296:332])                            # shadowFast .. anyInvisibleLight of KzParams
    sc.render()
    assert same_bits(sc.film(), fresh_film(kz, sc.desc))
    sc.set_lights(original)
    assert sc.table(6, 0).size == 16 * 48 and device_differs(sc) == []
    sc.render()
    assert same_bits(sc.film(), fresh_film(kz, sc.desc))


def test_refused_edits_leave_the_replica_and_its_film_as_they_were(gpu_lib, kz):
    a, S = kz.abi, kz.scenes
    d = S.cornell_box(32, 32, 8)
    sc = kz.Scene(d, device=0)
    sc.set_transforms({6: turn(0.1, centre(d, 6))})            # (makes the BVH2 resident: table 0 is compared too)
    sc.render()
    before = sc.film()
    tabs = {t: sc.table(t, 0) for t in (0,) + DEVICE_TABLES}
    w0 = np.diag([1, 1, 1, 0]).astype(np.float32)
    far = np.eye(4, dtype=np.float32)
    far[3] = (0, 1.0, 0, -float(d.meshes[5]["V"][0, 1]))         # w = y - y0: zero for the vertices at the height of vertex 0
    for name, call in {"w = 0 on a mesh that is no light (the device flag)": lambda: sc.set_transforms({6: turn(0.3), 5: w0}),
                       "w = 0 at some vertices only": lambda: sc.set_transforms({5: far}),
                       "w = 0 on the light": lambda: sc.set_transforms({7: w0}),
                       "a NaN entry": lambda: sc.set_transforms({5: np.full((4, 4), np.nan, np.float32)}),
                       "mesh out of range": lambda: sc.set_transforms({99: np.eye(4)}),
                       "light out of range": lambda: _raw_light(sc, 3),
                       "bsdf type 99": lambda: sc.set_bsdfs({5: {"type": "whitted"}})}.items():
        with pytest.raises(a.KzError) as e:
            call()
        assert e.value.code in (a.KZ_ERR_INVALID_ARG, a.KZ_ERR_UNSUPPORTED), name
        assert [t for t in tabs if not np.array_equal(sc.table(t, 0), tabs[t])] == [], name
        assert device_differs(sc, 0, (0,) + DEVICE_TABLES) == [], name
    sc.render()
    assert same_bits(sc.film(), before)
    sc.set_transforms({5: turn(0.3, centre(d, 5))})            # and the scene still takes a good edit
    sc.render()
    assert same_bits(sc.film(), fresh_film(kz, sc.desc)) and not same_bits(sc.film(), before)


def _raw_light(sc, index):
    a = __import__("importlib").import_module("nano-kazen_amd").abi
    arr = (a.KzLightUpdate * 1)(a.KzLightUpdate(index, a.KzLight((1.0, 1.0, 1.0), 1.0, 0)))
    a.check(sc.lib, sc.lib.kz_scene_set_lights(sc.h, arr, 1))


def test_bsdf_query_on_an_edited_row_has_the_oracles_bits(gpu_lib, kz, O):
    S = kz.scenes
    rows = [S.diffuse((0.5, 0.6, 0.7)), S.kazenstandard((0.8, 0.5, 0.3), 0.4, 0.5, 0.3), S.mirror()]
    edited = [S.roughconductor(0.3, "Au"), S.ggx((0.9, 0.6, 0.3), 0.3, 0.2), S.roughplastic(0.25, kd=(0.2, 0.4, 0.7))]
    s = S.SceneDescription()
    for r in rows:
        s.add_mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.uint32), bsdf=r)
    s.camera.update(width=32, height=32)
    sc = kz.Scene(s, device=0)
    sc.set_bsdfs({m: b for m, b in enumerate(edited)})
    ora = O.OracleScene(sc.desc)
    rng = np.random.default_rng(13)
    m = 300
    wi = rng.normal(size=(m, 3)).astype(np.float32); wi[:, 2] = np.abs(wi[:, 2]) + 0.02; wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo = rng.normal(size=(m, 3)).astype(np.float32); wo[:, 2] = np.abs(wo[:, 2]) + 0.02; wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    s3 = rng.random((m, 3)).astype(np.float32)
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    for r in range(len(edited)):
        ev, pd, sm = sc.bsdf_query(np.full(m, r, np.int32), wi, wo, np.zeros(m, np.float32), s3)
        so = np.stack([ora.bsdf(r, "sample", wi[k], None, 0.0, float(s3[k, 0]), (float(s3[k, 1]), float(s3[k, 2]))) for k in range(m)])
        e = np.stack([ora.bsdf(r, "eval", wi[k], wo[k]) for k in range(m)])
        p = np.array([ora.bsdf(r, "pdf", wi[k], wo[k]) for k in range(m)], np.float32)
        ok = (so[:, 6] > 0) & (sm[:, 6] > 0)
        assert np.array_equal(so[:, 6] > 0, sm[:, 6] > 0) and ok.any(), r
        assert np.array_equal(bits(sm[ok, 3:6]), bits(so[ok, 3:6])) and np.array_equal(bits(sm[ok, :3]), bits(so[ok, :3])), (r, "sample")
        assert np.array_equal(bits(ev), bits(e)) and np.array_equal(bits(pd), bits(p)) and np.abs(e).max() > 0, (r, "eval / pdf")


@pytest.fixture()
def aliased(dev_lib, kz):
    dev_lib.kz_debug_alias_devices(4)
    assert dev_lib.kz_device_count() == 4
    yield dev_lib
    for d in range(4):
        dev_lib.kz_device_trim(d)
    dev_lib.kz_debug_alias_devices(0)


def _budget(lib, n):
    f, t = C.c_uint64(), C.c_uint64()
    assert lib.kz_device_mem_info(0, C.byref(f), C.byref(t)) == 0
    return int(0.8 * min(f.value, t.value) / n)


def test_edits_of_all_three_kinds_reach_every_replica(aliased, kz):
    """Aliased replicas (the development library): after a material, a light and a transform edit every replica holds the host's tables, kz_render_multi's
    film is a fresh one-replica film, and a replica uploaded AFTER the edits renders them too (and takes the next transform like the others)."""
    n = 3
    S = kz.scenes
    d = S.random_triangles(3000, 128, 96, 8, sampler="independent")
    sc = kz.Scene(d, lib=aliased)
    cap = _budget(aliased, n + 1)
    first, _ = sc.render_multi(list(range(n)), max_state_bytes=cap)
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    soup = [m for m, x in enumerate(d.meshes) if x["light"] is None and x["bsdf"] is not None]
    sc.set_bsdfs({soup[0]: S.mirror(), soup[1]: S.roughdielectric(0.2)})
    sc.set_lights({lights[0]: S.area((1.0, 0.5, 0.2), 40.0, True), lights[1]: dict(d.meshes[lights[1]]["light"], intensity=3.0)})
    sc.set_transforms({soup[0]: turn(0.2, centre(d, soup[0])), soup[3]: turn(-0.1, centre(d, soup[3]), (1.1, 0.9, 1.0)), lights[0]: turn(0.3, centre(d, lights[0]))})
    for dev in range(n):
        assert device_differs(sc, dev, (0,) + DEVICE_TABLES) == [], dev
    film, _ = sc.render_multi(list(range(n + 1)), max_state_bytes=cap)          # (device n: uploaded now, from the edited host tables)
    assert device_differs(sc, n) == []
    ref = kz.Scene(sc.desc, lib=aliased)
    one, _ = ref.render_multi([0], max_state_bytes=cap)
    assert same_bits(film, one) and not same_bits(film, first) and film.max() > 0
    ref.close()
    sc.set_transforms({soup[0]: turn(0.4, centre(d, soup[0])), lights[0]: turn(0.1, centre(d, lights[0]))})      # the late replica's first transform of these meshes
    for dev in range(n + 1):
        assert device_differs(sc, dev, (0,) + DEVICE_TABLES) == [], dev
    film, _ = sc.render_multi(list(range(n + 1)), max_state_bytes=cap)
    ref = kz.Scene(sc.desc, lib=aliased)
    one, _ = ref.render_multi([0], max_state_bytes=cap)
    assert same_bits(film, one)


def test_accumulating_across_an_edit_sums_both_halves(gpu_lib, kz):
    """Half the samples before a material + transform edit, half after, accumulated: the film is the running sum of the two halves. The two halves are taken
    from scenes that render one half each; their float sum regroups at most 25 taps x 8 samples non-negative terms per texel (gaussian filter, radius 2),
    so it may differ from the running sum by 200 x 2^-24 = 1.2e-5 of the value: rtol 2e-5."""
    S = kz.scenes
    d = S.cornell_box(40, 32, 8)
    sc = kz.Scene(d, device=0)
    sc.render(sample_begin=0, sample_end=4)
    a_half = sc.film()
    sc.set_bsdfs({5: S.mirror()})
    sc.set_transforms({6: turn(0.4, centre(d, 6))})
    sc.render(sample_begin=4, sample_end=8, accumulate=True)
    got = sc.film()
    b = kz.Scene(sc.desc, device=0)
    b.render(sample_begin=4, sample_end=8)
    b_half = b.film()
    assert a_half.max() > 0 and b_half.max() > 0 and not np.array_equal(a_half, b_half)
    assert np.allclose(got, a_half + b_half, rtol=2e-5, atol=1e-7)
    b.render()
    assert not np.allclose(got, b.film(), rtol=2e-5, atol=1e-7)


def test_probe_of_large_passes_starts_over_when_bsdf_ext_changes(gpu_lib, kz):
    """The replica's large-pass probe timed the shade kernel bsdfExt selected: an edit that changes bsdfExt resets it (kz_pass_mode_info: not known, no pass
    timed), one that keeps bsdfExt does not."""
    from conftest import wait_for_wipe
    desc = kz.scenes.load_npz(Q1, overrides={"camera": {"width": 1920, "height": 1080}, "sampler": {"type": "independent", "sampleCount": 128, "seed": 0}})
    wait_for_wipe(gpu_lib)
    sc = kz.Scene(desc, device=0)
    for _ in range(2):
        sc.render(shadow_beside=1)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 30.0:
            i_ = sc.last_pass_info()
            if i_["contextItems"] >= i_["itemsPerPass"] or sc.last_grow_note():
                break
            time.sleep(0.05)
    sc.render()
    sc.render()
    assert sc.pass_mode_info()["timed_passes"] >= 1
    timed = sc.pass_mode_info()["timed_passes"]
    sc.set_bsdfs({4: dict(sc.desc.meshes[4]["bsdf"], roughness=0.2)})          # kazenstandard -> kazenstandard: bsdfExt stays 0
    assert sc.pass_mode_info()["timed_passes"] == timed
    sc.set_bsdfs({4: kz.scenes.mirror()})                                       # bsdfExt 0 -> 1
    m = sc.pass_mode_info()
    assert m["kept"] is None and m["timed_passes"] == 0, m
