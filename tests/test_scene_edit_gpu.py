"""-m gpu: editing a resident scene (include/kazen_mi355x_edit.h). After kz_scene_set_camera / kz_scene_set_vertices the GPU renders exactly what a
fresh kz_scene_create of the edited description renders - film for film, and sample for sample against the oracle - and every replica's tables
equal the host's, bit for bit."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from checks import all_samples_equal_the_oracle, same_bits
from film_cases import fresh_film

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = range(7)           # KZ_TABLE_NODES .. KZ_TABLE_IL_TRIS


def camera_b(kz, d):
    return {"toWorld": kz.scenes.look_at((0.6, 0.3, 3.3), (0.1, -0.1, 0), (0, 1, 0)), "fov": 44.0}


@pytest.mark.parametrize("integrator,pipeline", [("path_mis", 0), ("path_mis", 1), ("path_mis", 2), ("ao", 0), ("ao", 1)])
def test_set_camera_renders_what_a_fresh_scene_renders(gpu_lib, kz, O, integrator, pipeline):
    """Pinhole A -> pinhole B (pixel beams on both), on the wavefront pipelines (0, 2) and the megakernel (1): the film after the edit is a fresh B scene's film."""
    d = kz.scenes.cornell_box(48, 40, 8)
    d.integrator["type"] = integrator
    sc = kz.Scene(d, device=0)
    assert sc.table(kz.abi.KZ_TABLE_PARAMS).view(np.int32)[kz_beam_ok_word()] == 1
    sc.render(pipeline=pipeline)
    sc.set_camera(camera_b(kz, d))
    assert sc.table(kz.abi.KZ_TABLE_PARAMS).view(np.int32)[kz_beam_ok_word()] == 1
    sc.render(pipeline=pipeline)
    db = kz.scenes.cornell_box(48, 40, 8)
    db.integrator["type"] = integrator
    db.camera.update(camera_b(kz, db))
    assert same_bits(sc.film(), fresh_film(kz, db, pipeline=pipeline))
    assert np.array_equal(sc.table(kz.abi.KZ_TABLE_PARAMS), kz.Scene(db).table(kz.abi.KZ_TABLE_PARAMS))
    if integrator == "path_mis":
        ok, bad = all_samples_equal_the_oracle(kz, O, sc, sc.desc)
        assert ok, bad
    else:                   # (the oracle serves path_mis; ao's samples against a fresh B scene's, which tests/test_integrators_gpu.py holds to the CPU reference)
        yy, xx, ii = np.meshgrid(np.arange(40), np.arange(48), np.arange(8), indexing="ij")
        pxy, idx = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32), ii.ravel().astype(np.uint32)
        assert same_bits(sc.render_samples(pxy, idx), kz.Scene(db, device=0).render_samples(pxy, idx))


def kz_beam_ok_word():
    return 344 // 4             # offsetof(KzParams, beamOk) (tests/test_scene_edit_cpu.py pins it)


def test_set_camera_pinhole_thinlens_pinhole(gpu_lib, kz, O):
    d = kz.scenes.cornell_box(40, 40, 8)
    sc = kz.Scene(d, device=0)
    sc.render()
    lens = {"type": "thinlens", "apertureRadius": 0.05, "focusDistance": 3.4}
    sc.set_camera(lens)
    sc.render()
    dl = kz.scenes.cornell_box(40, 40, 8)
    dl.camera.update(lens)
    assert same_bits(sc.film(), fresh_film(kz, dl))
    ok, bad = all_samples_equal_the_oracle(kz, O, sc, sc.desc)
    assert ok, bad
    sc.set_camera(dict(camera_b(kz, d), type="perspective"))
    sc.render()
    db = kz.scenes.cornell_box(40, 40, 8)
    db.camera.update(dict(camera_b(kz, db), type="perspective"))
    assert same_bits(sc.film(), fresh_film(kz, db))


def rigid_plus_noise(rng, V, scale, noise):
    a = rng.normal(size=3) * scale
    cx, cy, cz, sx, sy, sz = np.cos(a[0]), np.cos(a[1]), np.cos(a[2]), np.sin(a[0]), np.sin(a[1]), np.sin(a[2])
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    c = V.astype(np.float64).mean(axis=0)
    out = (V.astype(np.float64) - c) @ R.T + c + rng.normal(size=3) * scale * 0.2 + rng.normal(size=V.shape) * noise
    return out.astype(np.float32), R


def deform(rng, desc, meshes, scale=0.02, noise=0.004):
    upd = {}
    for m in meshes:
        V, R = rigid_plus_noise(rng, desc.meshes[m]["V"], scale, noise)
        N = desc.meshes[m]["N"]
        upd[m] = (V, (N.astype(np.float64) @ R.T).astype(np.float32)) if N is not None else V
    return upd


def tables_equal(sc, device, tables=TABLES):
    return [t for t in tables if not np.array_equal(sc.table(t, device), sc.table(t))]


def test_set_vertices_ten_frames_equal_fresh_scenes_and_the_oracle(gpu_lib, kz, O):
    """Random rigid motion + per-vertex noise on a box, the metal block and the (invisible) ceiling light, ten frames in a row, the tree drifting
    from its build: device tables = host tables, every sample = the oracle's for the deformed description, the film = a fresh scene's."""
    rng = np.random.default_rng(7)
    d = kz.scenes.cornell_box(48, 48, 8)
    sc = kz.Scene(d, device=0)
    sc.render()
    assert sc.desc.meshes[7]["light"] is not None and not sc.desc.meshes[7]["light"]["lightPrimaryVisibility"]
    sah0 = sc.bvh_info()["sahCost"]
    for frame in range(10):
        sc.set_vertices(deform(rng, sc.desc, [5, 6, 7]))
        sc.render()
        if frame in (0, 9):
            assert tables_equal(sc, 0) == []
            ok, bad = all_samples_equal_the_oracle(kz, O, sc, sc.desc)
            assert ok, (frame, bad)
            assert same_bits(sc.film(), fresh_film(kz, sc.desc)), frame
    assert sc.bvh_info()["sahCost"] != sah0
    # the BVH2 paths (megakernel) read the refit BVH2
    sc.render(pipeline=1)
    assert same_bits(sc.film(), fresh_film(kz, sc.desc, pipeline=1))


def test_set_vertices_random_triangles_and_an_emissive_mesh(gpu_lib, kz, O):
    """A C4-shaped soup (5 000 triangles, 8 light quads): every soup mesh and two lights move; tables, samples and film as a fresh scene's."""
    rng = np.random.default_rng(11)
    d = kz.scenes.random_triangles(5000, 64, 48, 4, sampler="independent")
    sc = kz.Scene(d, device=0)
    sc.render()
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    for frame in range(3):
        sc.set_vertices(deform(rng, sc.desc, list(range(8)) + lights[:2], scale=0.01, noise=0.002))
    sc.render()
    assert tables_equal(sc, 0) == []
    ok, bad = all_samples_equal_the_oracle(kz, O, sc, sc.desc, stride=3)
    assert ok, bad
    assert same_bits(sc.film(), fresh_film(kz, sc.desc))


def test_failed_updates_leave_the_render_as_it_was(gpu_lib, kz):
    d = kz.scenes.cornell_box(32, 32, 8)
    sc = kz.Scene(d, device=0)
    sc.render()
    before = sc.film()
    tabs = {t: sc.table(t, 0) for t in TABLES[1:]}         # (the BVH2 is not resident: no BVH2 path or edit has run)
    for bad in ({5: (d.meshes[5]["V"][:-1], d.meshes[5]["N"][:-1])}, {5: d.meshes[5]["V"]}, {99: d.meshes[5]["V"]},
                {5: (np.where(np.arange(d.meshes[5]["V"].size).reshape(-1, 3) == 4, np.nan, d.meshes[5]["V"]).astype(np.float32), d.meshes[5]["N"])}):
        with pytest.raises(kz.abi.KzError):
            sc.set_vertices(bad)
    with pytest.raises(kz.abi.KzError):
        sc.set_camera({"width": 33})
    assert [t for t in tabs if not np.array_equal(sc.table(t, 0), tabs[t])] == []
    sc.render()
    assert same_bits(sc.film(), before)


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


@pytest.mark.parametrize("n", [2, 4])
def test_replicas_follow_an_update(aliased, kz, n):
    """Aliased replicas (the development library): render_multi after an update equals a one-device fresh film, every replica holds the host's tables,
    and a replica uploaded AFTER the update gets the updated tables."""
    rng = np.random.default_rng(3 + n)
    d = kz.scenes.random_triangles(3000, 128, 96, 8, sampler="independent")
    sc = kz.Scene(d, lib=aliased)
    cap = _budget(aliased, n)
    sc.render_multi(list(range(n - 1)), max_state_bytes=cap)
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    sc.set_vertices(deform(rng, sc.desc, [0, 3, 7, lights[0]], scale=0.01, noise=0.002))
    for dev in range(n - 1):
        assert tables_equal(sc, dev) == [], dev
    film, _ = sc.render_multi(list(range(n)), max_state_bytes=cap)          # (device n - 1: uploaded now, from the refit host tables)
    assert tables_equal(sc, n - 1, TABLES[1:]) == []
    ref = kz.Scene(sc.desc, lib=aliased)
    one, _ = ref.render_multi([0], max_state_bytes=cap)
    assert same_bits(film, one)


def test_c4_scale_refit_then_crop_equals_a_fresh_build(gpu_lib, kz):
    """All 1 M triangles of C4 refit on the device (a mild deformation of every soup mesh), then a crop rendered: the crop equals a fresh build's."""
    rng = np.random.default_rng(1)
    d = kz.scenes.random_triangles(1000000, 1920, 1080, 16, sampler="pmj02bn", seed=1)
    sc = kz.Scene(d, device=0)
    tile = [(896, 476, 128, 128)]
    sc.render(tiles=tile)
    upd = {m: (d.meshes[m]["V"] + rng.normal(size=d.meshes[m]["V"].shape).astype(np.float32) * np.float32(0.001), d.meshes[m]["N"]) for m in range(8)}
    t0 = time.perf_counter()
    sc.set_vertices(upd)
    dt = time.perf_counter() - t0
    sc.render(tiles=tile)
    got = sc.film()
    assert dt < 2.0, dt
    fresh = kz.Scene(sc.desc, device=0)
    fresh.render(tiles=tile)
    assert same_bits(got, fresh.film())
