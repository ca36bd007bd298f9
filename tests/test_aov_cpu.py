"""Feature films (include/kazen_mi355x_aov.h) without a GPU: the header against the library's exports, the refusals that need no device, sanity checks of the
test-only CPU reference (tests/cpu_ref/kz_aov_ref.cpp) the GPU tests compare against, the layered EXR writer, and the precondition of the cross-check scene."""
import re

import numpy as np
import pytest

from checks import header_surface, refused
from cpu_refs import AovRef, lib
from film_cases import grid_of, octant_scene


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("aov", tmp_path_factory.mktemp("kza"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: nothing added to the pinned lists or to the two existing headers
    _, src = header_surface(kz, "include/kazen_mi355x_aov.h", a.AOV_EXPORTS, 6, [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS],
                            ["include/kazen_mi355x.h", "include/kazen_mi355x_dev.h", "include/kazen_mi355x_edit.h"], ["aov"], resolve=False)
    assert (a.KZ_AOV_ALBEDO, a.KZ_AOV_NORMAL, a.KZ_AOV_DEPTH, a.KZ_AOV_ALL) == tuple(int(re.search(r"#define %s\s+(\d+)u" % n, src).group(1)) for n in ("KZ_AOV_ALBEDO", "KZ_AOV_NORMAL", "KZ_AOV_DEPTH", "KZ_AOV_ALL"))


def test_refusals_without_a_device(kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert sc.aovs() == []
    for bad in (8, 15, 1 << 31):
        refused(kz, lambda: sc.set_aovs(bad), a.KZ_ERR_INVALID_ARG, "kz_scene_set_aovs")
    assert sc.aovs() == []
    sc.set_aovs(["albedo", "depth"])                                  # (a scene on no device: the mask alone)
    assert sc.aovs() == ["albedo", "depth"]
    with pytest.raises(ValueError):
        sc.set_aovs(["position"])
    # exactly one enabled bit
    for bad in (0, 2, 3, 5, 8):
        refused(kz, lambda: sc.aov_film(bad), a.KZ_ERR_INVALID_ARG, "kz_aov_download")
    refused(kz, lambda: sc.aov_film("albedo"), a.KZ_ERR_STATE)       # one enabled bit, but no device
    tiles = [(0, 0, 16, 16)]
    counter = np.zeros(2, np.uint32)
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "pipeline = 1")
    refused(kz, lambda: sc.render_multi([0]), a.KZ_ERR_UNSUPPORTED, "kz_render_multi")
    refused(kz, lambda: sc.render_dealt(tiles, counter, device=0), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "KzTileDealer")
    refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "packedOutput")
    refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_UNSUPPORTED, "kz_film_download_tiles")
    # with the mask 0 the same calls get as far as they got before: the scene is on no device
    sc.set_aovs(())
    assert sc.aovs() == []
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_STATE)


# ---------------------------------------------------------------- the reference itself
def test_reference_sanity(kz, ref):
    d = kz.scenes.cornell_box(32, 24, 4)
    d.camera["fov"] = 80.0                                            # (wide enough to look past the box: misses)
    pxy, idx = grid_of(d)
    s = AovRef(ref, d).samples(pxy, idx)
    hit = s[:, 9] == 1.0
    assert hit.any() and (~hit).any() and set(np.unique(s[:, 9])) == {0.0, 1.0}
    assert not s[~hit][:, 2:].any()                                   # a miss: every feature 0
    assert (s[hit][:, 8] > 0).all() and np.isfinite(s).all()
    assert np.array_equal(np.floor(s[:, :2]).astype(np.int32), pxy)
    # albedo of a constant row is its constant: the rows of the box
    consts = np.array([(0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.75, 0.75, 0.75), (0.9, 0.6, 0.2), (0, 0, 0)], np.float32)
    alb = s[hit][:, 2:5]
    assert (alb[:, None, :] == consts[None]).all(axis=2).any(axis=1).all()
    assert len(np.unique(alb, axis=0)) >= 4
    # unit normals to 4 ulp (of 1: 4 x 2^-23 on the squared length's square root)
    n = s[hit][:, 5:8].astype(np.float64)
    assert np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0).max() <= 4 * 2.0 ** -23
    assert (s[hit][:, 5:8] < 0).any()                                 # signed: the right wall and the ceiling face -x / -y
    # a single constant diffuse row in front of the whole frame
    one = kz.scenes.SceneDescription()
    q = kz.scenes.quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    one.add_mesh(q[0], q[3], N=q[1], UV=q[2], bsdf=kz.scenes.diffuse((0.25, 0.5, 0.125)))
    one.camera.update(width=8, height=8, fov=40.0, nearClip=0.1, farClip=100.0, toWorld=kz.scenes.look_at((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    one.sampler = {"type": "independent", "sampleCount": 2, "seed": 0}
    s1 = AovRef(ref, one).samples(*grid_of(one))
    assert (s1[:, 9] == 1).all() and (s1[:, 2:5] == np.array([0.25, 0.5, 0.125], np.float32)).all() and (s1[:, 5:8] == np.array([0, 0, 1], np.float32)).all()
    f = AovRef(ref, one).film("albedo")
    b = (f.shape[0] - 8) // 2
    inner = f[b:b + 8, b:b + 8]
    assert np.allclose(inner[:, :, :3] / inner[:, :, 3:], [0.25, 0.5, 0.125], rtol=1e-6)


def test_octant_scene_has_no_negative_normal_component(kz, ref):
    """The precondition of the GPU cross-check (NORMAL film of path_mis == picture of `normals`): over the whole grid, zero samples with a negative component."""
    d = octant_scene(kz)
    assert d.meshes[0]["F"].shape[0] == 200 and d.meshes[0]["N"] is None
    s = AovRef(ref, d).samples(*grid_of(d))
    hit = s[:, 9] == 1.0
    assert hit.sum() > len(hit) // 4 and (~hit).sum() > 0
    assert int((s[:, 5:8] < 0).sum()) == 0
    assert s[hit][:, 5:8].min() >= 0.2


def test_exr_layers_round_trip(kz, tmp_path):
    out = kz.output
    rng = np.random.default_rng(1)
    layers = {"": rng.random((9, 13, 3), dtype=np.float32), "albedo": rng.random((9, 13, 3), dtype=np.float32),
              "normal": rng.random((9, 13, 3), dtype=np.float32) * 2 - 1, "depth": np.repeat(rng.random((9, 13, 1), dtype=np.float32) * 50, 3, axis=2)}
    layers["normal"][0, 0] = (-0.0, np.float32(1e-42), -1.0)          # bit for bit: a negative zero and a subnormal survive
    p = out.save_exr_layers(str(tmp_path / "frame"), layers)
    assert p.endswith(".exr")
    raw = open(p, "rb").read()
    names = [n.decode() for n in re.findall(rb"((?:[a-z]+\.)?[RGBZ])\0\x02\0\0\0", raw)]
    assert names == ["B", "G", "R", "albedo.B", "albedo.G", "albedo.R", "depth.Z", "normal.B", "normal.G", "normal.R"] and names == sorted(names)
    back = out.load_exr_layers(p)
    assert sorted(back) == ["", "albedo", "depth", "normal"]
    for k in ("", "albedo", "normal"):
        assert back[k].tobytes() == layers[k].tobytes(), k
    assert back["depth"].tobytes() == np.ascontiguousarray(layers["depth"][:, :, 0]).tobytes()
    # the plain pair is untouched and reads the beauty layer of a one-layer file
    q = out.save_exr_layers(str(tmp_path / "rgb.exr"), {"": layers[""]})
    assert np.array_equal(out.load_exr(q), layers[""]) and open(q, "rb").read() == out.exr_bytes(layers[""])
