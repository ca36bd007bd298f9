"""ID mattes (include_ext/kazen_mi355x_matte.h) without a GPU: the header against the library's exports, the record's size, the refusals that need no device, and the
test-only CPU reference (tests/cpu_ref/kz_matte_ref.cpp) the GPU tests compare against - its rule on hand-written sequences with the expected records written out,
its tables of two scenes against a numpy restatement of the rule over its own per-sample keys, and its rank, layer and top against numpy."""
import ctypes as C
import re

import numpy as np
import pytest

from checks import c_layout, header_surface, refused
from cpu_refs import AovRef, MatteRef, lib, ref_accumulate, ref_layer, ref_rank, ref_top
from film_cases import KEYS, NONE, grid_of, looks_at_the_light, record, with_integrator

W, H, SPP = 24, 18, 16


def np_rule(keys, start=None):
    """The rule of the header restated over one pixel's key sequence (NONE = a miss): dict id -> count in slot order, other, miss."""
    slots, other, miss = ({}, 0, 0) if start is None else start
    for k in keys:
        k = int(k)
        if k == NONE:
            miss += 1
        elif k in slots:
            slots[k] += 1
        elif len(slots) < 7:
            slots[k] = 1
        else:
            other += 1
    return slots, other, miss


def np_record(dtype, state):
    slots, other, miss = state
    return record(dtype, list(slots.keys()), list(slots.values()), other, miss)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("matte", tmp_path_factory.mktemp("kzm"))


# ---------------------------------------------------------------- ABI
def test_header_declarations_are_exported(kz):
    a = kz.abi
    # a surface of its own: nothing added to the other lists or to the other headers (the header lives beside include/, whose set of files an older test pins)
    _, src = header_surface(kz, "include_ext/kazen_mi355x_matte.h", a.MATTE_EXPORTS, 8,
                            [a.EXPORTS, a.PRODUCT_EXPORTS, a.EDIT_EXPORTS, a.AOV_EXPORTS, a.DENOISE_EXPORTS, a.VARIANCE_EXPORTS, a.TEMPORAL_EXPORTS, a.MOTION_EXPORTS, a.RESPONSIVE_EXPORTS,
                             a.DEV_ONLY_EXPORTS], ["include"], ["matte"], resolve=False)
    consts = {n: int(re.search(r"#define %s\s+(0x[0-9A-Fa-f]+|\d+)u?" % n, src).group(1), 0) for n in ("KZ_MATTE_MESH", "KZ_MATTE_BSDF", "KZ_MATTE_ALL", "KZ_MATTE_SLOTS", "KZ_MATTE_NONE")}
    assert consts == {"KZ_MATTE_MESH": a.KZ_MATTE_MESH, "KZ_MATTE_BSDF": a.KZ_MATTE_BSDF, "KZ_MATTE_ALL": a.KZ_MATTE_ALL, "KZ_MATTE_SLOTS": a.KZ_MATTE_SLOTS, "KZ_MATTE_NONE": a.KZ_MATTE_NONE}
    assert (a.KZ_MATTE_MESH, a.KZ_MATTE_BSDF, a.KZ_MATTE_NONE) == (1, 2, a.KZ_MOTION_MISS)


def test_texel_is_64_bytes_as_gcc_sees_it(kz, tmp_path):
    a = kz.abi
    assert c_layout(tmp_path, "kazen_mi355x_matte.h", ["sizeof(KzMatteTexel)", "offsetof(KzMatteTexel, count)", "offsetof(KzMatteTexel, other)", "offsetof(KzMatteTexel, miss)"],
                    include="include_ext") == ["64", "28", "56", "60"]
    assert C.sizeof(a.KzMatteTexel) == 64 and np.dtype(a.MATTE_DTYPE).itemsize == 64
    assert (a.KzMatteTexel.count.offset, a.KzMatteTexel.other.offset, a.KzMatteTexel.miss.offset) == (28, 56, 60)
    d = np.dtype(a.MATTE_DTYPE)
    assert (d.fields["count"][1], d.fields["other"][1], d.fields["miss"][1]) == (28, 56, 60)


def test_refusals_without_a_device(kz):
    a = kz.abi
    sc = kz.Scene(kz.scenes.cornell_box(16, 16, 2))
    assert sc.mattes() == []
    for bad in (4, 7, 1 << 31):
        refused(kz, lambda: sc.set_mattes(bad), a.KZ_ERR_INVALID_ARG, "kz_scene_set_mattes")
    assert sc.mattes() == []
    sc.set_mattes(["mesh", "bsdf"])                                    # (a scene on no device: the mask alone)
    assert sc.mattes() == ["mesh", "bsdf"]
    sc.set_mattes("bsdf")
    assert sc.mattes() == ["bsdf"]
    with pytest.raises(ValueError):
        sc.set_mattes(["object"])
    # exactly one enabled bit
    for bad in (0, 1, 3, 4):
        refused(kz, lambda: sc.matte(bad), a.KZ_ERR_INVALID_ARG, "kz_matte_download")
        refused(kz, lambda: sc.matte_layer(bad, 0), a.KZ_ERR_INVALID_ARG, "kz_matte_layer")
        refused(kz, lambda: sc.matte_top(bad), a.KZ_ERR_INVALID_ARG, "kz_matte_top")
    refused(kz, lambda: sc.matte_layer("bsdf", NONE), a.KZ_ERR_INVALID_ARG, "kz_matte_layer")
    refused(kz, lambda: sc.matte("bsdf"), a.KZ_ERR_STATE)             # one enabled bit, but no device
    tiles = [(0, 0, 16, 16)]
    counter = np.zeros(2, np.uint32)
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "pipeline = 1", "mattes")
    refused(kz, lambda: sc.render_multi([0]), a.KZ_ERR_UNSUPPORTED, "kz_render_multi", "mattes")
    refused(kz, lambda: sc.render_dealt(tiles, counter, device=0), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "KzTileDealer", "mattes")
    refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "packedOutput", "mattes")
    refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_UNSUPPORTED, "kz_film_download_tiles", "mattes")
    # the test surface checks its arguments before it looks for a device
    k = np.zeros((2, 3), np.uint32)
    refused(kz, lambda: sc.matte_accumulate_items(k, [0, 1], form=3), a.KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items")
    refused(kz, lambda: sc.matte_accumulate_items(np.zeros((2, 0), np.uint32), [0, 1]), a.KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items")
    # with the mask 0 the same calls get as far as they got before: the scene is on no device
    sc.set_mattes(())
    assert sc.mattes() == []
    refused(kz, lambda: sc.render(pipeline=1), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_STATE)
    refused(kz, lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_STATE)


# ---------------------------------------------------------------- the rule, on hand-written sequences
def test_the_rule_on_hand_written_sequences(kz, ref):
    dt = np.dtype(kz.abi.MATTE_DTYPE)
    acc = lambda keys, start=None: ref_accumulate(ref, dt, np.array([keys], np.uint32), None if start is None else np.array([start], dt))[0]
    # nine distinct keys round-robin over 27 samples: the slots are the first seven in order, 3 each, and the other two keys' 6 samples are `other`
    nine = [10, 20, 30, 40, 50, 60, 70, 80, 90]
    assert acc(nine * 3) == record(dt, nine[:7], [3] * 7, other=6)
    # a key first seen after the slots are full never gets one, however often it comes; keys that have a slot keep counting
    assert acc([1, 2, 3, 4, 5, 6, 7, 99, 99, 99, 99, 1, 99, 7, 7]) == record(dt, [1, 2, 3, 4, 5, 6, 7], [2, 1, 1, 1, 1, 1, 3], other=5)
    # all misses
    assert acc([NONE] * 5) == record(dt, miss=5)
    # slot order is first-seen order, not id order; the id 0 is an id like any other; ids with the top bit set
    assert acc([5, 0, 5, 0x80000001, 0, 0, NONE]) == record(dt, [5, 0, 0x80000001], [2, 3, 1], miss=1)
    # a non-empty starting record: its keys keep their slots, a new key takes the lowest free one, the totals add up
    start = record(dt, [7, 3, 9], [4, 1, 2], other=0, miss=6)
    assert acc([9, 11, NONE, 3, 11, 12], start) == record(dt, [7, 3, 9, 11, 12], [4, 2, 3, 2, 1], other=0, miss=7)
    # a full starting record
    full = record(dt, [1, 2, 3, 4, 5, 6, 7], [1] * 7, other=2, miss=0)
    assert acc([8, 7, 1, 8], full) == record(dt, [1, 2, 3, 4, 5, 6, 7], [2, 1, 1, 1, 1, 1, 2], other=4)
    # two calls over [0, a) and [a, b) are one call over [0, b)
    rng = np.random.default_rng(3)
    seq = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, NONE], np.uint32), 200)
    for a_ in (0, 1, 63, 64, 199):
        assert acc(seq[a_:], acc(seq[:a_])) == acc(seq) == np_record(dt, np_rule(seq))


# ---------------------------------------------------------------- the reference's tables
@pytest.fixture(scope="module")
def ref_scenes(kz, ref):
    dt = np.dtype(kz.abi.MATTE_DTYPE)
    out = {}
    for name, d in (("cornell", kz.scenes.cornell_box(W, H, SPP)), ("invisible light", looks_at_the_light(kz))):
        r = MatteRef(ref, d, dt)
        pxy, idx = grid_of(d)
        out[name] = (d, r, pxy, idx, r.samples(pxy, idx))
    return out


@pytest.mark.parametrize("name", ["cornell", "invisible light"])
def test_reference_tables_are_the_rule_over_its_own_samples(kz, ref, ref_scenes, name):
    dt = np.dtype(kz.abi.MATTE_DTYPE)
    d, r, pxy, idx, s = ref_scenes[name]
    assert set(np.unique(s[:, 2])) <= {0, 1} and s[:, 2].any()
    per_pixel = s.reshape(H, W, SPP, 3)
    for col, key in enumerate(KEYS):
        t = r.table(key, 0, SPP)
        seq = np.where(per_pixel[..., 2] == 1, per_pixel[..., col], NONE)
        want = np.array([[np_record(dt, np_rule(seq[y, x])) for x in range(W)] for y in range(H)], dt)
        assert np.array_equal(t, want), key                            # exact: integers, no left-out share
        # per pixel the counts + other + miss are the samples rendered
        assert np.array_equal(t["count"].sum(axis=2) + t["other"] + t["miss"], np.full((H, W), SPP))
        assert int(t["miss"].sum()) == int((s[:, 2] == 0).sum())
        # the sample range split over two calls, and a rectangle of the frame with the rest untouched
        assert np.array_equal(r.table(key, 5, SPP, start=r.table(key, 0, 5)), t)
        part = r.table(key, 0, SPP, rect=(8, 0, 16, 9))
        assert np.array_equal(part[:9, 8:], t[:9, 8:]) and not part[9:].tobytes().strip(b"\0") and not part[:, :8].tobytes().strip(b"\0")
    if name == "cornell":                                              # (the other view shows the ceiling behind the light and nothing else)
        assert len(np.unique(s[s[:, 2] == 1][:, 0])) >= 4 and len(np.unique(s[s[:, 2] == 1][:, 1])) >= 3


@pytest.mark.parametrize("name", ["cornell", "invisible light"])
def test_a_samples_hit_is_the_feature_films_hit(kz, ref, ref_scenes, tmp_path_factory, name):
    d, r, pxy, idx, s = ref_scenes[name]
    a = AovRef(lib("aov", tmp_path_factory.mktemp("kza")), d).samples(pxy, idx)
    assert np.array_equal(s[:, 2], a[:, 9].astype(np.uint32))


def test_the_light_shows_to_normals_and_not_to_path_mis(kz, ref, ref_scenes):
    """The invisible-light view: path_mis walks through the ceiling light, `normals` keeps its hit - the light's own mesh is in one table and not in the other."""
    dt = np.dtype(kz.abi.MATTE_DTYPE)
    d, r, pxy, idx, s = ref_scenes["invisible light"]
    light = [m for m, mesh in enumerate(d.meshes) if mesh["light"]]
    assert len(light) == 1
    sn = MatteRef(ref, with_integrator(d, "normals"), dt).samples(pxy, idx)
    assert not (s[s[:, 2] == 1][:, 0] == light[0]).any() and (sn[sn[:, 2] == 1][:, 0] == light[0]).sum() > len(idx) // 20


# ---------------------------------------------------------------- rank, layer, top
def _np_rank(t):
    out = t.copy()
    for i in np.ndindex(t.shape):
        e = sorted(zip(t[i]["count"].tolist(), t[i]["id"].tolist()), key=lambda ci: (-ci[0], ci[1]))
        out[i]["count"], out[i]["id"] = [c for c, _ in e], [d for _, d in e]
    return out


def random_tables(dtype, n, seed):
    """Records as the rule makes them: 0 .. 7 slots taken from 0 upwards, distinct ids (some with the top bit set), counts with many ties, free slots all zero."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype)
    for i in range(n):
        k = int(rng.integers(0, 8))
        t[i]["id"][:k] = rng.choice(np.array([0, 1, 2, 3, 5, 8, 13, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], np.uint32), k, replace=False)
        t[i]["count"][:k] = rng.integers(1, 4, k) if i % 3 else rng.integers(1, 1 << 29, k)
        t[i]["other"] = rng.integers(0, 3) if k == 7 else 0
        t[i]["miss"] = rng.integers(0, 5) if i % 4 else 0
    return t


def test_rank_layer_top_against_numpy(kz, ref):
    dt = np.dtype(kz.abi.MATTE_DTYPE)
    t = random_tables(dt, 400, 11)
    t[0] = record(dt)                                                  # no samples at all
    t[1] = record(dt, miss=3)                                          # misses alone
    t[2] = record(dt, [9, 4], [2, 2], miss=2)                          # a tie between ids, and the misses reach the best count
    t[3] = record(dt, [9, 4], [2, 2], miss=1)
    ranked = ref_rank(ref, t)
    assert np.array_equal(ranked, _np_rank(t))
    assert np.array_equal(ranked["other"], t["other"]) and np.array_equal(ranked["miss"], t["miss"])
    assert (np.diff(ranked["count"].astype(np.int64), axis=1) <= 0).all()
    assert list(ranked[2]["id"][:2]) == [4, 9]
    total = t["count"].astype(np.uint64).sum(axis=1) + t["other"] + t["miss"]
    assert total.max() < 2 ** 32
    for id in (0, 5, 0x80000000, 77):
        cnt = np.where((t["id"] == id) & (t["count"] > 0), t["count"], 0).sum(axis=1).astype(np.uint32)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(total > 0, cnt.astype(np.float32) / total.astype(np.uint32).astype(np.float32), np.float32(0)).astype(np.float32)
        got = ref_layer(ref, t, id)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), id
    top = ref_top(ref, t)
    want = np.where((ranked["count"][:, 0] > 0) & (t["miss"] < ranked["count"][:, 0]), ranked["id"][:, 0], NONE).astype(np.uint32)
    assert np.array_equal(top, want)
    assert top[0] == NONE and top[1] == NONE and top[2] == NONE and top[3] == 4
    # rank, layer and top do not depend on the slot order
    assert np.array_equal(ref_top(ref, ranked), top) and np.array_equal(ref_layer(ref, ranked, 5), ref_layer(ref, t, 5))
