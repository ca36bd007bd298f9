"""ID mattes (include_ext/kazen_mi355x_matte.h) on the GPU: the accumulate kernel on caller-supplied keys against the CPU reference (tests/cpu_ref/kz_matte_ref.cpp),
exactly; rendered tables against the reference's, exactly, whatever the schedule; the other films untouched; lifecycle and refusals. Everything here is integers
(and one IEEE division): every comparison is bit for bit."""
import numpy as np
import pytest

from cpu_refs import MatteRef, lib, ref_accumulate, ref_layer, ref_rank, ref_top
from film_cases import KEYS, NONE, looks_at_the_light, record, with_integrator

pytestmark = pytest.mark.gpu

W, H = 24, 18
SPPS = (1, 4, 64, 130)
SMAX = 130


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lib("matte", tmp_path_factory.mktemp("kzm"))


@pytest.fixture(scope="module")
def dt(kz):
    return np.dtype(kz.abi.MATTE_DTYPE)


def _scenes(kz):
    S = kz.scenes
    return {"cornell": S.cornell_box(W, H, SMAX), "materials": S.materials_scene(W, H, SMAX), "invisible light": looks_at_the_light(kz, W, H, SMAX),
            "invisible light/normals": with_integrator(looks_at_the_light(kz, W, H, SMAX), "normals")}


_tables = {}


def ref_table(ref, dt, kz, name, key, s0, s1, rect=None):
    """The reference's unranked table, computed once per case and shared."""
    k = (name, key, s0, s1, rect)
    if k not in _tables:
        if ("scene", name) not in _tables:
            _tables[("scene", name)] = MatteRef(ref, _scenes(kz)[name], dt)
        _tables[k] = _tables[("scene", name)].table(key, s0, s1, rect=rect)
        _tables[k].setflags(write=False)
    return _tables[k]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the kernel on caller-supplied keys
@pytest.fixture(scope="module")
def surface(gpu_lib, kz):
    """The scene behind the test surface: there for the replica and the 24 x 18 frame only."""
    return kz.Scene(kz.scenes.cornell_box(W, H, 1), device=0)


def pix_list(n, seed=0):
    """n distinct frame pixels in no particular order, x | y << 16."""
    p = np.random.default_rng(seed).permutation(W * H)[:n]
    return ((p % W) | ((p // W) << 16)).astype(np.uint32)


def key_patterns(n_pix, S, seed):
    """The key planes (n_pix, S) of one shape, by name."""
    rng = np.random.default_rng(seed)
    nine = np.array([11, 22, 33, 44, 55, 66, 77, 88, 99], np.uint32)
    top = np.array([0x80000000, 0xFFFFFFFE, 0x80000001, 0xC0000000, 0x7FFFFFFF, 0, 1, 0xFFFF0000, 0x8000FFFF], np.uint32)
    out = {"one key": np.full((n_pix, S), 5, np.uint32), "all misses": np.full((n_pix, S), NONE, np.uint32),
           "nine keys round-robin": np.tile(nine, (n_pix, S // 9 + 1))[:, :S].copy(),
           "top bit": top[rng.integers(0, len(top), (n_pix, S))],
           "random with misses": np.where(rng.random((n_pix, S)) < 0.2, NONE, nine[rng.integers(0, 9, (n_pix, S))]).astype(np.uint32)}
    out["nine keys round-robin"] += (np.arange(n_pix, dtype=np.uint32) * 1000)[:, None]        # (other ids in every pixel)
    last = np.full((n_pix, S), 5, np.uint32)                                                 # a new key in the last lane of a chunk (or the last sample)
    last[:, min(S, 64) - 1] = 6
    out["new key in the last lane of a chunk"] = last
    if S > 64:
        tail = np.full((n_pix, S), 5, np.uint32)                                             # a new key in the first lane of the tail chunk
        tail[:, 64] = 6
        out["new key in the first lane of the tail chunk"] = tail
        fill = np.tile(nine[:6], (n_pix, S // 6 + 1))[:, :S].copy()                              # six slots from the first chunk, the seventh and an overflow from the tail
        fill[:, 64], fill[:, S - 1] = 1234, 4321
        out["slots run out in the tail chunk"] = fill
    return out


def starts(dt, n_pix):
    """Starting records with 0, 3 and 7 slots taken (ids that the patterns use, and ids they do not)."""
    three = record(dt, [5, 77, 0x80000000], [2, 1, 9], other=0, miss=4)
    seven = record(dt, [5, 11, 22, 1011, 0xFFFFFFFE, 6, 3], [1, 2, 3, 4, 5, 6, 7], other=8, miss=9)
    return {"0 slots": None, "3 slots": np.full(n_pix, three, dt), "7 slots": np.full(n_pix, seven, dt)}


SHAPES = [(1, 1), (3, 1), (5, 3), (70, 4), (2, 63), (2, 64), (3, 65), (1, 130)]


@pytest.mark.parametrize("n_pix,S", SHAPES)
def test_accumulate_items_equals_the_reference(surface, ref, dt, n_pix, S):
    """Every key pattern x every starting record, through the kernel a render picks for S - and S = 64 (where the two forms meet) and every other shape through
    both forms, which must give the same bits."""
    pl = pix_list(n_pix, seed=S)
    ran = 0
    for sname, start in starts(dt, n_pix).items():
        for pname, keys in key_patterns(n_pix, S, seed=7 * S + n_pix).items():
            want = ref_accumulate(ref, dt, keys, start)
            assert int(want["count"].astype(np.uint64).sum() + want["other"].sum() + want["miss"].sum()) == n_pix * S + (0 if start is None else int(start["count"].sum() + start["other"].sum() + start["miss"].sum()))
            for form in (0, 1, 2):
                got = surface.matte_accumulate_items(keys, pl, start, form=form)
                assert same(got, want), (n_pix, S, sname, pname, form, got[0], want[0])
                ran += 1
    assert ran >= 3 * 6 * 3


def test_two_calls_are_one_call(surface, ref, dt):
    rng = np.random.default_rng(5)
    n_pix, b = 6, 130
    keys = np.where(rng.random((n_pix, b)) < 0.1, NONE, rng.integers(0, 12, (n_pix, b)) * 0x11111111).astype(np.uint32)
    pl = pix_list(n_pix, seed=1)
    want = ref_accumulate(ref, dt, keys)
    assert (want["other"] > 0).any() and (want["miss"] > 0).any() and (want["count"][:, 6] > 0).all()
    for form in (0, 1, 2):
        assert same(surface.matte_accumulate_items(keys, pl, form=form), want)
        for a in (1, 63, 64, 65, 129):
            first = surface.matte_accumulate_items(keys[:, :a], pl, form=form)
            assert same(first, ref_accumulate(ref, dt, keys[:, :a]))
            assert same(surface.matte_accumulate_items(keys[:, a:], pl, first, form=form), want), (form, a)


def test_accumulate_items_refusals(surface, kz, dt):
    a = kz.abi

    def refused(fn, code):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == code and "kz_matte_accumulate_items" in str(e.value), str(e.value)
    k = np.zeros((2, 3), np.uint32)
    refused(lambda: surface.matte_accumulate_items(k, [5, 5]), a.KZ_ERR_INVALID_ARG)                      # a pixel twice
    refused(lambda: surface.matte_accumulate_items(k, [5, W]), a.KZ_ERR_INVALID_ARG)                      # x = width
    refused(lambda: surface.matte_accumulate_items(k, [5, H << 16]), a.KZ_ERR_INVALID_ARG)                # y = height
    gap = np.full(2, record(dt, [1, 0, 2], [1, 0, 1]), dt)
    refused(lambda: surface.matte_accumulate_items(k, [5, 6], gap), a.KZ_ERR_INVALID_ARG)                 # a free slot below a taken one
    refused(lambda: surface.matte_accumulate_items(k, [5, 6], np.full(2, record(dt, [NONE], [1]), dt)), a.KZ_ERR_INVALID_ARG)
    # a record that would pass 2^32 - 1 samples
    refused(lambda: surface.matte_accumulate_items(k, [5, 6], np.full(2, record(dt, [1], [0xFFFFFFFF - 2]), dt)), a.KZ_ERR_STATE)
    edge = surface.matte_accumulate_items(np.ones((2, 3), np.uint32), [5, 6], np.full(2, record(dt, [1], [0xFFFFFFFF - 3]), dt))
    assert list(edge["count"][:, 0]) == [0xFFFFFFFF] * 2
    assert surface.mattes() == [] and surface.matte_info() == 0          # the scene's own tables are not touched: there are none


# ---------------------------------------------------------------- rendered tables
def check_tables(sc, ref, dt, kz, name, s0, s1, what, rect=None):
    for key in KEYS:
        want = ref_table(ref, dt, kz, name, key, s0, s1, rect)
        got = sc.matte(key)
        assert same(got, ref_rank(ref, want)), (name, key, what)
    return want


@pytest.mark.parametrize("name", ["cornell", "materials", "invisible light", "invisible light/normals"])
def test_rendered_tables_equal_the_reference(gpu_lib, kz, ref, dt, name):
    sc = kz.Scene(_scenes(kz)[name], device=0)
    sc.set_mattes(KEYS)
    for spp in SPPS:
        sc.render(sample_begin=0, sample_end=spp)
        check_tables(sc, ref, dt, kz, name, 0, spp, spp)
        for key in KEYS:
            want = ref_table(ref, dt, kz, name, key, 0, spp)
            assert np.array_equal(want["count"].sum(axis=2) + want["other"] + want["miss"], np.full((H, W), spp))
            assert same(sc.matte_top(key), ref_top(ref, want)), (name, key, spp)
            ids = np.unique(want["id"][want["count"] > 0])
            for id in list(ids[:3]) + [int(ids.max()) + 1]:
                assert same(sc.matte_layer(key, int(id)), ref_layer(ref, want, int(id))), (name, key, spp, id)
    mesh = ref_table(ref, dt, kz, name, "mesh", 0, SMAX)
    seen = set(np.unique(mesh["id"][mesh["count"] > 0]).tolist())
    light = [m for m, msh in enumerate(sc.desc.meshes) if msh["light"]]
    if name == "invisible light":
        assert light and not (seen & set(light))                      # walked through
    if name == "invisible light/normals":
        assert set(light) <= seen                                      # the light's own mesh appears
    if name in ("cornell", "materials"):
        assert len(seen) >= 4 and (mesh["count"][..., 1] > 0).sum() > 20      # silhouettes: pixels with more than one id


def test_tables_do_not_depend_on_the_schedule(gpu_lib, kz, ref, dt):
    """One table whatever the sample chunking, passes in flight (the ordering hazard: the next pass counts the same pixels on another stream), halves, and the split
    of the sample range over accumulating calls; a static tile set leaves the other pixels zero."""
    name = "materials"
    sc = kz.Scene(_scenes(kz)[name], device=0)
    sc.set_mattes(KEYS)
    for kw in ({"tune": {"sppPerPass": 1}}, {"tune": {"sppPerPass": 50}}, {"passes_in_flight": 2, "pass_items": W * H * 8}, {"pass_halves": 2},
               {"passes_in_flight": 2, "pass_items": W * H * 8, "tune": {"sppPerPass": 3}}):
        sc.render(**kw)
        info = sc.last_pass_info()
        if "passes_in_flight" in kw:
            assert info["passesInFlight"] == 2 and info["passes"] >= 3, info
        if "tune" in kw:
            assert info["sppPerPass"] == kw["tune"]["sppPerPass"] and info["passes"] >= 3, info
        check_tables(sc, ref, dt, kz, name, 0, SMAX, kw)
    for a in (37, 64):
        sc.render(sample_begin=0, sample_end=a)
        check_tables(sc, ref, dt, kz, name, 0, a, ("first call", a))
        sc.render(sample_begin=a, sample_end=SMAX, accumulate=True)
        check_tables(sc, ref, dt, kz, name, 0, SMAX, ("two calls", a))
    rect = (0, 0, W // 2, H)
    sc.render_tiles([rect], device=0, sample_begin=0, sample_end=4, download=False)
    want = check_tables(sc, ref, dt, kz, name, 0, 4, "half the tiles", rect)
    assert not want[:, W // 2:].tobytes().strip(b"\0") and want[:, :W // 2]["count"].any()
    assert not sc.matte("mesh")[:, W // 2:].tobytes().strip(b"\0")


def test_path_mis_without_bounces_still_counts(gpu_lib, kz, ref, dt):
    """maxDepth = 0: the picture is black and the pass would end behind the sample generation - with a key enabled the camera stage runs for the mattes."""
    d = _scenes(kz)["cornell"]
    d.integrator["maxDepth"] = 0
    sc = kz.Scene(d, device=0)
    sc.set_mattes("mesh")
    sc.render(sample_begin=0, sample_end=4)
    assert same(sc.matte("mesh"), ref_rank(ref, ref_table(ref, dt, kz, "cornell", "mesh", 0, 4)))
    assert not sc.film()[..., :3].any()


def test_the_other_films_are_unchanged(gpu_lib, kz):
    d = kz.scenes.materials_scene(W, H, 8)
    aovs = ("albedo", "normal", "depth")
    films = []
    for mask in ((), KEYS):
        sc = kz.Scene(d, device=0)
        sc.set_aovs(aovs)
        sc.set_mattes(mask)
        sc.render()
        sc.render(passes_in_flight=2, pass_items=W * H * 2)
        films.append([sc.film()] + [sc.aov_film(a) for a in aovs])
        assert sc.matte_info() == (2 * 64 * W * H if mask else 0)
    assert films[0][0][..., :3].max() > 0
    for off, on in zip(*films):
        assert np.array_equal(off, on)


# ---------------------------------------------------------------- lifecycle, refusals
def test_lifecycle(gpu_lib, kz, ref, dt):
    a = kz.abi
    name = "cornell"
    sc = kz.Scene(_scenes(kz)[name], device=0)

    def refused(fn, code, *words):
        with pytest.raises(a.KzError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    sc.render(sample_begin=0, sample_end=1)
    assert sc.matte_info() == 0                                        # mask 0: nothing allocated
    sc.set_mattes("mesh")
    assert sc.matte_info() == 0
    refused(lambda: sc.matte("mesh"), a.KZ_ERR_STATE, "kz_matte_download")      # enabled, nothing rendered with it
    refused(lambda: sc.matte_top("mesh"), a.KZ_ERR_STATE, "kz_matte_top")
    refused(lambda: sc.matte("bsdf"), a.KZ_ERR_INVALID_ARG)
    sc.render(sample_begin=0, sample_end=4)
    assert sc.matte_info() == 64 * W * H
    check = lambda key, s0, s1, what: same(sc.matte(key), ref_rank(ref, ref_table(ref, dt, kz, name, key, s0, s1)))
    assert check("mesh", 0, 4, "first")
    # a key that enters starts at zero and covers the samples rendered from then on; the other keeps counting
    sc.set_mattes(KEYS)
    assert sc.matte_info() == 64 * W * H
    refused(lambda: sc.matte("bsdf"), a.KZ_ERR_STATE)
    sc.render(sample_begin=4, sample_end=8, accumulate=True)
    assert sc.matte_info() == 2 * 64 * W * H
    assert check("mesh", 0, 8, "accumulated") and check("bsdf", 4, 8, "entered late")
    # the edits leave the tables alone
    before = [sc.matte(k) for k in KEYS]
    M = np.eye(4, dtype=np.float32)
    M[0, 3] = 0.05
    sc.set_transforms({2: M})
    sc.set_camera(dict(sc.desc.camera, fov=sc.desc.camera["fov"] + 1.0))
    assert all(same(sc.matte(k), b) for k, b in zip(KEYS, before))
    sc.set_transforms({2: np.eye(4, dtype=np.float32)})
    sc.set_camera(dict(sc.desc.camera, fov=sc.desc.camera["fov"] - 1.0))
    # a render that does not accumulate clears; so does kz_film_clear
    sc.render(sample_begin=0, sample_end=4)
    assert check("mesh", 0, 4, "cleared by the render") and check("bsdf", 0, 4, "cleared by the render")
    sc.film_clear()
    for k in KEYS:
        assert not sc.matte(k).tobytes().strip(b"\0")
        assert (sc.matte_top(k) == NONE).all() and not sc.matte_layer(k, 0).any()
    sc.render(sample_begin=0, sample_end=4, accumulate=True)
    assert check("mesh", 0, 4, "after the clear")
    # a key that leaves the mask loses its table
    sc.set_mattes("bsdf")
    assert sc.matte_info() == 64 * W * H
    refused(lambda: sc.matte("mesh"), a.KZ_ERR_INVALID_ARG)
    assert check("bsdf", 0, 4, "kept")
    sc.set_mattes("mesh")
    refused(lambda: sc.matte("mesh"), a.KZ_ERR_STATE)                  # back, and empty until the next render
    assert sc.matte_info() == 0
    # refused while the mask is non-zero, by name
    tiles = [(0, 0, W, H)]
    counter = np.zeros(2, np.uint32)
    refused(lambda: sc.render(pipeline=1), a.KZ_ERR_UNSUPPORTED, "kz_render", "pipeline = 1", "mattes")
    refused(lambda: sc.render_multi([0]), a.KZ_ERR_UNSUPPORTED, "kz_render_multi", "mattes")
    refused(lambda: sc.render_dealt(tiles, counter, device=0), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "KzTileDealer", "mattes")
    refused(lambda: sc.render_tiles(tiles, device=0, packed=True), a.KZ_ERR_UNSUPPORTED, "kz_render_tiles", "packedOutput", "mattes")
    refused(lambda: sc.film_tiles(tiles, device=0), a.KZ_ERR_UNSUPPORTED, "kz_film_download_tiles", "mattes")
    refused(lambda: sc.set_mattes(4), a.KZ_ERR_INVALID_ARG, "kz_scene_set_mattes")
    with pytest.raises(a.KzError):
        sc.matte_layer("mesh", NONE)
    # with the mask 0 they all work again
    sc.set_mattes(())
    sc.render(pipeline=1, sample_begin=0, sample_end=1)
    assert sc.film_tiles(tiles, device=0).size > 0 and sc.matte_info() == 0
