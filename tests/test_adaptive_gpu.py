"""-m gpu: adaptive sampling (include_ext/kazen_mi355x_adaptive.h) on the MI355X. The classification stage has the CPU reference's records
(tests/cpu_ref/kz_adaptive_ref.cpp), integer for integer, on crafted films that hold the corners of the pixel and block tests; a call in which no block converges
leaves the films of a plain render, one in which every block converges at once those of a render of the first round; a call in which the blocks stop at different
counts leaves the films, records, counts and summary of the reference's whole call and of a host-driven loop over the existing API, under several pass schedules.
Comparisons are array_equal / same_bits, never a tolerance."""
import numpy as np
import pytest

import adaptive_refs as A
from checks import differing, refused

pytestmark = pytest.mark.gpu

# Picked by running kzad_adaptive on the CPU alone: at this threshold the reference gives cornell_box(72, 40, 64) in blocks of 8, under the independent and under the
# stratified sampler, at least three distinct per-block counts, at least one block at the cap and at least one at the minimum (the test asserts the three).
MIXED_THRESHOLD = 0.2
W, H, SPP = 72, 40, 64


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return A.lib(tmp_path_factory.mktemp("kzad"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return A.aov_lib(tmp_path_factory.mktemp("kzada"))


# ---------------------------------------------------------------- 1. the classification kernel on caller films
@pytest.mark.parametrize("frame", [(40, 24), (72, 40)])
@pytest.mark.parametrize("block", [8, 16, 32, 64])
def test_classification_equals_the_reference(gpu_lib, kz, ref, frame, block):
    """Edge blocks are partial at every size; the 64 block takes 64 steps of a wave. Thresholds 0.05 and 1e-18 (v and the bound subnormal), outlierPermille 0 and 500
    with noisy counts on both sides of the bound, a cap and none, n = 0 (skipped) and 65536 among the blocks' counts."""
    w, h = frame
    seen = set()
    for border in (0, 2):
        for threshold in (0.05, 1e-18):
            film, moment, ns = A.crafted_films(w, h, border, block, threshold, seed=block + border)
            assert ns.size < 6 or (0 in ns and 65536 in ns)
            for permille in (0, 500):
                for cap in (0, 16):
                    kw = dict(block=block, outlier_permille=permille, max_samples=cap)
                    want = A.ref_classify(ref, film, moment, ns, kz.adaptive_opts(threshold, **kw), border)
                    got = kz.adaptive_classify_films(film, moment, ns, threshold, border=border, **kw)
                    assert np.array_equal(got, want), (border, threshold, permille, cap, got[got != want][:4], want[got != want][:4])
                    seen |= set(got["flags"].tolist())
    assert want["noisy"].max() > 0
    if block <= 16:
        assert seen == {0, A.CONVERGED, A.AT_CAP}


# ---------------------------------------------------------------- 2. every block runs to the cap
@pytest.mark.parametrize("scene", ["cornell", "materials"])
def test_nothing_converges_equals_a_plain_render(gpu_lib, kz, ref, scene):
    desc = kz.scenes.cornell_box(W, H, SPP, sampler="pmj02bn") if scene == "cornell" else kz.scenes.materials_scene(64, 40, 32)
    w, h, spp = desc.camera["width"], desc.camera["height"], desc.sampler["sampleCount"]
    plain = kz.Scene(desc, device=0)
    plain.set_variance(True)
    plain.render()
    sc = kz.Scene(desc, device=0)
    sc.set_variance(True)
    info = sc.render_adaptive(1e-9)
    blocks = ((w + 15) // 16) * ((h + 15) // 16)
    assert info == dict(rounds=len(A.py_schedule(spp)), blocks=blocks, converged=0, atCap=blocks, samples=w * h * spp, bytes=17 * blocks)
    rec = sc.adaptive_blocks()
    assert (rec["samples"] == spp).all() and (rec["flags"] == A.AT_CAP).all() and (rec["noisy"] > 0).all() and (rec["noisy"] <= rec["valid"]).all()
    r = A.AdaptiveRef(ref, desc)
    for got, same, want in ((sc.film(), plain.film(), r.film()), (sc.moment_film(), plain.moment_film(), r.moment_film())):
        assert np.array_equal(got, same), differing(got, same)
        assert np.array_equal(got, want), differing(got, want)
    assert sc.variance_info()[1] == spp


# ---------------------------------------------------------------- 3. every block stops at the minimum
def test_everything_converges_at_the_minimum(gpu_lib, kz):
    desc = kz.scenes.cornell_box(W, H, SPP, sampler="pmj02bn")
    plain = kz.Scene(desc, device=0)
    plain.set_variance(True)
    sc = kz.Scene(desc, device=0)
    sc.set_variance(True)
    for kw, n0 in ((dict(), 16), (dict(min_samples=5, block=32), 5)):
        info = sc.render_adaptive(1e9, **kw)
        plain.render(sample_end=n0)
        assert np.array_equal(sc.film(), plain.film()) and np.array_equal(sc.moment_film(), plain.moment_film())
        rec = sc.adaptive_blocks()
        assert (rec["flags"] == A.CONVERGED).all() and (rec["samples"] == n0).all() and (rec["noisy"] == 0).all() and rec["valid"].sum() == W * H
        assert info["rounds"] == 1 and info["converged"] == info["blocks"] == rec.size and info["atCap"] == 0 and info["samples"] == W * H * n0
        assert (sc.adaptive_counts() == n0).all() and sc.variance_info()[1] == n0


# ---------------------------------------------------------------- 4. blocks stop at different counts
def host_driven(kz, ref, sc, opts):
    """The rule over the existing API: render a round, download the two films, classify with the reference, build the tiles with the restatement, render the next
    round on them with accumulate. Returns the records and the rounds."""
    e = opts.block or 16
    nb = ((sc.width + e - 1) // e) * ((sc.height + e - 1) // e)
    rec, active = np.zeros(nb, A.BLOCK_DTYPE), np.ones(nb, bool)
    bounds, prev, rounds = A.py_schedule(sc.sample_count, opts.minSamples, opts.maxSamples, opts.step), 0, 0
    for n in bounds:
        if rounds == 0:
            sc.render(sample_begin=0, sample_end=n)
        else:
            sc.render(sample_begin=prev, sample_end=n, tiles=A.py_tiles(sc.width, sc.height, e, active), accumulate=True)
        new = A.ref_classify(ref, sc.film(), sc.moment_film(), np.where(active, n, 0), opts, sc.border)
        rec[active] = new[active]
        active &= rec["flags"] == 0
        rounds, prev = rounds + 1, n
        if not active.any():
            break
    return rec, rounds


@pytest.mark.parametrize("sampler", ["independent", "stratified"])
def test_mixed_counts_equal_the_reference_and_a_host_driven_loop(gpu_lib, kz, ref, aref, sampler):
    desc = kz.scenes.cornell_box(W, H, SPP, sampler=sampler)
    rule = dict(block=8, max_samples=SPP)
    opts = kz.adaptive_opts(MIXED_THRESHOLD, **rule)
    film, moment, rec, counts, rounds = A.AdaptiveRef(ref, desc).adaptive(opts)
    # the reference alone: the case is a mixed one
    assert len(np.unique(rec["samples"])) >= 3 and (rec["flags"] == A.AT_CAP).any() and (rec["samples"] == 16).any()
    assert ((rec["samples"] == SPP) | (rec["flags"] == A.CONVERGED)).all()
    albedo = A.ref_aov_counts(aref, desc, "albedo", counts)
    want_info = dict(rounds=rounds, blocks=rec.size, converged=int((rec["flags"] == A.CONVERGED).sum()), atCap=int((rec["flags"] == A.AT_CAP).sum()),
                     samples=int(counts.sum(dtype=np.uint64)), bytes=17 * rec.size)

    def check(sc, info, what):
        for name, got, want in (("picture", sc.film(), film), ("moment", sc.moment_film(), moment), ("albedo", sc.aov_film("albedo"), albedo)):
            assert np.array_equal(got, want), (what, name, differing(got, want))
        assert np.array_equal(sc.adaptive_blocks(), rec), what
        assert np.array_equal(sc.adaptive_counts(), counts), what
        assert info == want_info and sc.adaptive_info() == want_info, (what, info, want_info)
        assert sc.variance_info()[1] == rec["samples"].max()

    sc = kz.Scene(desc, device=0)
    sc.set_variance(True)
    sc.set_aovs(["albedo"])
    check(sc, sc.render_adaptive(MIXED_THRESHOLD, **rule), "default schedule")
    # several passes per round, and two of them in flight
    info = sc.render_adaptive(MIXED_THRESHOLD, pass_items=512 * 4, tune={"sppPerPass": 4}, **rule)
    assert sc.last_pass_info()["passes"] >= 2
    check(sc, info, "small passes")
    info = sc.render_adaptive(MIXED_THRESHOLD, pass_items=512 * 4, passes_in_flight=2, **rule)
    assert sc.last_pass_info()["passesInFlight"] == 2
    check(sc, info, "two passes in flight")
    # the same rule driven from the host over the existing API
    host = kz.Scene(desc, device=0)
    host.set_variance(True)
    host.set_aovs(["albedo"])
    hrec, hrounds = host_driven(kz, ref, host, opts)
    assert np.array_equal(hrec, rec) and hrounds == rounds
    for name, got, want in (("picture", host.film(), film), ("moment", host.moment_film(), moment), ("albedo", host.aov_film("albedo"), albedo)):
        assert np.array_equal(got, want), ("host-driven", name, differing(got, want))


# ---------------------------------------------------------------- 5. lifecycle
def test_lifecycle_of_the_records(gpu_lib, kz):
    a = kz.abi
    desc = kz.scenes.cornell_box(W, H, SPP)
    sc = kz.Scene(desc, device=0)
    reads = (sc.adaptive_info, sc.adaptive_blocks, sc.adaptive_counts, sc.adaptive_stage_ms)
    refused(kz, lambda: sc.render_adaptive(0.2), a.KZ_ERR_STATE, "kz_scene_set_variance(scene, 1) first")
    sc.set_variance(True)
    for read in reads:
        refused(kz, read, a.KZ_ERR_STATE)
    info = sc.render_adaptive(MIXED_THRESHOLD, block=8)
    counts = sc.adaptive_counts()
    assert len(sc.adaptive_stage_ms()) == 3 and min(sc.adaptive_stage_ms()) > 0
    assert info["samples"] == int(counts.sum(dtype=np.uint64)) and info == sc.adaptive_info() and info["blocks"] == 45 and info["bytes"] == 17 * 45
    assert sc.variance_info()[1] == counts.max() == sc.adaptive_blocks()["samples"].max()
    assert np.array_equal(np.repeat(np.repeat(sc.adaptive_blocks()["samples"].reshape(5, 9), 8, 0), 8, 1), counts)
    # a second call with other options rewrites them
    info2 = sc.render_adaptive(MIXED_THRESHOLD, block=32, min_samples=4, step=20, max_samples=44)
    assert info2["blocks"] == 6 and info2["bytes"] == 17 * 6 and sc.adaptive_blocks().size == 6 and set(np.unique(sc.adaptive_counts())) <= {4, 24, 44}
    assert info2["samples"] == int(sc.adaptive_counts().sum(dtype=np.uint64)) and sc.variance_info()[1] == sc.adaptive_counts().max()
    # an accumulating render leaves them, a clear and a plain render take them
    sc.render(sample_begin=44, sample_end=48, accumulate=True)
    assert sc.adaptive_info() == info2
    sc.film_clear()
    for read in reads:
        refused(kz, read, a.KZ_ERR_STATE)
    sc.render_adaptive(MIXED_THRESHOLD, block=8)
    assert sc.adaptive_info() == info
    sc.render()
    for read in reads:
        refused(kz, read, a.KZ_ERR_STATE)
    refused(kz, lambda: sc.adaptive_blocks(device=3), a.KZ_ERR_STATE)
    sc.set_variance(False)
    refused(kz, lambda: sc.render_adaptive(MIXED_THRESHOLD), a.KZ_ERR_STATE, "kz_scene_set_variance(scene, 1) first")
