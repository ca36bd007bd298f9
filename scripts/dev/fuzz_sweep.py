"""A wider randomized parity sweep than the CI suite carries (tests/film_cases.py _fuzz_scene, other seeds): HIP film vs the CPU oracle, megakernel == wavefront bit
for bit, counting == product kernels, one stream / shadow rays beside / pass halves, tile sets / sample ranges / dealer == one shot. Run through gpurun when GPU minutes are to spare:
    python scripts/dev/fuzz_sweep.py [first_seed] [n_scenes] [--rich]"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
kz = importlib.import_module("nano-kazen_amd")
import oracle as O
from checks import tie_bracket
from film_cases import _fuzz_scene

rich = "--rich" in sys.argv                 # bicubic lookups and environment backgrounds on top (tests/film_cases.py _fuzz_scene)
argv = [a for a in sys.argv if a != "--rich"]
first, n = (int(argv[1]) if len(argv) > 1 else 5000), (int(argv[2]) if len(argv) > 2 else 60)
bad = []
t0 = time.time()
for seed in range(first, first + n):
    d = _fuzz_scene(kz.scenes, seed, rich)
    sc = kz.Scene(d, device=0)
    sc.render()
    film = sc.film()
    ora = O.OracleScene(d)
    fc = ora.render(threads=0)
    err = float(np.sqrt(np.mean((sc.rgb(film) - ora.rgb(fc)) ** 2)))
    scale = max(1.0, float(np.abs(ora.rgb(fc)).max()))
    ok = err < 1e-3 * scale and np.allclose(film[..., 3], fc[..., 3], rtol=1e-4, atol=1e-5)
    bits = np.array_equal(film, ora.render_canonical(threads=0))           # round 6: the whole film in the build's fixed summation order (ties of the reference's shadow loop aside)
    note = ""
    if not ok and np.allclose(film[..., 3], fc[..., 3], rtol=1e-4, atol=1e-5):
        # the reference's shadow tie (tests/checks.py tie_bracket): inside the oracle's bracket is parity
        outside, n_tie = tie_bracket(ora, sc, d)
        ok = outside < 1e-4 and n_tie > 0
        note = " [literal L2 fails; %d tie samples, share of samples outside the tie bracket %.1e]" % (n_tie, outside)
    sc.render(pipeline=1)
    ok_mega = np.array_equal(sc.film(), film)
    sc.set_stats(True); sc.render(); ok_stats = np.array_equal(sc.film(), film); sc.set_stats(False)
    # how a pass runs (the first render above: shadow rays beside the closest-hit rays, the default of a small pass): one stream; two halves side by side
    sc.render(shadow_beside=1, pass_halves=1); ok_modes = np.array_equal(sc.film(), film)
    sc.render(shadow_beside=seed % 3, pass_halves=2); ok_modes = ok_modes and np.array_equal(sc.film(), film)
    w, h = d.camera["width"], d.camera["height"]
    tiles = kz.shard.deal_tiles(w, h, 1, 0, 32)
    counter = np.zeros(1, np.uint32)
    took = sc.render_dealt(tiles, counter, takers=1, batch_tiles=2, pass_items=4096)
    ok_deal = took == tiles and np.array_equal(sc.film(), film)          # (round 6: the film does not depend on the cut - bit for bit)
    half = sc.sample_count // 2
    if half > 0:
        sc.render(0, half); sc.render(half, sc.sample_count, accumulate=True)
        ok_rng = np.array_equal(sc.film(), film)
    else:
        ok_rng = True
    # the packed rects of a 64-px tiling merged in tile order ARE the film (the resolve's canonical grid)
    t64 = kz.shard.deal_tiles(w, h, 1, 0, 64)
    sc.render()
    ok_rng = ok_rng and np.array_equal(sc.merge_tiles(sc.empty_film(), t64, sc.film_tiles(t64)), film)
    line = "seed %d %s %dx%dx%d depth %d tris %d: L2 %.2e (scale %.1f) film-bits %s %s" % (seed, d.sampler["type"], w, h, sc.sample_count, d.integrator["maxDepth"], d.n_tris(), err, scale, "equal" if bits else "DIFFER",
            ("ok" + note) if (ok and ok_mega and ok_stats and ok_deal and ok_rng and ok_modes) else "FAIL oracle=%s mega=%s stats=%s deal=%s ranges=%s modes=%s%s" % (ok, ok_mega, ok_stats, ok_deal, ok_rng, ok_modes, note))
    print(line, flush=True)
    if "FAIL" in line:
        bad.append(seed)
    sc.close()
print("done: %d scenes in %.0f s, failures: %s" % (n, time.time() - t0, bad))
sys.exit(1 if bad else 0)
