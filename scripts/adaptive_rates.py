"""What adaptive sampling (include_ext/kazen_mi355x_adaptive.h) costs and what it buys, in ONE process on one MI355X. One JSON line on stdout (and in --out).
 (a) round overhead: C4 at 1920 x 1080, cap 256, the default doubling from 16 (rounds end at 16, 32, 64, 128, 256), a threshold that converges nothing, against a
     plain kz_render of the same 256 samples - three alternating runs each, host clock around synchronised calls - and, with --parent-lib (a build of the parent
     commit: scripts/build_rev.sh <rev> parent), against that library's kz_render, beside the spread of its own repeats. The stage clock of the call
     (kz_adaptive_stage_ms) gives what ran between the renders, summed over the rounds: the moment film's resolve (the picture's is as long), classification, read-back.
 (b) the classification kernel against a device-to-device copy of its bytes - it reads 32 B per frame texel it touches and writes 17 B per block - timed in the same
     process (hipMemcpy, host clock, synchronised), for the four block edges.
 (c) benefit: on C3 (hero scene) and on the reference's own q1 scene (tests/golden/q1_default_m0_r0.5.npz) at 1920 x 1080, cap --cap, for a few thresholds the
     total samples, the wall time and the RMSE against a --truth-spp picture, beside a uniform render at the cap.
    python scripts/adaptive_rates.py [--parts a,b,c] [--cap 256] [--truth-spp 1024] [--thresholds 0.02,0.05,0.1] [--parent-lib PATH] [--size 1920x1080]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
kz = importlib.import_module("nano-kazen_amd")
from matte_rates import copy_ms      # noqa: E402  (the same yardstick: a synchronised device-to-device hipMemcpy through the library's own HIP runtime)


def timed(fn, sc):
    sc.sync()
    t0 = time.perf_counter()
    out = fn()
    sc.sync()
    return time.perf_counter() - t0, out


def c4(W, H, spp):
    return kz.scenes.random_triangles(1000000, W, H, spp, sampler="pmj02bn", seed=1)


def part_a(W, H, cap, parent_lib):
    desc = c4(W, H, cap)
    sc = kz.Scene(desc, device=0)
    sc.set_variance(True)
    plain = kz.Scene(desc, device=0)
    plain.set_variance(True)
    base = None
    if parent_lib:
        base = kz.Scene(desc, device=0, lib=kz.abi.load_library(parent_lib))
        base.set_variance(True)
    for s in (sc, plain, base):                                        # warm: contexts grown, beam lists built, pass modes settled
        if s is not None:
            s.render()
            s.render()
    rows = {"adaptive_s": [], "plain_s": [], "parent_s": [], "stage_ms": []}
    for _ in range(3):
        t, info = timed(lambda: sc.render_adaptive(1e-9, max_samples=cap), sc)
        rows["adaptive_s"].append(t)
        rows["stage_ms"].append(sc.adaptive_stage_ms())
        rows["plain_s"].append(timed(plain.render, plain)[0])
        if base is not None:
            rows["parent_s"].append(timed(base.render, base)[0])
    rows["info"] = info
    rows["rounds"] = kz.adaptive_schedule(cap)
    rows["overhead_vs_plain_pct"] = 100.0 * (np.median(rows["adaptive_s"]) / np.median(rows["plain_s"]) - 1.0)
    rows["plain_spread_pct"] = 100.0 * (max(rows["plain_s"]) - min(rows["plain_s"])) / np.median(rows["plain_s"])
    if base is not None:
        rows["overhead_vs_parent_pct"] = 100.0 * (np.median(rows["adaptive_s"]) / np.median(rows["parent_s"]) - 1.0)
        rows["parent_spread_pct"] = 100.0 * (max(rows["parent_s"]) - min(rows["parent_s"])) / np.median(rows["parent_s"])
    return rows


def part_b(W, H):
    desc = kz.scenes.cornell_box(W, H, 16)
    sc = kz.Scene(desc, device=0)
    sc.set_variance(True)
    out = {}
    for block in (8, 16, 32, 64):
        ms = []
        for _ in range(5):
            info = sc.render_adaptive(1e9, block=block)                # one round: the stage clock holds one classification of the whole frame
            ms.append(sc.adaptive_stage_ms()[1])
        n_bytes = 32 * W * H + 17 * info["blocks"]
        c = copy_ms(n_bytes)
        out[str(block)] = {"classify_ms": float(np.median(ms)), "bytes": n_bytes, "GBps": n_bytes / np.median(ms) / 1e6, "copy_ms": c, "copy_GBps": n_bytes / c / 1e6}
    return out


def rmse(sc, film, truth):
    a, b = sc.rgb(film), truth
    return float(np.sqrt(np.mean((a - b) ** 2)))


def part_c(W, H, cap, truth_spp, thresholds):
    scenes = {"C3": lambda spp: kz.scenes.hero_scene(W, H, spp, detail=2.0),
              "q1": lambda spp: kz.scenes.load_npz(os.path.join(ROOT, "tests", "golden", "q1_default_m0_r0.5.npz"),
                                                   overrides={"camera": {"width": W, "height": H}, "sampler": {"type": "independent", "sampleCount": spp, "seed": 0}})}
    out = {}
    for name, make in scenes.items():
        sc = kz.Scene(make(truth_spp), device=0)
        sc.set_variance(True)
        sc.render()
        truth = sc.rgb(sc.film())
        sc.render(sample_end=cap)                                      # warm at the cap's shape
        t, _ = timed(lambda: sc.render(sample_end=cap), sc)
        row = {"uniform": {"samples": W * H * cap, "s": t, "rmse": rmse(sc, sc.film(), truth)}}
        for thr in thresholds:
            sc.render_adaptive(thr, max_samples=cap)
            t, info = timed(lambda: sc.render_adaptive(thr, max_samples=cap), sc)
            row["%g" % thr] = {"samples": info["samples"], "s": t, "rmse": rmse(sc, sc.film(), truth), "rounds": info["rounds"], "converged": info["converged"], "atCap": info["atCap"],
                               "blocks": info["blocks"]}
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--truth-spp", type=int, default=1024)
    ap.add_argument("--thresholds", default="0.02,0.05,0.1")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(x) for x in args.size.split("x"))
    res = {"size": [W, H], "cap": args.cap}
    parts = args.parts.split(",")
    if "a" in parts:
        res["a_round_overhead"] = part_a(W, H, args.cap, args.parent_lib)
    if "b" in parts:
        res["b_classify_vs_copy"] = part_b(W, H)
    if "c" in parts:
        res["c_benefit"] = part_c(W, H, args.cap, args.truth_spp, [float(x) for x in args.thresholds.split(",")])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
