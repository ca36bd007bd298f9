"""Rates of the four integrators on C3 (hero scene, 508 k triangles, 256 spp, independent) and C4 (1 M random triangles + 8 mesh lights, pmj02bn) at the
default pass size: warm, device-synchronised kz_render calls, Msamples/s per (scene, integrator). Prints one JSON line.
    python scripts/integrator_rates.py [--c4-spp 256] [--reps 3]
(For the kernel trace run it again under rocprofv3 --kernel-trace --stats, with no counters in that run.)"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-spp", type=int, default=256)
    ap.add_argument("--c4-spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--integrators", default="path_mis,normals,ao,path_mats")
    a = ap.parse_args()
    scenes = {"C3": lambda: kz.scenes.hero_scene(1920, 1080, a.c3_spp, detail=2.0),
              "C4": lambda: kz.scenes.random_triangles(1000000, 1920, 1080, a.c4_spp, sampler="pmj02bn", seed=1)}
    out = {"reps": a.reps, "rates_msamples_s": {}, "ms_per_frame": {}, "passes": {}}
    for sname, make in scenes.items():
        base = make()
        for integ in a.integrators.split(","):
            d = copy.copy(base)
            d.integrator = dict(base.integrator, type=integ)
            sc = kz.Scene(d, device=0)
            sc.render(); sc.sync()                                  # warm: context, beams, BVH upload
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                sc.render(); sc.sync()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            n = d.camera["width"] * d.camera["height"] * d.sampler["sampleCount"]
            key = "%s/%s" % (sname, integ)
            out["rates_msamples_s"][key] = round(n / best / 1e6, 1)
            out["ms_per_frame"][key] = round(best * 1e3, 2)
            out["passes"][key] = sc.last_pass_info().get("passes") if isinstance(sc.last_pass_info(), dict) else None
            sc.close()
            print("%s: %.1f Msamples/s (%.1f ms)" % (key, n / best / 1e6, best * 1e3), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
