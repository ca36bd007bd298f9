"""What the feature films (include/kazen_mi355x_aov.h) cost, on C3 (hero scene, 508 k triangles, independent) and C4 (1 M random triangles + 8 mesh lights,
pmj02bn) at 1920 x 1080, in ONE process: warm, device-synchronised kz_render calls with the mask 0 and with the mask 7 (albedo + normal + depth), alternated
render by render; the film entry of kz_last_stage_ms of both; kz_aov_info's bytes. With --parent-lib (a build of the parent commit: scripts/build_rev.sh
<rev> parent) the mask-0 rate is also measured against that library: a fresh scene of each, the two alternating in the same process, beside the spread of the
parent's own repeats and the large-pass mode each replica kept.
One JSON line on stdout (and in --out).
    python scripts/aov_rates.py [--spp 64] [--reps 7] [--parent-lib nano-kazen_amd/csrc/variants/parent/libkazen_mi355x.so] [--scenes C3,C4]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")


def render_s(sc):
    t0 = time.perf_counter()
    sc.render()
    sc.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="C3,C4")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    scenes = {"C3": lambda: kz.scenes.hero_scene(1920, 1080, a.spp, detail=2.0),
              "C4": lambda: kz.scenes.random_triangles(1000000, 1920, 1080, a.spp, sampler="pmj02bn", seed=1)}
    rec = {"spp": a.spp, "reps": a.reps, "scenes": {}}
    for name in a.scenes.split(","):
        d = scenes[name]()
        n = d.camera["width"] * d.camera["height"] * d.sampler["sampleCount"]
        rate = lambda s: round(n / s / 1e6, 1)
        r = {}
        sc = kz.Scene(d, device=0)
        render_s(sc)                                                    # warm: context, beams
        t = {0: [], 7: []}
        film_ms = {0: [], 7: []}
        for _ in range(a.reps):                                         # mask 0 and mask 7 take turns
            for mask in (0, 7):
                sc.set_aovs(mask)
                render_s(sc)                                            # (not timed: the AOV sums are allocated and zeroed by the first render after the switch)
                t[mask].append(render_s(sc))
                film_ms[mask].append(sc.last_stage_ms()["film"])
                if mask:
                    r["aov_info_bytes"] = sc.aov_info()
        sc.set_aovs(0)
        for mask in (0, 7):
            r["mask%d_msamples_s" % mask] = [rate(x) for x in t[mask]]
            r["mask%d_msamples_s_median" % mask] = rate(float(np.median(t[mask])))
            r["mask%d_film_stage_ms_last_pass_median" % mask] = round(float(np.median(film_ms[mask])), 3)
        r["passes"] = sc.last_pass_info()["passes"]
        r["mask7_over_mask0_time"] = round(float(np.median(t[7]) / np.median(t[0])), 4)
        if a.parent_lib:
            plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
            assert not hasattr(plib, "kz_scene_set_aovs"), "--parent-lib must be a build of the parent commit"
            # two FRESH scenes with the same history (the one above has settled its large-pass mode - kz_pass_mode_info - on passes of both masks): five
            # renders each, taking turns, let both replicas time their four probe passes and keep a mode; then A B A B ...
            sc.close()
            sc = kz.Scene(d, device=0)
            ps = kz.Scene(d, device=0, lib=plib)
            for _ in range(5):
                render_s(sc)
                render_s(ps)
            mine, parent = [], []
            for _ in range(a.reps):
                mine.append(render_s(sc))
                parent.append(render_s(ps))
            r["ab_pass_mode_kept"] = {"this": sc.pass_mode_info()["kept"], "parent": ps.pass_mode_info()["kept"]}
            r["ab_mask0_msamples_s"], r["ab_parent_msamples_s"] = [rate(x) for x in mine], [rate(x) for x in parent]
            pm = float(np.median(parent))
            r["ab_mask0_over_parent_time"] = round(float(np.median(mine)) / pm, 4)
            r["ab_parent_spread"] = round((max(parent) - min(parent)) / pm, 4)
            r["ab_inside_parent_spread"] = bool(abs(float(np.median(mine)) - pm) <= max(parent) - min(parent))
            ps.close()
        sc.close()
        rec["scenes"][name] = r
        print("%s: %s" % (name, json.dumps(r)), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
