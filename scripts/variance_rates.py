"""What the second-moment film and kz_denoise_variance (include/kazen_mi355x_variance.h) cost, on C4 (1 M random triangles + 8 mesh lights, pmj02bn) and C3 (hero
scene, 508 k triangles) at 1920 x 1080, in ONE process, warmed, every timing a host clock around a call that ends in a device synchronise:
  * a render of 64 spp with the switch off, on with two tap launches (KZ_VARIANCE_TWO_LAUNCHES) and on with the one-pass tap kernel (KZ_VARIANCE_ONE_PASS): three
    replicas of one scene taking turns, the medians, the film stage's own time (kz_last_stage_ms), and whether the films are the same bits;
  * kz_denoise_variance against kz_denoise at equal iterations and guides (all three feature films, 4 spp), medians, per call and per step;
  * --variants name=lib,...: builds of the same sources with another a-trous form per step (scripts/build_variant.sh dn_direct -DKZ_DN_LDS_MAX_STEP=0: direct
    gather at every step), alternated with the product library call by call; their results must have the product's bits;
  * --parent-lib: a build of the parent commit; a render with the switch off, the two libraries alternating, beside the parent's own spread - twice, with the two
    replicas created in either order.
One JSON record in <out>/variance_rates.json.
    python scripts/variance_rates.py [--reps 9] [--spp 64] [--scenes C4,C3] [--variants dn_direct=...so] [--parent-lib ...so] [--out profiles/r17a_variance]"""
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


def timed(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def steps_of(ms):
    return {"1": round(ms[1], 4), **{str(1 << (k - 1)): round(ms[k] - ms[k - 1], 4) for k in range(2, 6)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scenes", default="C4,C3")
    ap.add_argument("--variants", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17a_variance"))
    a = ap.parse_args()
    W, H, A = 1920, 1080, kz.abi
    scenes = {"C3": lambda: kz.scenes.hero_scene(W, H, a.spp, detail=2.0),
              "C4": lambda: kz.scenes.random_triangles(1000000, W, H, a.spp, sampler="pmj02bn", seed=1)}
    variants = dict(v.split("=", 1) for v in a.variants.split(",") if v)
    rec = {"width": W, "height": H, "spp": a.spp, "reps": a.reps, "scenes": {}}
    for name in a.scenes.split(","):
        d = scenes[name]()
        r = {}
        # ---- the render, switch off / two launches / one pass, taking turns
        modes = {"off": A.KZ_VARIANCE_OFF, "two_launches": A.KZ_VARIANCE_TWO_LAUNCHES, "one_pass": A.KZ_VARIANCE_ONE_PASS}
        reps = {}
        for m, v in modes.items():
            reps[m] = kz.Scene(d, device=0)
            reps[m].set_variance(v)
        for _ in range(5):                                              # every replica times its probe passes and keeps a pass mode
            for s in reps.values():
                timed(s.render, s.sync)
        t, film_ms = {m: [] for m in modes}, {m: [] for m in modes}
        for _ in range(a.reps):
            for m, s in reps.items():
                t[m].append(timed(s.render, s.sync))
                film_ms[m].append(s.last_stage_ms()["film"])
        off = float(np.median(t["off"]))
        r["render_ms"] = {m: med_ms(x) for m, x in t.items()}
        r["render_ms_all"] = {m: [round(x * 1e3, 3) for x in xs] for m, xs in t.items()}
        r["film_stage_ms_last_pass"] = {m: round(float(np.median(x)), 3) for m, x in film_ms.items()}
        r["render_over_off"] = {m: round(float(np.median(x)) / off, 4) for m, x in t.items()}
        r["off_spread"] = round((max(t["off"]) - min(t["off"])) / off, 4)
        r["passes"] = reps["off"].last_pass_info()
        picture = reps["off"].film()
        moment = reps["two_launches"].moment_film()
        r["same_bits"] = {"picture_two_launches": bool(np.array_equal(reps["two_launches"].film(), picture)), "picture_one_pass": bool(np.array_equal(reps["one_pass"].film(), picture)),
                          "moment_one_pass": bool(np.array_equal(reps["one_pass"].moment_film().view(np.uint32), moment.view(np.uint32))),
                          "moment_w_is_pictures": bool(np.array_equal(moment[..., 3].view(np.uint32), picture[..., 3].view(np.uint32)))}
        r["variance_info"] = reps["two_launches"].variance_info()
        for s in reps.values():
            s.close()
        # ---- the denoise call
        sc = kz.Scene(d, device=0)
        sc.set_aovs(7)
        sc.set_variance(True)
        sc.render(sample_begin=0, sample_end=4)                         # the picture a look-dev user denoises
        sc.sync()
        sc.denoise_variance()
        base = sc.denoised_film()
        r["denoise_info_bytes"] = sc.denoise_info()
        calls = {"kz_denoise": lambda k: sc.denoise(iterations=k, sigma_color=2.0), "kz_denoise_variance": lambda k: sc.denoise_variance(iterations=k)}
        t = {c: {k: [] for k in range(1, 6)} for c in calls}
        for _ in range(a.reps):
            for k in range(1, 6):
                for c, fn in calls.items():
                    t[c][k].append(timed(lambda: fn(k), lambda: None))   # (both calls return synchronised)
        r["call_ms_by_iterations"] = {c: {k: med_ms(v) for k, v in tk.items()} for c, tk in t.items()}
        r["step_ms"] = {c: steps_of(m) for c, m in r["call_ms_by_iterations"].items()}
        r["variance_over_plain_5_iterations"] = round(r["call_ms_by_iterations"]["kz_denoise_variance"][5] / r["call_ms_by_iterations"]["kz_denoise"][5], 4)
        if variants:
            others = {}
            for vn, path in variants.items():
                lib = kz.abi.load_library(os.path.abspath(path))
                vs = kz.Scene(d, device=0, lib=lib)
                vs.set_aovs(7)
                vs.set_variance(True)
                vs.render(sample_begin=0, sample_end=4)
                vs.sync()
                vs.denoise_variance()
                others[vn] = vs
                r.setdefault("variant_same_bits", {})[vn] = bool(np.array_equal(vs.denoised_film().view(np.uint32), base.view(np.uint32)))
            t = {vn: {k: [] for k in range(1, 6)} for vn in ["product"] + list(others)}
            for _ in range(a.reps):
                for k in range(1, 6):
                    t["product"][k].append(timed(lambda: sc.denoise_variance(iterations=k), lambda: None))
                    for vn, vs in others.items():
                        t[vn][k].append(timed(lambda: vs.denoise_variance(iterations=k), lambda: None))
            r["variants_call_ms_by_iterations"] = {vn: {k: med_ms(v) for k, v in tk.items()} for vn, tk in t.items()}
            r["variants_step_ms"] = {vn: steps_of(m) for vn, m in r["variants_call_ms_by_iterations"].items()}
            for vs in others.values():
                vs.close()
        sc.close()
        # ---- the switch off against the parent commit's library
        if a.parent_lib:
            plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
            assert not hasattr(plib, "kz_denoise_variance"), "--parent-lib must be a build of the parent commit"
            # (twice, with the two replicas created in either order: on C3 the difference between two replicas of ONE library has been larger than the parent's spread)
            for order in ("this_first", "parent_first"):
                if order == "this_first":
                    sc = kz.Scene(d, device=0)
                    ps = kz.Scene(d, device=0, lib=plib)
                else:
                    ps = kz.Scene(d, device=0, lib=plib)
                    sc = kz.Scene(d, device=0)
                for _ in range(5):
                    timed(sc.render, sc.sync)
                    timed(ps.render, ps.sync)
                mine, parent = [], []
                for _ in range(a.reps):
                    mine.append(timed(sc.render, sc.sync))
                    parent.append(timed(ps.render, ps.sync))
                pm = float(np.median(parent))
                r["ab_" + order] = {"this_ms": [round(x * 1e3, 3) for x in mine], "parent_ms": [round(x * 1e3, 3) for x in parent],
                                    "this_over_parent_time": round(float(np.median(mine)) / pm, 4), "parent_spread": round((max(parent) - min(parent)) / pm, 4),
                                    "inside_parent_spread": bool(abs(float(np.median(mine)) - pm) <= max(parent) - min(parent)),
                                    "same_bits": bool(np.array_equal(sc.film(), ps.film())),
                                    "pass_mode": {"this": sc.pass_mode_info()["kept"], "parent": ps.pass_mode_info()["kept"]}}
                ps.close()
                sc.close()
        rec["scenes"][name] = r
        print("%s: %s" % (name, json.dumps(r)), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "variance_rates.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
