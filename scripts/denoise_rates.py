"""What kz_denoise (include/kazen_mi355x_denoise.h) costs, on C4 (1 M random triangles + 8 mesh lights, pmj02bn) and C3 (hero scene, 508 k triangles) at
1920 x 1080 with all three feature films, in ONE process, warmed, every timing a host clock around a call that ends in a device synchronise:
  * kz_denoise at 1 .. 5 iterations (the call's time, and the increments: what each a-trous launch of step 1, 2, 4, 8, 16 adds), colour weights alone too;
  * beside a plain device-to-device copy of the 64 bytes per pixel one iteration cannot avoid (48 read + 16 written; the copy moves 32 and writes 32);
  * beside the render of that frame at 1, 4 and 16 samples per pixel;
  * --variants name=lib,...: builds of the same sources with another a-trous form per step (scripts/build_variant.sh dn_direct -DKZ_DN_LDS_MAX_STEP=0: direct
    gather at every step), alternated with the product library call by call; their results must have the product's bits;
  * --parent-lib: a build of the parent commit; a render with no denoise call, the two libraries alternating, beside the parent's own spread.
One JSON record in <out>/denoise_rates.json.
    python scripts/denoise_rates.py [--reps 9] [--scenes C4,C3] [--variants dn_direct=...so] [--parent-lib ...so] [--out profiles/r16a_denoise]"""
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


def copy_ms(n_bytes, reps):
    """A plain copy of n_bytes on the device (hipMemcpyAsync device to device through torch), timed like everything else."""
    import torch
    src = torch.empty(n_bytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    return [timed(lambda: dst.copy_(src), torch.cuda.synchronize) for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scenes", default="C4,C3")
    ap.add_argument("--variants", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_denoise"))
    a = ap.parse_args()
    W, H = 1920, 1080
    scenes = {"C3": lambda: kz.scenes.hero_scene(W, H, 16, detail=2.0),
              "C4": lambda: kz.scenes.random_triangles(1000000, W, H, 16, sampler="pmj02bn", seed=1)}
    variants = dict(v.split("=", 1) for v in a.variants.split(",") if v)
    rec = {"width": W, "height": H, "reps": a.reps, "compulsory_bytes_per_iteration": 64 * W * H, "scenes": {}}
    rec["copy_32B_per_pixel_ms"] = med_ms(copy_ms(32 * W * H, a.reps))
    for name in a.scenes.split(","):
        d = scenes[name]()
        r = {}
        sc = kz.Scene(d, device=0)
        sc.set_aovs(7)
        for spp in (1, 4, 16):
            run = lambda: sc.render(sample_begin=0, sample_end=spp)
            timed(run, sc.sync)
            r["render_%dspp_ms" % spp] = med_ms([timed(run, sc.sync) for _ in range(a.reps)])
        sc.render(sample_begin=0, sample_end=4)                         # the picture a look-dev user denoises
        sc.sync()
        sc.denoise()
        base = sc.denoised_film()
        r["valid_pixels"] = int((base[..., 3] == 1).sum())
        r["denoise_info_bytes"] = sc.denoise_info()
        for label, kw in (("guided", {}), ("colour_only", {"use_guides": False})):
            t = {k: [] for k in range(1, 6)}
            for _ in range(a.reps):
                for k in t:
                    t[k].append(timed(lambda: sc.denoise(iterations=k, **kw), lambda: None))      # (kz_denoise returns synchronised)
            ms = {k: med_ms(v) for k, v in t.items()}
            r[label] = {"call_ms_by_iterations": ms, "step_ms": {str(1 << (k - 1)): round(ms[k] - ms[k - 1], 4) for k in range(2, 6)},
                        "per_iteration_ms": round((ms[5] - ms[1]) / 4, 4), "prepare_finish_and_first_ms": ms[1],
                        "copy_over_iteration": round(rec["copy_32B_per_pixel_ms"] / max((ms[5] - ms[1]) / 4, 1e-9), 4)}
        r["denoise5_over_render_4spp"] = round(r["guided"]["call_ms_by_iterations"][5] / r["render_4spp_ms"], 4)
        if variants:
            others = {}
            for vn, path in variants.items():
                lib = kz.abi.load_library(os.path.abspath(path))
                vs = kz.Scene(d, device=0, lib=lib)
                vs.set_aovs(7)
                vs.render(sample_begin=0, sample_end=4)
                vs.sync()
                vs.denoise()
                others[vn] = vs
                r.setdefault("variant_same_bits", {})[vn] = bool(np.array_equal(vs.denoised_film().view(np.uint32), base.view(np.uint32)))
            t = {vn: {k: [] for k in (1, 2, 3, 4, 5)} for vn in ["product"] + list(others)}
            for _ in range(a.reps):
                for k in (1, 2, 3, 4, 5):
                    t["product"][k].append(timed(lambda: sc.denoise(iterations=k), lambda: None))
                    for vn, vs in others.items():
                        t[vn][k].append(timed(lambda: vs.denoise(iterations=k), lambda: None))
            r["variants_call_ms_by_iterations"] = {vn: {k: med_ms(v) for k, v in tk.items()} for vn, tk in t.items()}
            r["variants_step_ms"] = {vn: {"1": round(m[1], 4), **{str(1 << (k - 1)): round(m[k] - m[k - 1], 4) for k in range(2, 6)}}
                                     for vn, m in r["variants_call_ms_by_iterations"].items()}
            for vs in others.values():
                vs.close()
        if a.parent_lib:
            plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
            assert not hasattr(plib, "kz_denoise"), "--parent-lib must be a build of the parent commit"
            sc.close()
            sc = kz.Scene(d, device=0)
            ps = kz.Scene(d, device=0, lib=plib)
            for _ in range(5):                                          # both replicas time their probe passes and keep a pass mode
                timed(sc.render, sc.sync)
                timed(ps.render, ps.sync)
            mine, parent = [], []
            for _ in range(a.reps):
                mine.append(timed(sc.render, sc.sync))
                parent.append(timed(ps.render, ps.sync))
            pm = float(np.median(parent))
            r["ab_render_16spp_ms"] = {"this": [round(x * 1e3, 3) for x in mine], "parent": [round(x * 1e3, 3) for x in parent]}
            r["ab_this_over_parent_time"] = round(float(np.median(mine)) / pm, 4)
            r["ab_parent_spread"] = round((max(parent) - min(parent)) / pm, 4)
            r["ab_inside_parent_spread"] = bool(abs(float(np.median(mine)) - pm) <= max(parent) - min(parent))
            ps.close()
        sc.close()
        rec["scenes"][name] = r
        print("%s: %s" % (name, json.dumps(r)), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "denoise_rates.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
