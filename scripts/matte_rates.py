"""What the ID mattes (include_ext/kazen_mi355x_matte.h) cost, on C3 (hero scene, 508 k triangles, independent) and C4 (1 M random triangles + 8 mesh lights,
pmj02bn) at 1920 x 1080, at 1 spp and at 64 spp, in ONE process: warm, device-synchronised kz_render calls with the matte mask 0 and with the mask 3 (mesh +
BSDF row), alternated render by render. The yardstick is what ONE feature film (kazen_mi355x_aov.h, the depth film: kz_wf_aov plus one tap launch) costs in the
same process, measured the same way, and a device-to-device copy of the stage's compulsory bytes - 16 B read and 16 B gathered per item, 64 B read and 64 B
written per pixel, key and pass over the pixel - timed in the same process (hipMemcpy, host clock). With --parent-lib (a build of the parent commit: scripts/build_rev.sh <rev>
parent) the mask-0 rate is also measured against that library: a fresh scene of each, the two alternating in the same process, beside the spread of the parent's
own repeats.
One JSON line on stdout (and in --out).
    python scripts/matte_rates.py [--spps 1,64] [--reps 9] [--parent-lib nano-kazen_amd/csrc/variants/parent/libkazen_mi355x.so] [--scenes C3,C4]"""
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


def render_s(sc, spp):
    t0 = time.perf_counter()
    sc.render(sample_begin=0, sample_end=spp)
    sc.sync()
    return time.perf_counter() - t0


def copy_ms(n_bytes, reps=9):
    """Median host-clock time of a synchronised device-to-device hipMemcpy that reads n_bytes / 2 and writes n_bytes / 2, through the HIP runtime the library
    itself has loaded (found in this process's maps: another copy of the runtime would be another world)."""
    import ctypes as C
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    n = max(1, n_bytes // 2)
    a, b = C.c_void_p(), C.c_void_p()
    if hip.hipMalloc(C.byref(a), n) or hip.hipMalloc(C.byref(b), n):
        raise RuntimeError("hipMalloc of 2 x %d bytes failed" % n)
    ms = []
    try:
        for _ in range(reps + 2):
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            rc = hip.hipMemcpy(b, a, n, 3)                              # hipMemcpyDeviceToDevice
            rc = rc or hip.hipDeviceSynchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            if rc:
                raise RuntimeError("hipMemcpy failed: %d" % rc)
    finally:
        hip.hipFree(a)
        hip.hipFree(b)
    return float(np.median(ms[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spps", default="1,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scenes", default="C3,C4")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-spp", type=int, default=64)
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    scenes = {"C3": lambda spp: kz.scenes.hero_scene(1920, 1080, spp, detail=2.0),
              "C4": lambda spp: kz.scenes.random_triangles(1000000, 1920, 1080, spp, sampler="pmj02bn", seed=1)}
    rec = {"reps": a.reps, "scenes": {}}
    spps = [int(s) for s in a.spps.split(",")]
    for name in a.scenes.split(","):
        rec["scenes"][name] = {}
        d = scenes[name](max(spps + [a.parent_spp]))                    # one description - one BVH build - per scene: a render takes the first spp samples of it
        sc = None
        for spp in spps:
            n_pix = d.camera["width"] * d.camera["height"]
            n = n_pix * spp
            rate = lambda s: round(n / s / 1e6, 1)
            r = {}
            sc = sc or kz.Scene(d, device=0)
            render_s(sc, spp)                                           # warm: context, beams
            # three states take turns: nothing beside the picture, the two matte keys, one feature film (depth)
            states = {"off": (0, 0), "matte3": (0, 3), "aov_depth": (4, 0)}
            t = {k: [] for k in states}
            film_ms = {k: [] for k in states}
            for _ in range(a.reps):
                for k, (aov, matte) in states.items():
                    sc.set_aovs(aov)
                    sc.set_mattes(matte)
                    render_s(sc, spp)                                   # (not timed: tables and sums are allocated and zeroed by the first render after the switch)
                    t[k].append(render_s(sc, spp))
                    film_ms[k].append(sc.last_stage_ms()["film"])
                    if matte:
                        r["matte_info_bytes"] = sc.matte_info()
            sc.set_aovs(0)
            sc.set_mattes(0)
            info = sc.last_pass_info()
            r["passes"], r["spp_per_pass"] = info["passes"], info["sppPerPass"]
            for k in states:
                r[k + "_ms"] = [round(x * 1e3, 3) for x in t[k]]
                r[k + "_ms_median"] = round(float(np.median(t[k])) * 1e3, 3)
                r[k + "_msamples_s_median"] = rate(float(np.median(t[k])))
                r[k + "_film_stage_ms_last_pass_median"] = round(float(np.median(film_ms[k])), 3)
            off = float(np.median(t["off"]))
            r["off_spread_ms"] = round((max(t["off"]) - min(t["off"])) * 1e3, 3)
            r["matte3_minus_off_ms"] = round((float(np.median(t["matte3"])) - off) * 1e3, 3)
            r["aov_depth_minus_off_ms"] = round((float(np.median(t["aov_depth"])) - off) * 1e3, 3)
            r["matte3_over_off_time"] = round(float(np.median(t["matte3"])) / off, 4)
            # the stage's compulsory traffic of one render: per item 16 B read + 16 B gathered; per pixel, key and pass over the pixel 64 B read + 64 B written
            passes_over_pixel = -(-spp // max(1, info["sppPerPass"]))
            r["compulsory_bytes"] = n * 32 + n_pix * 2 * 128 * passes_over_pixel
            if not a.no_copy:
                try:
                    r["copy_of_compulsory_bytes_ms"] = round(copy_ms(r["compulsory_bytes"]), 3)
                except Exception as e:                                  # (no room for the two buffers: the figure is left out, and said so)
                    r["copy_of_compulsory_bytes_error"] = repr(e)[:200]
            if a.parent_lib and spp == a.parent_spp:
                plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
                assert not hasattr(plib, "kz_scene_set_mattes"), "--parent-lib must be a build of the parent commit"
                # two FRESH scenes with the same history: five renders each, taking turns, let both replicas time their four probe passes and keep a mode; then A B A B ...
                sc.close()
                sc = kz.Scene(d, device=0)
                ps = kz.Scene(d, device=0, lib=plib)
                for _ in range(5):
                    render_s(sc, spp)
                    render_s(ps, spp)
                mine, parent = [], []
                for _ in range(a.reps):
                    mine.append(render_s(sc, spp))
                    parent.append(render_s(ps, spp))
                r["ab_pass_mode_kept"] = {"this": sc.pass_mode_info()["kept"], "parent": ps.pass_mode_info()["kept"]}
                r["ab_mask0_msamples_s"], r["ab_parent_msamples_s"] = [rate(x) for x in mine], [rate(x) for x in parent]
                pm = float(np.median(parent))
                r["ab_mask0_over_parent_time"] = round(float(np.median(mine)) / pm, 4)
                r["ab_parent_spread"] = round((max(parent) - min(parent)) / pm, 4)
                r["ab_inside_parent_spread"] = bool(abs(float(np.median(mine)) - pm) <= max(parent) - min(parent))
                ps.close()
            rec["scenes"][name]["%dspp" % spp] = r
            print("%s %d spp: %s" % (name, spp, json.dumps(r)), file=sys.stderr, flush=True)
        sc.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
