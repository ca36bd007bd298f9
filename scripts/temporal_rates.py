"""What kz_denoise_temporal (include/kazen_mi355x_temporal.h) costs, at 1920 x 1080 with all three guides, in ONE process, warmed, every timing a host clock around a
call that ends in a device synchronise, the calls alternating, medians of --reps:
  * kz_denoise_temporal against kz_denoise_variance at the same options, at 1 and 5 iterations, on a Cornell box of 4 spp whose camera turns by a quarter of a degree
    between the calls (so that the taps of a wave fall on neighbouring records that are not its own). The difference of the two at equal iterations is what
    kz_dn_prepare_temporal costs beyond kz_dn_prepare_var;
  * a device-to-device copy (hipMemcpy) that moves the stage's compulsory bytes: per pixel it must read five resolved film texels (5 x 16 B) and four history records
    (4 x 36 B) and write three planes (3 x 16 B) and one history record (36 B) - 308 B, of which 200 B are distinct once neighbouring lanes share their taps'
    records. The copy reads and writes half of the figure each. Both figures are timed;
  * --loop N: nothing but N kz_denoise_temporal calls - the process to run under `rocprofv3 --kernel-trace --stats` for the kernel's own time;
  * --parent-lib: a build of the parent commit; a plain render of 64 spp of C4 and C3 (scripts/variance_rates.py's scenes), the two libraries alternating, beside
    the parent's own spread - twice, with the two replicas created in either order; --control-lib: a second copy of the parent's build, measured against the
    parent's in the same way.
One JSON record in <out>/temporal_rates.json.
    python scripts/temporal_rates.py [--reps 9] [--parent-lib ...so] [--control-lib ...so] [--scenes C4,C3] [--out profiles/r19a_temporal]"""
import argparse
import copy
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")

READ_BYTES, WRITE_BYTES, DISTINCT_BYTES = 5 * 16 + 4 * 36, 3 * 16 + 36, 5 * 16 + 36 + 3 * 16 + 36


def timed(fn, sync=lambda: None):
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def turned(desc, degrees):
    """The description's camera turned about the world's y axis through the point 4 units along its axis."""
    m = np.array(desc.camera["toWorld"], np.float64).reshape(4, 4)
    centre = m[:3, 3] + 4.0 * m[:3, 2]
    t = np.radians(degrees)
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    out = m.copy()
    out[:3, :3] = R @ m[:3, :3]
    out[:3, 3] = centre + R @ (m[:3, 3] - centre)
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scenes", default="C4,C3")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--control-lib", default="")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19a_temporal"))
    a = ap.parse_args()
    W, H = 1920, 1080
    d = kz.scenes.cornell_box(W, H, 4)
    start = copy.copy(d)
    start.camera = dict(d.camera)
    sc = kz.Scene(d, device=0)
    sc.set_aovs(7)
    sc.set_variance(True)
    sc.render()
    sc.sync()
    step = [0]

    def temporal(k):
        step[0] += 1
        sc.set_camera({"toWorld": turned(start, 0.25 * (step[0] % 8))})      # (the films stay the first camera's: the cost does not depend on what they show)
        return timed(lambda: sc.denoise_temporal(iterations=k))

    if a.loop:
        for _ in range(a.loop):
            temporal(5)
        print(json.dumps({"loop": a.loop, "temporal_info": sc.temporal_info()}))
        return
    rec = {"width": W, "height": H, "reps": a.reps, "bytes_per_pixel": {"read": READ_BYTES, "write": WRITE_BYTES, "distinct": DISTINCT_BYTES}}
    for k in (1, 5):                                                    # warm: every kernel of both calls, the history allocated
        temporal(k)
        sc.denoise_variance(iterations=k)
    t = {c: {1: [], 5: []} for c in ("kz_denoise_temporal", "kz_denoise_variance")}
    for _ in range(a.reps):
        for k in (1, 5):
            t["kz_denoise_temporal"][k].append(temporal(k))
            t["kz_denoise_variance"][k].append(timed(lambda: sc.denoise_variance(iterations=k)))
    rec["call_ms"] = {c: {str(k): med_ms(v) for k, v in tk.items()} for c, tk in t.items()}
    rec["call_ms_all"] = {c: {str(k): [round(x * 1e3, 4) for x in v] for k, v in tk.items()} for c, tk in t.items()}
    rec["temporal_minus_variance_ms"] = {str(k): round(rec["call_ms"]["kz_denoise_temporal"][str(k)] - rec["call_ms"]["kz_denoise_variance"][str(k)], 4) for k in (1, 5)}
    rec["temporal_over_variance"] = {str(k): round(rec["call_ms"]["kz_denoise_temporal"][str(k)] / rec["call_ms"]["kz_denoise_variance"][str(k)], 4) for k in (1, 5)}
    rec["temporal_info"] = sc.temporal_info()
    rec["found_history"] = round(float((sc.temporal_history()[..., 8] > 1).mean()), 4)
    sc.close()
    # ---- the copy of the compulsory bytes: hipMemcpy device to device through the runtime the library has loaded
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc

    for name, per_pixel in (("copy_nominal", READ_BYTES + WRITE_BYTES), ("copy_distinct", DISTINCT_BYTES)):
        n = W * H * per_pixel // 2                                      # the copy reads n and writes n
        src, dst = C.c_void_p(), C.c_void_p()
        ok(hip.hipMalloc(C.byref(src), n)); ok(hip.hipMalloc(C.byref(dst), n)); ok(hip.hipMemset(src, 0, n))
        copy_once = lambda: ok(hip.hipMemcpy(dst, src, n, 3))           # hipMemcpyDeviceToDevice
        sync = lambda: ok(hip.hipDeviceSynchronize())
        for _ in range(3):
            copy_once()
        sync()
        xs = [timed(copy_once, sync) for _ in range(a.reps)]
        rec[name] = {"bytes_moved": 2 * n, "ms": med_ms(xs), "TB_per_s": round(2 * n / float(np.median(xs)) / 1e12, 3)}
        ok(hip.hipFree(src)); ok(hip.hipFree(dst))
    # ---- a plain render against the parent commit's library; --control-lib: a second copy of the parent's build, measured against it the same way (how far two
    # loads of the SAME code lie apart is what a difference between this tree and the parent has to exceed)
    if a.parent_lib:
        plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
        assert not hasattr(plib, "kz_denoise_temporal"), "--parent-lib must be a build of the parent commit"
        sides = {"this": None}
        if a.control_lib:
            sides["control"] = kz.abi.load_library(os.path.abspath(a.control_lib))
            assert not hasattr(sides["control"], "kz_denoise_temporal"), "--control-lib must be a build of the parent commit"
        scenes = {"C3": lambda: kz.scenes.hero_scene(W, H, a.spp, detail=2.0), "C4": lambda: kz.scenes.random_triangles(1000000, W, H, a.spp, sampler="pmj02bn", seed=1)}
        rec["ab"] = {}
        for name in a.scenes.split(","):
            dd = scenes[name]()
            r = {}
            for side, lib in sides.items():
                for order in ("first", "second"):                       # the replica of `side` created before / after the parent's
                    if order == "first":
                        mine_s, parent_s = kz.Scene(dd, device=0, lib=lib), kz.Scene(dd, device=0, lib=plib)
                    else:
                        parent_s, mine_s = kz.Scene(dd, device=0, lib=plib), kz.Scene(dd, device=0, lib=lib)
                    for _ in range(5):
                        timed(mine_s.render, mine_s.sync)
                        timed(parent_s.render, parent_s.sync)
                    mine, parent = [], []
                    for _ in range(a.reps):
                        mine.append(timed(mine_s.render, mine_s.sync))
                        parent.append(timed(parent_s.render, parent_s.sync))
                    pm = float(np.median(parent))
                    r["%s_%s" % (side, order)] = {"ms": [round(x * 1e3, 3) for x in mine], "parent_ms": [round(x * 1e3, 3) for x in parent],
                                                  "over_parent_time": round(float(np.median(mine)) / pm, 4), "parent_spread": round((max(parent) - min(parent)) / pm, 4),
                                                  "inside_parent_spread": bool(abs(float(np.median(mine)) - pm) <= max(parent) - min(parent)),
                                                  "same_bits": bool(np.array_equal(mine_s.film(), parent_s.film()))}
                    parent_s.close()
                    mine_s.close()
            rec["ab"][name] = r
            print("%s: %s" % (name, json.dumps({k: (v["over_parent_time"], v["parent_spread"]) for k, v in r.items()})), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "temporal_rates.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
