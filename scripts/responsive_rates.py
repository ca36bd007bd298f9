"""What kz_denoise_responsive (include/kazen_mi355x_responsive.h) costs, at 1920 x 1080 with all three guides, in ONE process, warmed, every timing a host clock around
a call that ends in a device synchronise, the calls alternating, medians of --reps (scripts/motion_rates.py's protocol and scenes). Per scene:
  * three replicas of the scene, 1 spp rendered: kz_denoise_temporal with a camera that turns by a quarter of a degree between the calls; kz_denoise_motion and
    kz_denoise_responsive with the same camera AND mesh 0 moved by kz_scene_set_transforms between the calls (outside the clock), so that both compute the ids and
    upload the rows; at 1 and 5 iterations. responsive - motion is the stage: what kz_dn_prepare_responsive costs beyond kz_dn_prepare_motion, and kz_dn_clamp_history;
  * --parent-lib: a build of the parent commit (scripts/build_rev.sh); a fourth replica from it runs ITS kz_denoise_motion in the same alternation;
  * a device-to-device copy (hipMemcpy) of the stage's compulsory bytes. Per pixel the two kernels read five resolved film texels (5 x 16 B), the id (4 B), four taps
    of the history (4 x 36 B) and of the fast plane (4 x 16 B), then pass B the fast plane's tile (16 B x 68 x 8 / 256 = 34 B with the apron), its own N (4 B) and
    colour (16 B); they write three planes (3 x 16 B), one history record (36 B) and one fast record (16 B): 346 B read + 100 B written, of which 272 B are distinct
    once neighbouring lanes share their taps' records and tiles their aprons (a clamped pixel writes 36 B more; not counted). The copy reads and writes half of the
    figure each;
  * --loop N: nothing but N kz_denoise_responsive calls of that kind on the first scene - the process to run under `rocprofv3 --kernel-trace --stats`
    (--radius 2: with the 5 x 5 window instead of the default).
One JSON record in <out>/responsive_rates.json (--tag: another file name, for a second run).
    python scripts/responsive_rates.py [--reps 9] [--scenes C4,C3] [--parent-lib ...so] [--out profiles/r21a_responsive] [--tag run2]"""
import argparse
import copy
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
from temporal_rates import med_ms, timed, turned      # noqa: E402  (the same clock and the same camera path)

READ_BYTES, WRITE_BYTES = 5 * 16 + 4 + 4 * 36 + 4 * 16 + 34 + 4 + 16, 3 * 16 + 36 + 16
DISTINCT_BYTES = 5 * 16 + 4 + 36 + 16 + 16 + 4 + 16 + WRITE_BYTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scenes", default="C4,C3")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--radius", type=int, default=0, help="KzResponsiveOpts.radius of the responsive calls (0: the default)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21a_responsive"))
    a = ap.parse_args()
    W, H = 1920, 1080
    scenes = {"C3": lambda: kz.scenes.hero_scene(W, H, 1, detail=2.0), "C4": lambda: kz.scenes.random_triangles(1000000, W, H, 1, sampler="pmj02bn", seed=1)}
    plib = None
    if a.parent_lib:
        plib = kz.abi.load_library(os.path.abspath(a.parent_lib))
        assert not hasattr(plib, "kz_denoise_responsive"), "--parent-lib must be a build of the parent commit"
    rec = {"width": W, "height": H, "reps": a.reps, "radius": a.radius, "lib": os.path.basename(os.path.dirname(kz.abi.LIB_PATH)),
           "bytes_per_pixel": {"read": READ_BYTES, "write": WRITE_BYTES, "distinct": DISTINCT_BYTES}, "scenes": {}}
    for name in a.scenes.split(","):
        d = scenes[name]()
        start = copy.copy(d)
        start.camera = dict(d.camera)
        mover = next(i for i, m in enumerate(d.meshes) if m["light"] is None)
        calls = ["kz_denoise_temporal", "kz_denoise_motion", "kz_denoise_responsive"] + (["parent kz_denoise_motion"] if plib else [])
        reps = {}
        for c in calls:
            s = kz.Scene(copy.copy(d), device=0, lib=plib if c.startswith("parent") else None)
            s.set_aovs(7)
            s.set_variance(True)
            s.render()
            s.sync()
            reps[c] = s
        step = [0]

        def run(c, k):
            s = reps[c]
            step[0] += 1
            j = step[0] % 8
            if c != "kz_denoise_temporal":
                M = np.eye(4, dtype=np.float32)
                M[0, 3] = 0.002 * j
                s.set_transforms({mover: M})
            s.set_camera({"toWorld": turned(start, 0.25 * j)})          # (the films stay the first camera's: the cost does not depend on what they show)
            fn = {"kz_denoise_temporal": s.denoise_temporal, "kz_denoise_motion": s.denoise_motion, "parent kz_denoise_motion": s.denoise_motion,
                  "kz_denoise_responsive": lambda **kw: s.denoise_responsive(radius=a.radius, **kw)}[c]
            return timed(lambda: fn(iterations=k))

        if a.loop:
            for _ in range(a.loop):
                run("kz_denoise_responsive", 5)
            s = reps["kz_denoise_responsive"]
            print(json.dumps({"loop": a.loop, "scene": name, "temporal_info": s.temporal_info(), "responsive_info": s.responsive_info()}))
            return
        for k in (1, 5):                                                # warm: every kernel of every call, the buffers allocated, the histories long enough for pass B to run
            for _ in range(3):
                for c in calls:
                    run(c, k)
        t = {c: {1: [], 5: []} for c in calls}
        for _ in range(a.reps):
            for k in (1, 5):
                for c in calls:
                    t[c][k].append(run(c, k))
        r = {"call_ms": {c: {str(k): med_ms(v) for k, v in tk.items()} for c, tk in t.items()},
             "call_ms_all": {c: {str(k): [round(x * 1e3, 4) for x in v] for k, v in tk.items()} for c, tk in t.items()}}
        ms = r["call_ms"]
        r["responsive_minus_motion_ms"] = {str(k): round(ms["kz_denoise_responsive"][str(k)] - ms["kz_denoise_motion"][str(k)], 4) for k in (1, 5)}
        r["responsive_over_motion"] = {str(k): round(ms["kz_denoise_responsive"][str(k)] / ms["kz_denoise_motion"][str(k)], 4) for k in (1, 5)}
        if plib:
            r["responsive_over_parent_motion"] = {str(k): round(ms["kz_denoise_responsive"][str(k)] / ms["parent kz_denoise_motion"][str(k)], 4) for k in (1, 5)}
            r["motion_over_parent_motion"] = {str(k): round(ms["kz_denoise_motion"][str(k)] / ms["parent kz_denoise_motion"][str(k)], 4) for k in (1, 5)}
        s = reps["kz_denoise_responsive"]
        hist = s.temporal_history()
        r["responsive_info"], r["temporal_info"], r["motion_info"] = s.responsive_info(), s.temporal_info(), s.motion_info()
        r["found_history"] = round(float((hist[..., 8] > 1).mean()), 4)
        r["above_fast_history"] = round(float((hist[..., 8] > 2).mean()), 4)
        rec["scenes"][name] = r
        print("%s: %s" % (name, json.dumps({k: r[k] for k in r if k != "call_ms_all"})), file=sys.stderr, flush=True)
        for s in reps.values():
            s.close()
    # ---- the copy of the compulsory bytes: hipMemcpy device to device through the runtime the library has loaded (scripts/temporal_rates.py's)
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
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "responsive_rates%s.json" % (("_" + a.tag) if a.tag else "")), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
