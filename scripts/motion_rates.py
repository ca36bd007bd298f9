"""What kz_denoise_motion (include/kazen_mi355x_motion.h) costs, at 1920 x 1080 with all three guides, in ONE process, warmed, every timing a host clock around a call
that ends in a device synchronise, the calls alternating, medians of --reps. Per scene (C4: a million random triangles, C3: the hero scene; scripts/variance_rates.py's):
  * two replicas of the scene, 1 spp rendered: on one kz_denoise_temporal with a camera that turns by a quarter of a degree between the calls (scripts/temporal_rates.py's
    setting: the history is kept), on the other kz_denoise_motion with the same camera AND mesh 0 moved by kz_scene_set_transforms between the calls (outside the
    clock), so that every call computes the ids, uploads the rows and takes kz_dn_prepare_motion; at 1 and 5 iterations. The difference is the motion stage: the id
    kernel, the row upload and what kz_dn_prepare_motion costs beyond kz_dn_prepare_temporal;
  * kz_motion_ids alone (the kernel and the download of width x height words), beside the 1-spp render of the frame in the same process;
  * --loop N: nothing but N kz_denoise_motion calls of that kind on the first scene - the process to run under `rocprofv3 --kernel-trace --stats` for the two kernels'
    own times.
A build with -DKZ_MOTION_TILE=0 (scripts/build_variant.sh, KZ_LIB_PATH) times the row mapping of the id kernel the same way.
One JSON record in <out>/motion_rates.json (--tag: another file name, for a second run or a variant).
    python scripts/motion_rates.py [--reps 9] [--scenes C4,C3] [--out profiles/r20a_motion] [--tag run2]"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
from temporal_rates import med_ms, timed, turned      # noqa: E402  (the same clock and the same camera path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scenes", default="C4,C3")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20a_motion"))
    a = ap.parse_args()
    W, H = 1920, 1080
    scenes = {"C3": lambda: kz.scenes.hero_scene(W, H, 1, detail=2.0), "C4": lambda: kz.scenes.random_triangles(1000000, W, H, 1, sampler="pmj02bn", seed=1)}
    rec = {"width": W, "height": H, "reps": a.reps, "lib": os.path.basename(os.path.dirname(kz.abi.LIB_PATH)), "scenes": {}}
    for name in a.scenes.split(","):
        d = scenes[name]()
        start = copy.copy(d)
        start.camera = dict(d.camera)
        mover = next(i for i, m in enumerate(d.meshes) if m["light"] is None)
        both = []
        for _ in range(2):
            s = kz.Scene(copy.copy(d), device=0)
            s.set_aovs(7)
            s.set_variance(True)
            s.render()
            s.sync()
            both.append(s)
        st, sm = both
        step = [0]

        def nudge(s, move):
            step[0] += 1
            k = step[0] % 8
            if move:
                M = np.eye(4, dtype=np.float32)
                M[0, 3] = 0.002 * k
                s.set_transforms({mover: M})
            s.set_camera({"toWorld": turned(start, 0.25 * k)})      # (the films stay the first camera's: the cost does not depend on what they show)

        def temporal(k):
            nudge(st, False)
            return timed(lambda: st.denoise_temporal(iterations=k))

        def motion(k):
            nudge(sm, True)
            return timed(lambda: sm.denoise_motion(iterations=k))

        if a.loop:
            for _ in range(a.loop):
                motion(5)
            print(json.dumps({"loop": a.loop, "scene": name, "temporal_info": sm.temporal_info(), "motion_info": sm.motion_info()}))
            return
        for k in (1, 5):                                                # warm: every kernel of both calls, the buffers allocated
            temporal(k)
            motion(k)
        t = {c: {1: [], 5: []} for c in ("kz_denoise_motion", "kz_denoise_temporal")}
        for _ in range(a.reps):
            for k in (1, 5):
                t["kz_denoise_motion"][k].append(motion(k))
                t["kz_denoise_temporal"][k].append(temporal(k))
        r = {"call_ms": {c: {str(k): med_ms(v) for k, v in tk.items()} for c, tk in t.items()},
             "call_ms_all": {c: {str(k): [round(x * 1e3, 4) for x in v] for k, v in tk.items()} for c, tk in t.items()}}
        r["motion_minus_temporal_ms"] = {str(k): round(r["call_ms"]["kz_denoise_motion"][str(k)] - r["call_ms"]["kz_denoise_temporal"][str(k)], 4) for k in (1, 5)}
        r["motion_info"], r["temporal_info"] = sm.motion_info(), sm.temporal_info()
        r["found_history"] = {"motion": round(float((sm.temporal_history()[..., 8] > 1).mean()), 4), "temporal": round(float((st.temporal_history()[..., 8] > 1).mean()), 4)}
        ids_t, render_t = [], []
        sm.motion_ids()
        for _ in range(a.reps):
            ids_t.append(timed(sm.motion_ids))
            render_t.append(timed(sm.render, sm.sync))
        r["motion_ids_call_ms"], r["render_1spp_ms"] = med_ms(ids_t), med_ms(render_t)
        ids = sm.motion_ids()
        r["ids_hit_share"] = round(float((ids != kz.abi.KZ_MOTION_MISS).mean()), 4)
        rec["scenes"][name] = r
        print("%s: %s" % (name, json.dumps({k: r[k] for k in ("call_ms", "motion_minus_temporal_ms", "motion_ids_call_ms", "render_1spp_ms")})), file=sys.stderr, flush=True)
        st.close()
        sm.close()
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "motion_rates%s.json" % (("_" + a.tag) if a.tag else "")), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
