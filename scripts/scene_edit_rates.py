"""What an edit of a resident scene costs (include/kazen_mi355x_edit.h), on C4 (1 M random triangles + 8 mesh lights, 1920 x 1080, pmj02bn):
kz_scene_set_vertices of all 1 M triangles against kz_scene_create + kz_scene_upload, kz_scene_set_camera + the beam-list rebuild it causes, and the
render rate after a mild refit against a fresh build's. One JSON line on stdout (and in --out). profiles/r08a_scene_edit/README.md holds a run."""
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def render_s(sc, spp, **kw):
    sc.render(sample_begin=0, sample_end=spp, **kw)
    sc.sync()
    return timed(lambda: (sc.render(sample_begin=0, sample_end=spp, **kw), sc.sync()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--spp", type=int, default=64, help="samples per pixel of the timed renders")
    ap.add_argument("--frames", type=int, default=10, help="kz_scene_set_vertices calls timed")
    ap.add_argument("--builds", type=int, default=3, help="kz_scene_create + kz_scene_upload timed")
    ap.add_argument("--noise", type=float, default=0.001, help="per-vertex noise of a mild refit (C4 edges are 0.02)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    d = kz.scenes.random_triangles(a.tris, 1920, 1080, 1024, sampler="pmj02bn", seed=1)
    base = [(m["V"].copy(), m["N"]) for m in d.meshes[:8]]
    rec = {"scene": "C4", "tris": a.tris, "spp": a.spp}

    builds = []
    for _ in range(a.builds):
        t0 = time.perf_counter()
        sc = kz.Scene(d, device=0)
        sc.sync()
        builds.append(time.perf_counter() - t0)
        info = sc.bvh_info()
        if _ < a.builds - 1:
            sc.close()
    rec["create_upload_s"] = sorted(builds)
    rec["create_upload_median_s"] = float(np.median(builds))
    rec["build_s"] = info["buildSeconds"]
    rec["sah_build"] = info["sahCost"]
    pix = 1920 * 1080
    t_fresh = min(render_s(sc, a.spp) for _ in range(3))
    rec["msamples_fresh"] = pix * a.spp / t_fresh / 1e6

    # set_camera + the beam lists it leaves unbuilt: the first render after the edit against a render that reuses its lists
    cam0 = dict(d.camera)
    cams = [{"toWorld": kz.scenes.look_at((0.1 * np.sin(k), 0.05, 3.4), (0, 0, 0), (0, 1, 0))} for k in range(1, 6)]
    t_cam, t_first, t_again = [], [], []
    for c in cams:
        t_cam.append(timed(lambda: sc.set_camera(c)))
        t_first.append(timed(lambda: (sc.render(sample_begin=0, sample_end=1), sc.sync())))
        t_again.append(timed(lambda: (sc.render(sample_begin=0, sample_end=1), sc.sync())))
    sc.set_camera({"toWorld": cam0["toWorld"]})
    rec["set_camera_median_ms"] = 1e3 * float(np.median(t_cam))
    rec["render_1spp_after_set_camera_median_ms"] = 1e3 * float(np.median(t_first))
    rec["render_1spp_again_median_ms"] = 1e3 * float(np.median(t_again))

    # set_vertices of all eight soup meshes (every one of the 1 M triangles), each frame a new mild deformation of the BUILD's positions
    t_set = []
    for f in range(a.frames):
        upd = {m: (V + rng.normal(size=V.shape).astype(np.float32) * np.float32(a.noise), N) for m, (V, N) in enumerate(base)}
        t_set.append(timed(lambda: sc.set_vertices(upd)))
    rec["set_vertices_s"] = t_set
    rec["set_vertices_median_ms"] = 1e3 * float(np.median(t_set))
    t_host = timed(lambda: sc.bvh_info())                                 # the lazy host refit, paid here once
    rec["host_refit_on_first_read_ms"] = 1e3 * t_host
    rec["sah_refit"] = sc.bvh_info()["sahCost"]
    t_refit = min(render_s(sc, a.spp) for _ in range(3))
    rec["msamples_after_refit"] = pix * a.spp / t_refit / 1e6
    fresh = kz.Scene(sc.desc, device=0)
    rec["sah_fresh_of_refit_positions"] = fresh.bvh_info()["sahCost"]
    t_fresh2 = min(render_s(fresh, a.spp) for _ in range(3))
    rec["msamples_fresh_of_refit_positions"] = pix * a.spp / t_fresh2 / 1e6
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
