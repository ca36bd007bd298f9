"""What kz_denoise_motion's history is worth while a mesh moves, on the CPU alone (no GPU): the C++ reference chain (tests/cpu_ref/kz_motion_ref.cpp) on the oracle's
canonical films. Cornell box, 96 x 72, eight frames of 4 spp from the sample ranges [4f, 4f + 4), a static camera; the short box slides by a fixed step per frame,
its transformed vertices baked into each frame's description (scenes.transform_vertices: the arithmetic of kz_scene_set_transforms). MSE of frame 8 over the MSE of
its noisy film, against 1024 spp of the last pose, for: the motion chain; the same chain with every row STATIC (a history that ignores the motion); the frame alone -
which is also what kz_denoise_temporal gives on this sequence, since it restarts after every transform. Printed, and written to <out>/motion_quality_mesh<m>.json.
    python scripts/motion_quality.py [--frames 8] [--step 0.04] [--mesh 6] [--out profiles/r20a_motion]"""
import argparse
import copy
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
kz = importlib.import_module("nano-kazen_amd")
import oracle as O      # noqa: E402
from cpu_refs import AovRef, MomentRef, lib, ref_denoise_motion, ref_ids      # noqa: E402
from film_cases import GUIDES, frame_rgb, static_rows, translate      # noqa: E402

SHORT_BOX = 6                                                         # scenes.cornell_box: the short box (metallic, roughness 0.3); 5 is the tall one (dielectric grey, roughness 0.5)


def posed(spp, M, mover):
    d = kz.scenes.cornell_box(96, 72, spp)
    mesh = d.meshes[mover]
    V, N = kz.scenes.transform_vertices(M, mesh["V"], mesh["N"])
    d.meshes[mover] = dict(mesh, V=V, N=N)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--step", type=float, default=0.04)
    ap.add_argument("--mesh", type=int, default=SHORT_BOX)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20a_motion"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    mref, tref, aref = lib("motion", tmp), lib("temporal", tmp), lib("aov", tmp)
    n_meshes = len(kz.scenes.cornell_box(96, 72, 4).meshes)
    at = lambda f: translate((-a.step * f, 0.0, 0.5 * a.step * f)).astype(np.float32)
    mats = np.tile(np.eye(4, dtype=np.float32), (n_meshes, 1, 1))
    hist = {"motion": None, "static rows": None}
    prev_mats, view = None, None
    for f in range(a.frames):
        d = posed(4, at(f), a.mesh)
        mats[a.mesh] = at(f)
        mr = MomentRef(tref, d)
        b = mr.border
        noisy, moment = mr.film(4 * f, 4 * f + 4), mr.moment_film(4 * f, 4 * f + 4)
        films = [AovRef(aref, d).film(g, 4 * f, 4 * f + 4) for g in GUIDES]
        ids = ref_ids(mref, d)
        view = kz.temporal_view(d.camera)
        rows = {"motion": kz.motion_rows(mats, prev_mats), "static rows": static_rows(kz, n_meshes)}
        out = {}
        for k in hist:
            out[k], hist[k], _ = ref_denoise_motion(mref, kz, noisy, moment, *films, border=b, samples=4, current=view, previous=view if f else None, history=hist[k], ids=ids, rows=rows[k])
        prev_mats = mats.copy()
    out["frame alone"], _, _ = ref_denoise_motion(mref, kz, noisy, moment, *films, border=b, samples=4, current=view, ids=ids, rows=rows["motion"])
    clean = O.OracleScene(posed(1024, at(a.frames - 1), a.mesh)).render_canonical(threads=0)
    want = frame_rgb(clean, b).astype(np.float64)
    mse = lambda x: float(((frame_rgb(x, b).astype(np.float64) - want) ** 2).mean())
    box = ids == a.mesh
    mse_box = lambda x: float((((frame_rgb(x, b).astype(np.float64) - want) ** 2)[box]).mean())
    rec = {"mesh": a.mesh, "frames": a.frames, "step": a.step, "box_pixels": int(box.sum()), "found_history": {k: round(float((h[..., 8] > 1).mean()), 4) for k, h in hist.items()},
           "found_history_on_the_box": {k: round(float((h[..., 8][box] > 1).mean()), 4) for k, h in hist.items()},
           "mse_over_noisy": {k: round(mse(v) / mse(noisy), 4) for k, v in out.items()}, "mse_over_noisy_on_the_box": {k: round(mse_box(v) / mse_box(noisy), 4) for k, v in out.items()}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "motion_quality_mesh%d.json" % a.mesh), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
