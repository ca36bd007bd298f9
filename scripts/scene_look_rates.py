"""What a material, light or transform edit of a resident scene costs (include/kazen_mi355x_edit.h), on C4 (1 M random triangles + 8 mesh lights,
1920 x 1080, pmj02bn), in ONE process: kz_scene_set_bsdfs of one row and of all rows, kz_scene_set_lights of all eight lights and a visibility toggle -
each against kz_scene_create + kz_scene_upload of the edited description, the only way without these calls - the first render after each, and
kz_scene_set_transforms of the eight soup meshes against kz_scene_set_vertices of the same meshes with host-transformed arrays, alternated frame by frame.
Host clock around calls that end in a device synchronise, one warm-up, medians of >= 10. One JSON line on stdout (and in --out).
--copy-probe runs a short fixed sequence of edits for a memory-copy trace (see profiles/r09a_scene_look/README.md); --summarise-copies prints such a trace."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
abi = kz.abi


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def med_ms(v):
    return 1e3 * float(np.median(v))


def rot_y(ang, about):
    c, s = np.cos(ang), np.sin(ang)
    T = lambda t: np.array([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1.0]])
    R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    return (T(about) @ R @ T(-np.asarray(about))).astype(np.float32)


def transform_rows(mats):
    rows = []
    for m, M in mats.items():
        k = abi.KzTransformUpdate()
        k.mesh = m
        k.toWorld[:] = np.asarray(M, np.float32).reshape(16).tolist()
        rows.append(k)
    return (abi.KzTransformUpdate * len(rows))(*rows)


def vertex_rows(arrays):
    return (abi.KzVertexUpdate * len(arrays))(*[abi.KzVertexUpdate(m, V.shape[0], V.ctypes.data_as(abi.f32p), N.ctypes.data_as(abi.f32p)) for m, (V, N) in arrays.items()])


def first_render_ms(sc):
    return 1e3 * timed(lambda: (sc.render(sample_begin=0, sample_end=1), sc.sync()))


def create_upload_s(desc, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        s = kz.Scene(desc, device=0)
        s.sync()
        out.append(time.perf_counter() - t0)
        s.close()
    return out


def rates(a):
    S = kz.scenes
    d = S.random_triangles(a.tris, 1920, 1080, 1024, sampler="pmj02bn", seed=1)
    rec = {"scene": "C4", "tris": a.tris, "frames": a.frames}
    sc = kz.Scene(d, device=0)
    lib = sc.lib
    sc.render(sample_begin=0, sample_end=1); sc.sync()
    rec["render_1spp_no_edit_ms"] = med_ms([timed(lambda: (sc.render(sample_begin=0, sample_end=1), sc.sync())) for _ in range(5)])
    lights = [m for m, x in enumerate(d.meshes) if x["light"] is not None]
    rows = [dict(d.meshes[m]["bsdf"]) for m in range(8)]

    # ---- materials: one row, all eight soup rows (the Python wrapper: flattening + the call)
    def one_row(f):
        return {3: dict(rows[3], roughness=0.2 + 0.05 * (f % 8))}

    def all_rows(f):
        return {m: dict(rows[m], roughness=0.15 + 0.05 * ((f + m) % 8)) for m in range(8)}

    for name, make in (("set_bsdfs_one_row", one_row), ("set_bsdfs_all_rows", all_rows)):
        sc.set_bsdfs(make(-1))
        t, first = [], []
        for f in range(a.frames):
            u = make(f)
            t.append(timed(lambda: sc.set_bsdfs(u)))
            first.append(first_render_ms(sc))
        rec[name + "_median_ms"], rec[name + "_first_render_1spp_median_ms"] = med_ms(t), float(np.median(first))
    # the call alone (rows prepared): one row
    cd = sc.desc.to_c()
    arr = (abi.KzBsdfUpdate * 1)(abi.KzBsdfUpdate(3, cd.bsdfs[3]))
    lib.kz_scene_set_bsdfs(sc.h, arr, 1)
    rec["set_bsdfs_one_row_c_call_median_ms"] = med_ms([timed(lambda: abi.check(lib, lib.kz_scene_set_bsdfs(sc.h, arr, 1))) for _ in range(a.frames)])
    rec["create_upload_edited_bsdfs_s"] = create_upload_s(sc.desc, a.builds)

    # ---- lights: all eight scaled; one visibility toggled
    orig = {m: dict(d.meshes[m]["light"]) for m in lights}
    sc.set_lights(orig)
    t, first = [], []
    for f in range(a.frames):
        u = {m: dict(l, intensity=20.0 + f) for m, l in orig.items()}
        t.append(timed(lambda: sc.set_lights(u)))
        first.append(first_render_ms(sc))
    rec["set_lights_all_eight_median_ms"], rec["set_lights_first_render_1spp_median_ms"] = med_ms(t), float(np.median(first))
    t, first = [], []
    for f in range(a.frames):
        u = {lights[0]: dict(orig[lights[0]], lightPrimaryVisibility=(f % 2 == 0))}
        t.append(timed(lambda: sc.set_lights(u)))
        first.append(first_render_ms(sc))
    rec["set_lights_visibility_toggle_median_ms"], rec["visibility_toggle_first_render_1spp_median_ms"] = med_ms(t), float(np.median(first))
    rec["create_upload_edited_lights_s"] = create_upload_s(sc.desc, a.builds)
    sc.set_lights(orig)

    # ---- a turntable of the eight soup meshes: kz_scene_set_transforms against kz_scene_set_vertices of host-transformed arrays, the C calls alone, alternated
    base = {m: (d.meshes[m]["V"], d.meshes[m]["N"]) for m in range(8)}
    centres = {m: base[m][0].astype(np.float64).mean(axis=0) for m in range(8)}
    # (on a twin replica of the same scene: kz_scene_set_vertices replaces a mesh's base data, so the two calls cannot take turns on one scene and stay a turntable)
    twin = kz.Scene(d, device=0)
    t_xf, t_sv, t_host = [], [], []
    for f in range(-1, a.frames):                                   # (frame -1: warm-up - staging, base data and the BVH2 go up)
        mats = {m: rot_y(0.01 * (f + 2), centres[m]) for m in range(8)}
        xr = transform_rows(mats)
        t0 = time.perf_counter()
        arrays = {m: S.transform_vertices(mats[m], *base[m]) for m in range(8)}
        th = time.perf_counter() - t0
        vr = vertex_rows(arrays)
        tv = timed(lambda: abi.check(lib, lib.kz_scene_set_vertices(twin.h, vr, 8)))
        tx = timed(lambda: abi.check(lib, lib.kz_scene_set_transforms(sc.h, xr, 8)))
        if f >= 0:
            t_xf.append(tx); t_sv.append(tv); t_host.append(th)
    rec["set_transforms_ms"], rec["set_vertices_ms"] = [1e3 * x for x in t_xf], [1e3 * x for x in t_sv]
    rec["set_transforms_median_ms"], rec["set_vertices_median_ms"] = med_ms(t_xf), med_ms(t_sv)
    rec["host_transform_numpy_median_ms"] = med_ms(t_host)
    spread = (max(t_sv) - min(t_sv)) / float(np.median(t_sv))
    rec["set_vertices_spread"] = spread
    rec["transforms_over_vertices"] = rec["set_transforms_median_ms"] / rec["set_vertices_median_ms"]
    rec["requirement_met"] = bool(rec["set_transforms_median_ms"] <= rec["set_vertices_median_ms"] * (1.0 + spread))
    # the same bits either way
    rec["device_tables_equal_the_twins"] = bool(all(np.array_equal(sc.table(t, 0), twin.table(t, 0)) for t in (0, 1, 2, 3)))
    twin.close()

    # ---- render rate after a turntable step beside a fresh scene's of the same positions
    def msamples(s):
        s.render(sample_begin=0, sample_end=a.spp); s.sync()
        return 1920 * 1080 * a.spp / min(timed(lambda: (s.render(sample_begin=0, sample_end=a.spp), s.sync())) for _ in range(3)) / 1e6
    rec["msamples_after_turntable"] = msamples(sc)
    meshes = list(sc.desc.meshes)
    for m in range(8):
        meshes[m] = dict(meshes[m], V=arrays[m][0], N=arrays[m][1])
    sc.desc.meshes = meshes
    fresh = kz.Scene(sc.desc, device=0)
    rec["msamples_fresh_of_those_positions"] = msamples(fresh)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if rec["requirement_met"] else 3


def copy_probe(a):
    """A fixed sequence for a memory-copy trace: upload, then ONE kz_scene_set_bsdfs of three rows, then kz_scene_set_transforms of the eight soup meshes twice."""
    S = kz.scenes
    d = S.random_triangles(a.tris, 256, 144, 16, sampler="pmj02bn", seed=1)
    sc = kz.Scene(d, device=0)
    sc.render(); sc.sync()
    nV = [int(d.meshes[m]["V"].shape[0]) for m in range(8)]
    print("probe: %d triangles; soup meshes hold %s vertices: base V / N = %s bytes each" % (a.tris, nV, [24 * n for n in nV]))
    sc.set_bsdfs({m: dict(d.meshes[m]["bsdf"], roughness=0.33) for m in (1, 4, 6)})
    centres = {m: d.meshes[m]["V"].astype(np.float64).mean(axis=0) for m in range(8)}
    lib = sc.lib
    for f in range(2):
        xr = transform_rows({m: rot_y(0.02 * (f + 1), centres[m]) for m in range(8)})
        abi.check(lib, lib.kz_scene_set_transforms(sc.h, xr, 8))
    sc.render(); sc.sync()
    return 0


def summarise_copies(path):
    rows = list(csv.DictReader(open(path)))
    if not rows:
        print("no memory copies in", path)
        return 1
    size_col = next((c for c in rows[0] if c.lower() in ("bytes", "size", "size_bytes")), None)
    print("columns:", ", ".join(rows[0].keys()))
    rows.sort(key=lambda r: int(r.get("Start_Timestamp", 0)))
    runs = []
    for r in rows:
        key = (r.get("Direction", "?"), int(r[size_col]) if size_col else -1)
        if runs and runs[-1][0] == key:
            runs[-1][1] += 1
        else:
            runs.append([key, 1])
    for (direction, size), n in runs[-60:]:
        print("%4d x %-28s %s" % (n, direction, ("%d B" % size) if size >= 0 else ""))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--spp", type=int, default=64, help="samples per pixel of the timed renders")
    ap.add_argument("--frames", type=int, default=10, help="timed calls per figure (after one warm-up)")
    ap.add_argument("--builds", type=int, default=3, help="kz_scene_create + kz_scene_upload timed per edited description")
    ap.add_argument("--out", default="")
    ap.add_argument("--copy-probe", action="store_true")
    ap.add_argument("--summarise-copies", default="")
    args = ap.parse_args()
    sys.exit(summarise_copies(args.summarise_copies) if args.summarise_copies else copy_probe(args) if args.copy_probe else rates(args))
