"""What kz_denoise_responsive's fast history is worth, on the CPU alone (no GPU): the C++ reference chain (tests/cpu_ref/kz_responsive_ref.cpp) on the oracle's
canonical films, 96 x 72, frames of 4 spp from the sample ranges [4f, 4f + 4). The sequences:
    static / orbit   DESIGN.md 4g's: eight frames of cornell_box, materials_scene and textured_scene, the camera at rest or turned by 2 degrees per frame; frame 8
                     against 1024 spp (static) or 256 spp from the last camera (orbit)
    mover 6 / 5      DESIGN.md 4h's: Cornell, eight frames, the short or the tall box slid by 0.04 per frame; frame 8 against 1024 spp of the last pose, the whole
                     frame and the mover's pixels
    light step       Cornell, a camera at rest, eight frames, then the lamp turns from white 15 to orange 12 (tests/film_cases.py NEW_LIGHT) and eight more
                     frames follow; frames 9, 12 and 16 against 1024 spp of the new lighting
Per sequence the MSE over the noisy frame's MSE for the responsive chain, the kz_motion_ref chain and the frame alone; for the orbits and the movers also the share of
eligible pixels (N_l > fastHistory) that the clamp changed in the last frame, from the same call with KZ_RESPONSIVE_CLAMP_OFF. --sweep runs every sequence over
fastHistory {2, 4, 8} x clampSigma {1, 2, 3} x radius {1, 2} and writes the table; without it the defaults alone.
    python scripts/responsive_quality.py [--sweep] [--out profiles/r21a_responsive]"""
import argparse
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
from cpu_refs import lib      # noqa: E402
from film_cases import _orbit, chains, frame_rgb, light_step, reference_frames, static_rows, translate      # noqa: E402

MAKE = {"cornell": kz.scenes.cornell_box, "materials": kz.scenes.materials_scene, "textured": kz.scenes.textured_scene}


def posed(spp, M, mover):
    d = kz.scenes.cornell_box(96, 72, spp)
    mesh = d.meshes[mover]
    V, N = kz.scenes.transform_vertices(M, mesh["V"], mesh["N"])
    d.meshes[mover] = dict(mesh, V=V, N=N)
    return d


def sequences(L, aov_lib):
    """name -> (frames, rows_of, {frame number: clean film}, mask of the mover's pixels in the last frame or None)"""
    seqs = {}
    for scene, make in MAKE.items():
        n = len(make(96, 72, 4).meshes)
        rows = (lambda n: lambda f: static_rows(kz, n))(n)
        seqs["static " + scene] = (reference_frames(kz, L, aov_lib, [make(96, 72, 4) for f in range(8)]), rows, {8: O.OracleScene(make(96, 72, 1024)).render_canonical(threads=0)}, None)
        seqs["orbit " + scene] = (reference_frames(kz, L, aov_lib, [_orbit(kz, make(96, 72, 4), 2.0 * f) for f in range(8)]), rows,
                                  {8: O.OracleScene(_orbit(kz, make(96, 72, 256), 14.0)).render_canonical(threads=0)}, None)
    for mover in (6, 5):
        at = lambda f: translate((-0.04 * f, 0.0, 0.02 * f)).astype(np.float32)
        frames = reference_frames(kz, L, aov_lib, [posed(4, at(f), mover) for f in range(8)])
        def rows(f, mover=mover, at=at):
            mats, prev = np.tile(np.eye(4, dtype=np.float32), (8, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (8, 1, 1))
            mats[mover], prev[mover] = at(f), at(max(f - 1, 0))
            return kz.motion_rows(mats, prev)
        seqs["mover %d" % mover] = (frames, rows, {8: O.OracleScene(posed(1024, at(7), mover)).render_canonical(threads=0)}, frames[-1][5] == mover)
    clean = O.OracleScene(light_step(kz, 1024, 8)).render_canonical(threads=0)
    seqs["light step"] = (reference_frames(kz, L, aov_lib, [light_step(kz, 4, f) for f in range(16)]), None, {9: clean, 12: clean, 16: clean}, None)
    return seqs


def ratios(pic, noisy, clean, b, mask=None):
    want = frame_rgb(clean, b).astype(np.float64)
    err = lambda x: ((frame_rgb(x, b).astype(np.float64) - want) ** 2)
    out = [float(err(pic).mean() / err(noisy).mean())]
    if mask is not None:
        out.append(float(err(pic)[mask].mean() / err(noisy)[mask].mean()))
    return [round(x, 4) for x in out]


def measure(L, seqs, base=None, **ropts):
    """name -> {"frame F": {chain: [whole frame, (the mover's pixels)]}, "clamped": share of the last frame's eligible pixels}; `base`: a record whose motion and alone
    chains are reused (they do not depend on the options)."""
    rec = {}
    for name, (frames, rows_of, cleans, mask) in seqs.items():
        pics, hists, counts = chains(kz, L, frames, rows_of, which=("responsive",) if base else ("responsive", "motion", "alone"), **ropts)
        b = frames[0][3]
        rec[name] = {}
        for f, clean in cleans.items():
            rec[name]["frame %d" % f] = {k: ratios(v[f - 1], frames[f - 1][0], clean, b, mask) for k, v in pics.items()}
            if base:
                for k in ("motion", "alone"):
                    rec[name]["frame %d" % f][k] = base[name]["frame %d" % f][k]
        eligible, clamped = counts[-1]
        rec[name]["clamped"] = round(clamped / eligible, 4) if eligible else 0.0
        rec[name]["eligible"] = round(eligible / (96 * 72), 4)
    return rec


def show(title, rec):
    print(title)
    for name, r in rec.items():
        for f, chains_ in r.items():
            if f.startswith("frame"):
                print("  %-18s %-9s responsive %-18s motion %-18s alone %-18s clamped %.1f %% of the %.1f %% eligible" % (
                    name, f, chains_["responsive"], chains_["motion"], chains_["alone"], 100 * r["clamped"], 100 * r["eligible"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21a_responsive"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    L, aov_lib = lib("responsive", tmp), lib("aov", tmp)
    seqs = sequences(L, aov_lib)
    os.makedirs(a.out, exist_ok=True)
    base = measure(L, seqs)
    show("defaults", base)
    with open(os.path.join(a.out, "responsive_quality.json"), "w") as fh:
        fh.write(json.dumps(base) + "\n")
    if a.sweep:
        with open(os.path.join(a.out, "responsive_sweep.jsonl"), "w") as fh:
            for fh_ in (2, 4, 8):
                for k in (1.0, 2.0, 3.0):
                    for r in (1, 2):
                        rec = measure(L, seqs, base, fast_history=fh_, clamp_sigma=k, radius=r)
                        show("fastHistory %d, clampSigma %g, radius %d" % (fh_, k, r), rec)
                        fh.write(json.dumps({"fastHistory": fh_, "clampSigma": k, "radius": r, "sequences": rec}) + "\n")
                        fh.flush()


if __name__ == "__main__":
    main()
