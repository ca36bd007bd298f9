"""The denoise calls at 1920 x 1080 with all three guides: the parent commit's library against this tree's, one replica per library (and call) in ONE process on
C3 (hero scene, 4 spp), alternating call by call in either order, medians of 9, each beside the parent's own spread; plus the bits against the parent's. For a
change that must leave the calls where they were (profiles/r18a_denoise_once, profiles/r22a_history_once). Two sections:
  spatial  kz_denoise and kz_denoise_variance at 1..5 iterations; the bits also against the direct-form variant's (scripts/build_variant.sh dn_direct -DKZ_DN_LDS_MAX_STEP=0)
  history  kz_denoise_temporal, kz_denoise_motion and kz_denoise_responsive at 1 and 5 iterations. Between the calls, outside the clock, the camera turns by a quarter
           of a degree and - motion and responsive - mesh 0 moves (scripts/responsive_rates.py's path), so the id plane and the moved-row path run. Both libraries'
           replicas of a call see the same sequence of edits and calls; at its end the picture, the history and the fast plane are compared bit for bit.
    scripts/build_rev.sh <parent> parent && python scripts/denoise_ab.py [out directory] [spatial,history]
One JSON record in <out directory>/denoise_ab.json (default: profiles/r22a_history_once, both sections)."""
import copy, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
from temporal_rates import turned      # noqa: E402  (the camera path of the *_rates scripts)
V = os.path.join(ROOT, "nano-kazen_amd", "csrc", "variants")
W, H, REPS = 1920, 1080, 9
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22a_history_once")
SECTIONS = (sys.argv[2] if len(sys.argv) > 2 else "spatial,history").split(",")

def timed(fn):
    t0 = time.perf_counter(); fn(); return time.perf_counter() - t0      # (every call returns synchronised)

def replica(d, lib=None):
    s = kz.Scene(d, device=0, lib=lib) if lib is not None else kz.Scene(d, device=0)
    s.set_aovs(7); s.set_variance(True)
    s.render(sample_begin=0, sample_end=4); s.sync()
    return s

def cell(m, p):
    """One cell of the table: this tree's nine (m) beside the parent's (p); inside = |median(this) - median(parent)| <= max(parent) - min(parent)."""
    pm, mm = float(np.median(p)), float(np.median(m))
    return {"this_ms": round(mm * 1e3, 4), "parent_ms": round(pm * 1e3, 4), "ratio": round(mm / pm, 4), "parent_spread": round((max(p) - min(p)) / pm, 4),
            "inside_parent_spread": bool(abs(mm - pm) <= max(p) - min(p)), "this_all_ms": [round(x * 1e3, 4) for x in m], "parent_all_ms": [round(x * 1e3, 4) for x in p]}

def alternate(calls, shapes, pairs, prepare):
    """Both orders of the alternation over calls x shapes; pairs[c] = {"this": replica, "parent": replica}; prepare(c, replica, k) does what is outside the clock
    and returns the call to time. -> (record, cells outside the parent's spread)."""
    out, outside = {}, 0
    for order in ("parent_first", "this_first"):
        t = {c: {k: {"this": [], "parent": []} for k in shapes} for c in calls}
        for _ in range(REPS):
            for k in shapes:
                for c in calls:
                    for who in (("parent", "this") if order == "parent_first" else ("this", "parent")):
                        t[c][k][who].append(timed(prepare(c, pairs[c][who], k)))
        out[order] = {c: {k: cell(t[c][k]["this"], t[c][k]["parent"]) for k in shapes} for c in calls}
        for c in calls:
            for k in shapes:
                r = out[order][c][k]
                outside += not r["inside_parent_spread"]
                print(order, c, k, {x: r[x] for x in ("this_ms", "parent_ms", "ratio", "parent_spread", "inside_parent_spread")}, flush=True)
    return out, outside

same = lambda a, b: bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
d = kz.scenes.hero_scene(W, H, 4, detail=2.0)
plib = kz.abi.load_library(os.path.join(V, "parent", "libkazen_mi355x.so"))
rec = {"width": W, "height": H, "reps": REPS, "sections": SECTIONS}

if "spatial" in SECTIONS:
    dlib = kz.abi.load_library(os.path.join(V, "dn_direct", "libkazen_mi355x.so"))
    this, parent, direct = replica(d), replica(d, plib), replica(d, dlib)
    calls = {"kz_denoise": lambda s, k: s.denoise(iterations=k, sigma_color=2.0), "kz_denoise_variance": lambda s, k: s.denoise_variance(iterations=k)}
    rec["same_bits"] = {}
    for c, fn in calls.items():
        for k in range(1, 6):
            out = []
            for s in (this, parent, direct):
                fn(s, k); out.append(s.denoised_film())
            rec["same_bits"]["%s_%d" % (c, k)] = {"parent": same(out[0], out[1]), "dn_direct": same(out[0], out[2])}
    rec["picture_same_bits_as_parent"] = same(this.film(), parent.film())
    direct.close()
    for _ in range(3):                                                        # warm every shape of the timed window
        for c, fn in calls.items():
            for k in range(1, 6):
                fn(parent, k); fn(this, k)
    rec["calls"], outside = alternate(list(calls), range(1, 6), {c: {"this": this, "parent": parent} for c in calls}, lambda c, s, k: lambda: calls[c](s, k))
    rec["all_inside_parent_spread"] = outside == 0
    print(json.dumps(rec["same_bits"]), rec["picture_same_bits_as_parent"], flush=True)
    this.close(); parent.close()

if "history" in SECTIONS:
    calls = ("kz_denoise_temporal", "kz_denoise_motion", "kz_denoise_responsive")
    start = copy.copy(d); start.camera = dict(d.camera)
    mover = next(i for i, m in enumerate(d.meshes) if m["light"] is None)
    pairs = {c: {"this": replica(copy.copy(d)), "parent": replica(copy.copy(d), plib)} for c in calls}
    steps = {}                                                                # per replica: how many calls it has seen - equal on both sides of a pair at every call

    def prepare(c, s, k):
        j = steps[id(s)] = steps.get(id(s), 0) + 1
        if c != "kz_denoise_temporal":
            M = np.eye(4, dtype=np.float32)
            M[0, 3] = 0.002 * (j % 8)
            s.set_transforms({mover: M})
        s.set_camera({"toWorld": turned(start, 0.25 * (j % 8))})              # (the films stay the first camera's: the cost does not depend on what they show)
        fn = {"kz_denoise_temporal": s.denoise_temporal, "kz_denoise_motion": s.denoise_motion, "kz_denoise_responsive": s.denoise_responsive}[c]
        return lambda: fn(iterations=k)

    for _ in range(3):                                                        # warm: every kernel of every call, the histories long enough for pass B to run
        for k in (1, 5):
            for c in calls:
                for who in ("parent", "this"):
                    prepare(c, pairs[c][who], k)()
    rec["history_calls"], outside = alternate(calls, (1, 5), pairs, prepare)
    rec["history_cells_outside_parent_spread"] = outside
    rec["history_same_bits_as_parent"] = {}
    for c in calls:                                                           # after the same sequence on both sides: the result, the history and the fast plane
        a, b = pairs[c]["this"], pairs[c]["parent"]
        bits = {"calls": steps[id(a)], "picture": same(a.denoised_film(), b.denoised_film()), "temporal_history": same(a.temporal_history(), b.temporal_history()),
                "motion_info": list(a.motion_info()[1])}
        assert steps[id(a)] == steps[id(b)]
        if c == "kz_denoise_responsive":
            bits["responsive_fast"] = same(a.responsive_fast(), b.responsive_fast())
        rec["history_same_bits_as_parent"][c] = bits
        a.close(); b.close()
    print(json.dumps(rec["history_same_bits_as_parent"]), flush=True)

os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "denoise_ab.json"), "w").write(json.dumps(rec) + "\n")
