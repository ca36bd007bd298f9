"""kz_denoise and kz_denoise_variance at 1920 x 1080 with all three guides, 1..5 iterations: the parent commit's library against this tree's, one replica per
library in ONE process on C3 (hero scene, 4 spp), alternating call by call in either order, medians of 9, each beside the parent's own spread; plus the bits of
both calls against the parent's and against the direct-form variant's. For a change that must leave both calls where they were (profiles/r18a_denoise_once).
    scripts/build_rev.sh <parent> parent && scripts/build_variant.sh dn_direct -DKZ_DN_LDS_MAX_STEP=0 && python scripts/denoise_ab.py [out directory]
One JSON record in <out directory>/denoise_ab.json (default: profiles/r18a_denoise_once)."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
V = os.path.join(ROOT, "nano-kazen_amd", "csrc", "variants")
W, H, REPS = 1920, 1080, 9

def timed(fn):
    t0 = time.perf_counter(); fn(); return time.perf_counter() - t0      # (both calls return synchronised)

def replica(d, lib=None):
    s = kz.Scene(d, device=0, lib=lib) if lib is not None else kz.Scene(d, device=0)
    s.set_aovs(7); s.set_variance(True)
    s.render(sample_begin=0, sample_end=4); s.sync()
    return s

d = kz.scenes.hero_scene(W, H, 4, detail=2.0)
plib = kz.abi.load_library(os.path.join(V, "parent", "libkazen_mi355x.so"))
dlib = kz.abi.load_library(os.path.join(V, "dn_direct", "libkazen_mi355x.so"))
this, parent, direct = replica(d), replica(d, plib), replica(d, dlib)
calls = {"kz_denoise": lambda s, k: s.denoise(iterations=k, sigma_color=2.0), "kz_denoise_variance": lambda s, k: s.denoise_variance(iterations=k)}
rec = {"width": W, "height": H, "reps": REPS, "same_bits": {}, "calls": {}}
for c, fn in calls.items():
    for k in range(1, 6):
        out = []
        for s in (this, parent, direct):
            fn(s, k); out.append(s.denoised_film().view(np.uint32))
        rec["same_bits"]["%s_%d" % (c, k)] = {"parent": bool(np.array_equal(out[0], out[1])), "dn_direct": bool(np.array_equal(out[0], out[2]))}
rec["picture_same_bits_as_parent"] = bool(np.array_equal(this.film().view(np.uint32), parent.film().view(np.uint32)))
direct.close()
for _ in range(3):                                                        # warm every shape of the timed window
    for c, fn in calls.items():
        for k in range(1, 6):
            fn(parent, k); fn(this, k)
ok = True
for order in ("parent_first", "this_first"):
    t = {c: {k: {"this": [], "parent": []} for k in range(1, 6)} for c in calls}
    for _ in range(REPS):
        for k in range(1, 6):
            for c, fn in calls.items():
                for who, s in ((("parent", parent), ("this", this)) if order == "parent_first" else (("this", this), ("parent", parent))):
                    t[c][k][who].append(timed(lambda: fn(s, k)))
    rec["calls"][order] = {}
    for c in calls:
        rec["calls"][order][c] = {}
        for k in range(1, 6):
            m, p = t[c][k]["this"], t[c][k]["parent"]
            pm, mm = float(np.median(p)), float(np.median(m))
            inside = abs(mm - pm) <= max(p) - min(p)
            ok &= inside
            r = rec["calls"][order][c][k] = {"this_ms": round(mm * 1e3, 4), "parent_ms": round(pm * 1e3, 4), "ratio": round(mm / pm, 4), "parent_spread": round((max(p) - min(p)) / pm, 4),
                                             "inside_parent_spread": bool(inside), "this_all_ms": [round(x * 1e3, 4) for x in m], "parent_all_ms": [round(x * 1e3, 4) for x in p]}
            print(order, c, k, {x: r[x] for x in ("this_ms", "parent_ms", "ratio", "parent_spread", "inside_parent_spread")}, flush=True)
rec["all_inside_parent_spread"] = bool(ok)
print(json.dumps(rec["same_bits"]), rec["picture_same_bits_as_parent"], flush=True)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18a_denoise_once")
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "denoise_ab.json"), "w").write(json.dumps(rec) + "\n")
this.close(); parent.close()
