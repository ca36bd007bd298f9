#!/usr/bin/env python3
"""The fixtures that let the tests on the reference's scene/2022_q1 files and published pictures run without a reference checkout. Data only - no reference
text, no reference file copied:

  tests/golden/q1_published_pngs.npz   block statistics of the 22 published 4096-spp pictures doc/2022_q1/img/param/<name>.png (1920 x 1080 sRGB), what
                                       tests/test_xmlscene.py::test_reference_scene_files_match_their_published_pngs compares the oracle's renders to:
                                         names       (22,)            the picture of each row
                                         lin_blocks  (22, 27, 48)     mean linear radiance over 40 x 40-pixel blocks (sRGB decoded, channels averaged)
                                         clipped     (22, 27, 48)     some pixel of the 40 x 40 block has a channel at 255
                                         srgb_blocks (22, 9, 16, 3)   mean sRGB value per channel over 120 x 120-pixel blocks
                                         clipped9    (22, 9, 16)      some pixel of the 120 x 120 block has a channel at 255
  tests/golden/q1_warmstudio.npz       scene/2022_q1/WarmStudio/WarmStudio.xml flattened like q1_default_m0_r0.5.npz (make_q1_scene.py): the arrays the
                                       loader produces + the scene's parameters as JSON (kz.scenes.load_npz reads it)

With q1_default_m0_r0.5.npz and q1_params.json they are what tests/conftest.py::q1_scene_dir writes back out as scene files. Only runs where /root/reference
exists; the .npz files are the committed fixtures.

    python tests/golden/make_q1_files.py
"""
import glob
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
kz = importlib.import_module("nano-kazen_amd")
REF = "/root/reference"
PNGS = os.path.join(REF, "doc", "2022_q1", "img", "param")
WARMSTUDIO = os.path.join(REF, "scene", "2022_q1", "WarmStudio", "WarmStudio.xml")


def pin_statistics():
    from PIL import Image
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PNGS, "*.png")))
    rows = {"lin_blocks": [], "clipped": [], "srgb_blocks": [], "clipped9": []}
    for name in names:
        png = np.asarray(Image.open(os.path.join(PNGS, name + ".png")).convert("RGB"), np.float64) / 255
        assert png.shape == (1080, 1920, 3), name
        lin_png = np.where(png <= 0.04045, png / 12.92, np.power((png + 0.055) / 1.055, 2.4))        # common.cpp:368-382
        rows["clipped"].append((png >= 1.0).any(axis=2).reshape(27, 40, 48, 40).any(axis=(1, 3)))
        rows["lin_blocks"].append(lin_png.mean(axis=2).reshape(27, 40, 48, 40).mean(axis=(1, 3)))
        rows["clipped9"].append((png >= 1.0).any(axis=2).reshape(9, 120, 16, 120).any(axis=(1, 3)))
        rows["srgb_blocks"].append(png.reshape(9, 120, 16, 120, 3).mean(axis=(1, 3)))
    out = os.path.join(HERE, "q1_published_pngs.npz")
    np.savez_compressed(out, names=np.array(names), **{k: np.stack(v) for k, v in rows.items()})
    print("wrote %s: %d pictures, %.2f MB" % (out, len(names), os.path.getsize(out) / 1e6))


def flatten_warmstudio():
    d = kz.xmlscene.load_xml(WARMSTUDIO)
    arrays, meshes = {}, []
    for i, m in enumerate(d.meshes):
        for k in ("V", "F", "N", "UV"):
            if m[k] is not None:
                arrays["m%d_%s" % (i, k)] = m[k]
        meshes.append({"bsdf": m["bsdf"], "light": m["light"], "has": [k for k in ("V", "F", "N", "UV") if m[k] is not None]})
    cam = dict(d.camera)
    arrays["camera_toWorld"] = np.asarray(cam.pop("toWorld"), np.float32)
    meta = {"source": "scene/2022_q1/WarmStudio/WarmStudio.xml", "meshes": meshes, "camera": cam, "sampler": d.sampler, "integrator": d.integrator,
            "background": d.background, "n_tris": d.n_tris()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    out = os.path.join(HERE, "q1_warmstudio.npz")
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d meshes, %d triangles, %.2f MB" % (out, len(meshes), d.n_tris(), os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    pin_statistics()
    flatten_warmstudio()
