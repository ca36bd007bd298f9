"""The rows of a scene's tables (Scene.table) as numpy records, the offsets into KzParams the tests read, and the check that a refit left every box conservative.
A support module beside the tests, like sample_corners.py: imported, never collected."""
import numpy as np

NODE = np.dtype([("q", "<f4", 12), ("child", "<u4", 2), ("pad", "<u4", 2)])
NODE4 = np.dtype([("p", "<f4", 3), ("sx", "<f4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("sy", "<f4"), ("sz", "<f4"), ("child", "<u4", 4)])
TRI = np.dtype([("p0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("mesh", "<u4"), ("prim", "<u4"), ("gid", "<u4")])
SHADE = np.dtype([("p", "<f4", 9), ("n", "<f4", 9), ("uv", "<f4", 6), ("mesh", "<u4"), ("prim", "<u4"), ("bsdf", "<u4"), ("lightFlags", "<u4")])
LIGHT = np.dtype([("radiance", "<f4", 3), ("primaryVisibility", "<i4"), ("mesh", "<u4"), ("triOffset", "<u4"), ("nF", "<u4"), ("cdfOffset", "<u4"),
                  ("normalization", "<f4"), ("hasN", "<u4"), ("pad", "<u4", 2)])
# offsets into KzParams (nano-kazen_amd/csrc/kz_internal.h), pinned by tests/test_scene_edit_cpu.py::test_param_offsets_and_update_struct
P_NIL, P_ILLO, P_ILHI, P_BEAMOK, P_SIZE = 300, 304, 316, 344, 400


def deq(p, q, s):
    return (np.float32(p) + np.float32(q) * np.float32(s)).astype(np.float32)      # q * s exact, one rounding in the add (kz_bvh.cpp deq)


def check_refit(kz, sc):
    nodes = sc.table(kz.abi.KZ_TABLE_NODES).view(NODE)
    nodes4 = sc.table(kz.abi.KZ_TABLE_NODES4).view(NODE4)
    tris = sc.table(kz.abi.KZ_TABLE_TRIS).view(TRI)
    shade = sc.table(kz.abi.KZ_TABLE_SHADE).view(SHADE)
    verts = shade["p"].reshape(-1, 3, 3)
    # leaf triangles from the shading records, as the build forms them
    p = verts[tris["gid"]]
    assert np.array_equal(tris["p0"], p[:, 0]) and np.array_equal(tris["e1"], (p[:, 1] - p[:, 0]).astype(np.float32))
    tri_lo, tri_hi = p.min(axis=1), p.max(axis=1)

    def leaf_range(ref):
        s = (ref & 0x7fffffff) >> 3
        return s, s + (ref & 7) + 1

    # BVH2: every triangle inside its leaf's box and every box on its path
    stack, checked = [(0, [])], 0
    while stack:
        h, path = stack.pop()
        q = nodes[h]["q"]
        for k in range(2):
            box = (q[6 * k:6 * k + 3], q[6 * k + 3:6 * k + 6])
            c = int(nodes[h]["child"][k])
            if c & 0x80000000:
                a, b = leaf_range(c)
                for lo, hi in path + [box]:
                    assert (tri_lo[a:b] >= lo).all() and (tri_hi[a:b] <= hi).all()
                checked += b - a
            else:
                stack.append((c, path + [box]))
    assert checked == len(tris)
    # BVH4: every triangle inside every dequantised slot box on its path
    stack, checked = [(0, [])], 0
    while stack:
        h, path = stack.pop()
        nd = nodes4[h]
        s = (nd["sx"], nd["sy"], nd["sz"])
        for i in range(4):
            ql = [(int(nd["qlo"][a]) >> (8 * i)) & 255 for a in range(3)]
            qh = [(int(nd["qhi"][a]) >> (8 * i)) & 255 for a in range(3)]
            if ql[0] > qh[0]:
                continue                                    # empty slot
            box = (np.array([deq(nd["p"][a], ql[a], s[a]) for a in range(3)]), np.array([deq(nd["p"][a], qh[a], s[a]) for a in range(3)]))
            c = int(nd["child"][i])
            if c & 0x80000000:
                a0, b0 = leaf_range(c)
                for lo, hi in path + [box]:
                    assert (tri_lo[a0:b0] >= lo).all() and (tri_hi[a0:b0] <= hi).all()
                checked += b0 - a0
            else:
                stack.append((c, path + [box]))
    assert checked == len(tris)
    # light CDFs = kz_kat_dpdf of the new areas; the invisible-light box holds the invisible lights' triangles
    lights = sc.table(kz.abi.KZ_TABLE_LIGHTS).view(LIGHT)
    cdf = sc.table(kz.abi.KZ_TABLE_CDF).view(np.float32)
    prm = sc.table(kz.abi.KZ_TABLE_PARAMS)
    il_lo, il_hi = prm[P_ILLO:P_ILLO + 12].view(np.float32), prm[P_ILHI:P_ILHI + 12].view(np.float32)
    for lr in lights:
        v = verts[lr["triOffset"]:lr["triOffset"] + lr["nF"]]
        e1, e2 = (v[:, 1] - v[:, 0]).astype(np.float32), (v[:, 2] - v[:, 0]).astype(np.float32)
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = (np.float32(0.5) * np.sqrt(cx * cx + cy * cy + cz * cz)).astype(np.float32)
        want, sn = np.zeros(lr["nF"] + 1, np.float32), np.zeros(2, np.float32)
        assert sc.lib.kz_kat_dpdf(int(lr["nF"]), area.ctypes.data_as(kz.abi.f32p), want.ctypes.data_as(kz.abi.f32p), sn.ctypes.data_as(kz.abi.f32p)) == 0
        assert np.array_equal(cdf[lr["cdfOffset"]:lr["cdfOffset"] + lr["nF"] + 1], want) and lr["normalization"] == sn[1]
        if not lr["primaryVisibility"]:
            assert (v.reshape(-1, 3) >= il_lo).all() and (v.reshape(-1, 3) <= il_hi).all()
