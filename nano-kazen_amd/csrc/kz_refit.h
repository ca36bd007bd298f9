// kz_refit.h - the box arithmetic of the BVH build that a refit repeats (kz_bvh.cpp on the host, kz_refit.hip on the device, kz_edit.cpp's
// host refit): one text, compiled for both sides, so that a refit on either side writes the bits the build would write for the same boxes.
// Every operation is a single IEEE operation (no contraction: -ffp-contract=off, and the dequantisation is spelled with explicit roundings),
// min / max keep the FIRST of two equal values (std::min / std::max: a box grown in any grouping of the same sequence keeps the same zero
// signs), and the exponent of frexp is read from the bits (glibc's answer for every float, LAB_NOTES H17).
#pragma once
#include "kz_internal.h"

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define KZ_HD __host__ __device__ inline
#else
#define KZ_HD inline
#endif

KZ_HD float kzMin(float a, float b) { return b < a ? b : a; }        // std::min(a, b)
KZ_HD float kzMax(float a, float b) { return a < b ? b : a; }        // std::max(a, b)
KZ_HD float kzAbs(float a) { uint32_t u; __builtin_memcpy(&u, &a, 4); u &= 0x7fffffffu; float r; __builtin_memcpy(&r, &u, 4); return r; }
KZ_HD float kzPow2(int e) { const uint32_t u = (uint32_t)(e + 127) << 23; float r; __builtin_memcpy(&r, &u, 4); return r; }     // 2^e, e in [-126, 127]
// the exponent std::frexp stores for x > 0: x = m * 2^e, m in [0.5, 1); 0 for 0, inf and NaN (as glibc)
KZ_HD int kzFrexpExp(float x) {
    uint32_t u; __builtin_memcpy(&u, &x, 4); u &= 0x7fffffffu;
    const int be = (int)(u >> 23);
    if (u == 0 || be == 255) return 0;
    if (be) return be - 126;
    int top = 31; while (!((u >> top) & 1u)) --top;                  // subnormal: x = m * 2^-149
    return top + 1 - 149;
}
// the kernels' dequantisation p + q * s: q * s is exact (s a power of two, q < 256), one rounding in the add
KZ_HD float kzDeq(float p, uint32_t q, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(p, __fmul_rn((float)q, s));
#else
    volatile float prod = (float)q * s; return p + prod;
#endif
}

struct KzBox { float lo[3], hi[3]; };
KZ_HD void kzBoxReset(KzBox &b) { for (int a = 0; a < 3; ++a) { b.lo[a] = __builtin_inff(); b.hi[a] = -__builtin_inff(); } }
KZ_HD void kzBoxGrow(KzBox &b, const float *p) { for (int a = 0; a < 3; ++a) { b.lo[a] = kzMin(b.lo[a], p[a]); b.hi[a] = kzMax(b.hi[a], p[a]); } }
KZ_HD void kzBoxGrow(KzBox &b, const KzBox &c) { for (int a = 0; a < 3; ++a) { b.lo[a] = kzMin(b.lo[a], c.lo[a]); b.hi[a] = kzMax(b.hi[a], c.hi[a]); } }
// the box of a leaf: its triangles' vertices in leaf order (the build grows each triangle's box, then the leaf's, from the same sequence)
KZ_HD void kzLeafBox(KzBox &b, const KzTri *tris, const KzTriShade *shade, uint32_t ref) {
    kzBoxReset(b);
    const uint32_t s = (ref & 0x7fffffffu) >> 3, n = (ref & 7u) + 1u;
    for (uint32_t i = s; i < s + n; ++i) { const KzTriShade &t = shade[tris[i].gid]; for (int v = 0; v < 3; ++v) kzBoxGrow(b, t.p + 3 * v); }
}
// KzNode child boxes <-> KzBox (kz_internal.h: q0..q11 = lo0 hi0 lo1 hi1)
KZ_HD void kzNodeBox(const float *q, int k, KzBox &b) { for (int a = 0; a < 3; ++a) { b.lo[a] = q[6 * k + a]; b.hi[a] = q[6 * k + 3 + a]; } }
KZ_HD void kzSetNodeBox(float *q, int k, const KzBox &b) { for (int a = 0; a < 3; ++a) { q[6 * k + a] = b.lo[a]; q[6 * k + 3 + a] = b.hi[a]; } }
// absolute padding of every box of the tree, from the (unpadded) root box: 1e-6 x the scene extent (kz_bvh.cpp padBox)
KZ_HD float kzAbsPad(const KzBox &root) {
    float absPad = 0.f;
    for (int a = 0; a < 3; ++a) absPad = kzMax(absPad, 1e-6f * kzMax(root.hi[a] - root.lo[a], kzMax(kzAbs(root.hi[a]), kzAbs(root.lo[a]))));
    return absPad;
}
KZ_HD void kzPadBox(KzBox &b, float absPad) {
    for (int a = 0; a < 3; ++a) {
        const float m = kzMax(kzAbs(b.lo[a]), kzAbs(b.hi[a]));
        const float e = kzMax(m * 4e-7f, absPad) + 1e-30f;
        b.lo[a] -= e; b.hi[a] += e;
    }
}
// surface area as the builder's SAH statistics form it (kz_bvh.cpp Box::area)
KZ_HD float kzBoxArea(const KzBox &b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (!(dx >= 0) || !(dy >= 0) || !(dz >= 0)) return 0.f;
    return 2.f * (dx * dy + dy * dz + dz * dx);
}
// The quantised boxes of one BVH4 packet from the exact (padded BVH2) boxes of its n <= 4 slots: p, the per-axis scales and the 8-bit
// bounds, rounded outward against kzDeq. The packet's child words are left as they are.
KZ_HD void kzQuantiseNode4(KzNode4 &nd, const KzBox *cb, int n) {
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) { lo[a] = kzMin(lo[a], cb[i].lo[a]); hi[a] = kzMax(hi[a], cb[i].hi[a]); }
    float scale[3];
    for (int a = 0; a < 3; ++a) {
        nd.p[a] = lo[a];
        const float ext = hi[a] - lo[a];
        int e = ext > 0.f ? kzFrexpExp(ext / 255.0f) : -126;         // ext/255 = m * 2^e, m in [0.5,1) -> 2^e >= ext/255
        e = e < -126 ? -126 : (e > 127 ? 127 : e);
        while (e < 127 && kzDeq(lo[a], 255u, kzPow2(e)) < hi[a]) ++e;   // 255 steps reach hi even after the rounding of p + 255*s
        scale[a] = kzPow2(e);
        nd.qlo[a] = 0; nd.qhi[a] = 0;
    }
    nd.scaleX = scale[0]; nd.scaleY = scale[1]; nd.scaleZ = scale[2];
    for (int i = 0; i < 4; ++i) {
        if (i >= n) { for (int a = 0; a < 3; ++a) nd.qlo[a] |= 255u << (8 * i); continue; }      // qhi = 0: inverted, never hit
        for (int a = 0; a < 3; ++a) {
            int ql = (int)__builtin_floorf((cb[i].lo[a] - lo[a]) / scale[a]);
            ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql);
            while (ql > 0 && kzDeq(lo[a], (uint32_t)ql, scale[a]) > cb[i].lo[a]) --ql;
            int qh = (int)__builtin_ceilf((cb[i].hi[a] - lo[a]) / scale[a]);
            qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
            while (qh < 255 && kzDeq(lo[a], (uint32_t)qh, scale[a]) < cb[i].hi[a]) ++qh;
            nd.qlo[a] |= (uint32_t)ql << (8 * i);
            nd.qhi[a] |= (uint32_t)qh << (8 * i);
        }
    }
}
