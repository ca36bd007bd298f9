// kz_xform.h - a mesh's object-to-world matrix applied to its base vertex data (kz_scene_set_transforms): the scene loaders' arithmetic
// (host/kazen_host.hpp Transform::point / Transform::normal and xmlscene.py xf_point / xf_normal, which tests/test_host_mirror.py holds equal),
// stated once for both sides as kz_refit.h states the box arithmetic: kz_edit.cpp evaluates it on the host (light meshes at once, every other
// mesh in the lazy host sync), kz_refit.hip's kz_edit_xform on every replica. Every operation is a single IEEE operation (-ffp-contract=off; the
// device unit keeps subnormals), so both sides write the same bits.
#pragma once
#include "kz_refit.h"

// KzXform (kz_internal.h): the matrix and, formed ONCE per mesh on the host in double, the cofactors and the determinant - per-mesh constants.
inline void kzXformFromMatrix(const float *m, KzXform &x) {
    double a[16];
    for (int i = 0; i < 16; ++i) { x.m[i] = m[i]; a[i] = m[i]; }
    const double i0 = a[5]*a[10]*a[15]-a[5]*a[11]*a[14]-a[9]*a[6]*a[15]+a[9]*a[7]*a[14]+a[13]*a[6]*a[11]-a[13]*a[7]*a[10];
    const double i4 = -a[4]*a[10]*a[15]+a[4]*a[11]*a[14]+a[8]*a[6]*a[15]-a[8]*a[7]*a[14]-a[12]*a[6]*a[11]+a[12]*a[7]*a[10];
    const double i8 = a[4]*a[9]*a[15]-a[4]*a[11]*a[13]-a[8]*a[5]*a[15]+a[8]*a[7]*a[13]+a[12]*a[5]*a[11]-a[12]*a[7]*a[9];
    const double i12 = -a[4]*a[9]*a[14]+a[4]*a[10]*a[13]+a[8]*a[5]*a[14]-a[8]*a[6]*a[13]-a[12]*a[5]*a[10]+a[12]*a[6]*a[9];
    const double i1 = -a[1]*a[10]*a[15]+a[1]*a[11]*a[14]+a[9]*a[2]*a[15]-a[9]*a[3]*a[14]-a[13]*a[2]*a[11]+a[13]*a[3]*a[10];
    const double i5 = a[0]*a[10]*a[15]-a[0]*a[11]*a[14]-a[8]*a[2]*a[15]+a[8]*a[3]*a[14]+a[12]*a[2]*a[11]-a[12]*a[3]*a[10];
    const double i9 = -a[0]*a[9]*a[15]+a[0]*a[11]*a[13]+a[8]*a[1]*a[15]-a[8]*a[3]*a[13]-a[12]*a[1]*a[11]+a[12]*a[3]*a[9];
    const double i2 = a[1]*a[6]*a[15]-a[1]*a[7]*a[14]-a[5]*a[2]*a[15]+a[5]*a[3]*a[14]+a[13]*a[2]*a[7]-a[13]*a[3]*a[6];
    const double i6 = -a[0]*a[6]*a[15]+a[0]*a[7]*a[14]+a[4]*a[2]*a[15]-a[4]*a[3]*a[14]-a[12]*a[2]*a[7]+a[12]*a[3]*a[6];
    const double i10 = a[0]*a[5]*a[15]-a[0]*a[7]*a[13]-a[4]*a[1]*a[15]+a[4]*a[3]*a[13]+a[12]*a[1]*a[7]-a[12]*a[3]*a[5];
    x.c[0] = i0; x.c[1] = i4; x.c[2] = i8; x.c[3] = i1; x.c[4] = i5; x.c[5] = i9; x.c[6] = i2; x.c[7] = i6; x.c[8] = i10;
    x.det = a[0] * i0 + a[1] * i4 + a[2] * i8 + a[3] * i12;
}

// Transform * Point3f: four float dot products ((m0 x + m1 y) + m2 z) + m3, then three float divisions by w
KZ_HD void kzXfPoint(const KzXform &x, const float *p, float *out) {
    float q[4];
    for (int i = 0; i < 4; ++i) q[i] = ((x.m[4 * i] * p[0] + x.m[4 * i + 1] * p[1]) + x.m[4 * i + 2] * p[2]) + x.m[4 * i + 3];
    for (int a = 0; a < 3; ++a) out[a] = q[a] / q[3];
}
// Transform * Normal3f: the inverse transpose of the upper 3x3 in double (the normal unchanged when the determinant is 0), narrowed once, then
// normalised in float when its squared length is > 0
KZ_HD void kzXfNormal(const KzXform &x, const float *n, float *out) {
    float r[3];
    if (x.det == 0.0) { r[0] = n[0]; r[1] = n[1]; r[2] = n[2]; }
    else {
        const double n0 = n[0], n1 = n[1], n2 = n[2];
        for (int i = 0; i < 3; ++i) r[i] = (float)(((x.c[3 * i] * n0 + x.c[3 * i + 1] * n1) + x.c[3 * i + 2] * n2) / x.det);
    }
    const float l2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (l2 > 0.f) { const float ln = __builtin_sqrtf(l2); r[0] = r[0] / ln; r[1] = r[1] / ln; r[2] = r[2] / ln; }
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2];
}
// a float is neither infinite nor NaN (read from the bits: no fast-math assumption can fold it away)
KZ_HD bool kzFinite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }
