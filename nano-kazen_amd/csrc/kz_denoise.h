// kz_denoise.h - the edge-avoiding a-trous filter of include/kazen_mi355x_denoise.h and its variance-guided form (include/kazen_mi355x_variance.h), stated once for
// the device: what one film texel is worth, what a tap weighs, and what one iteration makes of a pixel. The reference renderer has no denoiser; THIS ARITHMETIC
// defines the result, and tests/cpu_ref/kz_denoise_ref.cpp and kz_variance_ref.cpp restate it independently in plain C++ (same bits: the unit that includes this file
// is compiled without flush-to-zero and without contraction, build.sh).
// Every operation below is one fp32 IEEE operation in the order written; dnMax(a, b) is a > b ? a : b (no fmaxf: its NaN rule is not part of the definition).
// Lines marked VAR are what kz_denoise_variance adds (the template argument VAR); everything else is both calls'.
//
//   value of a film texel t:  t.w != 0 ? t.xyz / t.w : 0                               (dnValue; a null film: 0)
//   planes, frame-sized, no apron:  colour (e.rgb, valid ? 1 : 0) | (n.xyz, z) | (a.rgb, 0)
//     VAR: the colour plane's fourth float holds v, the variance estimate of the pixel's (demodulated) colour, and a NEGATIVE value (-1) where the pixel is not
//          valid (dnValid): a tap's v(q) arrives with the 16 bytes the tap loads anyway, and the call needs no plane beyond kz_denoise's
//   am = dnMax(a, 1e-3f) per channel;  e_0 = demodulate ? c / am : c                       (dnPrepare)
//     VAR: s = dnValue(moment), n = (float)samples:  var_k = dnMax(s_k - c_k * c_k, 0) / n
//          v_0 = demodulate ? (var_r / (am_r * am_r) + var_g / (am_g * am_g)) + var_b / (am_b * am_b) : (var_r + var_g) + var_b
//   one iteration at a valid pixel p (dnAtrous, dnAtrousLds):
//     VAR: gn = gd = 0; dy = -1..1 outer, dx = -1..1 inner, q = p + (dx, dy) inside the frame and valid: gn += dnK(dy) * dnK(dx) * v(q), gd += dnK(dy) * dnK(dx)   (dnPrefilter)
//          kv = 1.0f / (sv2 * (gn / gd) + 1e-12f), kc = dnMax(kc, kv) from here on     sv2 = sigmaVariance * sigmaVariance, formed on the host      (dnTolerance)
//     taps dy = -2..2 outer, dx = -2..2 inner, q = p + step * (dx, dy) inside the frame and valid (dnTap):
//       dc = dnSq(e(q) - e(p)), dn = dnSq(n(q) - n(p)), da = dnSq(a(q) - a(p))           dnSq(v) = (v.x * v.x + v.y * v.y) + v.z * v.z
//       m = dnMax(dnMax(z_p, z_q), 1e-20f), t = (z_q - z_p) / m, dz = t * t
//       arg = ((dc * kc + dn * kn) + dz * kz) + da * ka                                  (colour weights only: arg = dc * kc)
//       wgt = (h[dy + 2] * h[dx + 2]) * dnExp(-arg)                                      h = {1/16, 1/4, 3/8, 1/4, 1/16}; the products are exact
//       num.k += wgt * e(q).k (k = r, g, b), den += wgt;     VAR: nv += (wgt * wgt) * v(q)
//     e'(p) = num / den;     VAR: v'(p) = nv / (den * den)
//   result = demodulate ? e_last * am : e_last, weight 1; (0, 0, 0, 0) where the pixel is not valid and in the apron   (dnFinish)
//     VAR: v_last of a valid pixel beside it, 0 where the pixel is not valid
// The constants kc (per iteration: sigmaColor halves), kn, kz, ka = 1.0f / (sigma * sigma) are computed on the host (kz_denoise.hip dnPlan).
#pragma once
#include "../../include/kazen_mi355x_denoise.h"
#include "kz_crmath.h"

// One iteration's constants, by value to the kernel
struct KzDnIter { int width, height, step; float kc, kn, kz, ka; };

// What kz_denoise_temporal (include/kazen_mi355x_temporal.h, which holds the definition) puts in front of the VAR filter, by value to kz_dn_prepare_temporal:
// the current view's (o, a, u, v), the history's view (po, pinv), the tolerances as the taps compare them - depthTol, normalTol2 = normalTolerance^2 formed
// on the host - and (float)maxHistory. The history of a pixel is 36 bytes in three frame-sized planes, (e.rgb, v) | (n.xyz, z) | N, the first two the layout of the
// colour and the guide plane; in*: the copy the taps read (null: no history, every pixel starts at N = 1), out*: the copy the pixel's record goes to.
struct KzDnTemporal {
    float o[3], a[3], u[3], v[3], po[3], pinv[9];
    float depthTol, normalTol2, maxHistory;
    const float4 *inE, *inG; const float *inN;
    float4 *outE, *outG; float *outN;
};

// What kz_denoise_motion (include/kazen_mi355x_motion.h, which holds the definition) adds to KzDnTemporal, by value to kz_dn_prepare_motion: the mesh id of every
// frame pixel (0xFFFFFFFF: a miss), the rows - where a point of each mesh was when the history was stored - and their number. A struct of its own, not a part of
// KzDnTemporal: that one is a kernel argument of kz_dn_prepare_temporal, whose argument list stays what it was.
// (The stage that reads the two, stated once for the three history calls: kz_history.h. This file is the spatial filter's statement.)
struct KzMotionRow;
struct KzDnMotion { const uint32_t *ids; const KzMotionRow *rows; uint32_t nRows; };

#define KZ_DN_BLOCK 256
#define KZ_DN_ROW 64                  // pixels of a row per block (one wave), KZ_DN_BLOCK / KZ_DN_ROW rows
// The a-trous form per step (measured): the LDS-tile kernel for the steps up to KZ_DN_LDS_MAX_STEP, the direct-gather kernel beyond. 0 builds the
// direct form alone (scripts/denoise_rates.py and scripts/variance_rates.py time the two side by side); the results are the same bits.
#ifndef KZ_DN_LDS_MAX_STEP
#define KZ_DN_LDS_MAX_STEP 2
#endif
static_assert(KZ_DN_LDS_MAX_STEP == 0 || KZ_DN_LDS_MAX_STEP == 1 || KZ_DN_LDS_MAX_STEP == 2, "the LDS-tile kernel is built for the steps 1 and 2");

#define KZ_DN_FN __device__ __forceinline__
KZ_DN_FN float dnMax(float a, float b) { return a > b ? a : b; }
KZ_DN_FN float dnSq(float x, float y, float z) { return (x * x + y * y) + z * z; }
KZ_DN_FN float4 dnValue(const float4 *__restrict__ film, size_t i) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (film) { const float4 t = film[i]; if (t.w != 0.f) { v.x = t.x / t.w; v.y = t.y / t.w; v.z = t.z / t.w; } v.w = t.w; }
    return v;
}
// kzExp (kz_crmath.h), the same statement inlined: as a call inside the 25-tap loop it keeps the taps' loads from being issued ahead of the arithmetic
KZ_DN_FN float dnExp(float x) {
    if (!(x > -104.0f)) return x != x ? x : 0.0f;
    if (x > 89.0f) return __builtin_inff();
    return kzcrNarrow(kzcrExpD((double)x));
}
// the B3-spline weights: h[|d|] for d = -2..2
KZ_DN_FN float dnH(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
// whether a colour plane texel is a valid pixel's
template <bool VAR> KZ_DN_FN bool dnValid(const float4 &e) { return VAR ? !(e.w < 0.f) : e.w != 0.f; }

// (e_0, valid | v_0) of a pixel from the values of its texels: c the picture's, a the albedo's, s the moment film's (VAR alone, like `samples`). The pixel that is
// not valid gets its v = -1 from the caller.
template <bool VAR> KZ_DN_FN float4 dnCurrent(const float4 &c, const float4 &a, const float4 &s, int demodulate, float samples) {
    float4 e = make_float4(c.x, c.y, c.z, c.w != 0.f ? 1.f : 0.f);
    float vr = 0.f, vg = 0.f, vb = 0.f;
    if (VAR) {
        vr = dnMax(s.x - c.x * c.x, 0.f) / samples; vg = dnMax(s.y - c.y * c.y, 0.f) / samples; vb = dnMax(s.z - c.z * c.z, 0.f) / samples;
        e.w = (vr + vg) + vb;
    }
    if (demodulate) {
        const float ar = dnMax(a.x, 1e-3f); e.x = c.x / ar;
        const float ag = dnMax(a.y, 1e-3f); e.y = c.y / ag;
        const float ab = dnMax(a.z, 1e-3f); e.z = c.z / ab;
        if (VAR) e.w = (vr / (ar * ar) + vg / (ag * ag)) + vb / (ab * ab);
    }
    return e;
}

// VAR, the 3 x 3 prefilter's weights: k[|d|] for d = -1..1; the products are exact
KZ_DN_FN float dnK(int d) { return d == 0 ? 0.5f : 0.25f; }
KZ_DN_FN void dnPrefilter(int dy, int dx, float vq, float &gn, float &gd) { const float kk = dnK(dy) * dnK(dx); gn += kk * vq; gd += kk; }
KZ_DN_FN float dnTolerance(float kc, float sv2, float gn, float gd) {
    const float g = gn / gd;
    const float kv = 1.0f / (sv2 * g + 1e-12f);
    return dnMax(kc, kv);
}

// What tap q adds to the sums of pixel p: (wgt * e(q), wgt) and, VAR, wgt^2 * v(q). kc: the iteration's colour constant (I.kc; VAR: dnTolerance's);
// ep / eq: colour plane texels, gp / gq: (n.xyz, z), ap / aq: (a.rgb, -).
template <bool GUIDED, bool VAR>
KZ_DN_FN void dnTap(const KzDnIter &I, float kc, float hh, const float4 &ep, const float4 &eq, const float4 &gp, const float4 &gq, const float4 &ap, const float4 &aq,
                    float &nr, float &ng, float &nb, float &den, float &nv) {
    const float dc = dnSq(eq.x - ep.x, eq.y - ep.y, eq.z - ep.z);
    float arg = dc * kc;
    if (GUIDED) {
        const float dn = dnSq(gq.x - gp.x, gq.y - gp.y, gq.z - gp.z);
        const float da = dnSq(aq.x - ap.x, aq.y - ap.y, aq.z - ap.z);
        const float m = dnMax(dnMax(gp.w, gq.w), 1e-20f);
        const float t = (gq.w - gp.w) / m;
        const float dz = t * t;
        arg = ((arg + dn * I.kn) + dz * I.kz) + da * I.ka;
    }
    const float wgt = hh * dnExp(-arg);
    nr += wgt * eq.x; ng += wgt * eq.y; nb += wgt * eq.z;
    den += wgt;
    if (VAR) nv += (wgt * wgt) * eq.w;
}
