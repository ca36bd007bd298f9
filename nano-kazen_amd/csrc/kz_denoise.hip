// kz_denoise.hip - the device side and the entry points of include/kazen_mi355x_denoise.h and of its variance-guided form, include/kazen_mi355x_variance.h (the
// second-moment film itself is a film like the others: kz_film.hip): the picture denoised by an edge-avoiding a-trous filter guided by the feature films, a separate
// call after a render (nothing here runs inside a pass).
//
// Per kz_denoise / kz_denoise_variance, on the replica's lastStream:
//   kz_dn_prepare[_var]   per frame pixel: the films' values into frame-sized planes without an apron - (e_0.rgb, valid | v_0), (n.xyz, z), (a.rgb, -); the guide
//                         planes are written once, the colour plane ping-pongs between the iterations
//   kz_dn_atrous[_var]    one launch per iteration, one lane per pixel: steps 1 and 2 from an LDS tile with a halo (kz_dn_atrous[_var]_lds), the larger steps by
//                         direct gather with a wave along a row - every tap of a wave is one contiguous 1 KB load per plane
//   kz_dn_finish[_var]    per film texel: remodulated colour and weight 1 in a valid frame pixel, (0, 0, 0, 0) elsewhere (the apron too)
//   kz_dn_prepare_temporal, kz_dn_prepare_motion   kz_denoise_temporal (include/kazen_mi355x_temporal.h) and kz_denoise_motion (include/kazen_mi355x_motion.h), in
//                         kz_dn_prepare_var's place: the replica's history reprojected into the current view and blended into (e_0, v_0), the new history stored;
//                         the _var kernels follow unchanged. Two instances of the history prepare stage's one body (kz_history.h: dnHistory<MOTION, FAST>); the
//                         third, kz_denoise_responsive's, is kz_responsive.hip's
// Each of the first four is ONE body (dnPrepare, dnAtrous, dnAtrousLds, dnFinish) templated on VAR; the eight kernels are its two instances under the names the profiles
// know. With VAR the colour plane's .w carries v (negative: not valid) instead of the valid flag, so the planes and the tap loads are the same and the variance-
// guided call needs no buffer of its own. Each kernel's result is a function of its inputs alone: no atomics, no order between threads, the taps of a pixel summed
// by its own lane in the stated order (kz_denoise.h). This unit is compiled WITHOUT -fgpu-flush-denormals-to-zero (build.sh), so a subnormal weight is the C++
// restatements' (tests/cpu_ref/kz_denoise_ref.cpp, kz_variance_ref.cpp) to the bit.
#include <hip/hip_runtime.h>

#include "../../include/kazen_mi355x_denoise.h"
#include "../../include/kazen_mi355x_variance.h"
#include "../../include/kazen_mi355x_temporal.h"
#include "../../include/kazen_mi355x_motion.h"
#include "kz_state.h"
#include "kz_denoise.h"
#include "kz_history.h"
#include "kz_responsive.h"

#include <cmath>
#include <cstring>

// `moment`, `samples`: VAR alone
template <bool VAR>
KZ_DN_FN void dnPrepare(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                        const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples,
                        float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    const uint32_t i = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const size_t t = (size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border);      // < (height + 2b)(width + 2b): the films' texels
    const float4 c = dnValue(film, t), a = dnValue(albedo, t), n = dnValue(normal, t), z = dnValue(depth, t);
    float4 s = c;
    if (VAR) s = dnValue(moment, t);
    float4 e = dnCurrent<VAR>(c, a, s, demodulate, samples);
    if (VAR && c.w == 0.f) e.w = -1.f;                                 // not valid
    colour[i] = e;
    normalZ[i] = make_float4(n.x, n.y, n.z, z.x);
    albedoP[i] = make_float4(a.x, a.y, a.z, 0.f);
}

// The direct-gather form: lane (x, y) loads its 25 taps from the planes (the rows of a wave's taps are contiguous; L1 / L2 serve the 25-fold reuse); VAR: behind
// the nine .w of the pixel's unit-spaced neighbours (the prefilter that sets its tolerance). `sv2`: VAR alone. (I by value, as the kernel has it: by reference the
// compiler schedules the taps of the direct form anew, with up to 170 instructions more.)
template <bool GUIDED, bool VAR>
KZ_DN_FN void dnAtrous(const KzDnIter I, float sv2, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                       float4 *__restrict__ colOut) {
    const int x = (int)(blockIdx.x * KZ_DN_ROW + threadIdx.x), y = (int)(blockIdx.y * (KZ_DN_BLOCK / KZ_DN_ROW) + threadIdx.y);
    if (x >= I.width || y >= I.height) return;
    const size_t ip = (size_t)y * (size_t)I.width + (size_t)x;
    const float4 ep = colIn[ip];
    if (!dnValid<VAR>(ep)) { colOut[ip] = ep; return; }                 // not valid: neither gives nor receives (its colour stays 0)
    float kc = I.kc;
    if (VAR) {
        float gn = 0.f, gd = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            const bool rowIn = qy >= 0 && qy < I.height;
            const size_t rowAt = (size_t)(rowIn ? qy : y) * (size_t)I.width;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                const bool in = rowIn && qx >= 0 && qx < I.width;
                const float vq = colIn[rowAt + (size_t)(qx >= 0 && qx < I.width ? qx : x)].w;
                if (in && !(vq < 0.f)) dnPrefilter(dy, dx, vq, gn, gd);
            }
        }
        kc = dnTolerance(I.kc, sv2, gn, gd);
    }
    float4 gp = ep, ap = ep;
    if (GUIDED) { gp = normalZ[ip]; ap = albedoP[ip]; }
    float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f, nv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * I.step;
        const bool rowIn = qy >= 0 && qy < I.height;
        const size_t rowAt = (size_t)(rowIn ? qy : y) * (size_t)I.width;      // (a tap outside the frame loads the pixel's own row / column and is skipped)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * I.step;
            const bool in = rowIn && qx >= 0 && qx < I.width;
            const size_t iq = rowAt + (size_t)(qx >= 0 && qx < I.width ? qx : x);
            const float4 eq = colIn[iq];
            float4 gq = eq, aq = eq;
            if (GUIDED) { gq = normalZ[iq]; aq = albedoP[iq]; }
            if (in && dnValid<VAR>(eq)) dnTap<GUIDED, VAR>(I, kc, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den, nv);
        }
    }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, VAR ? nv / (den * den) : 1.f);
}

#if KZ_DN_LDS_MAX_STEP
// The LDS-tile form, for the small steps: a 16 x 16 tile of pixels with a halo of 2 * STEP (20 x 20 / 24 x 24 texels of up to 48 B), staged once per workgroup;
// a texel outside the frame is staged as not valid. The halo (>= 2) holds the prefilter's neighbours too. The same taps in the same order as the direct form:
// the same bits.
template <bool GUIDED, int STEP, bool VAR>
KZ_DN_FN void dnAtrousLds(const KzDnIter I, float sv2, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                          float4 *__restrict__ colOut) {
    constexpr int R = 2 * STEP, T = 16 + 2 * R, N = T * T;
    __shared__ float4 tile[(GUIDED ? 3 : 1) * N];
    const int x0 = (int)blockIdx.x * 16, y0 = (int)blockIdx.y * 16;
    for (int k = (int)threadIdx.x; k < N; k += KZ_DN_BLOCK) {
        const int ty = k / T, tx = k - ty * T, gx = x0 - R + tx, gy = y0 - R + ty;
        float4 e = make_float4(0.f, 0.f, 0.f, VAR ? -1.f : 0.f), g = make_float4(0.f, 0.f, 0.f, 0.f), a = g;
        if (gx >= 0 && gx < I.width && gy >= 0 && gy < I.height) {
            const size_t i = (size_t)gy * (size_t)I.width + (size_t)gx;
            e = colIn[i];
            if (GUIDED) { g = normalZ[i]; a = albedoP[i]; }
        }
        tile[k] = e;
        if (GUIDED) { tile[N + k] = g; tile[2 * N + k] = a; }
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4), x = x0 + lx, y = y0 + ly;
    if (x >= I.width || y >= I.height) return;
    const size_t ip = (size_t)y * (size_t)I.width + (size_t)x;
    const int c = (ly + R) * T + lx + R;
    const float4 ep = tile[c];
    if (!dnValid<VAR>(ep)) { colOut[ip] = ep; return; }
    float kc = I.kc;
    if (VAR) {
        float gn = 0.f, gd = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float vq = tile[c + dy * T + dx].w;
                if (!(vq < 0.f)) dnPrefilter(dy, dx, vq, gn, gd);
            }
        kc = dnTolerance(I.kc, sv2, gn, gd);
    }
    float4 gp = ep, ap = ep;
    if (GUIDED) { gp = tile[N + c]; ap = tile[2 * N + c]; }
    float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f, nv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int k = c + dy * STEP * T + dx * STEP;
            const float4 eq = tile[k];
            float4 gq = eq, aq = eq;
            if (GUIDED) { gq = tile[N + k]; aq = tile[2 * N + k]; }
            if (dnValid<VAR>(eq)) dnTap<GUIDED, VAR>(I, kc, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den, nv);
        }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, VAR ? nv / (den * den) : 1.f);
}
#endif

// `variance` (VAR alone, may be null): v_last per frame pixel, 0 where the pixel is not valid
template <bool VAR>
KZ_DN_FN void dnFinish(int width, int height, int border, const float4 *__restrict__ colour, const float4 *__restrict__ albedoP, int demodulate,
                       float4 *__restrict__ out, float *__restrict__ variance) {
    const uint32_t t = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    const uint32_t cols = (uint32_t)(width + 2 * border), rows = (uint32_t)(height + 2 * border);
    if (t >= cols * rows) return;
    const int y = (int)(t / cols) - border, x = (int)(t - (t / cols) * cols) - border;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x >= 0 && x < width && y >= 0 && y < height) {
        const size_t i = (size_t)y * (size_t)width + (size_t)x;
        const float4 e = colour[i];
        const bool valid = dnValid<VAR>(e);
        if (valid) {
            r = make_float4(e.x, e.y, e.z, 1.f);
            if (demodulate) { const float4 a = albedoP[i]; r.x = e.x * dnMax(a.x, 1e-3f); r.y = e.y * dnMax(a.y, 1e-3f); r.z = e.z * dnMax(a.z, 1e-3f); }
        }
        if (VAR && variance) variance[i] = valid ? e.w : 0.f;
    }
    out[t] = r;
}

// The eight kernels: the bodies above under the names and with the arguments they have always had
#define KZ_DN_KERNEL __global__ __launch_bounds__(KZ_DN_BLOCK) void
#define KZ_DN_PLANES const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP, float4 *__restrict__ colOut
KZ_DN_KERNEL kz_dn_prepare(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ albedo, const float4 *__restrict__ normal,
                           const float4 *__restrict__ depth, int demodulate, float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    dnPrepare<false>(width, height, border, film, nullptr, albedo, normal, depth, demodulate, 0.f, colour, normalZ, albedoP);
}
KZ_DN_KERNEL kz_dn_prepare_var(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                               const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples,
                               float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    dnPrepare<true>(width, height, border, film, moment, albedo, normal, depth, demodulate, samples, colour, normalZ, albedoP);
}
template <bool GUIDED> KZ_DN_KERNEL kz_dn_atrous(KzDnIter I, KZ_DN_PLANES) { dnAtrous<GUIDED, false>(I, 0.f, colIn, normalZ, albedoP, colOut); }
template <bool GUIDED> KZ_DN_KERNEL kz_dn_atrous_var(KzDnIter I, float sv2, KZ_DN_PLANES) { dnAtrous<GUIDED, true>(I, sv2, colIn, normalZ, albedoP, colOut); }
#if KZ_DN_LDS_MAX_STEP
template <bool GUIDED, int STEP> KZ_DN_KERNEL kz_dn_atrous_lds(KzDnIter I, KZ_DN_PLANES) { dnAtrousLds<GUIDED, STEP, false>(I, 0.f, colIn, normalZ, albedoP, colOut); }
template <bool GUIDED, int STEP> KZ_DN_KERNEL kz_dn_atrous_var_lds(KzDnIter I, float sv2, KZ_DN_PLANES) { dnAtrousLds<GUIDED, STEP, true>(I, sv2, colIn, normalZ, albedoP, colOut); }
#endif
KZ_DN_KERNEL kz_dn_finish(int width, int height, int border, const float4 *__restrict__ colour, const float4 *__restrict__ albedoP, int demodulate, float4 *__restrict__ out) {
    dnFinish<false>(width, height, border, colour, albedoP, demodulate, out, nullptr);
}
KZ_DN_KERNEL kz_dn_finish_var(int width, int height, int border, const float4 *__restrict__ colour, const float4 *__restrict__ albedoP, int demodulate,
                              float4 *__restrict__ out, float *__restrict__ variance) {
    dnFinish<true>(width, height, border, colour, albedoP, demodulate, out, variance);
}

// The history prepare stage (kz_history.h: dnHistory, the one body) in kz_dn_prepare_var's place: kz_denoise_temporal's kernel, and kz_denoise_motion's - the same
// lines plus the pixel's mesh id and that mesh's row (MOTION). kz_denoise_responsive's (MOTION and FAST) is in kz_responsive.hip.
KZ_DN_KERNEL kz_dn_prepare_temporal(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                                    const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples, const KzDnTemporal T,
                                    float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    dnHistory<false, false>(width, height, border, film, moment, albedo, normal, depth, demodulate, samples, T, KzDnMotion{}, KzDnFast{}, colour, normalZ, albedoP);
}
KZ_DN_KERNEL kz_dn_prepare_motion(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                                  const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples, const KzDnTemporal T, const KzDnMotion M,
                                  float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    dnHistory<true, false>(width, height, border, film, moment, albedo, normal, depth, demodulate, samples, T, M, KzDnFast{}, colour, normalZ, albedoP);
}

// ---- host side ----
// What a call does, from its options: `avail` = the guides there are (the scene's mask / the films given to kz_denoise_films);
// defaultSigmaColor: 1.0 for kz_denoise, 2.0 for kz_denoise_variance
struct KzDnPlan { uint32_t iterations, guides; bool demodulate, guided; float kc[KZ_DENOISE_MAX_ITERATIONS], kn, kz, ka; };
static int dnPlan(const KzDenoiseOpts *opts, uint32_t avail, const char *call, KzDnPlan *plan, float defaultSigmaColor) {
    static const KzDenoiseOpts defaults = {};
    const KzDenoiseOpts &o = opts ? *opts : defaults;
    if (o.iterations > KZ_DENOISE_MAX_ITERATIONS) return kz_fail(KZ_ERR_INVALID_ARG, "%s: iterations = %u (1 .. %u; 0: the default, 5)", call, o.iterations, KZ_DENOISE_MAX_ITERATIONS);
    if (o.flags & ~(KZ_DENOISE_NO_DEMODULATE | KZ_DENOISE_NO_GUIDES)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: flags = %u has bits outside KZ_DENOISE_NO_DEMODULATE | KZ_DENOISE_NO_GUIDES", call, o.flags);
    if (o.reserved) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzDenoiseOpts.reserved = %u must be 0", call, o.reserved);
    if (o.guides & ~avail) return kz_fail(KZ_ERR_INVALID_ARG, "%s: guides = %u is not a subset of the AOVs there are (mask %u)", call, o.guides, avail);
    const float sig[4] = {o.sigmaColor, o.sigmaNormal, o.sigmaDepth, o.sigmaAlbedo};
    static const char *const names[4] = {"sigmaColor", "sigmaNormal", "sigmaDepth", "sigmaAlbedo"};
    const float dflt[4] = {defaultSigmaColor, 0.3f, 0.1f, 0.1f};
    float s[4];
    for (int k = 0; k < 4; ++k) {
        if (!(std::isfinite(sig[k]) && sig[k] >= 0.f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: %s = %g must be finite and > 0 (0: the default, %g)", call, names[k], (double)sig[k], (double)dflt[k]);
        s[k] = sig[k] == 0.f ? dflt[k] : sig[k];
    }
    plan->iterations = o.iterations ? o.iterations : 5;
    plan->guides = o.guides ? o.guides : avail;
    plan->demodulate = (plan->guides & KZ_AOV_ALBEDO) && !(o.flags & KZ_DENOISE_NO_DEMODULATE);
    plan->guided = plan->guides && !(o.flags & KZ_DENOISE_NO_GUIDES);
    float scale = 1.0f;                                                 // 2^-i
    for (uint32_t i = 0; i < KZ_DENOISE_MAX_ITERATIONS; ++i, scale *= 0.5f) { const float sc = s[0] * scale; plan->kc[i] = 1.0f / (sc * sc); }
    plan->kn = 1.0f / (s[1] * s[1]); plan->kz = 1.0f / (s[2] * s[2]); plan->ka = 1.0f / (s[3] * s[3]);
    return KZ_OK;
}

// What kz_denoise_variance adds to a call (null: kz_denoise). `moment`: the second-moment film (null: zeros); `variance`: null or width x height floats.
// `temporal` (null: kz_denoise_variance): what kz_denoise_temporal puts in front - its prepare kernel takes the place of kz_dn_prepare_var.
// `motion` (with `temporal` alone; null: kz_denoise_temporal): what kz_denoise_motion adds - kz_dn_prepare_motion takes that place.
// `responsive` (with `temporal` alone; null: one of the calls above): what kz_denoise_responsive adds - the two kernels of kz_responsive.hip take that place, with
// `motion` or without it (no mesh has moved: every pixel static).
struct KzDnVar { float sv2, samples; const float4 *moment; float *variance; const KzDnTemporal *temporal; const KzDnMotion *motion; const KzDnResponsive *responsive; };

// KzTemporalOpts, checked, as the kernel takes them (the views and the history's planes are filled in by the caller)
static int dnTemporalOpts(const KzTemporalOpts *topts, const char *call, KzDnTemporal *T) {
    static const KzTemporalOpts defaults = {};
    const KzTemporalOpts &o = topts ? *topts : defaults;
    if (!(std::isfinite(o.depthTolerance) && o.depthTolerance >= 0.f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzTemporalOpts.depthTolerance = %g must be finite and > 0 (0: the default, 0.05)", call, (double)o.depthTolerance);
    if (!(std::isfinite(o.normalTolerance) && o.normalTolerance >= 0.f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzTemporalOpts.normalTolerance = %g must be finite and > 0 (0: the default, 0.5)", call, (double)o.normalTolerance);
    if (o.maxHistory > 65535u) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzTemporalOpts.maxHistory = %u (1 .. 65535; 0: the default, 32)", call, o.maxHistory);
    if (o.flags) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzTemporalOpts.flags = %u must be 0", call, o.flags);
    for (int k = 0; k < 4; ++k) if (o.reserved[k]) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzTemporalOpts.reserved[%d] = %u must be 0", call, k, o.reserved[k]);
    const float nt = o.normalTolerance == 0.f ? 0.5f : o.normalTolerance;
    *T = KzDnTemporal{};
    T->depthTol = o.depthTolerance == 0.f ? 0.05f : o.depthTolerance;
    T->normalTol2 = nt * nt;
    T->maxHistory = (float)(o.maxHistory ? o.maxHistory : 32u);
    return KZ_OK;
}
// KzResponsiveOpts (include/kazen_mi355x_responsive.h), checked, with the defaults in (the fast plane's copies are filled in by the caller)
static int dnResponsiveOpts(const KzResponsiveOpts *ropts, const char *call, KzDnResponsive *R) {
    static const KzResponsiveOpts defaults = {};
    const KzResponsiveOpts &o = ropts ? *ropts : defaults;
    if (o.fastHistory > 65535u) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzResponsiveOpts.fastHistory = %u (1 .. 65535; 0: the default, 2)", call, o.fastHistory);
    if (!(std::isfinite(o.clampSigma) && o.clampSigma >= 0.f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzResponsiveOpts.clampSigma = %g must be finite and > 0 (0: the default, 2)", call, (double)o.clampSigma);
    if (o.radius > 2u) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzResponsiveOpts.radius = %u (1 or 2; 0: the default, 1)", call, o.radius);
    if (o.flags & ~KZ_RESPONSIVE_CLAMP_OFF) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzResponsiveOpts.flags = %u has bits outside KZ_RESPONSIVE_CLAMP_OFF", call, o.flags);
    for (int k = 0; k < 4; ++k) if (o.reserved[k]) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzResponsiveOpts.reserved[%d] = %u must be 0", call, k, o.reserved[k]);
    *R = KzDnResponsive{};
    R->fastHistory = (float)(o.fastHistory ? o.fastHistory : 2u);
    R->clampSigma = o.clampSigma == 0.f ? 2.0f : o.clampSigma;
    R->radius = o.radius ? (int)o.radius : 1;
    R->clampOff = (o.flags & KZ_RESPONSIVE_CLAMP_OFF) != 0;
    return KZ_OK;
}
// A fast plane as it leaves the device: (f.rgb, vf), four zeros where the pixel is not valid (the device marks those with vf = -1, kz_responsive.hip)
static int dnFastDownload(const DevBuf<float4> &F, size_t nPix, float *fast) {
    int rc;
    if ((rc = F.download((float4 *)fast, nPix))) return rc;
    for (size_t i = 0; i < nPix; ++i) if (fast[4 * i + 3] < 0.f) fast[4 * i] = fast[4 * i + 1] = fast[4 * i + 2] = fast[4 * i + 3] = 0.f;
    return KZ_OK;
}
// the reprojection reads the depth film whatever the weights use: a KzDenoiseOpts.guides without it is refused
static int dnTemporalGuides(const KzDnPlan &plan, uint32_t avail, const char *call) {
    if ((avail & KZ_AOV_DEPTH) && !(plan.guides & KZ_AOV_DEPTH)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: guides = %u leaves out KZ_AOV_DEPTH (%u), which the reprojection reads", call, plan.guides, KZ_AOV_DEPTH);
    return KZ_OK;
}
// The view of the camera words in `P` (kzPinholeWords: a thin-lens camera is taken as the pinhole through its lens centre); inv from a double inverse narrowed once
static int dnViewOf(const KzParams &P, const char *call, KzTemporalView *view) {
    std::memset(view, 0, sizeof *view);
    if (!kzPinholeWords(P, view->o, view->a, view->u, view->v))
        return kz_fail(KZ_ERR_UNSUPPORTED, "%s: the camera's pixel -> direction map is not affine (a sampleToCamera whose divide depends on the sample position, or a toWorld that is not affine) or is not finite", call);
    const double m[9] = {view->u[0], view->v[0], view->a[0], view->u[1], view->v[1], view->a[1], view->u[2], view->v[2], view->a[2]};      // columns (u, v, a)
    const double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};      // the adjugate, row-major
    const double det = m[0] * c[0] + m[1] * c[3] + m[2] * c[6];
    bool fin = det != 0.0 && std::isfinite(det);
    for (int k = 0; k < 9 && fin; ++k) { view->inv[k] = (float)(c[k] / det); fin = std::isfinite(view->inv[k]); }
    if (!fin) { std::memset(view, 0, sizeof *view); return kz_fail(KZ_ERR_UNSUPPORTED, "%s: the matrix (u, v, a) of the camera's view is singular (determinant %g)", call, det); }
    return KZ_OK;
}
static void dnSetViews(KzDnTemporal *T, const KzTemporalView &cur, const float po[3], const float pinv[9]) {
    for (int k = 0; k < 3; ++k) { T->o[k] = cur.o[k]; T->a[k] = cur.a[k]; T->u[k] = cur.u[k]; T->v[k] = cur.v[k]; T->po[k] = po[k]; }
    for (int k = 0; k < 9; ++k) T->pinv[k] = pinv[k];
}

// KzVarianceOpts, checked: sv2 = sigmaVariance^2 with the default filled in
static int dnVarianceOpts(const KzVarianceOpts *vopts, const char *call, float *sv2, uint32_t *samples) {
    static const KzVarianceOpts defaults = {};
    const KzVarianceOpts &v = vopts ? *vopts : defaults;
    if (!(std::isfinite(v.sigmaVariance) && v.sigmaVariance >= 0.f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzVarianceOpts.sigmaVariance = %g must be finite and > 0 (0: the default, 3)", call, (double)v.sigmaVariance);
    if (v.flags) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzVarianceOpts.flags = %u must be 0", call, v.flags);
    if (v.reserved) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzVarianceOpts.reserved = %u must be 0", call, v.reserved);
    const float sv = v.sigmaVariance == 0.f ? 3.0f : v.sigmaVariance;
    *sv2 = sv * sv;
    *samples = v.samples;
    return KZ_OK;
}

// The launches of one call on `stream`. The films are device buffers of (height + 2b) x (width + 2b) texels, a guide that is absent is null; colour[2], normalZ and
// albedoP hold width x height texels each, `out` a film. Nothing but these planes, `out` and var->variance is written.
static int dnRun(const KzDnPlan &plan, const KzDnVar *var, int width, int height, int border, const float4 *film, const float4 *albedo, const float4 *normal,
                 const float4 *depth, float4 *const colour[2], float4 *normalZ, float4 *albedoP, float4 *out, hipStream_t stream) {
    const uint32_t nPix = (uint32_t)width * (uint32_t)height, nTexels = (uint32_t)(width + 2 * border) * (uint32_t)(height + 2 * border);
    const int demod = plan.demodulate ? 1 : 0;
    const dim3 gPix((nPix + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), gTexels((nTexels + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), b1(KZ_DN_BLOCK);
    albedo = (plan.guides & KZ_AOV_ALBEDO) ? albedo : nullptr; normal = (plan.guides & KZ_AOV_NORMAL) ? normal : nullptr; depth = (plan.guides & KZ_AOV_DEPTH) ? depth : nullptr;
    if (var && var->temporal && var->responsive) {
        static const KzDnMotion none = {};
        int rc;
        if ((rc = kzDnResponsiveRun(width, height, border, film, var->moment, albedo, normal, depth, demod, var->samples, *var->temporal, var->motion ? *var->motion : none,
                                    *var->responsive, colour[0], normalZ, albedoP, stream))) return rc;
    }
    else if (var && var->temporal && var->motion) hipLaunchKernelGGL(kz_dn_prepare_motion, gPix, b1, 0, stream, width, height, border, film, var->moment, albedo, normal, depth, demod, var->samples, *var->temporal, *var->motion, colour[0], normalZ, albedoP);
    else if (var && var->temporal) hipLaunchKernelGGL(kz_dn_prepare_temporal, gPix, b1, 0, stream, width, height, border, film, var->moment, albedo, normal, depth, demod, var->samples, *var->temporal, colour[0], normalZ, albedoP);
    else if (var) hipLaunchKernelGGL(kz_dn_prepare_var, gPix, b1, 0, stream, width, height, border, film, var->moment, albedo, normal, depth, demod, var->samples, colour[0], normalZ, albedoP);
    else hipLaunchKernelGGL(kz_dn_prepare, gPix, b1, 0, stream, width, height, border, film, albedo, normal, depth, demod, colour[0], normalZ, albedoP);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((width + KZ_DN_ROW - 1) / KZ_DN_ROW), (unsigned)((height + KZ_DN_BLOCK / KZ_DN_ROW - 1) / (KZ_DN_BLOCK / KZ_DN_ROW))), blk(KZ_DN_ROW, KZ_DN_BLOCK / KZ_DN_ROW);
    for (uint32_t i = 0; i < plan.iterations; ++i) {
        const KzDnIter I = {width, height, 1 << i, plan.kc[i], plan.kn, plan.kz, plan.ka};
        // one iteration with the kernel of the call's kind: `plain` for kz_denoise, `withVar` for kz_denoise_variance
        auto atrous = [&](auto plain, auto withVar, dim3 g, dim3 b) {
            const float4 *in = colour[i & 1], *nz = normalZ, *al = albedoP;
            if (var) hipLaunchKernelGGL(withVar, g, b, 0, stream, I, var->sv2, in, nz, al, colour[(i + 1) & 1]);
            else hipLaunchKernelGGL(plain, g, b, 0, stream, I, in, nz, al, colour[(i + 1) & 1]);
        };
#if KZ_DN_LDS_MAX_STEP
        if ((1 << i) <= KZ_DN_LDS_MAX_STEP) {
            const dim3 g16((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
            if (plan.guided) { if (i == 0) atrous(kz_dn_atrous_lds<true, 1>, kz_dn_atrous_var_lds<true, 1>, g16, b1); else atrous(kz_dn_atrous_lds<true, 2>, kz_dn_atrous_var_lds<true, 2>, g16, b1); }
            else { if (i == 0) atrous(kz_dn_atrous_lds<false, 1>, kz_dn_atrous_var_lds<false, 1>, g16, b1); else atrous(kz_dn_atrous_lds<false, 2>, kz_dn_atrous_var_lds<false, 2>, g16, b1); }
            HIP_TRY(hipGetLastError());
            continue;
        }
#endif
        if (plan.guided) atrous(kz_dn_atrous<true>, kz_dn_atrous_var<true>, grid, blk);
        else atrous(kz_dn_atrous<false>, kz_dn_atrous_var<false>, grid, blk);
        HIP_TRY(hipGetLastError());
    }
    const float4 *last = colour[plan.iterations & 1], *al = albedoP;
    if (var) hipLaunchKernelGGL(kz_dn_finish_var, gTexels, b1, 0, stream, width, height, border, last, al, demod, out, var->variance);
    else hipLaunchKernelGGL(kz_dn_finish, gTexels, b1, 0, stream, width, height, border, last, al, demod, out);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

// A history's three planes into the interchange format: per pixel (e.rgb, v), (n.xyz, z), (N, 0, 0, 0)
static int dnHistoryDownload(const DevBuf<float4> &E, const DevBuf<float4> &G, const DevBuf<float> &N, size_t nPix, float *history) {
    std::vector<float> e(4 * nPix), g(4 * nPix), n(nPix);
    int rc;
    if ((rc = E.download((float4 *)e.data(), nPix)) || (rc = G.download((float4 *)g.data(), nPix)) || (rc = N.download(n.data(), nPix))) return rc;
    for (size_t i = 0; i < nPix; ++i) {
        std::memcpy(history + 12 * i, &e[4 * i], 16); std::memcpy(history + 12 * i + 4, &g[4 * i], 16);
        history[12 * i + 8] = n[i]; history[12 * i + 9] = history[12 * i + 10] = history[12 * i + 11] = 0.f;
    }
    return KZ_OK;
}

// A call on a replica's own films, into its denoise buffers: behind the replica's queued work, with the guides the plan wants (and the moment film) resolved
// `T` (kz_denoise_temporal alone): its checked options; the views and the replica's history are filled in here, and the history moves on when the call has succeeded
// `motion` (with T; kz_denoise_motion): the history survives kz_scene_set_transforms - stale only by baseEdits -, and when a mesh has moved since it was stored the
// call computes this frame's ids and the rows and takes kz_dn_prepare_motion
// `R` (with T and motion; kz_denoise_responsive): its checked options; the replica's fast plane is filled in here - absent unless it was written with the history the
// call reads - and moves on with the history
static int dnOnReplica(KzScene *scene, KzDeviceState *ds, const KzDnPlan &plan, KzDnVar *var, KzDnTemporal *T = nullptr, bool motion = false, KzDnResponsive *R = nullptr) {
    const KzParams &P = scene->prm;
    const size_t nPix = (size_t)P.width * (size_t)P.height;
    const char *const call = R ? "kz_denoise_responsive" : (motion ? "kz_denoise_motion" : "kz_denoise_temporal");
    int rc;
    KzTemporalView view;
    KzDnMotion M = {};
    bool fresh = true;                                                  // T: nothing stored, or what is stored is stale
    if (T) {
        if ((rc = dnViewOf(P, call, &view))) return rc;
        const bool stale = motion ? ds->tpBaseEdits != scene->baseEdits : ds->tpEdits != scene->geometryEdits;
        fresh = !ds->tpFrames || stale || ds->tpE[0].cap() != nPix;
        if (!fresh && ds->tpDemod != plan.demodulate)
            return kz_fail(KZ_ERR_STATE, "%s: this call %s, the history of %u frame(s) holds colours that %s: kz_temporal_reset first", call, plan.demodulate ? "demodulates" : "does not demodulate",
                           ds->tpFrames, ds->tpDemod ? "are demodulated" : "are not");
    }
    const std::vector<float> &xfNow = kzMeshXf(scene);
    if (motion) {
        const uint32_t nMeshes = (uint32_t)scene->meshRows.size();
        std::vector<KzMotionRow> rows(nMeshes);
        const bool known = !fresh && ds->tpXf.size() == xfNow.size();    // (a fresh call reads no history: every row static)
        if ((rc = kz_motion_rows(xfNow.data(), known ? ds->tpXf.data() : xfNow.data(), nMeshes, rows.data()))) return rc;
        uint32_t counts[3] = {0, 0, 0};
        for (const KzMotionRow &r : rows) ++counts[(r.flags & KZ_MOTION_STATIC) ? 0 : ((r.flags & KZ_MOTION_UNTRACKED) ? 2 : 1)];
        std::memcpy(ds->mtCounts, counts, sizeof counts);
        if (counts[1] + counts[2]) {                                    // something moved: this frame's ids, and the rows
            if ((rc = kzMotionIds(scene, ds))) return rc;
            if (ds->mtRows.cap() != nMeshes && (rc = ds->mtRows.regrow(nMeshes))) return rc;
            if ((rc = ds->mtRows.upload(rows.data(), nMeshes))) return rc;
            M.ids = ds->mtIds; M.rows = ds->mtRows; M.nRows = nMeshes;
        }
    }
    HIP_TRY(hipStreamSynchronize(ds->lastStream));                      // the replica's queued work: the films and the sums are final
    if (var && ds->moment().sums && ds->moment().texels) {
        if ((rc = kzFilmResolve(scene, ds->moment(), ds->lastStream))) return rc;
        var->moment = ds->moment().texels;
    }
    const float4 *guide[3] = {nullptr, nullptr, nullptr};
    for (int f = 0; f < 3; ++f) {
        const bool wanted = f == 0 ? (plan.demodulate || (plan.guided && (plan.guides & KZ_AOV_ALBEDO))) : ((plan.guided || T) && (plan.guides & (1u << f)));      // (T: the reprojection reads n and z whatever the weights use)
        KzFilm &film = ds->aov(f);
        if (!wanted || !film.sums || !film.texels) continue;                // (enabled, nothing rendered yet: zeros, as kz_aov_download gives)
        if ((rc = kzFilmResolve(scene, film, ds->lastStream))) return rc;
        guide[f] = film.texels;
    }
    ds->dnValid = false;
    for (DevBuf<float4> *b : {&ds->dnColor[0], &ds->dnColor[1], &ds->dnNormalZ, &ds->dnAlbedo})
        if (b->cap() != nPix && (rc = b->regrow(nPix))) return rc;
    if (ds->dnOut.cap() != ds->filmPixels && (rc = ds->dnOut.regrow(ds->filmPixels))) return rc;
    if (T) {
        if (fresh) ds->tpFrames = 0;                                    // (from here on a call that fails leaves either the history it found or none)
        for (int k = 0; k < 2; ++k) {
            for (DevBuf<float4> *b : {&ds->tpE[k], &ds->tpG[k]}) if (b->cap() != nPix && (rc = b->regrow(nPix))) return rc;
            if (ds->tpN[k].cap() != nPix && (rc = ds->tpN[k].regrow(nPix))) return rc;
        }
        const int in = ds->tpCur, out = in ^ 1;
        dnSetViews(T, view, ds->tpO, ds->tpInv);
        if (!fresh && T->maxHistory != 1.0f) { T->inE = ds->tpE[in]; T->inG = ds->tpG[in]; T->inN = ds->tpN[in]; }      // (maxHistory = 1: without history, by definition)
        T->outE = ds->tpE[out]; T->outG = ds->tpG[out]; T->outN = ds->tpN[out];
        var->temporal = T;
        if (M.ids && T->inE) var->motion = &M;                          // (without a history to read, kz_dn_prepare_temporal's lines are the motion kernel's)
        if (R) {
            for (int k = 0; k < 2; ++k) if (ds->rsF[k].cap() != nPix) { ds->rsStore = 0; if ((rc = ds->rsF[k].regrow(nPix))) return rc; }
            if (T->inE && ds->rsStore && ds->rsStore == ds->tpStore) R->inF = ds->rsF[in];      // (written with the history this call reads; otherwise absent)
            R->outF = ds->rsF[out];
            var->responsive = R;
        }
    }
    float4 *const colour[2] = {ds->dnColor[0].get(), ds->dnColor[1].get()};
    if ((rc = dnRun(plan, var, P.width, P.height, P.border, ds->picture().texels, guide[0], guide[1], guide[2], colour, ds->dnNormalZ, ds->dnAlbedo, ds->dnOut, ds->lastStream))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    ds->dnValid = true;
    if (T) {
        ds->tpCur ^= 1; ds->tpFrames += 1; ds->tpDemod = plan.demodulate; ds->tpEdits = scene->geometryEdits;
        ds->tpStore += 1;
        if (R) ds->rsStore = ds->tpStore;                               // (the fast plane's copy tpCur goes with this store of the history)
        ds->tpBaseEdits = scene->baseEdits; ds->tpXf = xfNow;           // (what kz_denoise_motion's rows are formed from, whichever call stored the history)
        std::memcpy(ds->tpO, view.o, sizeof ds->tpO); std::memcpy(ds->tpInv, view.inv, sizeof ds->tpInv);
    }
    return KZ_OK;
}

// What kz_denoise_temporal_films adds to a call on host films: the views and the history in the interchange format (12 floats per pixel), in and out
// (ids non-null: kz_denoise_motion_films - the id plane, the rows and their number, checked by the caller)
struct KzDnHostTemporal { const KzTemporalOpts *topts; const KzTemporalView *current, *previous; const float *historyIn; float *historyOut;
                          const uint32_t *ids; const KzMotionRow *rows; uint32_t nRows;
                          const KzDnResponsive *responsive; const float *fastIn; float *fastOut; };      // (responsive non-null: kz_denoise_responsive_films - its checked options, the fast plane in and out)

// A call on films of the host's: kz_denoise_films, with `moment` kz_denoise_variance_films (`vopts`, `outVariance`: its alone), with `ht` kz_denoise_temporal_films
static int dnFilms(const char *call, int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal,
                   const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance, const KzDnHostTemporal *ht = nullptr) {
    if (width < 1 || height < 1 || border < 0 || border > 64 || (uint64_t)(width + 2 * (int64_t)border) * (uint64_t)(height + 2 * (int64_t)border) >= (1ull << 31))
        return kz_fail(KZ_ERR_INVALID_ARG, "%s: a frame of %d x %d with border %d (at least 1 x 1, border 0 .. 64, fewer than 2^31 texels)", call, width, height, border);
    KzDnPlan plan; KzDnVar var = {}; int rc;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | (depth ? KZ_AOV_DEPTH : 0u);
    if ((rc = dnPlan(opts, avail, call, &plan, moment ? 2.0f : 1.0f))) return rc;
    if (moment) {
        uint32_t samples;
        if ((rc = dnVarianceOpts(vopts, call, &var.sv2, &samples))) return rc;
        if (!samples) return kz_fail(KZ_ERR_STATE, "%s: KzVarianceOpts.samples = 0 (there is no replica whose count could stand in: state it)", call);
        var.samples = (float)samples;
    }
    KzDnTemporal T;
    if (ht && ((rc = dnTemporalOpts(ht->topts, call, &T)) || (rc = dnTemporalGuides(plan, avail, call)))) return rc;
    const size_t nPix = (size_t)width * (size_t)height, nTexels = (size_t)(width + 2 * border) * (size_t)(height + 2 * border);
    if (ht && ht->ids)                                                  // (the kernel reads no row for such an id; the caller is told before anything is launched)
        for (size_t i = 0; i < nPix; ++i)
            if (ht->ids[i] >= ht->nRows && ht->ids[i] != KZ_MOTION_MISS)
                return kz_fail(KZ_ERR_INVALID_ARG, "%s: pixel (%zu, %zu) names mesh %u, the table has %u rows (a miss is %u)", call, i % (size_t)width, i / (size_t)width, ht->ids[i], ht->nRows, KZ_MOTION_MISS);
    if (ht && ht->responsive && ht->historyIn)                          // (a negative vf is the device's mark of a pixel that is not valid, kz_responsive.hip: no input may produce one)
        for (size_t i = 0; i < nPix; ++i)
            if (ht->historyIn[12 * i + 3] < 0.f || (ht->fastIn && ht->fastIn[4 * i + 3] < 0.f))
                return kz_fail(KZ_ERR_INVALID_ARG, "%s: pixel (%zu, %zu): a negative variance in the history or in the fast plane", call, i % (size_t)width, i / (size_t)width);
    if ((rc = kzUseDevice(device))) return rc;
    DevBuf<float4> films[5], planes[4], result; DevBuf<float> variance;
    const float *host[5] = {film, albedo, normal, depth, moment};
    for (int k = 0; k < 5; ++k) {
        if (!host[k]) continue;
        if ((rc = films[k].alloc(nTexels)) || (rc = films[k].upload((const float4 *)host[k], nTexels))) return rc;
    }
    for (int k = 0; k < 4; ++k) if ((rc = planes[k].alloc(nPix))) return rc;
    if ((rc = result.alloc(nTexels))) return rc;
    if (outVariance && (rc = variance.alloc(nPix))) return rc;
    var.moment = films[4]; var.variance = variance;
    DevBuf<float4> hE[2], hG[2]; DevBuf<float> hN[2];                   // the history: [0] read (historyIn), [1] written
    DevBuf<uint32_t> mIds; DevBuf<KzMotionRow> mRows; KzDnMotion M = {};
    DevBuf<float4> hF[2]; KzDnResponsive R = {};                        // the fast plane: [0] read (fastIn), [1] written
    if (ht) {
        static const float noView[9] = {};
        dnSetViews(&T, *ht->current, ht->previous ? ht->previous->o : noView, ht->previous ? ht->previous->inv : noView);
        const bool in = ht->historyIn && T.maxHistory != 1.0f;           // (maxHistory = 1: without history, by definition)
        for (int k = in ? 0 : 1; k < 2; ++k) if ((rc = hE[k].alloc(nPix)) || (rc = hG[k].alloc(nPix)) || (rc = hN[k].alloc(nPix))) return rc;
        if (in) {
            std::vector<float> e(4 * nPix), g(4 * nPix), n(nPix);
            for (size_t i = 0; i < nPix; ++i) { std::memcpy(&e[4 * i], ht->historyIn + 12 * i, 16); std::memcpy(&g[4 * i], ht->historyIn + 12 * i + 4, 16); n[i] = ht->historyIn[12 * i + 8]; }
            if ((rc = hE[0].upload((const float4 *)e.data(), nPix)) || (rc = hG[0].upload((const float4 *)g.data(), nPix)) || (rc = hN[0].upload(n.data(), nPix))) return rc;
            T.inE = hE[0]; T.inG = hG[0]; T.inN = hN[0];
        }
        T.outE = hE[1]; T.outG = hG[1]; T.outN = hN[1];
        var.temporal = &T;
        if (ht->ids) {
            if ((rc = mIds.alloc(nPix)) || (rc = mIds.upload(ht->ids, nPix))) return rc;
            if (ht->nRows && ((rc = mRows.alloc(ht->nRows)) || (rc = mRows.upload(ht->rows, ht->nRows)))) return rc;
            M.ids = mIds; M.rows = mRows; M.nRows = ht->nRows;
            var.motion = &M;
        }
        if (ht->responsive) {
            R = *ht->responsive;
            if ((rc = hF[1].alloc(nPix))) return rc;
            if (in && ht->fastIn) {
                if ((rc = hF[0].alloc(nPix)) || (rc = hF[0].upload((const float4 *)ht->fastIn, nPix))) return rc;
                R.inF = hF[0];
            }
            R.outF = hF[1];
            var.responsive = &R;
        }
    }
    float4 *const colour[2] = {planes[0].get(), planes[1].get()};
    if ((rc = dnRun(plan, moment ? &var : nullptr, width, height, border, films[0], films[1], films[2], films[3], colour, planes[2], planes[3], result, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (ht && ht->historyOut && (rc = dnHistoryDownload(hE[1], hG[1], hN[1], nPix, ht->historyOut))) return rc;
    if (ht && ht->responsive && ht->fastOut && (rc = dnFastDownload(hF[1], nPix, ht->fastOut))) return rc;
    if (outVariance && (rc = variance.download(outVariance, nPix))) return rc;
    return result.download((float4 *)out, nTexels);
}

// What kz_denoise_temporal_films, kz_denoise_motion_films and kz_denoise_responsive_films refuse before anything else, under the call's own name: a null film, a
// null view and, `motion`, null ids or rows and a row that is not one of the three kinds
static int dnHistoryFilmsArgs(const char *call, const float *film, const float *moment, const float *depth, const float *out, const KzDnHostTemporal &ht, bool motion) {
    if (!film || !moment || !depth || !out) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null film (the picture, the moment film and the depth film are needed)", call);
    if (!ht.current || (ht.historyIn && !ht.previous)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null view (the current one, and with a history the one it was stored with)", call);
    if (!motion) return KZ_OK;
    if (!ht.ids || (ht.nRows && !ht.rows)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null ids or rows (the id plane, and %u rows)", call, ht.nRows);
    for (uint32_t m = 0; m < ht.nRows; ++m) {
        const KzMotionRow &r = ht.rows[m];
        if ((r.flags & ~(KZ_MOTION_STATIC | KZ_MOTION_UNTRACKED)) || r.flags == (KZ_MOTION_STATIC | KZ_MOTION_UNTRACKED) || r.reserved[0] || r.reserved[1])
            return kz_fail(KZ_ERR_INVALID_ARG, "%s: row %u: flags = %u (0, KZ_MOTION_STATIC or KZ_MOTION_UNTRACKED) or a non-zero reserved word", call, m, r.flags);
    }
    return KZ_OK;
}

extern "C" {

int kz_denoise_on(KzScene *scene, int device, const KzDenoiseOpts *opts) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise: null scene");
    KzDnPlan plan; KzDeviceState *ds; int rc;
    if ((rc = dnPlan(opts, scene->aovMask, "kz_denoise", &plan, 1.0f))) return rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    return dnOnReplica(scene, ds, plan, nullptr);
}
int kz_denoise(KzScene *scene, const KzDenoiseOpts *opts) { return kz_denoise_on(scene, -1, opts); }

static int dnResult(KzScene *scene, int device, const char *call, KzDeviceState **out) {
    int rc;
    if ((rc = findReplica(scene, device, out))) return rc;
    if (!(*out)->dnValid || !(*out)->dnOut) return kz_fail(KZ_ERR_STATE, "%s: no kz_denoise has run on this replica (or its result was released)", call);
    return KZ_OK;
}
int kz_denoise_download(KzScene *scene, int device, float *film, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = dnResult(scene, device, "kz_denoise_download", &ds))) return rc;
    if (!film || nFloats != ds->dnOut.cap() * 4) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_download: film buffer must hold %zu floats", ds->dnOut.cap() * 4);
    HIP_TRY(hipMemcpy(film, ds->dnOut, nFloats * sizeof(float), hipMemcpyDeviceToHost));
    return KZ_OK;
}
int kz_denoise_to_srgb8(KzScene *scene, int device, uint8_t *rgb8, size_t nBytes) {
    KzDeviceState *ds; int rc;
    if ((rc = dnResult(scene, device, "kz_denoise_to_srgb8", &ds))) return rc;
    if (ds->dnOut.cap() != ds->filmPixels) return kz_fail(KZ_ERR_STATE, "kz_denoise_to_srgb8: the frame has changed since the last kz_denoise");
    return kzFilmSrgb8(scene, ds, ds->dnOut, rgb8, nBytes);
}
int kz_denoise_info(KzScene *scene, int device, uint64_t *bytes) {
    KzDeviceState *ds; int rc;
    if (!bytes) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_info: null bytes");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    *bytes = ds->dnBytes();
    return KZ_OK;
}
int kz_denoise_release(KzScene *scene, int device) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    ds->dnColor[0].free(); ds->dnColor[1].free(); ds->dnNormalZ.free(); ds->dnAlbedo.free(); ds->dnOut.free();
    ds->dnValid = false;
    return KZ_OK;
}

int kz_denoise_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *albedo, const float *normal, const float *depth,
                     const KzDenoiseOpts *opts, float *out) {
    if (!film || !out) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_films: null film");
    return dnFilms("kz_denoise_films", device, width, height, border, film, nullptr, albedo, normal, depth, opts, nullptr, out, nullptr);
}

// The replica's side of a variance-guided call, under the call's own name: the second-moment film switched on, the replica, and the sample count the kernels
// divide by (`samples` 0: the replica's own), which must be the picture's
static int dnReplicaSamples(const char *call, KzScene *scene, int device, uint32_t samples, KzDeviceState **ds, float *out) {
    int rc;
    if (!scene->varianceMode) return kz_fail(KZ_ERR_STATE, "%s: the second-moment film is switched off (kz_scene_variance gives 0): kz_scene_set_variance(scene, 1), then render", call);
    if ((rc = findReplica(scene, device, ds))) return rc;
    if (!samples) samples = (*ds)->momentSamples;
    if (!samples) return kz_fail(KZ_ERR_STATE, "%s: KzVarianceOpts.samples = 0 and the replica's second-moment film has been given 0 samples per pixel (the picture's: %u)", call, (*ds)->pictureSamples);
    if ((*ds)->pictureSamples != (*ds)->momentSamples)
        return kz_fail(KZ_ERR_STATE, "%s: the picture's film holds %u samples per pixel, the second-moment film %u (switched on late: kz_film_clear, then render both)", call, (*ds)->pictureSamples, (*ds)->momentSamples);
    *out = (float)samples;
    return KZ_OK;
}

int kz_denoise_variance(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance: null scene");
    KzDnPlan plan; KzDnVar var = {}; KzDeviceState *ds; int rc; uint32_t samples;
    if ((rc = dnPlan(opts, scene->aovMask, "kz_denoise_variance", &plan, 2.0f)) || (rc = dnVarianceOpts(vopts, "kz_denoise_variance", &var.sv2, &samples)) ||
        (rc = dnReplicaSamples("kz_denoise_variance", scene, device, samples, &ds, &var.samples))) return rc;
    return dnOnReplica(scene, ds, plan, &var);
}

int kz_denoise_variance_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                              const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance) {
    if (!film || !moment || !out) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance_films: null film");
    return dnFilms("kz_denoise_variance_films", device, width, height, border, film, moment, albedo, normal, depth, opts, vopts, out, outVariance);
}

// ---- include/kazen_mi355x_temporal.h
int kz_temporal_view(const KzCamera *camera, KzTemporalView *view) {
    if (!camera || !view) return kz_fail(KZ_ERR_INVALID_ARG, "kz_temporal_view: null argument");
    std::memset(view, 0, sizeof *view);
    if (camera->width < 1 || camera->height < 1) return kz_fail(KZ_ERR_INVALID_ARG, "kz_temporal_view: a frame of %d x %d", camera->width, camera->height);
    KzParams P{};
    int rc;
    if ((rc = kzCameraParams(*camera, P))) return rc;
    return dnViewOf(P, "kz_temporal_view", view);
}

// kz_denoise_temporal and, with `motion`, kz_denoise_motion (include/kazen_mi355x_motion.h): one path, the same refusals under the call's own name
// and, with `responsive`, kz_denoise_responsive (include/kazen_mi355x_responsive.h; `ropts`: its alone)
static int dnTemporalCall(const char *call, bool motion, KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts,
                          bool responsive = false, const KzResponsiveOpts *ropts = nullptr) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null scene", call);
    KzDnPlan plan; KzDnVar var = {}; KzDnTemporal T; KzDnResponsive R; KzDeviceState *ds; int rc; uint32_t samples;
    if ((rc = dnPlan(opts, scene->aovMask, call, &plan, 2.0f)) || (rc = dnVarianceOpts(vopts, call, &var.sv2, &samples)) || (rc = dnTemporalOpts(topts, call, &T)) ||
        (rc = dnTemporalGuides(plan, scene->aovMask, call)) || (responsive && (rc = dnResponsiveOpts(ropts, call, &R)))) return rc;
    if (!(scene->aovMask & KZ_AOV_DEPTH)) return kz_fail(KZ_ERR_STATE, "%s: the depth film is not among the scene's AOVs (mask %u, KZ_AOV_DEPTH = %u): kz_scene_set_aovs, then render", call, scene->aovMask, KZ_AOV_DEPTH);
    if ((rc = dnReplicaSamples(call, scene, device, samples, &ds, &var.samples))) return rc;
    return dnOnReplica(scene, ds, plan, &var, &T, motion, responsive ? &R : nullptr);
}
int kz_denoise_temporal(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts) {
    return dnTemporalCall("kz_denoise_temporal", false, scene, device, opts, vopts, topts);
}

int kz_temporal_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *frames) {
    KzDeviceState *ds; int rc;
    if (!bytes && !frames) return kz_fail(KZ_ERR_INVALID_ARG, "kz_temporal_info: null bytes and frames");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (bytes) *bytes = ds->tpBytes();
    if (frames) *frames = ds->tpFrames;
    return KZ_OK;
}

int kz_temporal_reset(KzScene *scene, int device) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    for (int k = 0; k < 2; ++k) { ds->tpE[k].free(); ds->tpG[k].free(); ds->tpN[k].free(); }
    ds->tpFrames = 0; ds->tpCur = 0;
    ds->mtIds.free(); ds->mtRows.free(); ds->mtCounts[0] = ds->mtCounts[1] = ds->mtCounts[2] = 0;      // (kazen_mi355x_motion.h: the id plane and the rows go with the history)
    ds->rsF[0].free(); ds->rsF[1].free(); ds->rsStore = 0;              // (kazen_mi355x_responsive.h: so does the fast plane)
    return KZ_OK;
}

int kz_temporal_download(KzScene *scene, int device, float *history, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!ds->tpFrames) return kz_fail(KZ_ERR_STATE, "kz_temporal_download: no kz_denoise_temporal has run on this replica (or its history was reset)");
    const size_t nPix = ds->tpN[ds->tpCur].cap();
    if (!history || nFloats != nPix * 12) return kz_fail(KZ_ERR_INVALID_ARG, "kz_temporal_download: history buffer must hold %zu floats", nPix * 12);
    return dnHistoryDownload(ds->tpE[ds->tpCur], ds->tpG[ds->tpCur], ds->tpN[ds->tpCur], nPix, history);
}

int kz_denoise_temporal_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                              const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current, const KzTemporalView *previous,
                              const float *historyIn, float *out, float *historyOut, float *outVariance) {
    static const char *const call = "kz_denoise_temporal_films";
    const KzDnHostTemporal ht = {topts, current, previous, historyIn, historyOut};
    int rc;
    if ((rc = dnHistoryFilmsArgs(call, film, moment, depth, out, ht, false))) return rc;
    return dnFilms(call, device, width, height, border, film, moment, albedo, normal, depth, opts, vopts, out, outVariance, &ht);
}

// ---- include/kazen_mi355x_motion.h (kz_motion_rows and kz_motion_ids: kz_motion.hip)
int kz_denoise_motion(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts) {
    return dnTemporalCall("kz_denoise_motion", true, scene, device, opts, vopts, topts);
}

int kz_denoise_motion_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                            const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current, const KzTemporalView *previous,
                            const float *historyIn, const uint32_t *ids, const KzMotionRow *rows, uint32_t nRows, float *out, float *historyOut, float *outVariance) {
    static const char *const call = "kz_denoise_motion_films";
    const KzDnHostTemporal ht = {topts, current, previous, historyIn, historyOut, ids, rows, nRows};
    int rc;
    if ((rc = dnHistoryFilmsArgs(call, film, moment, depth, out, ht, true))) return rc;
    return dnFilms(call, device, width, height, border, film, moment, albedo, normal, depth, opts, vopts, out, outVariance, &ht);
}

int kz_motion_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *counts) {
    KzDeviceState *ds; int rc;
    if (!bytes && !counts) return kz_fail(KZ_ERR_INVALID_ARG, "kz_motion_info: null bytes and counts");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (bytes) *bytes = ds->mtBytes();
    if (counts) std::memcpy(counts, ds->mtCounts, sizeof ds->mtCounts);
    return KZ_OK;
}

// ---- include/kazen_mi355x_responsive.h (the kernels: kz_responsive.hip)
int kz_denoise_responsive(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzResponsiveOpts *ropts) {
    return dnTemporalCall("kz_denoise_responsive", true, scene, device, opts, vopts, topts, true, ropts);
}

int kz_denoise_responsive_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                                const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current, const KzTemporalView *previous,
                                const float *historyIn, const uint32_t *ids, const KzMotionRow *rows, uint32_t nRows, float *out, float *historyOut, float *outVariance,
                                const KzResponsiveOpts *ropts, const float *fastIn, float *fastOut) {
    static const char *const call = "kz_denoise_responsive_films";
    KzDnResponsive R; int rc;
    const KzDnHostTemporal ht = {topts, current, previous, historyIn, historyOut, ids, rows, nRows, &R, fastIn, fastOut};
    if ((rc = dnHistoryFilmsArgs(call, film, moment, depth, out, ht, true)) || (rc = dnResponsiveOpts(ropts, call, &R))) return rc;
    return dnFilms(call, device, width, height, border, film, moment, albedo, normal, depth, opts, vopts, out, outVariance, &ht);
}

int kz_responsive_download(KzScene *scene, int device, float *fast, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!ds->tpFrames || !ds->rsStore || ds->rsStore != ds->tpStore)
        return kz_fail(KZ_ERR_STATE, "kz_responsive_download: no kz_denoise_responsive stored this replica's history (none has run, the history was reset, or another call stored it since)");
    const size_t nPix = ds->rsF[ds->tpCur].cap();
    if (!fast || nFloats != nPix * 4) return kz_fail(KZ_ERR_INVALID_ARG, "kz_responsive_download: the buffer must hold %zu floats", nPix * 4);
    return dnFastDownload(ds->rsF[ds->tpCur], nPix, fast);
}

int kz_responsive_info(KzScene *scene, int device, uint64_t *bytes) {
    KzDeviceState *ds; int rc;
    if (!bytes) return kz_fail(KZ_ERR_INVALID_ARG, "kz_responsive_info: null bytes");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    *bytes = ds->rsBytes();
    return KZ_OK;
}

} // extern "C"
