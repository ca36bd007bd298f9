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
// Each of the four is ONE body (dnPrepare, dnAtrous, dnAtrousLds, dnFinish) templated on VAR; the eight kernels are its two instances under the names the profiles
// know. With VAR the colour plane's .w carries v (negative: not valid) instead of the valid flag, so the planes and the tap loads are the same and the variance-
// guided call needs no buffer of its own. Each kernel's result is a function of its inputs alone: no atomics, no order between threads, the taps of a pixel summed
// by its own lane in the stated order (kz_denoise.h). This unit is compiled WITHOUT -fgpu-flush-denormals-to-zero (build.sh), so a subnormal weight is the C++
// restatements' (tests/cpu_ref/kz_denoise_ref.cpp, kz_variance_ref.cpp) to the bit.
#include <hip/hip_runtime.h>

#include "../../include/kazen_mi355x_denoise.h"
#include "../../include/kazen_mi355x_variance.h"
#include "kz_state.h"
#include "kz_denoise.h"

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
    float4 e = make_float4(c.x, c.y, c.z, c.w != 0.f ? 1.f : 0.f);
    float vr = 0.f, vg = 0.f, vb = 0.f;
    if (VAR) {
        const float4 s = dnValue(moment, t);
        vr = dnMax(s.x - c.x * c.x, 0.f) / samples; vg = dnMax(s.y - c.y * c.y, 0.f) / samples; vb = dnMax(s.z - c.z * c.z, 0.f) / samples;
        e.w = (vr + vg) + vb;
    }
    if (demodulate) {
        const float ar = dnMax(a.x, 1e-3f); e.x = c.x / ar;
        const float ag = dnMax(a.y, 1e-3f); e.y = c.y / ag;
        const float ab = dnMax(a.z, 1e-3f); e.z = c.z / ab;
        if (VAR) e.w = (vr / (ar * ar) + vg / (ag * ag)) + vb / (ab * ab);
    }
    if (VAR && c.w == 0.f) e.w = -1.f;                                  // not valid
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
struct KzDnVar { float sv2, samples; const float4 *moment; float *variance; };

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
    if (var) hipLaunchKernelGGL(kz_dn_prepare_var, gPix, b1, 0, stream, width, height, border, film, var->moment, albedo, normal, depth, demod, var->samples, colour[0], normalZ, albedoP);
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

// A call on a replica's own films, into its denoise buffers: behind the replica's queued work, with the guides the plan wants (and the moment film) resolved
static int dnOnReplica(KzScene *scene, KzDeviceState *ds, const KzDnPlan &plan, KzDnVar *var) {
    const KzParams &P = scene->prm;
    const size_t nPix = (size_t)P.width * (size_t)P.height;
    int rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));                      // the replica's queued work: the films and the sums are final
    if (var && ds->moment().sums && ds->moment().texels) {
        if ((rc = kzFilmResolve(scene, ds->moment(), ds->lastStream))) return rc;
        var->moment = ds->moment().texels;
    }
    const float4 *guide[3] = {nullptr, nullptr, nullptr};
    for (int f = 0; f < 3; ++f) {
        const bool wanted = f == 0 ? (plan.demodulate || (plan.guided && (plan.guides & KZ_AOV_ALBEDO))) : (plan.guided && (plan.guides & (1u << f)));
        KzFilm &film = ds->aov(f);
        if (!wanted || !film.sums || !film.texels) continue;                // (enabled, nothing rendered yet: zeros, as kz_aov_download gives)
        if ((rc = kzFilmResolve(scene, film, ds->lastStream))) return rc;
        guide[f] = film.texels;
    }
    ds->dnValid = false;
    for (DevBuf<float4> *b : {&ds->dnColor[0], &ds->dnColor[1], &ds->dnNormalZ, &ds->dnAlbedo})
        if (b->cap() != nPix && (rc = b->regrow(nPix))) return rc;
    if (ds->dnOut.cap() != ds->filmPixels && (rc = ds->dnOut.regrow(ds->filmPixels))) return rc;
    float4 *const colour[2] = {ds->dnColor[0].get(), ds->dnColor[1].get()};
    if ((rc = dnRun(plan, var, P.width, P.height, P.border, ds->picture().texels, guide[0], guide[1], guide[2], colour, ds->dnNormalZ, ds->dnAlbedo, ds->dnOut, ds->lastStream))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    ds->dnValid = true;
    return KZ_OK;
}

// A call on films of the host's: kz_denoise_films, and with `moment` kz_denoise_variance_films (`vopts`, `outVariance`: its alone)
static int dnFilms(const char *call, int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal,
                   const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance) {
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
    if ((rc = kzUseDevice(device))) return rc;
    const size_t nPix = (size_t)width * (size_t)height, nTexels = (size_t)(width + 2 * border) * (size_t)(height + 2 * border);
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
    float4 *const colour[2] = {planes[0].get(), planes[1].get()};
    if ((rc = dnRun(plan, moment ? &var : nullptr, width, height, border, films[0], films[1], films[2], films[3], colour, planes[2], planes[3], result, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (outVariance && (rc = variance.download(outVariance, nPix))) return rc;
    return result.download((float4 *)out, nTexels);
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

int kz_denoise_variance(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance: null scene");
    KzDnPlan plan; KzDnVar var = {}; KzDeviceState *ds; int rc; uint32_t samples;
    if ((rc = dnPlan(opts, scene->aovMask, "kz_denoise_variance", &plan, 2.0f)) || (rc = dnVarianceOpts(vopts, "kz_denoise_variance", &var.sv2, &samples))) return rc;
    if (!scene->varianceMode) return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: the second-moment film is switched off (kz_scene_variance gives 0): kz_scene_set_variance(scene, 1), then render");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!samples) samples = ds->momentSamples;
    if (!samples) return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: KzVarianceOpts.samples = 0 and the replica's second-moment film has been given 0 samples per pixel (the picture's: %u)", ds->pictureSamples);
    if (ds->pictureSamples != ds->momentSamples)
        return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: the picture's film holds %u samples per pixel, the second-moment film %u (switched on late: kz_film_clear, then render both)", ds->pictureSamples, ds->momentSamples);
    var.samples = (float)samples;
    return dnOnReplica(scene, ds, plan, &var);
}

int kz_denoise_variance_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                              const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance) {
    if (!film || !moment || !out) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance_films: null film");
    return dnFilms("kz_denoise_variance_films", device, width, height, border, film, moment, albedo, normal, depth, opts, vopts, out, outVariance);
}

} // extern "C"
