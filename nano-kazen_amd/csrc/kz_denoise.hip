// kz_denoise.hip - the device side and the entry points of include/kazen_mi355x_denoise.h: the picture denoised by an edge-avoiding a-trous filter guided by the
// feature films, a separate call after a render (nothing here runs inside a pass).
//
// Per kz_denoise, on the replica's lastStream:
//   kz_dn_prepare   per frame pixel: the four films' values into frame-sized planes without an apron - (e_0.rgb, valid), (n.xyz, z), (a.rgb, -); the guide
//                   planes are written once, the colour plane ping-pongs between the iterations
//   kz_dn_atrous    one launch per iteration, one lane per pixel: steps 1 and 2 from an LDS tile with a halo (kz_dn_atrous_lds), the larger steps by direct
//                   gather with a wave along a row - every tap of a wave is one contiguous 1 KB load per plane
//   kz_dn_finish    per film texel: remodulated colour and weight 1 in a valid frame pixel, (0, 0, 0, 0) elsewhere (the apron too)
// Each kernel's result is a function of its inputs alone: no atomics, no order between threads, the taps of a pixel summed by its own lane in the stated order
// (kz_denoise.h). This unit is compiled WITHOUT -fgpu-flush-denormals-to-zero (build.sh), so a subnormal weight is the C++ restatement's to the bit.
#include <hip/hip_runtime.h>

#include "../../include/kazen_mi355x_denoise.h"
#include "kz_state.h"
#include "kz_denoise.h"

#include <cmath>
#include <cstring>

__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_prepare(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ albedo,
                                                             const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate,
                                                             float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    const uint32_t i = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const size_t t = (size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border);      // < (height + 2b)(width + 2b): the films' texels
    const float4 c = dnValue(film, t), a = dnValue(albedo, t), n = dnValue(normal, t), z = dnValue(depth, t);
    float4 e = make_float4(c.x, c.y, c.z, c.w != 0.f ? 1.f : 0.f);
    if (demodulate) { e.x = c.x / dnMax(a.x, 1e-3f); e.y = c.y / dnMax(a.y, 1e-3f); e.z = c.z / dnMax(a.z, 1e-3f); }
    colour[i] = e;
    normalZ[i] = make_float4(n.x, n.y, n.z, z.x);
    albedoP[i] = make_float4(a.x, a.y, a.z, 0.f);
}

// The direct-gather form: lane (x, y) loads its 25 taps from the planes (the rows of a wave's taps are contiguous; L1 / L2 serve the 25-fold reuse)
template <bool GUIDED>
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_atrous(KzDnIter I, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                                                            float4 *__restrict__ colOut) {
    const int x = (int)(blockIdx.x * KZ_DN_ROW + threadIdx.x), y = (int)(blockIdx.y * (KZ_DN_BLOCK / KZ_DN_ROW) + threadIdx.y);
    if (x >= I.width || y >= I.height) return;
    const size_t ip = (size_t)y * (size_t)I.width + (size_t)x;
    const float4 ep = colIn[ip];
    if (ep.w == 0.f) { colOut[ip] = ep; return; }                       // not valid: neither gives nor receives (its colour stays 0)
    float4 gp = ep, ap = ep;
    if (GUIDED) { gp = normalZ[ip]; ap = albedoP[ip]; }
    float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f;
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
            if (in && eq.w != 0.f) dnTap<GUIDED>(I, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den);
        }
    }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, 1.f);
}

#if KZ_DN_LDS_MAX_STEP
// The LDS-tile form, for the small steps: a 16 x 16 tile of pixels with a halo of 2 * STEP (20 x 20 / 24 x 24 texels of up to 48 B), staged once per workgroup;
// a texel outside the frame is staged as not valid. The same taps in the same order as the direct form: the same bits.
template <bool GUIDED, int STEP>
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_atrous_lds(KzDnIter I, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                                                                float4 *__restrict__ colOut) {
    constexpr int R = 2 * STEP, T = 16 + 2 * R, N = T * T;
    __shared__ float4 tile[(GUIDED ? 3 : 1) * N];
    const int x0 = (int)blockIdx.x * 16, y0 = (int)blockIdx.y * 16;
    for (int k = (int)threadIdx.x; k < N; k += KZ_DN_BLOCK) {
        const int ty = k / T, tx = k - ty * T, gx = x0 - R + tx, gy = y0 - R + ty;
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f), g = e, a = e;
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
    if (ep.w == 0.f) { colOut[ip] = ep; return; }
    float4 gp = ep, ap = ep;
    if (GUIDED) { gp = tile[N + c]; ap = tile[2 * N + c]; }
    float nr = 0.f, ng = 0.f, nb = 0.f, den = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int k = c + dy * STEP * T + dx * STEP;
            const float4 eq = tile[k];
            float4 gq = eq, aq = eq;
            if (GUIDED) { gq = tile[N + k]; aq = tile[2 * N + k]; }
            if (eq.w != 0.f) dnTap<GUIDED>(I, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den);
        }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, 1.f);
}
#endif

__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_finish(int width, int height, int border, const float4 *__restrict__ colour, const float4 *__restrict__ albedoP,
                                                            int demodulate, float4 *__restrict__ out) {
    const uint32_t t = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    const uint32_t cols = (uint32_t)(width + 2 * border), rows = (uint32_t)(height + 2 * border);
    if (t >= cols * rows) return;
    const int y = (int)(t / cols) - border, x = (int)(t - (t / cols) * cols) - border;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x >= 0 && x < width && y >= 0 && y < height) {
        const size_t i = (size_t)y * (size_t)width + (size_t)x;
        const float4 e = colour[i];
        if (e.w != 0.f) {
            r = make_float4(e.x, e.y, e.z, 1.f);
            if (demodulate) { const float4 a = albedoP[i]; r.x = e.x * dnMax(a.x, 1e-3f); r.y = e.y * dnMax(a.y, 1e-3f); r.z = e.z * dnMax(a.z, 1e-3f); }
        }
    }
    out[t] = r;
}

// ---- host side ----
// What a call does, from its options (KzDnPlan, kz_denoise.h): `avail` = the guides there are (the scene's mask / the films given to kz_denoise_films);
// defaultSigmaColor: 1.0 for kz_denoise, 2.0 for kz_denoise_variance (kz_variance.hip)
int dnPlan(const KzDenoiseOpts *opts, uint32_t avail, const char *call, KzDnPlan *plan, float defaultSigmaColor) {
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

// The launches of one call on `stream`. The films are device buffers of (height + 2b) x (width + 2b) texels, a guide that is absent is null; colour[2], normalZ and
// albedoP hold width x height texels each, `out` a film. Nothing but these planes and `out` is written.
static int dnRun(const KzDnPlan &plan, int width, int height, int border, const float4 *film, const float4 *albedo, const float4 *normal, const float4 *depth,
                 float4 *const colour[2], float4 *normalZ, float4 *albedoP, float4 *out, hipStream_t stream) {
    const uint32_t nPix = (uint32_t)width * (uint32_t)height, nTexels = (uint32_t)(width + 2 * border) * (uint32_t)(height + 2 * border);
    const int demod = plan.demodulate ? 1 : 0;
    hipLaunchKernelGGL(kz_dn_prepare, dim3((nPix + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), dim3(KZ_DN_BLOCK), 0, stream, width, height, border, film,
                       (plan.guides & KZ_AOV_ALBEDO) ? albedo : nullptr, (plan.guides & KZ_AOV_NORMAL) ? normal : nullptr, (plan.guides & KZ_AOV_DEPTH) ? depth : nullptr,
                       demod, colour[0], normalZ, albedoP);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((width + KZ_DN_ROW - 1) / KZ_DN_ROW), (unsigned)((height + KZ_DN_BLOCK / KZ_DN_ROW - 1) / (KZ_DN_BLOCK / KZ_DN_ROW))), blk(KZ_DN_ROW, KZ_DN_BLOCK / KZ_DN_ROW);
    for (uint32_t i = 0; i < plan.iterations; ++i) {
        const KzDnIter I = {width, height, 1 << i, plan.kc[i], plan.kn, plan.kz, plan.ka};
#if KZ_DN_LDS_MAX_STEP
        if ((1 << i) <= KZ_DN_LDS_MAX_STEP) {
            const dim3 g16((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
#define KZ_DN_LDS(G, S) hipLaunchKernelGGL((kz_dn_atrous_lds<G, S>), g16, dim3(KZ_DN_BLOCK), 0, stream, I, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1])
            if (plan.guided) { if (i == 0) KZ_DN_LDS(true, 1); else KZ_DN_LDS(true, 2); }
            else { if (i == 0) KZ_DN_LDS(false, 1); else KZ_DN_LDS(false, 2); }
#undef KZ_DN_LDS
            HIP_TRY(hipGetLastError());
            continue;
        }
#endif
        if (plan.guided) hipLaunchKernelGGL(kz_dn_atrous<true>, grid, blk, 0, stream, I, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1]);
        else hipLaunchKernelGGL(kz_dn_atrous<false>, grid, blk, 0, stream, I, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1]);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(kz_dn_finish, dim3((nTexels + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), dim3(KZ_DN_BLOCK), 0, stream, width, height, border,
                       (const float4 *)colour[plan.iterations & 1], (const float4 *)albedoP, demod, out);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

extern "C" {

int kz_denoise_on(KzScene *scene, int device, const KzDenoiseOpts *opts) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise: null scene");
    KzDnPlan plan; KzDeviceState *ds; int rc;
    if ((rc = dnPlan(opts, scene->aovMask, "kz_denoise", &plan))) return rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const KzParams &P = scene->prm;
    const size_t nPix = (size_t)P.width * (size_t)P.height;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));                      // the replica's queued work: the film and the sums are final
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
    if ((rc = dnRun(plan, P.width, P.height, P.border, ds->picture().texels, guide[0], guide[1], guide[2], colour, ds->dnNormalZ, ds->dnAlbedo, ds->dnOut, ds->lastStream))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    ds->dnValid = true;
    return KZ_OK;
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
    if (width < 1 || height < 1 || border < 0 || border > 64 || (uint64_t)(width + 2 * (int64_t)border) * (uint64_t)(height + 2 * (int64_t)border) >= (1ull << 31))
        return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_films: a frame of %d x %d with border %d (at least 1 x 1, border 0 .. 64, fewer than 2^31 texels)", width, height, border);
    KzDnPlan plan; int rc;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | (depth ? KZ_AOV_DEPTH : 0u);
    if ((rc = dnPlan(opts, avail, "kz_denoise_films", &plan))) return rc;
    if ((rc = kzUseDevice(device))) return rc;
    const size_t nPix = (size_t)width * (size_t)height, nTexels = (size_t)(width + 2 * border) * (size_t)(height + 2 * border);
    DevBuf<float4> films[4], planes[4], result;
    const float *host[4] = {film, albedo, normal, depth};
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        if ((rc = films[k].alloc(nTexels)) || (rc = films[k].upload((const float4 *)host[k], nTexels))) return rc;
    }
    for (int k = 0; k < 4; ++k) if ((rc = planes[k].alloc(nPix))) return rc;
    if ((rc = result.alloc(nTexels))) return rc;
    float4 *const colour[2] = {planes[0].get(), planes[1].get()};
    if ((rc = dnRun(plan, width, height, border, films[0], films[1], films[2], films[3], colour, planes[2], planes[3], result, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return result.download((float4 *)out, nTexels);
}

} // extern "C"
