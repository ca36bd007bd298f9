// kz_variance.hip - the variance-guided a-trous filter of include/kazen_mi355x_variance.h: its kernels and entry points (the second-moment film itself is a film
// like the others: kz_film.hip). A unit of its own beside kz_denoise.hip, whose kernels keep their code; what the two share is the arithmetic (kz_denoise.h), the
// options' plan (dnPlan) and the replica's denoise buffers, which kz_denoise_download / _to_srgb8 / _info / _release serve for both calls. Compiled like
// kz_denoise.hip WITHOUT -fgpu-flush-denormals-to-zero (build.sh): the result equals the C++ restatement's (tests/cpu_ref/kz_variance_ref.cpp) to the bit.
#include <hip/hip_runtime.h>

#include "../../include/kazen_mi355x_variance.h"
#include "kz_state.h"
#include "kz_denoise.h"

#include <cmath>
#include <cstring>

// The kernels: kz_denoise.hip's four, restated with the colour plane's .w carrying v (negative: not valid) instead of the valid flag, so the planes and the tap loads
// are kz_denoise's and the call needs no buffer of its own.
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_prepare_var(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment,
                                                                 const float4 *__restrict__ albedo, const float4 *__restrict__ normal, const float4 *__restrict__ depth,
                                                                 int demodulate, float samples, float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    const uint32_t i = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const size_t t = (size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border);
    const float4 c = dnValue(film, t), s = dnValue(moment, t), a = dnValue(albedo, t), n = dnValue(normal, t), z = dnValue(depth, t);
    const float vr = dnMax(s.x - c.x * c.x, 0.f) / samples, vg = dnMax(s.y - c.y * c.y, 0.f) / samples, vb = dnMax(s.z - c.z * c.z, 0.f) / samples;
    float4 e = make_float4(c.x, c.y, c.z, (vr + vg) + vb);
    if (demodulate) {
        const float ar = dnMax(a.x, 1e-3f), ag = dnMax(a.y, 1e-3f), ab = dnMax(a.z, 1e-3f);
        e.x = c.x / ar; e.y = c.y / ag; e.z = c.z / ab;
        e.w = (vr / (ar * ar) + vg / (ag * ag)) + vb / (ab * ab);
    }
    if (c.w == 0.f) e.w = -1.f;                                         // not valid
    colour[i] = e;
    normalZ[i] = make_float4(n.x, n.y, n.z, z.x);
    albedoP[i] = make_float4(a.x, a.y, a.z, 0.f);
}

// The direct-gather form: kz_dn_atrous's taps, behind the nine .w of the pixel's unit-spaced neighbours (the prefilter that sets its tolerance)
template <bool GUIDED>
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_atrous_var(KzDnIter I, float sv2, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                                                                float4 *__restrict__ colOut) {
    const int x = (int)(blockIdx.x * KZ_DN_ROW + threadIdx.x), y = (int)(blockIdx.y * (KZ_DN_BLOCK / KZ_DN_ROW) + threadIdx.y);
    if (x >= I.width || y >= I.height) return;
    const size_t ip = (size_t)y * (size_t)I.width + (size_t)x;
    const float4 ep = colIn[ip];
    if (!dnValidVar(ep)) { colOut[ip] = ep; return; }
    float gn = 0.f, gd = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        const bool rowIn = qy >= 0 && qy < I.height;
        const size_t rowAt = (size_t)(rowIn ? qy : y) * (size_t)I.width;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            const bool colIn_ = qx >= 0 && qx < I.width;
            const float vq = colIn[rowAt + (size_t)(colIn_ ? qx : x)].w;
            if (rowIn && colIn_ && !(vq < 0.f)) dnPrefilter(dy, dx, vq, gn, gd);
        }
    }
    const float kcv = dnTolerance(I.kc, sv2, gn, gd);
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
            if (in && dnValidVar(eq)) dnTapVar<GUIDED>(I, kcv, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den, nv);
        }
    }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, nv / (den * den));
}

#if KZ_DN_LDS_MAX_STEP
// The LDS-tile form: kz_dn_atrous_lds's tile (its halo of 2 * STEP >= 2 holds the prefilter's neighbours too); a texel outside the frame is staged as not valid
template <bool GUIDED, int STEP>
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_atrous_var_lds(KzDnIter I, float sv2, const float4 *__restrict__ colIn, const float4 *__restrict__ normalZ, const float4 *__restrict__ albedoP,
                                                                    float4 *__restrict__ colOut) {
    constexpr int R = 2 * STEP, T = 16 + 2 * R, N = T * T;
    __shared__ float4 tile[(GUIDED ? 3 : 1) * N];
    const int x0 = (int)blockIdx.x * 16, y0 = (int)blockIdx.y * 16;
    for (int k = (int)threadIdx.x; k < N; k += KZ_DN_BLOCK) {
        const int ty = k / T, tx = k - ty * T, gx = x0 - R + tx, gy = y0 - R + ty;
        float4 e = make_float4(0.f, 0.f, 0.f, -1.f), g = make_float4(0.f, 0.f, 0.f, 0.f), a = g;
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
    if (!dnValidVar(ep)) { colOut[ip] = ep; return; }
    float gn = 0.f, gd = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float vq = tile[c + dy * T + dx].w;
            if (!(vq < 0.f)) dnPrefilter(dy, dx, vq, gn, gd);
        }
    const float kcv = dnTolerance(I.kc, sv2, gn, gd);
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
            if (dnValidVar(eq)) dnTapVar<GUIDED>(I, kcv, dnH(dy) * dnH(dx), ep, eq, gp, gq, ap, aq, nr, ng, nb, den, nv);
        }
    colOut[ip] = make_float4(nr / den, ng / den, nb / den, nv / (den * den));
}
#endif

// kz_dn_finish with validity read from the sign of .w; `variance` (may be null): v_last per frame pixel, 0 where the pixel is not valid
__global__ __launch_bounds__(KZ_DN_BLOCK) void kz_dn_finish_var(int width, int height, int border, const float4 *__restrict__ colour, const float4 *__restrict__ albedoP,
                                                                int demodulate, float4 *__restrict__ out, float *__restrict__ variance) {
    const uint32_t t = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    const uint32_t cols = (uint32_t)(width + 2 * border), rows = (uint32_t)(height + 2 * border);
    if (t >= cols * rows) return;
    const int y = (int)(t / cols) - border, x = (int)(t - (t / cols) * cols) - border;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x >= 0 && x < width && y >= 0 && y < height) {
        const size_t i = (size_t)y * (size_t)width + (size_t)x;
        const float4 e = colour[i];
        const bool valid = dnValidVar(e);
        if (valid) {
            r = make_float4(e.x, e.y, e.z, 1.f);
            if (demodulate) { const float4 a = albedoP[i]; r.x = e.x * dnMax(a.x, 1e-3f); r.y = e.y * dnMax(a.y, 1e-3f); r.z = e.z * dnMax(a.z, 1e-3f); }
        }
        if (variance) variance[i] = valid ? e.w : 0.f;
    }
    out[t] = r;
}

// ---- host side ----
// The launches of one variance-guided call: dnRun's, with the kernels above. `moment`: the second-moment film (null: zeros); `variance`: null or width x height floats.
static int dnRunVar(const KzDnPlan &plan, float sv2, float samples, int width, int height, int border, const float4 *film, const float4 *moment, const float4 *albedo, const float4 *normal,
                    const float4 *depth, float4 *const colour[2], float4 *normalZ, float4 *albedoP, float4 *out, float *variance, hipStream_t stream) {
    const uint32_t nPix = (uint32_t)width * (uint32_t)height, nTexels = (uint32_t)(width + 2 * border) * (uint32_t)(height + 2 * border);
    const int demod = plan.demodulate ? 1 : 0;
    hipLaunchKernelGGL(kz_dn_prepare_var, dim3((nPix + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), dim3(KZ_DN_BLOCK), 0, stream, width, height, border, film, moment,
                       (plan.guides & KZ_AOV_ALBEDO) ? albedo : nullptr, (plan.guides & KZ_AOV_NORMAL) ? normal : nullptr, (plan.guides & KZ_AOV_DEPTH) ? depth : nullptr,
                       demod, samples, colour[0], normalZ, albedoP);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((width + KZ_DN_ROW - 1) / KZ_DN_ROW), (unsigned)((height + KZ_DN_BLOCK / KZ_DN_ROW - 1) / (KZ_DN_BLOCK / KZ_DN_ROW))), blk(KZ_DN_ROW, KZ_DN_BLOCK / KZ_DN_ROW);
    for (uint32_t i = 0; i < plan.iterations; ++i) {
        const KzDnIter I = {width, height, 1 << i, plan.kc[i], plan.kn, plan.kz, plan.ka};
#if KZ_DN_LDS_MAX_STEP
        if ((1 << i) <= KZ_DN_LDS_MAX_STEP) {
            const dim3 g16((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
#define KZ_DN_LDS(G, S) hipLaunchKernelGGL((kz_dn_atrous_var_lds<G, S>), g16, dim3(KZ_DN_BLOCK), 0, stream, I, sv2, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1])
            if (plan.guided) { if (i == 0) KZ_DN_LDS(true, 1); else KZ_DN_LDS(true, 2); }
            else { if (i == 0) KZ_DN_LDS(false, 1); else KZ_DN_LDS(false, 2); }
#undef KZ_DN_LDS
            HIP_TRY(hipGetLastError());
            continue;
        }
#endif
        if (plan.guided) hipLaunchKernelGGL(kz_dn_atrous_var<true>, grid, blk, 0, stream, I, sv2, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1]);
        else hipLaunchKernelGGL(kz_dn_atrous_var<false>, grid, blk, 0, stream, I, sv2, (const float4 *)colour[i & 1], (const float4 *)normalZ, (const float4 *)albedoP, colour[(i + 1) & 1]);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(kz_dn_finish_var, dim3((nTexels + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), dim3(KZ_DN_BLOCK), 0, stream, width, height, border,
                       (const float4 *)colour[plan.iterations & 1], (const float4 *)albedoP, demod, out, variance);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
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

extern "C" {

int kz_denoise_variance(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance: null scene");
    KzDnPlan plan; KzDeviceState *ds; int rc; float sv2; uint32_t samples;
    if ((rc = dnPlan(opts, scene->aovMask, "kz_denoise_variance", &plan, 2.0f)) || (rc = dnVarianceOpts(vopts, "kz_denoise_variance", &sv2, &samples))) return rc;
    if (!scene->varianceMode) return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: the second-moment film is switched off (kz_scene_variance gives 0): kz_scene_set_variance(scene, 1), then render");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!samples) samples = ds->momentSamples;
    if (!samples) return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: KzVarianceOpts.samples = 0 and the replica's second-moment film has been given 0 samples per pixel (the picture's: %u)", ds->pictureSamples);
    if (ds->pictureSamples != ds->momentSamples)
        return kz_fail(KZ_ERR_STATE, "kz_denoise_variance: the picture's film holds %u samples per pixel, the second-moment film %u (switched on late: kz_film_clear, then render both)", ds->pictureSamples, ds->momentSamples);
    const KzParams &P = scene->prm;
    const size_t nPix = (size_t)P.width * (size_t)P.height;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));                      // the replica's queued work: the films and the sums are final
    const float4 *guide[3] = {nullptr, nullptr, nullptr}, *moment = nullptr;
    if (ds->moment().sums && ds->moment().texels) {
        if ((rc = kzFilmResolve(scene, ds->moment(), ds->lastStream))) return rc;
        moment = ds->moment().texels;
    }
    for (int f = 0; f < 3; ++f) {
        const bool wanted = f == 0 ? (plan.demodulate || (plan.guided && (plan.guides & KZ_AOV_ALBEDO))) : (plan.guided && (plan.guides & (1u << f)));
        KzFilm &film = ds->aov(f);
        if (!wanted || !film.sums || !film.texels) continue;
        if ((rc = kzFilmResolve(scene, film, ds->lastStream))) return rc;
        guide[f] = film.texels;
    }
    ds->dnValid = false;
    for (DevBuf<float4> *b : {&ds->dnColor[0], &ds->dnColor[1], &ds->dnNormalZ, &ds->dnAlbedo})
        if (b->cap() != nPix && (rc = b->regrow(nPix))) return rc;
    if (ds->dnOut.cap() != ds->filmPixels && (rc = ds->dnOut.regrow(ds->filmPixels))) return rc;
    float4 *const colour[2] = {ds->dnColor[0].get(), ds->dnColor[1].get()};
    if ((rc = dnRunVar(plan, sv2, (float)samples, P.width, P.height, P.border, ds->picture().texels, moment, guide[0], guide[1], guide[2], colour, ds->dnNormalZ, ds->dnAlbedo, ds->dnOut, nullptr, ds->lastStream))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    ds->dnValid = true;
    return KZ_OK;
}

int kz_denoise_variance_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                              const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance) {
    if (!film || !moment || !out) return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance_films: null film");
    if (width < 1 || height < 1 || border < 0 || border > 64 || (uint64_t)(width + 2 * (int64_t)border) * (uint64_t)(height + 2 * (int64_t)border) >= (1ull << 31))
        return kz_fail(KZ_ERR_INVALID_ARG, "kz_denoise_variance_films: a frame of %d x %d with border %d (at least 1 x 1, border 0 .. 64, fewer than 2^31 texels)", width, height, border);
    KzDnPlan plan; int rc; float sv2; uint32_t samples;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | (depth ? KZ_AOV_DEPTH : 0u);
    if ((rc = dnPlan(opts, avail, "kz_denoise_variance_films", &plan, 2.0f)) || (rc = dnVarianceOpts(vopts, "kz_denoise_variance_films", &sv2, &samples))) return rc;
    if (!samples) return kz_fail(KZ_ERR_STATE, "kz_denoise_variance_films: KzVarianceOpts.samples = 0 (there is no replica whose count could stand in: state it)");
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
    float4 *const colour[2] = {planes[0].get(), planes[1].get()};
    if ((rc = dnRunVar(plan, sv2, (float)samples, width, height, border, films[0], films[4], films[1], films[2], films[3], colour, planes[2], planes[3], result, outVariance ? variance.get() : nullptr, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (outVariance && (rc = variance.download(outVariance, nPix))) return rc;
    return result.download((float4 *)out, nTexels);
}

} // extern "C"
