// kz_responsive.hip - the device side of include/kazen_mi355x_responsive.h (which holds the definition; every line of arithmetic below is one of its lines): the
// fast history beside the long one, and the long history clamped to the fast one's local statistics.
//   kz_dn_prepare_responsive  pass A, in kz_dn_prepare_motion's place: the history prepare stage's one body (kz_history.h: dnHistory) with MOTION and FAST - that
//                             kernel's lines plus one 16-byte fast-plane load per tap, the fast blend and one 16-byte store
//   kz_dn_clamp_history      pass B: a (2 r + 1)^2 stencil over the fast plane through an LDS tile; a pixel rewrites its own (e, v) in the colour plane and in the
//                             history's out copy, and its own N
// On the device the fast plane marks a pixel that is not valid with vf = -1 (the convention of the colour plane, kz_denoise.h: a variance is never negative), so pass
// B needs no plane but the fast one to know which texels of its window count; what leaves the device (kz_denoise.hip: dnFastDownload) has four zeros there, as the
// header says. Compiled like kz_denoise.hip (build.sh IEEE_UNITS): no flush to zero, no contraction - the results are tests/cpu_ref/kz_responsive_ref.cpp's to the bit.
#include <hip/hip_runtime.h>

#include "kz_state.h"
#include "kz_history.h"
#include "kz_responsive.h"

#define KZ_DN_KERNEL __global__ __launch_bounds__(KZ_DN_BLOCK) void

// dnHistory with everything on (KzDnFast: kz_history.h). M.ids null: every pixel static.
KZ_DN_KERNEL kz_dn_prepare_responsive(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                                      const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples, const KzDnTemporal T, const KzDnMotion M,
                                      const KzDnFast F, float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    dnHistory<true, true>(width, height, border, film, moment, albedo, normal, depth, demodulate, samples, T, M, F, colour, normalZ, albedoP);
}

// Pass B. A block is KZ_DN_ROW x KZ_DN_BLOCK / KZ_DN_ROW pixels (64 x 4: a wave along a row) plus an apron of R: (64 + 2R) x (4 + 2R) texels of the fast plane - 68 x 8
// float4 = 8704 bytes for R = 2 - staged with 16-byte loads, a texel outside the frame staged as not valid (vf = -1), so both loops skip by the one test. The tile
// holds f alone: a lane reads ITS OWN pixel's (e_l, v_l) and N_l from the planes and rewrites them in place - no lane reads another pixel's e, v or N, so the order
// between lanes and blocks does not matter - and its own vf only where the clamp bites. No atomics; every global index is y * width + x of a pixel inside the frame.
template <int R>
KZ_DN_KERNEL kz_dn_clamp_history(int width, int height, float fastHistory, float clampSigma, const float4 *__restrict__ fast, float4 *__restrict__ colour,
                                 float4 *__restrict__ histE, float *__restrict__ histN) {
    constexpr int ROWS = KZ_DN_BLOCK / KZ_DN_ROW, TW = KZ_DN_ROW + 2 * R, TH = ROWS + 2 * R, N = TW * TH;
    __shared__ float4 tile[N];
    const int x0 = (int)blockIdx.x * KZ_DN_ROW, y0 = (int)blockIdx.y * ROWS;
    const int tid = (int)(threadIdx.y * KZ_DN_ROW + threadIdx.x);
    for (int k = tid; k < N; k += KZ_DN_BLOCK) {
        const int ty = k / TW, tx = k - ty * TW, gx = x0 - R + tx, gy = y0 - R + ty;
        float4 f = make_float4(0.f, 0.f, 0.f, -1.f);
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) f = fast[(size_t)gy * (size_t)width + (size_t)gx];
        tile[k] = f;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t ip = (size_t)y * (size_t)width + (size_t)x;
    const int c = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
    if (tile[c].w < 0.f) return;                                        // not valid
    const float Nl = histN[ip];
    if (!(Nl > fastHistory)) return;
    const float4 el = colour[ip];
    float cnt = 0.f, Sr = 0.f, Sg = 0.f, Sb = 0.f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const float4 q = tile[c + dy * TW + dx];
            if (q.w < 0.f) continue;
            cnt += 1.0f; Sr += q.x; Sg += q.y; Sb += q.z;
        }
    const float mr = Sr / cnt, mg = Sg / cnt, mb = Sb / cnt;
    float Dr = 0.f, Dg = 0.f, Db = 0.f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const float4 q = tile[c + dy * TW + dx];
            if (q.w < 0.f) continue;
            const float tr = q.x - mr, tg = q.y - mg, tb = q.z - mb;
            Dr += tr * tr; Dg += tg * tg; Db += tb * tb;
        }
    const float wr = clampSigma * sqrtf(Dr / cnt), wg = clampSigma * sqrtf(Dg / cnt), wb = clampSigma * sqrtf(Db / cnt);
    const float lr = mr - wr, hr = mr + wr, lg = mg - wg, hg = mg + wg, lb = mb - wb, hb = mb + wb;
    const float cr = el.x < lr ? lr : (el.x > hr ? hr : el.x), cg = el.y < lg ? lg : (el.y > hg ? hg : el.y), cb = el.z < lb ? lb : (el.z > hb ? hb : el.z);
    if (cr != el.x || cg != el.y || cb != el.z) {
        const float4 e = make_float4(cr, cg, cb, fast[ip].w);           // (c, vf(p), Nf(p))
        colour[ip] = e; histE[ip] = e; histN[ip] = Nl < fastHistory ? Nl : fastHistory;
    }
}

int kzDnResponsiveRun(int width, int height, int border, const float4 *film, const float4 *moment, const float4 *albedo, const float4 *normal, const float4 *depth,
                      int demodulate, float samples, const KzDnTemporal &T, const KzDnMotion &M, const KzDnResponsive &R, float4 *colour, float4 *normalZ,
                      float4 *albedoP, hipStream_t stream) {
    const uint32_t nPix = (uint32_t)width * (uint32_t)height;
    const KzDnFast F = {R.inF, R.outF, R.fastHistory};
    hipLaunchKernelGGL(kz_dn_prepare_responsive, dim3((nPix + KZ_DN_BLOCK - 1) / KZ_DN_BLOCK), dim3(KZ_DN_BLOCK), 0, stream, width, height, border, film, moment, albedo, normal,
                       depth, demodulate, samples, T, M, F, colour, normalZ, albedoP);
    HIP_TRY(hipGetLastError());
    if (!T.inE || R.clampOff) return KZ_OK;                             // (without a history every N_l is 1: pass B's condition fails everywhere)
    const dim3 grid((unsigned)((width + KZ_DN_ROW - 1) / KZ_DN_ROW), (unsigned)((height + KZ_DN_BLOCK / KZ_DN_ROW - 1) / (KZ_DN_BLOCK / KZ_DN_ROW))), blk(KZ_DN_ROW, KZ_DN_BLOCK / KZ_DN_ROW);
    if (R.radius == 1) hipLaunchKernelGGL(kz_dn_clamp_history<1>, grid, blk, 0, stream, width, height, R.fastHistory, R.clampSigma, (const float4 *)R.outF, colour, T.outE, T.outN);
    else hipLaunchKernelGGL(kz_dn_clamp_history<2>, grid, blk, 0, stream, width, height, R.fastHistory, R.clampSigma, (const float4 *)R.outF, colour, T.outE, T.outN);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}
