// kz_responsive.hip - the device side of include/kazen_mi355x_responsive.h (which holds the definition; every line of arithmetic below is one of its lines): the
// fast history beside the long one, and the long history clamped to the fast one's local statistics.
//   kz_dn_prepare_responsive  pass A, in kz_dn_prepare_motion's place: that kernel restated - not shared: the kernels of kz_denoise.hip keep their instructions and
//                             their by-value argument structs - plus one 16-byte fast-plane load per tap, the fast blend and one 16-byte store
//   kz_dn_clamp_history       pass B: a (2 r + 1)^2 stencil over the fast plane through an LDS tile; a pixel rewrites its own (e, v) in the colour plane and in the
//                             history's out copy, and its own N
// On the device the fast plane marks a pixel that is not valid with vf = -1 (the convention of the colour plane, kz_denoise.h: a variance is never negative), so pass
// B needs no plane but the fast one to know which texels of its window count; what leaves the device (kz_denoise.hip: dnFastDownload) has four zeros there, as the
// header says. Compiled like kz_denoise.hip (build.sh IEEE_UNITS): no flush to zero, no contraction - the results are tests/cpu_ref/kz_responsive_ref.cpp's to the bit.
#include <hip/hip_runtime.h>

#include "kz_state.h"
#include "kz_responsive.h"

// By value to kz_dn_prepare_responsive, beside KzDnTemporal and KzDnMotion: the fast plane's two copies (inF null: absent) and (float)fastHistory
struct KzDnFast { const float4 *inF; float4 *outF; float fastHistory; };

#define KZ_DN_KERNEL __global__ __launch_bounds__(KZ_DN_BLOCK) void

// One lane per pixel, a wave along a row; no atomics, no LDS, every index below width x height (the films': below their texels). M.ids null: every pixel static.
KZ_DN_KERNEL kz_dn_prepare_responsive(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                                      const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples, const KzDnTemporal T, const KzDnMotion M,
                                      const KzDnFast F, float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    const uint32_t i = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const size_t t = (size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border);      // < (height + 2b)(width + 2b): the films' texels
    const float4 c = dnValue(film, t), a = dnValue(albedo, t), n = dnValue(normal, t), z = dnValue(depth, t), s = dnValue(moment, t);
    // (e_cur, v_cur): dnPrepare<true>'s lines
    const float vr = dnMax(s.x - c.x * c.x, 0.f) / samples, vg = dnMax(s.y - c.y * c.y, 0.f) / samples, vb = dnMax(s.z - c.z * c.z, 0.f) / samples;
    float4 e = make_float4(c.x, c.y, c.z, (vr + vg) + vb);
    if (demodulate) {
        const float ar = dnMax(a.x, 1e-3f); e.x = c.x / ar;
        const float ag = dnMax(a.y, 1e-3f); e.y = c.y / ag;
        const float ab = dnMax(a.z, 1e-3f); e.z = c.z / ab;
        e.w = (vr / (ar * ar) + vg / (ag * ag)) + vb / (ab * ab);
    }
    normalZ[i] = make_float4(n.x, n.y, n.z, z.x);
    albedoP[i] = make_float4(a.x, a.y, a.z, 0.f);
    if (c.w == 0.f) {                                                   // not valid: no part in the filter (v = -1), an empty record, no part in pass B's windows (vf = -1)
        e.w = -1.f;
        colour[i] = e;
        T.outE[i] = make_float4(0.f, 0.f, 0.f, 0.f); T.outG[i] = make_float4(0.f, 0.f, 0.f, 0.f); T.outN[i] = 0.f;
        F.outF[i] = make_float4(0.f, 0.f, 0.f, -1.f);
        return;
    }
    float count = 1.0f;
    float4 f = e;                                                       // without history: f = e_cur, vf = v_cur
    // the pixel's row: flags 0 = moved (d, n are read), STATIC also for a miss and without an id plane, UNTRACKED = no history
    uint32_t flags = KZ_MOTION_STATIC;
    const KzMotionRow *row = nullptr;
    if (T.inE && z.x > 0.f && M.ids) {
        const uint32_t m = M.ids[i];
        if (m < M.nRows) { row = M.rows + m; flags = row->flags; }
    }
    if (T.inE && z.x > 0.f && !(flags & KZ_MOTION_UNTRACKED)) {
        const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
        const float dx = (T.a[0] + fx * T.u[0]) + fy * T.v[0], dy = (T.a[1] + fx * T.u[1]) + fy * T.v[1], dz = (T.a[2] + fx * T.u[2]) + fy * T.v[2];
        const float len = sqrtf(dnSq(dx, dy, dz));
        const float r = z.x / len;
        float Xx = T.o[0] + dx * r, Xy = T.o[1] + dy * r, Xz = T.o[2] + dz * r;
        float nx = n.x, ny = n.y, nz = n.z;                             // the normal the taps compare: n(p), or n' of a moved mesh
        if (!(flags & KZ_MOTION_STATIC)) {
            const float *d = row->d, *w = row->n;
            const float px = ((d[0] * Xx + d[1] * Xy) + d[2] * Xz) + d[3], py = ((d[4] * Xx + d[5] * Xy) + d[6] * Xz) + d[7], pz = ((d[8] * Xx + d[9] * Xy) + d[10] * Xz) + d[11];
            Xx = px; Xy = py; Xz = pz;
            nx = (w[0] * n.x + w[1] * n.y) + w[2] * n.z; ny = (w[3] * n.x + w[4] * n.y) + w[5] * n.z; nz = (w[6] * n.x + w[7] * n.y) + w[8] * n.z;
        }
        const float qx = Xx - T.po[0], qy = Xy - T.po[1], qz = Xz - T.po[2];
        const float P0 = (T.pinv[0] * qx + T.pinv[1] * qy) + T.pinv[2] * qz, P1 = (T.pinv[3] * qx + T.pinv[4] * qy) + T.pinv[5] * qz,
                    P2 = (T.pinv[6] * qx + T.pinv[7] * qy) + T.pinv[8] * qz;
        if (P2 > 0.f) {
            const float sx = P0 / P2 - 0.5f, sy = P1 / P2 - 0.5f;
            if (sx >= -1.f && sx < (float)width && sy >= -1.f && sy < (float)height) {      // (so x0, y0 are in -1 .. width - 1, -1 .. height - 1: the int conversions are exact)
                const float fx0 = floorf(sx), fy0 = floorf(sy), tx = sx - fx0, ty = sy - fy0;
                const int x0 = (int)fx0, y0 = (int)fy0;
                const float zp = sqrtf(dnSq(qx, qy, qz)), ztol = T.depthTol * dnMax(zp, 1e-20f);
                float Wb = 0.f, Er = 0.f, Eg = 0.f, Eb = 0.f, V = 0.f, Mn = 0.f, Fr = 0.f, Fg = 0.f, Fb = 0.f, VF = 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ty_ = y0 + j;
                    const bool rowIn = ty_ >= 0 && ty_ < height;
                    const size_t rowAt = (size_t)(rowIn ? ty_ : y) * (size_t)width;      // (a tap outside the frame loads the pixel's own row / column and is skipped)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int tx_ = x0 + k;
                        const bool colIn = tx_ >= 0 && tx_ < width;
                        const size_t it = rowAt + (size_t)(colIn ? tx_ : x);             // < width * height
                        const float nh = T.inN[it];
                        const float4 gh = T.inG[it], eh = T.inE[it];
                        const float4 fh = F.inF ? F.inF[it] : eh;                        // the fast plane absent: the history's (e, v) in its place
                        const float b = (k ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        if (!(rowIn && colIn) || nh == 0.f || fabsf(gh.w - zp) > ztol || dnSq(gh.x - nx, gh.y - ny, gh.z - nz) > T.normalTol2) continue;
                        Wb += b; Er += b * eh.x; Eg += b * eh.y; Eb += b * eh.z; V += b * eh.w; Mn += b * nh;
                        Fr += b * fh.x; Fg += b * fh.y; Fb += b * fh.z; VF += b * fh.w;
                    }
                }
                if (Wb > 1e-3f) {
                    const float Nh = Mn / Wb, Nn1 = Nh + 1.0f, Nn = Nn1 < T.maxHistory ? Nn1 : T.maxHistory;
                    const float al = 1.0f / Nn, om = 1.0f - al;
                    const float Nf = Nn < F.fastHistory ? Nn : F.fastHistory;
                    const float af = 1.0f / Nf, of = 1.0f - af;
                    f.x = of * (Fr / Wb) + af * e.x; f.y = of * (Fg / Wb) + af * e.y; f.z = of * (Fb / Wb) + af * e.z;
                    f.w = (of * of) * (VF / Wb) + (af * af) * e.w;
                    e.x = om * (Er / Wb) + al * e.x; e.y = om * (Eg / Wb) + al * e.y; e.z = om * (Eb / Wb) + al * e.z;
                    e.w = (om * om) * (V / Wb) + (al * al) * e.w;
                    count = Nn;
                }
            }
        }
    }
    colour[i] = e;
    T.outE[i] = e; T.outG[i] = make_float4(n.x, n.y, n.z, z.x); T.outN[i] = count;
    F.outF[i] = f;
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
