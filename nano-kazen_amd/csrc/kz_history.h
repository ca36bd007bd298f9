// kz_history.h - the history prepare stage of kz_denoise_temporal, kz_denoise_motion and kz_denoise_responsive (include/kazen_mi355x_temporal.h, _motion.h and
// _responsive.h hold the definitions; every line of arithmetic below is one of theirs), stated once for the device: kz_dn_prepare_var's lines, then this frame's
// (e_cur, v_cur) blended with the history reprojected from the previous view, into the colour plane, and with (n, z) and the count into the history's other copy.
// dnHistory<MOTION, FAST> is the one body; the three kernels - kz_dn_prepare_temporal = <false, false> and kz_dn_prepare_motion = <true, false> in kz_denoise.hip,
// kz_dn_prepare_responsive = <true, true> in kz_responsive.hip - are its instances under the names and with the by-value arguments they have always had.
//   MOTION  the pixel's mesh id and that mesh's row: the point the history's view sees is the row's map of X, the normal the taps compare is the row's map of n(p),
//           and a pixel of an untracked mesh takes no history. A miss, a static row and a null M.ids (every pixel static) take the arithmetic without MOTION to the
//           bit: the multiply is skipped, not done with an identity.
//   FAST    one 16-byte fast-plane load per tap (the plane absent: the history's (e, v) in its place), four more sums, the fast blend and the store to F.outF -
//           (0, 0, 0, -1) at a pixel that is not valid (vf = -1: the colour plane's convention, kz_denoise.h).
// Every operation is one fp32 IEEE operation in the order written (the units that include this file are build.sh's IEEE_UNITS), so the results are
// tests/cpu_ref/kz_temporal_ref.cpp's, kz_motion_ref.cpp's and kz_responsive_ref.cpp's to the bit.
#pragma once
#include "../../include/kazen_mi355x_motion.h"
#include "kz_denoise.h"

// By value to kz_dn_prepare_responsive, beside KzDnTemporal and KzDnMotion: the fast plane's two copies (inF null: absent) and (float)fastHistory
struct KzDnFast { const float4 *inF; float4 *outF; float fastHistory; };

// One lane per pixel, a wave along a row: for the small view changes this is for, the 2 x 2 taps of neighbouring lanes fall on neighbouring records, so each of a
// wave's tap loads (two or three 16-byte planes and the count, four taps) touches little more than the 1 KB / 256 B its own pixels hold; a wave's lanes mostly show
// one mesh, so the row's 96 bytes are a plain load that the lanes share. A pixel's sums are its own lane's, in the stated order; the copy that is read is not
// written. No atomics, no LDS, no scratch and no index at or beyond width x height (the films': below their texels); an id at or beyond M.nRows - the host has
// refused it - reads no row: a miss. `M`: MOTION alone, `F`: FAST alone.
template <bool MOTION, bool FAST>
KZ_DN_FN void dnHistory(int width, int height, int border, const float4 *__restrict__ film, const float4 *__restrict__ moment, const float4 *__restrict__ albedo,
                        const float4 *__restrict__ normal, const float4 *__restrict__ depth, int demodulate, float samples, const KzDnTemporal &T, const KzDnMotion &M,
                        const KzDnFast &F, float4 *__restrict__ colour, float4 *__restrict__ normalZ, float4 *__restrict__ albedoP) {
    const uint32_t i = blockIdx.x * KZ_DN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const size_t t = (size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border);      // < (height + 2b)(width + 2b): the films' texels
    const float4 c = dnValue(film, t), a = dnValue(albedo, t), n = dnValue(normal, t), z = dnValue(depth, t), s = dnValue(moment, t);
    float4 e = dnCurrent<true>(c, a, s, demodulate, samples);          // (e_cur, v_cur): kz_dn_prepare_var's
    normalZ[i] = make_float4(n.x, n.y, n.z, z.x);
    albedoP[i] = make_float4(a.x, a.y, a.z, 0.f);
    if (c.w == 0.f) {                                                   // not valid: no part in the filter (v = -1), an empty record; FAST: no part in pass B's windows (vf = -1)
        e.w = -1.f;
        colour[i] = e;
        T.outE[i] = make_float4(0.f, 0.f, 0.f, 0.f); T.outG[i] = make_float4(0.f, 0.f, 0.f, 0.f); T.outN[i] = 0.f;
        if (FAST) F.outF[i] = make_float4(0.f, 0.f, 0.f, -1.f);
        return;
    }
    float count = 1.0f;
    float4 f = e;                                                       // FAST, without history: f = e_cur, vf = v_cur
    // MOTION, the pixel's row: flags 0 = moved (d, n are read), STATIC also for a miss and without an id plane, UNTRACKED = no history
    uint32_t flags = KZ_MOTION_STATIC;
    const KzMotionRow *row = nullptr;
    if (MOTION && T.inE && z.x > 0.f && M.ids) {
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
        if (MOTION && !(flags & KZ_MOTION_STATIC)) {
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
                        const float4 fh = FAST && F.inF ? F.inF[it] : eh;                // FAST, the fast plane absent: the history's (e, v) in its place
                        const float b = (k ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        if (!(rowIn && colIn) || nh == 0.f || fabsf(gh.w - zp) > ztol || dnSq(gh.x - nx, gh.y - ny, gh.z - nz) > T.normalTol2) continue;
                        Wb += b; Er += b * eh.x; Eg += b * eh.y; Eb += b * eh.z; V += b * eh.w; Mn += b * nh;
                        if (FAST) { Fr += b * fh.x; Fg += b * fh.y; Fb += b * fh.z; VF += b * fh.w; }
                    }
                }
                if (Wb > 1e-3f) {
                    const float Nh = Mn / Wb, Nn1 = Nh + 1.0f, Nn = Nn1 < T.maxHistory ? Nn1 : T.maxHistory;
                    const float al = 1.0f / Nn, om = 1.0f - al;
                    if (FAST) {
                        const float Nf = Nn < F.fastHistory ? Nn : F.fastHistory;
                        const float af = 1.0f / Nf, of = 1.0f - af;
                        f.x = of * (Fr / Wb) + af * e.x; f.y = of * (Fg / Wb) + af * e.y; f.z = of * (Fb / Wb) + af * e.z;
                        f.w = (of * of) * (VF / Wb) + (af * af) * e.w;
                    }
                    e.x = om * (Er / Wb) + al * e.x; e.y = om * (Eg / Wb) + al * e.y; e.z = om * (Eb / Wb) + al * e.z;
                    e.w = (om * om) * (V / Wb) + (al * al) * e.w;
                    count = Nn;
                }
            }
        }
    }
    colour[i] = e;
    T.outE[i] = e; T.outG[i] = make_float4(n.x, n.y, n.z, z.x); T.outN[i] = count;
    if (FAST) F.outF[i] = f;
}
