// kz_responsive_ref.cpp - TEST-ONLY CPU reference of include/kazen_mi355x_responsive.h. Never linked into the product; tests/test_responsive_cpu.py compiles it with
// the oracle's flags (-O2 -ffp-contract=off, no fast math). It includes kz_motion_ref.cpp unchanged - for kzm_denoise, which the identity tests compare against, and
// through it the temporal reference's a-trous restatement tFilter and the project's own oracle - and restates from the headers' definitions in plain C++: pass A (the
// motion stage with the fast history's sums and blend beside it), pass B (the window's mean and deviation, the clamp, the fall-back to the fast count and variance),
// the new history and the fast plane. Nothing of nano-kazen_amd/csrc is read.
#include "kz_motion_ref.cpp"
#include "kazen_mi355x_responsive.h"

// history (in and out): width x height x 12 floats as kzt_denoise takes it; fast (in and out): width x height x 4 floats, (f.rgb, vf); fastIn null with a history:
// the fast plane is absent. Returns 0, 1 where the library refuses the options, 2 where it refuses the ids or the rows, 3 where it refuses KzResponsiveOpts.
extern "C" int kzr_denoise(int width, int height, int border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                           const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current,
                           const KzTemporalView *previous, const float *historyIn, const uint32_t *ids, const KzMotionRow *rows, uint32_t nRows, float *out,
                           float *historyOut, float *outVariance, const KzResponsiveOpts *ropts, const float *fastIn, float *fastOut) {
    KzDenoiseOpts o; KzVarianceOpts vo; KzTemporalOpts to; KzResponsiveOpts ro;
    std::memset(&o, 0, sizeof o); std::memset(&vo, 0, sizeof vo); std::memset(&to, 0, sizeof to); std::memset(&ro, 0, sizeof ro);
    if (opts) o = *opts;
    if (vopts) vo = *vopts;
    if (topts) to = *topts;
    if (ropts) ro = *ropts;
    if (!depth || !current || (historyIn && !previous)) return 1;
    if (!ids || (nRows && !rows)) return 2;
    for (uint32_t m = 0; m < nRows; ++m) if (rows[m].flags > 2u || rows[m].reserved[0] || rows[m].reserved[1]) return 2;
    for (size_t j = 0; j < (size_t)width * height; ++j) if (ids[j] >= nRows && ids[j] != KZ_MOTION_MISS) return 2;
    if (ro.fastHistory > 65535u || !std::isfinite(ro.clampSigma) || ro.clampSigma < 0.0f || ro.radius > 2u || (ro.flags & ~KZ_RESPONSIVE_CLAMP_OFF) || ro.reserved[0] ||
        ro.reserved[1] || ro.reserved[2] || ro.reserved[3]) return 3;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | KZ_AOV_DEPTH;
    if (o.iterations > 8 || (o.flags & ~3u) || o.reserved || (o.guides & ~avail)) return 1;
    if (!std::isfinite(vo.sigmaVariance) || vo.sigmaVariance < 0.0f || vo.flags || vo.reserved || !vo.samples) return 1;
    if (!std::isfinite(to.depthTolerance) || to.depthTolerance < 0.0f || !std::isfinite(to.normalTolerance) || to.normalTolerance < 0.0f || to.maxHistory > 65535u || to.flags ||
        to.reserved[0] || to.reserved[1] || to.reserved[2] || to.reserved[3]) return 1;
    float sigma[4] = {o.sigmaColor, o.sigmaNormal, o.sigmaDepth, o.sigmaAlbedo};
    const float dflt[4] = {2.0f, 0.3f, 0.1f, 0.1f};
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return 1;
        if (sigma[k] == 0.0f) sigma[k] = dflt[k];
    }
    const float sigmaV = vo.sigmaVariance == 0.0f ? 3.0f : vo.sigmaVariance;
    const float sv2 = sigmaV * sigmaV;
    const float ns = (float)vo.samples;
    const int iterations = o.iterations ? (int)o.iterations : 5;
    const uint32_t guides = o.guides ? o.guides : avail;
    if (!(guides & KZ_AOV_DEPTH)) return 1;
    const bool weightsUseGuides = !(o.flags & KZ_DENOISE_NO_GUIDES);
    const bool demodulate = (guides & KZ_AOV_ALBEDO) && !(o.flags & KZ_DENOISE_NO_DEMODULATE);
    if (!(guides & KZ_AOV_ALBEDO)) albedo = nullptr;
    if (!(guides & KZ_AOV_NORMAL)) normal = nullptr;
    const float depthTol = to.depthTolerance == 0.0f ? 0.05f : to.depthTolerance;
    const float normalTol = to.normalTolerance == 0.0f ? 0.5f : to.normalTolerance;
    const float normalTol2 = normalTol * normalTol;
    const float maxHistory = (float)(to.maxHistory ? to.maxHistory : 32u);
    const bool stored = historyIn && to.maxHistory != 1u;
    const float fastHistory = (float)(ro.fastHistory ? ro.fastHistory : 2u);
    const float clampSigma = ro.clampSigma == 0.0f ? 2.0f : ro.clampSigma;
    const int radius = ro.radius ? (int)ro.radius : 1;
    const bool clampOff = (ro.flags & KZ_RESPONSIVE_CLAMP_OFF) != 0;

    const int cols = width + 2 * border;
    std::vector<TPx> px((size_t)width * height);
    std::vector<float> fast((size_t)width * height * 4, 0.0f);          // (f.rgb, vf) per pixel
    // ---- pass A
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            TPx &p = px[(size_t)y * width + x];
            float *fp = &fast[((size_t)y * width + x) * 4];
            const size_t t = (size_t)(y + border) * cols + (x + border);
            float c[3], w, s[3], d[3], unused, var[3];
            vtexel(film, t, c, &w);
            p.valid = w != 0.0f;
            vtexel(moment, t, s, &unused);
            vtexel(albedo, t, p.a, &unused);
            vtexel(normal, t, p.n, &unused);
            vtexel(depth, t, d, &unused);
            p.z = d[0];
            for (int k = 0; k < 3; ++k) {
                p.am[k] = vpick(p.a[k], 1e-3f);
                p.e[k] = demodulate ? c[k] / p.am[k] : c[k];
                const float cc = c[k] * c[k];
                var[k] = vpick(s[k] - cc, 0.0f) / ns;
                if (demodulate) { const float aa = p.am[k] * p.am[k]; var[k] = var[k] / aa; }
            }
            p.v = (var[0] + var[1]) + var[2];
            p.count = p.valid ? 1.0f : 0.0f;
            if (!p.valid) continue;                                     // (four zeros in the fast plane)
            fp[0] = p.e[0]; fp[1] = p.e[1]; fp[2] = p.e[2]; fp[3] = p.v;      // without history: f = e_cur, vf = v_cur
            if (!stored || !(p.z > 0.0f)) continue;
            // ---- the pixel's row: none for a miss
            const uint32_t id = ids[(size_t)y * width + x];
            const KzMotionRow *row = id == KZ_MOTION_MISS ? nullptr : &rows[id];
            if (row && (row->flags & KZ_MOTION_UNTRACKED)) continue;
            const bool moved = row && !(row->flags & KZ_MOTION_STATIC);
            // ---- the reprojection
            const KzTemporalView &C = *current, &H = *previous;
            const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
            float dir[3], X[3], q[3], P[3], nt[3];
            for (int k = 0; k < 3; ++k) { const float au = C.a[k] + fx * C.u[k]; dir[k] = au + fy * C.v[k]; }
            float l2 = dir[0] * dir[0]; l2 = l2 + dir[1] * dir[1]; l2 = l2 + dir[2] * dir[2];
            const float len = std::sqrt(l2);
            const float r = p.z / len;
            for (int k = 0; k < 3; ++k) { X[k] = C.o[k] + dir[k] * r; nt[k] = p.n[k]; }
            if (moved) {
                float Xp[3];
                for (int k = 0; k < 3; ++k) {
                    float acc = row->d[4 * k] * X[0]; acc = acc + row->d[4 * k + 1] * X[1]; acc = acc + row->d[4 * k + 2] * X[2]; acc = acc + row->d[4 * k + 3];
                    Xp[k] = acc;
                    float nn = row->n[3 * k] * p.n[0]; nn = nn + row->n[3 * k + 1] * p.n[1]; nn = nn + row->n[3 * k + 2] * p.n[2];
                    nt[k] = nn;
                }
                for (int k = 0; k < 3; ++k) X[k] = Xp[k];
            }
            for (int k = 0; k < 3; ++k) q[k] = X[k] - H.o[k];
            for (int i = 0; i < 3; ++i) { float acc = H.inv[3 * i] * q[0]; acc = acc + H.inv[3 * i + 1] * q[1]; acc = acc + H.inv[3 * i + 2] * q[2]; P[i] = acc; }
            if (!(P[2] > 0.0f)) continue;
            const float sx = P[0] / P[2] - 0.5f, sy = P[1] / P[2] - 0.5f;
            if (!(sx >= -1.0f && sx < (float)width && sy >= -1.0f && sy < (float)height)) continue;
            const float fx0 = std::floor(sx), fy0 = std::floor(sy);
            const float tx = sx - fx0, ty = sy - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            float z2 = q[0] * q[0]; z2 = z2 + q[1] * q[1]; z2 = z2 + q[2] * q[2];
            const float zp = std::sqrt(z2);
            const float ztol = depthTol * vpick(zp, 1e-20f);
            // ---- the four taps: the long history's sums, and the fast one's beside them
            float Wb = 0.0f, E[3] = {0.0f, 0.0f, 0.0f}, V = 0.0f, M = 0.0f, F[3] = {0.0f, 0.0f, 0.0f}, VF = 0.0f;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int hx = x0 + i, hy = y0 + j;
                    const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    if (hx < 0 || hy < 0 || hx >= width || hy >= height) continue;
                    const float *rec = historyIn + 12 * ((size_t)hy * width + hx);
                    if (rec[8] == 0.0f) continue;
                    if (std::fabs(rec[7] - zp) > ztol) continue;
                    if (vsq3(rec + 4, nt) > normalTol2) continue;
                    const float *frec = fastIn ? fastIn + 4 * ((size_t)hy * width + hx) : rec;      // absent: (e_h, v_h) in the fast record's place
                    Wb = Wb + b;
                    for (int k = 0; k < 3; ++k) E[k] = E[k] + b * rec[k];
                    V = V + b * rec[3];
                    M = M + b * rec[8];
                    for (int k = 0; k < 3; ++k) F[k] = F[k] + b * frec[k];
                    VF = VF + b * frec[3];
                }
            if (!(Wb > 1e-3f)) continue;
            // ---- the two blends
            const float Nh = M / Wb, Nn1 = Nh + 1.0f;
            const float Nn = Nn1 < maxHistory ? Nn1 : maxHistory;
            const float al = 1.0f / Nn, om = 1.0f - al;
            const float Nf = Nn < fastHistory ? Nn : fastHistory;
            const float af = 1.0f / Nf, of = 1.0f - af;
            for (int k = 0; k < 3; ++k) { const float fh = F[k] / Wb; const float l = of * fh; fp[k] = l + af * p.e[k]; }
            const float vfh = VF / Wb;
            const float lf = (of * of) * vfh;
            fp[3] = lf + (af * af) * p.v;
            for (int k = 0; k < 3; ++k) { const float eh = E[k] / Wb; const float l = om * eh; p.e[k] = l + al * p.e[k]; }
            const float vh = V / Wb;
            const float lv = (om * om) * vh;
            p.v = lv + (al * al) * p.v;
            p.count = Nn;
        }
    // ---- pass B: a pixel reads the fast plane of its window and its own (e_l, v_l, N_l), and writes its own (e, v, N)
    if (!clampOff)
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                TPx &p = px[(size_t)y * width + x];
                if (!p.valid || !(p.count > fastHistory)) continue;
                float cnt = 0.0f, S[3] = {0.0f, 0.0f, 0.0f}, D[3] = {0.0f, 0.0f, 0.0f}, m[3], c[3];
                for (int dy = -radius; dy <= radius; ++dy)
                    for (int dx = -radius; dx <= radius; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height || !px[(size_t)qy * width + qx].valid) continue;
                        const float *fq = &fast[((size_t)qy * width + qx) * 4];
                        cnt = cnt + 1.0f;
                        for (int k = 0; k < 3; ++k) S[k] = S[k] + fq[k];
                    }
                for (int k = 0; k < 3; ++k) m[k] = S[k] / cnt;
                for (int dy = -radius; dy <= radius; ++dy)
                    for (int dx = -radius; dx <= radius; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height || !px[(size_t)qy * width + qx].valid) continue;
                        const float *fq = &fast[((size_t)qy * width + qx) * 4];
                        for (int k = 0; k < 3; ++k) { const float t = fq[k] - m[k]; D[k] = D[k] + t * t; }
                    }
                bool clamped = false;
                for (int k = 0; k < 3; ++k) {
                    const float sd = std::sqrt(D[k] / cnt);
                    const float wk = clampSigma * sd;
                    const float lo = m[k] - wk, hi = m[k] + wk;
                    c[k] = p.e[k] < lo ? lo : (p.e[k] > hi ? hi : p.e[k]);
                    if (c[k] != p.e[k]) clamped = true;
                }
                if (!clamped) continue;
                for (int k = 0; k < 3; ++k) p.e[k] = c[k];
                p.v = fast[((size_t)y * width + x) * 4 + 3];
                p.count = p.count < fastHistory ? p.count : fastHistory;
            }
    if (historyOut)
        for (size_t j = 0; j < px.size(); ++j) {
            const TPx &p = px[j];
            float *rec = historyOut + 12 * j;
            std::memset(rec, 0, 12 * sizeof(float));
            if (!p.valid) continue;
            rec[0] = p.e[0]; rec[1] = p.e[1]; rec[2] = p.e[2]; rec[3] = p.v;
            rec[4] = p.n[0]; rec[5] = p.n[1]; rec[6] = p.n[2]; rec[7] = p.z;
            rec[8] = p.count;
        }
    if (fastOut) std::memcpy(fastOut, fast.data(), fast.size() * sizeof(float));
    tFilter(px, width, height, border, iterations, sigma, sv2, weightsUseGuides, demodulate, out, outVariance);
    return 0;
}
