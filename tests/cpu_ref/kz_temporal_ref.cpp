// kz_temporal_ref.cpp - TEST-ONLY CPU reference of include/kazen_mi355x_temporal.h. Never linked into the product; tests/test_temporal_cpu.py compiles it with the
// oracle's flags (-O2 -ffp-contract=off, no fast math). It includes kz_variance_ref.cpp unchanged - for the oracle's exp, the texel helpers and the canonical films
// the quality test renders - and restates, from the two headers' definitions in plain C++: this frame's (e_cur, v_cur), the reprojection, the 2 x 2 history gather,
// the blend, the new history, and once more the variance-guided a-trous iterations that follow (kzv_denoise starts from the films and cannot be handed a blended
// e_0, v_0). Nothing of nano-kazen_amd/csrc is read.
#include "kz_variance_ref.cpp"
#include "kazen_mi355x_temporal.h"

namespace {

struct TPx { float e[3]; bool valid; float v, n[3], z, a[3], am[3], count; };

// The iterations, the remodulation and the result of kazen_mi355x_variance.h from (e_0, v_0) per pixel
void tFilter(std::vector<TPx> &px, int width, int height, int border, int iterations, const float sigma[4], float sv2, bool weightsUseGuides, bool demodulate,
             float *out, float *outVariance) {
    const float h[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    const float k3[3] = {1.0f / 4, 1.0f / 2, 1.0f / 4};
    const float kn = 1.0f / (sigma[1] * sigma[1]), kz = 1.0f / (sigma[2] * sigma[2]), ka = 1.0f / (sigma[3] * sigma[3]);
    std::vector<float> next((size_t)width * height * 4);
    for (int i = 0; i < iterations; ++i) {
        const int st = 1 << i;
        const float sc = sigma[0] * std::ldexp(1.0f, -i);
        const float kc = 1.0f / (sc * sc);
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                const TPx &p = px[(size_t)y * width + x];
                float *r = &next[((size_t)y * width + x) * 4];
                r[0] = p.e[0]; r[1] = p.e[1]; r[2] = p.e[2]; r[3] = p.v;
                if (!p.valid) continue;
                float gn = 0.0f, gd = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const TPx &q = px[(size_t)qy * width + qx];
                        if (!q.valid) continue;
                        const float kk = k3[dy + 1] * k3[dx + 1];
                        gn = gn + kk * q.v;
                        gd = gd + kk;
                    }
                const float g = gn / gd;
                const float kv = 1.0f / (sv2 * g + 1e-12f);
                const float kcv = vpick(kc, kv);
                float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, nv = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int qx = x + st * dx, qy = y + st * dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const TPx &q = px[(size_t)qy * width + qx];
                        if (!q.valid) continue;
                        const float dc = vsq3(q.e, p.e);
                        float arg = dc * kcv;
                        if (weightsUseGuides) {
                            const float dn = vsq3(q.n, p.n), da = vsq3(q.a, p.a);
                            const float m = vpick(vpick(p.z, q.z), 1e-20f);
                            const float t = (q.z - p.z) / m;
                            const float dz = t * t;
                            arg = arg + dn * kn;
                            arg = arg + dz * kz;
                            arg = arg + da * ka;
                        }
                        const float wgt = (h[dy + 2] * h[dx + 2]) * kzoExp(-arg);
                        for (int k = 0; k < 3; ++k) num[k] = num[k] + wgt * q.e[k];
                        den = den + wgt;
                        const float ww = wgt * wgt;
                        nv = nv + ww * q.v;
                    }
                for (int k = 0; k < 3; ++k) r[k] = num[k] / den;
                const float dd = den * den;
                r[3] = nv / dd;
            }
        for (size_t j = 0; j < px.size(); ++j) { for (int k = 0; k < 3; ++k) px[j].e[k] = next[4 * j + k]; px[j].v = next[4 * j + 3]; }
    }
    const int cols = width + 2 * border;
    std::memset(out, 0, sizeof(float) * 4 * (size_t)cols * (height + 2 * border));
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const TPx &p = px[(size_t)y * width + x];
            if (outVariance) outVariance[(size_t)y * width + x] = p.valid ? p.v : 0.0f;
            if (!p.valid) continue;
            float *t = out + 4 * ((size_t)(y + border) * cols + (x + border));
            for (int k = 0; k < 3; ++k) t[k] = demodulate ? p.e[k] * p.am[k] : p.e[k];
            t[3] = 1.0f;
        }
}

}  // namespace

// history (in and out): width x height x 12 floats, per pixel (e.rgb, v), (n.xyz, z), (N, 0, 0, 0). Returns 0, or 1 where the library refuses the options.
extern "C" int kzt_denoise(int width, int height, int border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                           const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current,
                           const KzTemporalView *previous, const float *historyIn, float *out, float *historyOut, float *outVariance) {
    KzDenoiseOpts o; KzVarianceOpts vo; KzTemporalOpts to;
    std::memset(&o, 0, sizeof o); std::memset(&vo, 0, sizeof vo); std::memset(&to, 0, sizeof to);
    if (opts) o = *opts;
    if (vopts) vo = *vopts;
    if (topts) to = *topts;
    if (!depth || !current || (historyIn && !previous)) return 1;
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

    const int cols = width + 2 * border;
    std::vector<TPx> px((size_t)width * height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            TPx &p = px[(size_t)y * width + x];
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
            if (!p.valid || !stored || !(p.z > 0.0f)) continue;
            // ---- the reprojection
            const KzTemporalView &C = *current, &H = *previous;
            const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
            float dir[3], q[3], P[3];
            for (int k = 0; k < 3; ++k) { const float au = C.a[k] + fx * C.u[k]; dir[k] = au + fy * C.v[k]; }
            float l2 = dir[0] * dir[0]; l2 = l2 + dir[1] * dir[1]; l2 = l2 + dir[2] * dir[2];
            const float len = std::sqrt(l2);
            const float r = p.z / len;
            for (int k = 0; k < 3; ++k) { const float X = C.o[k] + dir[k] * r; q[k] = X - H.o[k]; }
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
            // ---- the four taps
            float Wb = 0.0f, E[3] = {0.0f, 0.0f, 0.0f}, V = 0.0f, M = 0.0f;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int hx = x0 + i, hy = y0 + j;
                    const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    if (hx < 0 || hy < 0 || hx >= width || hy >= height) continue;
                    const float *rec = historyIn + 12 * ((size_t)hy * width + hx);
                    if (rec[8] == 0.0f) continue;
                    if (std::fabs(rec[7] - zp) > ztol) continue;
                    if (vsq3(rec + 4, p.n) > normalTol2) continue;
                    Wb = Wb + b;
                    for (int k = 0; k < 3; ++k) E[k] = E[k] + b * rec[k];
                    V = V + b * rec[3];
                    M = M + b * rec[8];
                }
            if (!(Wb > 1e-3f)) continue;
            // ---- the blend
            const float Nh = M / Wb, Nn1 = Nh + 1.0f;
            const float Nn = Nn1 < maxHistory ? Nn1 : maxHistory;
            const float al = 1.0f / Nn, om = 1.0f - al;
            for (int k = 0; k < 3; ++k) { const float eh = E[k] / Wb; const float l = om * eh; p.e[k] = l + al * p.e[k]; }
            const float vh = V / Wb;
            const float lv = (om * om) * vh;
            p.v = lv + (al * al) * p.v;
            p.count = Nn;
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
    tFilter(px, width, height, border, iterations, sigma, sv2, weightsUseGuides, demodulate, out, outVariance);
    return 0;
}
