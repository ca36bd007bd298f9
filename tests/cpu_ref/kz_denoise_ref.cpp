// kz_denoise_ref.cpp - test-only CPU restatement of the a-trous denoiser of include/kazen_mi355x_denoise.h, written from that header's definition and not from
// the device code: four films and options in, a film out. Compiled by tests/test_denoise_cpu.py with the oracle's flags (-O2 -ffp-contract=off, no fast math),
// so every line below is one IEEE fp32 operation; exp is the oracle's own statement of it (oracle/kz_oracle_math.h). The GPU tests compare bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "kazen_mi355x_denoise.h"
#include "../../oracle/kz_oracle_math.h"

namespace {

struct Px { float e[3]; bool valid; float n[3], z, a[3], am[3]; };

inline float pick(float a, float b) { return a > b ? a : b; }                 // the header's max
inline float sq3(const float *u, const float *v) {                            // |u - v|^2 = (x x + y y) + z z
    const float x = u[0] - v[0], y = u[1] - v[1], z = u[2] - v[2];
    float s = x * x;
    s = s + y * y;
    s = s + z * z;
    return s;
}
// the value of texel t of a film (null: an absent guide, all zeros) and its weight
inline void texel(const float *film, size_t t, float v[3], float *w) {
    v[0] = v[1] = v[2] = 0.0f; *w = 0.0f;
    if (!film) return;
    const float *p = film + 4 * t;
    *w = p[3];
    if (p[3] != 0.0f) for (int k = 0; k < 3; ++k) v[k] = p[k] / p[3];
}

}  // namespace

extern "C" int kzd_denoise(int width, int height, int border, const float *film, const float *albedo, const float *normal, const float *depth,
                           const KzDenoiseOpts *opts, float *out) {
    KzDenoiseOpts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | (depth ? KZ_AOV_DEPTH : 0u);
    if (o.iterations > 8 || (o.flags & ~3u) || o.reserved || (o.guides & ~avail)) return 1;
    float sigma[4] = {o.sigmaColor, o.sigmaNormal, o.sigmaDepth, o.sigmaAlbedo};
    const float dflt[4] = {1.0f, 0.3f, 0.1f, 0.1f};
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return 1;
        if (sigma[k] == 0.0f) sigma[k] = dflt[k];
    }
    const int iterations = o.iterations ? (int)o.iterations : 5;
    const uint32_t guides = o.guides ? o.guides : avail;
    const bool weightsUseGuides = guides != 0 && !(o.flags & KZ_DENOISE_NO_GUIDES);
    const bool demodulate = (guides & KZ_AOV_ALBEDO) && !(o.flags & KZ_DENOISE_NO_DEMODULATE);
    if (!(guides & KZ_AOV_ALBEDO)) albedo = nullptr;
    if (!(guides & KZ_AOV_NORMAL)) normal = nullptr;
    if (!(guides & KZ_AOV_DEPTH)) depth = nullptr;

    const int cols = width + 2 * border;
    std::vector<Px> px((size_t)width * height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            Px &p = px[(size_t)y * width + x];
            const size_t t = (size_t)(y + border) * cols + (x + border);
            float c[3], w, d[3], unused;
            texel(film, t, c, &w);
            p.valid = w != 0.0f;
            texel(albedo, t, p.a, &unused);
            texel(normal, t, p.n, &unused);
            texel(depth, t, d, &unused);
            p.z = d[0];
            for (int k = 0; k < 3; ++k) {
                p.am[k] = pick(p.a[k], 1e-3f);
                p.e[k] = demodulate ? c[k] / p.am[k] : c[k];
            }
        }

    const float h[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    const float kn = 1.0f / (sigma[1] * sigma[1]), kz = 1.0f / (sigma[2] * sigma[2]), ka = 1.0f / (sigma[3] * sigma[3]);
    std::vector<float> next((size_t)width * height * 3);
    for (int i = 0; i < iterations; ++i) {
        const int s = 1 << i;
        const float sc = sigma[0] * std::ldexp(1.0f, -i);                     // Dammertz' halving
        const float kc = 1.0f / (sc * sc);
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                const Px &p = px[(size_t)y * width + x];
                float *r = &next[((size_t)y * width + x) * 3];
                r[0] = p.e[0]; r[1] = p.e[1]; r[2] = p.e[2];
                if (!p.valid) continue;
                float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int qx = x + s * dx, qy = y + s * dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const Px &q = px[(size_t)qy * width + qx];
                        if (!q.valid) continue;
                        const float dc = sq3(q.e, p.e);
                        float arg = dc * kc;
                        if (weightsUseGuides) {
                            const float dn = sq3(q.n, p.n), da = sq3(q.a, p.a);
                            const float m = pick(pick(p.z, q.z), 1e-20f);
                            const float t = (q.z - p.z) / m;
                            const float dz = t * t;
                            arg = arg + dn * kn;
                            arg = arg + dz * kz;
                            arg = arg + da * ka;
                        }
                        const float wgt = (h[dy + 2] * h[dx + 2]) * kzoExp(-arg);
                        for (int k = 0; k < 3; ++k) num[k] = num[k] + wgt * q.e[k];
                        den = den + wgt;
                    }
                for (int k = 0; k < 3; ++k) r[k] = num[k] / den;
            }
        for (size_t j = 0; j < px.size(); ++j) for (int k = 0; k < 3; ++k) px[j].e[k] = next[3 * j + k];
    }

    std::memset(out, 0, sizeof(float) * 4 * (size_t)cols * (height + 2 * border));
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const Px &p = px[(size_t)y * width + x];
            if (!p.valid) continue;
            float *t = out + 4 * ((size_t)(y + border) * cols + (x + border));
            for (int k = 0; k < 3; ++k) t[k] = demodulate ? p.e[k] * p.am[k] : p.e[k];
            t[3] = 1.0f;
        }
    return 0;
}
