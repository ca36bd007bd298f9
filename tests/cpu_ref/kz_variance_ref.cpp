// kz_variance_ref.cpp - TEST-ONLY CPU reference of include/kazen_mi355x_variance.h, in two parts. Never linked into the product; tests/test_variance_cpu.py
// compiles it with the oracle's flags (-O2 -ffp-contract=off, no fast math).
//   1. The canonical second-moment film: kzi_render_canonical's loop (kz_integrators_ref.cpp, which includes oracle/kz_oracle.cpp unchanged and is included here
//      unchanged) with the SQUARES of the sample as the value, behind the validity test of the sample itself.
//   2. The variance-guided a-trous filter, restated from the header's definition in plain C++ with the oracle's exp: five films and options in, a film and v_last out.
#include "kz_integrators_ref.cpp"
#include "kazen_mi355x_variance.h"

extern "C" {

int kzv_render_canonical(void *s, int integ, uint32_t s0, uint32_t s1, int threads, int grid, float *film) {
    using namespace kzo;
    Scene *scp = (Scene *)s; if (!scp || !film || grid <= 0) return KZ_ERR_INVALID_ARG;
    Scene &sc = *scp;
    if (s0 == 0 && s1 == 0) s1 = sc.sampleCount;
    const int W = sc.cam.width, H = sc.cam.height, B = sc.border;
    const int cols = W + 2 * B, rows = H + 2 * B;
    const float r = sc.filterRadius, lf = sc.lookupFactor;
    const int tapLo = (int)std::floor(-r - 0.5f) + 1, tapHi = (int)std::floor(r + 0.5f), taps = tapHi - tapLo + 1;
    if (taps < 1 || taps > 9) return KZ_ERR_UNSUPPORTED;
    const size_t framePix = (size_t)W * H;
    std::vector<float> tapSums((size_t)taps * taps * framePix * 4, 0.f);
    const int BS = 32;
    const int nbx = (W + BS - 1) / BS, nby = (H + BS - 1) / BS;
    if (threads <= 0) threads = 8;
    threads = std::max(1, std::min(threads, nbx * nby));
    std::atomic<int> next{0};
    auto work = [&]() {
        _MM_SET_FLUSH_ZERO_MODE(_MM_FLUSH_ZERO_ON);
        _MM_SET_DENORMALS_ZERO_MODE(_MM_DENORMALS_ZERO_ON);
        Sampler sampler; sampler.sc = &sc; sampler.type = sc.smp.type;
        LocalStats ls;
        std::vector<float> acc((size_t)taps * taps * 4);
        for (;;) {
            const int bi = next.fetch_add(1);
            if (bi >= nbx * nby) break;
            const int bx0 = (bi % nbx) * BS, by0 = (bi / nbx) * BS, bw = std::min(BS, W - bx0), bh = std::min(BS, H - by0);
            for (int i = 0; i < bw * bh; ++i) {
                const int px = i % bw + bx0, py = i / bw + by0;
                std::fill(acc.begin(), acc.end(), 0.f);
                for (uint32_t j = s0; j < s1; ++j) {
                    float sx, sy;
                    const V3 sample = renderSampleI(sc, integ, sampler, px, py, j, sx, sy, ls);
                    if (!colorValid(sample)) continue;                                     // the SAMPLE's validity: what the picture skips is skipped here
                    const V3 value(sample.x * sample.x, sample.y * sample.y, sample.z * sample.z);      // (a square that overflows is added as computed)
                    const float posx = sx - 0.5f - (float)(bx0 - B), posy = sy - 0.5f - (float)(by0 - B);
                    const float lox = std::ceil(posx - r), hix = std::floor(posx + r), loy = std::ceil(posy - r), hiy = std::floor(posy + r);
                    float wx[9], wy[9];
                    for (int t = 0; t < taps; ++t) {
                        const float xb = (float)(px + B - tapLo - t - bx0), yb = (float)(py + B - tapLo - t - by0);
                        wx[t] = !(xb < lox || xb > hix) ? sc.filter[(int)(std::fabs(xb - posx) * lf)] : 0.f;
                        wy[t] = !(yb < loy || yb > hiy) ? sc.filter[(int)(std::fabs(yb - posy) * lf)] : 0.f;
                    }
                    for (int ty = 0; ty < taps; ++ty)
                        for (int tx = 0; tx < taps; ++tx) {
                            float *a = &acc[(size_t)(ty * taps + tx) * 4];
                            a[0] += value.x * wx[tx] * wy[ty]; a[1] += value.y * wx[tx] * wy[ty]; a[2] += value.z * wx[tx] * wy[ty]; a[3] += 1.0f * wx[tx] * wy[ty];
                        }
                }
                for (int k = 0; k < taps * taps; ++k) std::memcpy(&tapSums[((size_t)k * framePix + (size_t)py * W + px) * 4], &acc[(size_t)k * 4], 4 * sizeof(float));
            }
        }
    };
    {
        FtzScope ftz;
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        for (int fy = 0; fy < rows; ++fy)
            for (int fx = 0; fx < cols; ++fx) {
                const int x0s = fx - B + tapLo, y0s = fy - B + tapLo;
                const int xlo = std::max(x0s, 0), xhi = std::min(x0s + taps - 1, W - 1), ylo = std::max(y0s, 0), yhi = std::min(y0s + taps - 1, H - 1);
                float total[4] = {0.f, 0.f, 0.f, 0.f};
                if (xlo <= xhi && ylo <= yhi)
                    for (int tr = ylo / grid; tr <= yhi / grid; ++tr)
                        for (int tc = xlo / grid; tc <= xhi / grid; ++tc) {
                            float part[4] = {0.f, 0.f, 0.f, 0.f};
                            for (int y = std::max(ylo, tr * grid); y <= std::min(yhi, tr * grid + grid - 1); ++y)
                                for (int x = std::max(xlo, tc * grid); x <= std::min(xhi, tc * grid + grid - 1); ++x) {
                                    const float *t = &tapSums[((size_t)((y - y0s) * taps + (x - x0s)) * framePix + (size_t)y * W + x) * 4];
                                    part[0] += t[0]; part[1] += t[1]; part[2] += t[2]; part[3] += t[3];
                                }
                            total[0] += part[0]; total[1] += part[1]; total[2] += part[2]; total[3] += part[3];
                        }
                std::memcpy(&film[((size_t)fy * cols + fx) * 4], total, sizeof total);
            }
    }
    return KZ_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- 2. the filter
namespace {

struct VPx { float e[3]; bool valid; float v, n[3], z, a[3], am[3]; };

inline float vpick(float a, float b) { return a > b ? a : b; }                // the header's max
inline float vsq3(const float *u, const float *v) {                           // |u - v|^2 = (x x + y y) + z z
    const float x = u[0] - v[0], y = u[1] - v[1], z = u[2] - v[2];
    float s = x * x;
    s = s + y * y;
    s = s + z * z;
    return s;
}
inline void vtexel(const float *film, size_t t, float v[3], float *w) {       // the value of a film's texel (null: an absent film, all zeros) and its weight
    v[0] = v[1] = v[2] = 0.0f; *w = 0.0f;
    if (!film) return;
    const float *p = film + 4 * t;
    *w = p[3];
    if (p[3] != 0.0f) for (int k = 0; k < 3; ++k) v[k] = p[k] / p[3];
}

}  // namespace

extern "C" int kzv_denoise(int width, int height, int border, const float *film, const float *moment, const float *albedo, const float *normal, const float *depth,
                           const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance) {
    KzDenoiseOpts o; KzVarianceOpts vo;
    std::memset(&o, 0, sizeof o); std::memset(&vo, 0, sizeof vo);
    if (opts) o = *opts;
    if (vopts) vo = *vopts;
    const uint32_t avail = (albedo ? KZ_AOV_ALBEDO : 0u) | (normal ? KZ_AOV_NORMAL : 0u) | (depth ? KZ_AOV_DEPTH : 0u);
    if (o.iterations > 8 || (o.flags & ~3u) || o.reserved || (o.guides & ~avail)) return 1;
    if (!std::isfinite(vo.sigmaVariance) || vo.sigmaVariance < 0.0f || vo.flags || vo.reserved || !vo.samples) return 1;
    float sigma[4] = {o.sigmaColor, o.sigmaNormal, o.sigmaDepth, o.sigmaAlbedo};
    const float dflt[4] = {2.0f, 0.3f, 0.1f, 0.1f};                           // sigmaColor defaults to 2 in this call
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return 1;
        if (sigma[k] == 0.0f) sigma[k] = dflt[k];
    }
    const float sigmaV = vo.sigmaVariance == 0.0f ? 3.0f : vo.sigmaVariance;
    const float sv2 = sigmaV * sigmaV;
    const float n = (float)vo.samples;
    const int iterations = o.iterations ? (int)o.iterations : 5;
    const uint32_t guides = o.guides ? o.guides : avail;
    const bool weightsUseGuides = guides != 0 && !(o.flags & KZ_DENOISE_NO_GUIDES);
    const bool demodulate = (guides & KZ_AOV_ALBEDO) && !(o.flags & KZ_DENOISE_NO_DEMODULATE);
    if (!(guides & KZ_AOV_ALBEDO)) albedo = nullptr;
    if (!(guides & KZ_AOV_NORMAL)) normal = nullptr;
    if (!(guides & KZ_AOV_DEPTH)) depth = nullptr;

    const int cols = width + 2 * border;
    std::vector<VPx> px((size_t)width * height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            VPx &p = px[(size_t)y * width + x];
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
                var[k] = vpick(s[k] - cc, 0.0f) / n;
                if (demodulate) { const float aa = p.am[k] * p.am[k]; var[k] = var[k] / aa; }
            }
            p.v = (var[0] + var[1]) + var[2];
        }

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
                const VPx &p = px[(size_t)y * width + x];
                float *r = &next[((size_t)y * width + x) * 4];
                r[0] = p.e[0]; r[1] = p.e[1]; r[2] = p.e[2]; r[3] = p.v;
                if (!p.valid) continue;
                float gn = 0.0f, gd = 0.0f;                                   // the 3 x 3 prefilter of v, unit spacing
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const VPx &q = px[(size_t)qy * width + qx];
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
                        const VPx &q = px[(size_t)qy * width + qx];
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

    std::memset(out, 0, sizeof(float) * 4 * (size_t)cols * (height + 2 * border));
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const VPx &p = px[(size_t)y * width + x];
            if (outVariance) outVariance[(size_t)y * width + x] = p.valid ? p.v : 0.0f;
            if (!p.valid) continue;
            float *t = out + 4 * ((size_t)(y + border) * cols + (x + border));
            for (int k = 0; k < 3; ++k) t[k] = demodulate ? p.e[k] * p.am[k] : p.e[k];
            t[3] = 1.0f;
        }
    return 0;
}
