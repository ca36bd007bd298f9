// kz_integrators_ref.cpp - TEST-ONLY CPU reference of the integrators "normals", "ao" and "path_mats" (src/kazen/integrator.cpp:11-71, :137-181),
// restated over the oracle's own pieces: this translation unit includes oracle/kz_oracle.cpp unchanged and reuses its Sampler, rayIntersect,
// camera, lightEval and bsdfSample. Never linked into the product; tests/test_integrators_cpu.py compiles it with the oracle's flags.
//
// The scene is created by kzo_scene_create with the path_mis tag (the oracle refuses every other one); the integrator is the argument of the entry points.
#include "../../oracle/kz_oracle.cpp"

namespace kzo {

static const float INV_TWOPI = 0.15915494309189533577f;      // common.h:35

// Warp::squareToUniformHemisphere (warp.cpp:68-79): M_PI is the float of common.h:31-33, the product is a float product; sin / cos are the oracle's
// defined sequences (kz_oracle_math.h), as for every other angle of the path (LAB_NOTES H14)
static V3 squareToUniformHemisphere(float sx, float sy) {
    const float z = sx;
    const float tmp = std::sqrt(1.0f - z * z);
    float sinPhi, cosPhi; kzoSinCos(2.0f * kPi * sy, &sinPhi, &cosPhi);
    return V3(cosPhi * tmp, sinPhi * tmp, z);
}

static V3 LiNormals(const Scene &sc, Sampler &, const Ray &ray, LocalStats &ls) {
    Intersection its;
    if (!rayIntersect(sc, ray, its, false, ls)) return V3(0.f);
    const V3 n = its.geoFrame.n;
    return V3(std::fabs(n.x), std::fabs(n.y), std::fabs(n.z));
}

static V3 LiAo(const Scene &sc, Sampler &sampler, const Ray &ray, LocalStats &ls) {
    Intersection its;
    if (!rayIntersect(sc, ray, its, false, ls)) return V3(0.f);
    float sx, sy; sampler.next2D(sx, sy);
    const V3 sample = squareToUniformHemisphere(sx, sy);
    V3 point = its.shFrame.toWorld(sample);
    const Ray shadowRay(its.p, point);                                   // mint Epsilon, maxt inf
    Intersection sh;
    if (!rayIntersect(sc, shadowRay, sh, true, ls)) {
        its.shFrame.n = normalized(its.shFrame.n);
        point = normalized(point);
        const float cosTheta = its.shFrame.toLocal(point).z;
        return V3(0.f) + V3(cosTheta / kPi) / INV_TWOPI;                 // (a zero sum plus the value: -0 comes out as +0, as on the GPU)
    }
    return V3(0.f);
}

static const int kMatsMaxDepth = 512;      // H15: the reference has no cap
static V3 LiMats(const Scene &sc, Sampler &sampler, const Ray &ray0, LocalStats &ls) {
    V3 color(0.f), t(1.f);
    Ray ray = ray0;
    for (int depth = 0; depth < kMatsMaxDepth; ++depth) {
        Intersection its;
        if (!rayIntersect(sc, ray, its, false, ls)) return color;
        const MeshData &hm = sc.meshes[its.mesh];
        if (hm.light >= 0) {
            LRec lr; lr.ref = ray.o; lr.p = its.p; lr.n = its.shFrame.n; lr.wi = normalized(its.p - ray.o);
            color = color + t * lightEval(sc.lights[hm.light], lr);
        }
        const float probability = std::min(t.x, 0.95f);
        if (sampler.next1D() >= probability) return color;
        t = t / probability;
        BRec b; b.wi = its.shFrame.toLocal(-ray.d); b.uvx = its.uvx; b.uvy = its.uvy; b.sc = &sc;      // bRec.uv = its.uv; bRec.its default (no frame)
        float s2x, s2y; sampler.next2D(s2x, s2y);                                                       // H1
        const float s1 = sampler.next1D();
        bool ok;
        const V3 f = bsdfSample(meshBsdf(sc, its.mesh), b, s1, s2x, s2y, ok);
        t = t * f;
        if (!ok || (f.x == 0.f && f.y == 0.f && f.z == 0.f)) return color;                             // zero weight ends the path
        ray = Ray(its.p, its.shFrame.toWorld(b.wo));
    }
    return color;
}

static V3 renderSampleI(const Scene &sc, int integ, Sampler &sampler, int px, int py, uint32_t j, float &sx, float &sy, LocalStats &ls) {
    sampler.generateSample(px, py, j);
    float jx, jy; sampler.nextPixel2D(jx, jy);
    sx = (float)px + jx; sy = (float)py + jy;
    float ax, ay; sampler.next2D(ax, ay);
    Ray ray; cameraSampleRay(sc, sx, sy, ax, ay, ray);
    ls.samples++;
    if (integ == KZ_INTEGRATOR_NORMALS) return LiNormals(sc, sampler, ray, ls);
    if (integ == KZ_INTEGRATOR_AO) return LiAo(sc, sampler, ray, ls);
    if (integ == KZ_INTEGRATOR_PATH_MATS) return LiMats(sc, sampler, ray, ls);
    return Li(sc, sampler, ray, ls);
}

} // namespace kzo

extern "C" {

// (pixel sample x, y, r, g, b) per sample, as kzo_render_samples
void kzi_render_samples(void *s, int integ, uint32_t n, const int32_t *pxy, const uint32_t *idx, float *out) { kzo::FtzScope ftz_;
    using namespace kzo;
    Scene &sc = *(Scene *)s; Sampler sm; sm.sc = &sc; sm.type = sc.smp.type; LocalStats ls;
    for (uint32_t i = 0; i < n; ++i) {
        float sx, sy; V3 v = renderSampleI(sc, integ, sm, pxy[2 * i], pxy[2 * i + 1], idx[i], sx, sy, ls);
        out[5 * i] = sx; out[5 * i + 1] = sy; out[5 * i + 2] = v.x; out[5 * i + 3] = v.y; out[5 * i + 4] = v.z;
    }
}

// kzo_render_canonical's loop over renderSampleI: the film in the order of float additions the library fixes (whole frame, samples [s0, s1))
int kzi_render_canonical(void *s, int integ, uint32_t s0, uint32_t s1, int threads, int grid, float *film) {
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
                    const V3 value = renderSampleI(sc, integ, sampler, px, py, j, sx, sy, ls);
                    if (!colorValid(value)) continue;
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
    return KZ_OK;
}

// bounces a path_mats sample took (hits shaded), for the cap test
int kzi_mats_depth(void *s, int32_t px, int32_t py, uint32_t idx) { kzo::FtzScope ftz_;
    using namespace kzo;
    Scene &sc = *(Scene *)s; Sampler sampler; sampler.sc = &sc; sampler.type = sc.smp.type; LocalStats ls;
    float sx, sy;
    sampler.generateSample(px, py, idx);
    float jx, jy; sampler.nextPixel2D(jx, jy);
    sx = (float)px + jx; sy = (float)py + jy;
    float ax, ay; sampler.next2D(ax, ay);
    Ray ray; cameraSampleRay(sc, sx, sy, ax, ay, ray);
    LiMats(sc, sampler, ray, ls);
    return (int)ls.shadedHits;
}

} // extern "C"
