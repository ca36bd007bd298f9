// kz_aov_ref.cpp - TEST-ONLY CPU reference of the feature films (include/kazen_mi355x_aov.h): first-hit albedo, shading normal and depth, restated over the
// oracle's own pieces: this translation unit includes oracle/kz_oracle.cpp unchanged and reuses its Sampler, camera, rayIntersect, textureEval, its normal-map
// frame and the walk-through of Li. Never linked into the product; tests/test_aov_cpu.py compiles it with the oracle's flags.
//
// The scene is created by kzo_scene_create with the path_mis tag (the oracle refuses every other one); the integrator is the argument of the entry points:
// it decides one thing only, whether a first hit on an invisible light is walked through (path_mis) or kept (normals, ao, path_mats).
#include "../../oracle/kz_oracle.cpp"

namespace kzo {

struct Features { V3 albedo, normal; float depth; bool hit; };

// The hit's BSDF row (a normalmap unwrapped to its nested row): albedo / baseColor through its texture at its.uv, white for the models without a diffuse colour
static V3 albedoOf(const Scene &sc, const KzBSDF &m, const Intersection &its) {
    if (m.type == KZ_BSDF_MIRROR || m.type == KZ_BSDF_DIELECTRIC || m.type == KZ_BSDF_ROUGHDIELECTRIC || m.type == KZ_BSDF_ROUGHCONDUCTOR) return V3(1.0f);
    if (m.albedoTex) return textureEval(sc, m.albedoTex - 1, its.uvx, its.uvy);
    return m.type == KZ_BSDF_KAZENSTANDARD ? V3(m.baseColor[0], m.baseColor[1], m.baseColor[2]) : V3(m.albedo[0], m.albedo[1], m.albedo[2]);
}

static Features featuresOf(const Scene &sc, int integ, const Ray &ray, LocalStats &ls) {
    Features f; f.albedo = V3(0.f); f.normal = V3(0.f); f.depth = 0.f; f.hit = false;
    Intersection its;
    if (!rayIntersect(sc, ray, its, false, ls)) return f;
    if (integ == KZ_INTEGRATOR_PATH_MIS && sc.meshes[its.mesh].light >= 0 && !sc.lights[sc.meshes[its.mesh].light].primaryVisibility) {
        Ray newRay(its.p + sc.integ.traceBias * ray.d, ray.d);                     // integrator.cpp:214-219 (H6): the result is ignored on a miss
        rayIntersect(sc, newRay, its, false, ls);
    }
    const KzBSDF *m = &meshBsdf(sc, its.mesh);
    f.normal = its.shFrame.n;
    if (m->type == KZ_BSDF_NORMALMAP) {
        const V3 rgb = textureEval(sc, m->normalTex - 1, its.uvx, its.uvy);       // bsdf.cpp:292-293
        const V3 n(2 * rgb.x - 1, 2 * rgb.y - 1, 2 * rgb.z - 1);
        f.normal = normalMapFrame(its, normalized(n)).n;
        m = &sc.bsdfs[m->nested];
    }
    f.albedo = albedoOf(sc, *m, its);
    f.depth = its.t; f.hit = true;
    return f;
}

static Features sampleFeatures(const Scene &sc, int integ, Sampler &sampler, int px, int py, uint32_t j, float &sx, float &sy, LocalStats &ls) {
    sampler.generateSample(px, py, j);
    float jx, jy; sampler.nextPixel2D(jx, jy);
    sx = (float)px + jx; sy = (float)py + jy;
    float ax, ay; sampler.next2D(ax, ay);
    Ray ray; cameraSampleRay(sc, sx, sy, ax, ay, ray);
    return featuresOf(sc, integ, ray, ls);
}

static inline bool finite3(V3 c) { return std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.z); }      // the isfinite half of Color3f::isValid: normals are signed

} // namespace kzo

extern "C" {

// 10 floats per sample: sample x, y | albedo r g b | normal x y z | depth | hit
void kza_samples(void *s, int integ, uint32_t n, const int32_t *pxy, const uint32_t *idx, float *out) { kzo::FtzScope ftz_;
    using namespace kzo;
    Scene &sc = *(Scene *)s; Sampler sm; sm.sc = &sc; sm.type = sc.smp.type; LocalStats ls;
    for (uint32_t i = 0; i < n; ++i) {
        float sx, sy; const Features f = sampleFeatures(sc, integ, sm, pxy[2 * i], pxy[2 * i + 1], idx[i], sx, sy, ls);
        float *o = out + 10 * (size_t)i;
        o[0] = sx; o[1] = sy; o[2] = f.albedo.x; o[3] = f.albedo.y; o[4] = f.albedo.z; o[5] = f.normal.x; o[6] = f.normal.y; o[7] = f.normal.z; o[8] = f.depth; o[9] = f.hit ? 1.f : 0.f;
    }
}

// kzi_render_canonical's loop (tests/cpu_ref/kz_integrators_ref.cpp) with the feature `aov` (1 albedo, 2 normal, 4 depth) as the value and without the sign
// half of the validity test: the film in the order of float additions the library fixes (whole frame, samples [s0, s1))
int kza_render_canonical(void *s, int integ, uint32_t aov, uint32_t s0, uint32_t s1, int threads, int grid, float *film) {
    using namespace kzo;
    Scene *scp = (Scene *)s; if (!scp || !film || grid <= 0 || (aov != 1 && aov != 2 && aov != 4)) return KZ_ERR_INVALID_ARG;
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
                    const Features f = sampleFeatures(sc, integ, sampler, px, py, j, sx, sy, ls);
                    const V3 value = aov == 1 ? f.albedo : (aov == 2 ? f.normal : V3(f.depth));
                    if (!finite3(value)) continue;
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

} // extern "C"
