// kz_adaptive_aov_ref.cpp - TEST-ONLY: the feature films of a frame whose pixels hold different sample counts, for the adaptive tests. kz_aov_ref.cpp is included
// unchanged (it brings oracle/kz_oracle.cpp, which kz_adaptive_ref.cpp's chain brings too: the two cannot share a translation unit). kzada_render_counts is
// kza_render_canonical's loop with `j < samplesPerPixel[py * W + px]` in place of the uniform bound.
#include "kz_aov_ref.cpp"

extern "C" int kzada_render_counts(void *s, int integ, uint32_t aov, const uint32_t *samplesPerPixel, int threads, int grid, float *film) {
    using namespace kzo;
    Scene *scp = (Scene *)s; if (!scp || !film || !samplesPerPixel || grid <= 0 || (aov != 1 && aov != 2 && aov != 4)) return KZ_ERR_INVALID_ARG;
    Scene &sc = *scp;
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
                for (uint32_t j = 0; j < samplesPerPixel[(size_t)py * W + px]; ++j) {
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
