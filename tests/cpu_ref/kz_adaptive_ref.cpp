// kz_adaptive_ref.cpp - TEST-ONLY CPU reference of include_ext/kazen_mi355x_adaptive.h. Never linked into the product; tests/adaptive_refs.py compiles it with the
// oracle's flags (-O2 -ffp-contract=off, no fast math). kz_variance_ref.cpp - and through it kz_integrators_ref.cpp and oracle/kz_oracle.cpp - is included unchanged.
//   kzad_render_counts  the canonical loop of kzi_render_canonical / kzv_render_canonical with `j < samplesPerPixel[py * W + px]` in place of the uniform bound:
//                       the film of a frame whose pixels hold different prefixes [0, n_p) of their sample sequences
//   kzad_classify       the header's pixel and block tests, sequential, nothing flushed to zero
//   kzad_adaptive       the whole call: schedule, render by counts, classify, repeat
#include "kz_variance_ref.cpp"
#include "../../include_ext/kazen_mi355x_adaptive.h"

namespace {

// The pixel test runs with subnormals kept, whatever mode the calling thread is in (the render loops above flush, as the device's path kernels do).
struct KeepDenormals {
    unsigned saved;
    KeepDenormals() : saved(_mm_getcsr()) { _mm_setcsr(saved & ~0x8040u); }      // FTZ (bit 15) and DAZ (bit 6) off
    ~KeepDenormals() { _mm_setcsr(saved); }
};

struct AdRule { float thr2, floor; uint32_t minSamples, maxSamples, step, block, permille; };

// The header's defaults. sceneSamples 0: no scene (maxSamples stays as given; 0 = no cap is known). false: options the product refuses.
bool adRule(const KzAdaptiveOpts *o, uint32_t sceneSamples, AdRule *r) {
    if (!o || !std::isfinite(o->threshold) || !(o->threshold > 0.0f) || !std::isfinite(o->floor) || o->floor < 0.0f) return false;
    if ((sceneSamples && o->maxSamples > sceneSamples) || o->outlierPermille > 999u || o->flags) return false;
    if (o->block != 0 && o->block != 8 && o->block != 16 && o->block != 32 && o->block != 64) return false;
    r->thr2 = o->threshold * o->threshold;
    r->floor = o->floor == 0.0f ? 0.01f : o->floor;
    r->maxSamples = o->maxSamples ? o->maxSamples : sceneSamples;
    r->minSamples = o->minSamples ? o->minSamples : 16u;
    if (r->maxSamples && r->minSamples > r->maxSamples) r->minSamples = r->maxSamples;
    r->step = o->step; r->block = o->block ? o->block : 16u; r->permille = o->outlierPermille;
    return true;
}

// One test of every block that is still tested: rec[b] is rewritten unless the block's n is 0 or its record says CONVERGED. active[b] (may be null): sampled again.
void adClassify(int width, int height, int border, const float *film, const float *moment, const uint32_t *blockSamples, const AdRule &r, KzAdaptiveBlock *rec, uint8_t *active) {
    KeepDenormals keep;
    const int e = (int)r.block, nbx = (width + e - 1) / e, nby = (height + e - 1) / e, cols = width + 2 * border;
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const size_t b = (size_t)by * nbx + bx;
            const uint32_t n = blockSamples[b];
            if (active) active[b] = 0;
            if (n == 0u || (rec[b].flags & KZ_ADAPTIVE_CONVERGED)) continue;
            const float nf = (float)n;
            uint32_t valid = 0, noisy = 0;
            for (int y = by * e; y < std::min(by * e + e, height); ++y)
                for (int x = bx * e; x < std::min(bx * e + e, width); ++x) {
                    const float *T = film + 4 * ((size_t)(y + border) * cols + (x + border)), *M = moment + 4 * ((size_t)(y + border) * cols + (x + border));
                    if (!(T[3] != 0.0f)) continue;
                    ++valid;
                    volatile float c[3], var[3];                       // (volatile: every intermediate is an fp32 in memory, one rounding per operation)
                    for (int k = 0; k < 3; ++k) {
                        c[k] = T[k] / T[3];
                        const float s = M[3] != 0.0f ? M[k] / M[3] : 0.0f;
                        const float cc = c[k] * c[k];
                        const float d = s - cc;
                        var[k] = d > 0.0f ? d : 0.0f;
                    }
                    float v = var[0] + var[1];
                    v = v + var[2];
                    v = v / nf;
                    float m = c[0] + c[1];
                    m = m + c[2];
                    const float a = (m > 0.0f ? m : 0.0f) + r.floor;
                    const float aa = a * a;
                    const float bound = r.thr2 * aa;
                    if (v > bound) ++noisy;
                }
            const bool converged = (uint64_t)noisy * 1000u <= (uint64_t)r.permille * valid;
            const bool capped = !converged && r.maxSamples != 0u && n >= r.maxSamples;
            rec[b].samples = n; rec[b].noisy = noisy; rec[b].valid = valid;
            rec[b].flags = converged ? KZ_ADAPTIVE_CONVERGED : (capped ? KZ_ADAPTIVE_AT_CAP : 0u);
            if (active) active[b] = (!converged && !capped) ? 1 : 0;
        }
}

}  // namespace

extern "C" {

int kzad_render_counts(void *s, int integ, int which, const uint32_t *samplesPerPixel, int threads, int grid, float *film) {
    using namespace kzo;
    Scene *scp = (Scene *)s; if (!scp || !film || !samplesPerPixel || grid <= 0 || which < 0 || which > 1) return KZ_ERR_INVALID_ARG;
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
                    const V3 sample = renderSampleI(sc, integ, sampler, px, py, j, sx, sy, ls);
                    if (!colorValid(sample)) continue;
                    const V3 value = which ? V3(sample.x * sample.x, sample.y * sample.y, sample.z * sample.z) : sample;
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

// The records of one test of caller-supplied films: a block whose entry of blockSamples is 0 is skipped and its record all zeros. 1: options the product refuses.
int kzad_classify(int width, int height, int border, const float *film, const float *moment, const uint32_t *blockSamples, const KzAdaptiveOpts *opts, KzAdaptiveBlock *out) {
    AdRule r;
    if (!adRule(opts, 0u, &r) || width < 1 || height < 1 || border < 0) return 1;
    const int e = (int)r.block, nb = ((width + e - 1) / e) * ((height + e - 1) / e);
    std::memset(out, 0, sizeof(KzAdaptiveBlock) * (size_t)nb);
    adClassify(width, height, border, film, moment, blockSamples, r, out, nullptr);
    return 0;
}

// The whole call on the reference's scene: film and moment (the film's layout), one record per block, the width x height plane of samples per pixel, the rounds.
int kzad_adaptive(void *s, int integ, const KzAdaptiveOpts *opts, int threads, int grid, float *film, float *moment, KzAdaptiveBlock *rec, uint32_t *counts, uint32_t *rounds) {
    kzo::Scene *scp = (kzo::Scene *)s;
    AdRule r;
    if (!scp || !film || !moment || !rec || !counts || !rounds || !adRule(opts, scp->sampleCount, &r)) return 1;
    const int W = scp->cam.width, H = scp->cam.height, e = (int)r.block, nbx = (W + e - 1) / e, nby = (H + e - 1) / e, nb = nbx * nby;
    std::memset(rec, 0, sizeof(KzAdaptiveBlock) * (size_t)nb);
    std::vector<uint8_t> active((size_t)nb, 1);
    std::vector<uint32_t> ns((size_t)nb, 0u);
    *rounds = 0;
    for (uint32_t n = r.minSamples;;) {
        for (int b = 0; b < nb; ++b) if (active[b]) ns[b] = n;       // the blocks of this round's tile list receive [n_prev, n): they hold [0, n) now
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) counts[(size_t)y * W + x] = ns[(size_t)(y / e) * nbx + x / e];
        int rc;
        if ((rc = kzad_render_counts(s, integ, 0, counts, threads, grid, film)) || (rc = kzad_render_counts(s, integ, 1, counts, threads, grid, moment))) return rc;
        std::vector<uint32_t> tested((size_t)nb);
        for (int b = 0; b < nb; ++b) tested[b] = active[b] ? n : 0u;
        adClassify(W, H, scp->border, film, moment, tested.data(), r, rec, active.data());
        ++*rounds;
        if (n == r.maxSamples) break;
        bool any = false;
        for (int b = 0; b < nb; ++b) any = any || active[b];
        if (!any) break;
        const uint64_t next = r.step ? (uint64_t)n + r.step : 2ull * n;
        n = next < r.maxSamples ? (uint32_t)next : r.maxSamples;
    }
    return 0;
}

}  // extern "C"
