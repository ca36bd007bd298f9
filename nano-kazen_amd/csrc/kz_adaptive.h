// kz_adaptive.h - the kernel of include_ext/kazen_mi355x_adaptive.h: the pixel and block tests of adaptive sampling on two resolved films. ONE WAVE PER BLOCK of the
// frame: in every step the wave's 64 lanes take 64 consecutive pixels of the block in row-major order - 64 / EDGE whole rows of it - so its loads of the two float4
// films are contiguous row segments of EDGE x 16 bytes (8: 1 step, 16: 4, 32: 16, 64: 64 steps per lane). Each lane evaluates the pixel test in the header's order of
// operations (this unit keeps subnormals: build.sh IEEE_UNITS); `valid` and `noisy` are population counts of wave ballots, integers, so no reduction order enters.
// Lane 0 writes the 16-byte record and the block's byte of `active` with ordinary stores. The stage moves 32 bytes per frame pixel and computes next to nothing.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include_ext/kazen_mi355x_adaptive.h"

static_assert(sizeof(KzAdaptiveBlock) == 16 && sizeof(KzAdaptiveOpts) == 32 && sizeof(KzAdaptiveInfo) == 32, "the records of kazen_mi355x_adaptive.h");

#define KZ_ADAPTIVE_WAVES 4               // blocks of the frame per workgroup

// What the kernel takes of a call: the frame, the rule's numbers as the host resolved them (kzAdaptiveResolve), and the blocks' sample counts - blockSamples[b], or
// nAll for every block where blockSamples is null (a round of kz_render_adaptive: every block that is still tested holds the round's n).
struct KzAdaptiveArgs {
    const float4 *film, *moment;
    int32_t width, height, border;
    uint32_t nbx, nBlocks;
    const uint32_t *blockSamples; uint32_t nAll;
    float thr2, floor;                    // threshold * threshold (one fp32 product, made on the host), floor
    uint32_t permille, maxSamples;        // maxSamples 0: no cap is known
};

// The pixel test on texels T and M, n = (float)samples: true iff the pixel is noisy. The caller has seen that T.w != 0.
__device__ __forceinline__ bool kzAdaptiveNoisy(const float4 T, const float4 M, float n, float thr2, float floor_) {
    const float cr = T.x / T.w, cg = T.y / T.w, cb = T.z / T.w;
    const bool mw = M.w != 0.0f;
    const float sr = mw ? M.x / M.w : 0.0f, sg = mw ? M.y / M.w : 0.0f, sb = mw ? M.z / M.w : 0.0f;
    const float dr = sr - cr * cr, dg = sg - cg * cg, db = sb - cb * cb;
    const float vr = dr > 0.0f ? dr : 0.0f, vg = dg > 0.0f ? dg : 0.0f, vb = db > 0.0f ? db : 0.0f;
    const float v = ((vr + vg) + vb) / n;
    const float m = (cr + cg) + cb;
    const float a = (m > 0.0f ? m : 0.0f) + floor_;
    return v > thr2 * (a * a);
}

template <int EDGE>
__global__ __launch_bounds__(64 * KZ_ADAPTIVE_WAVES) void kz_adaptive_classify(const KzAdaptiveArgs A, KzAdaptiveBlock *__restrict__ rec, uint8_t *__restrict__ active) {
    constexpr int STEPS = EDGE * EDGE / 64, ROWS = 64 / EDGE;          // steps per lane; block rows a step covers
    constexpr int UNROLL = STEPS < 4 ? STEPS : 4;                      // loads in flight per lane and film
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * KZ_ADAPTIVE_WAVES + (threadIdx.x >> 6);
    if (b >= A.nBlocks) return;                                        // (the whole wave: b is the wave's)
    const uint32_t n = A.blockSamples ? A.blockSamples[b] : A.nAll;
    if (n == 0u || (rec[b].flags & KZ_ADAPTIVE_CONVERGED)) {           // not tested: the record stays, the block is not sampled again
        if (lane == 0u) active[b] = 0;
        return;
    }
    const int bx = (int)(b % A.nbx), by = (int)(b / A.nbx);
    const int lx = (int)(lane % EDGE), ly = (int)(lane / EDGE);
    const int x = bx * EDGE + lx;
    const size_t cols = (size_t)(A.width + 2 * A.border);
    const float nf = (float)n;
    uint32_t valid = 0u, noisy = 0u;
    for (int s0 = 0; s0 < STEPS; s0 += UNROLL) {
        float4 T[UNROLL], M[UNROLL]; bool in[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int y = by * EDGE + (s0 + u) * ROWS + ly;
            in[u] = x < A.width && y < A.height;                       // (edge blocks are clipped: a lane outside the frame loads nothing)
            const size_t t = (size_t)(y + A.border) * cols + (size_t)(x + A.border);
            T[u] = in[u] ? A.film[t] : make_float4(0.f, 0.f, 0.f, 0.f);
            M[u] = in[u] ? A.moment[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const bool v = in[u] && T[u].w != 0.0f;
            const bool z = v && kzAdaptiveNoisy(T[u], M[u], nf, A.thr2, A.floor);
            valid += (uint32_t)__popcll(__ballot(v));
            noisy += (uint32_t)__popcll(__ballot(z));
        }
    }
    if (lane == 0u) {
        const bool converged = (unsigned long long)noisy * 1000ull <= (unsigned long long)A.permille * (unsigned long long)valid;
        const bool capped = !converged && A.maxSamples != 0u && n >= A.maxSamples;
        KzAdaptiveBlock r;
        r.samples = n; r.noisy = noisy; r.valid = valid; r.flags = converged ? KZ_ADAPTIVE_CONVERGED : (capped ? KZ_ADAPTIVE_AT_CAP : 0u);
        rec[b] = r;
        active[b] = (uint8_t)((!converged && !capped) ? 1 : 0);
    }
}
