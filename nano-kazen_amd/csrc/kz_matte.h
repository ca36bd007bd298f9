// kz_matte.h - the kernels of include_ext/kazen_mi355x_matte.h: ID mattes, per frame pixel a 64-byte record of (id, sample count) slots counted from the first hits of
// the pass's own samples. The accumulate kernel runs where kz_wf_aov runs (wfPass, kz_render.hip): behind the camera stage every item's first-hit record sits at its
// own slot of W.hit, and the key - the mesh or the BSDF row of the hit triangle - is in the last quad of the triangle's 112-B shading record (mesh | prim | bsdf |
// lightFlags). It adds no per-item state: it reads the hit record (16 B, streaming), gathers that one quad (16 B) and read-modify-writes each pixel's record once.
// Items are pixel-major (item p * S + s is sample s of pixel pixList[p]) and a pixel belongs to ONE lane or ONE wave of the launch: no atomics, and the order of a
// pixel's samples - which the rule is defined by - is the order the lane or wave walks them in.
#pragma once
#include "kz_devfn.h"
#include "../../include_ext/kazen_mi355x_matte.h"

static_assert(sizeof(KzMatteTexel) == 64 && KZ_MATTE_SLOTS == 7, "a matte record is 7 ids, 7 counts, other, miss: one 64-B line");

// The key of item `item`. SRC 0: from the pass's hit records - k0 the mesh, k1 the BSDF row of the hit triangle; SRC 1: from a caller's key plane (k0; KZ_MATTE_NONE = miss).
template <int SRC>
__device__ __forceinline__ void matteItemKeys(const KzTriShade *__restrict__ shade, const float4 *__restrict__ hit, const uint32_t *__restrict__ keys, uint32_t item, bool on,
                                              bool &isHit, uint32_t &k0, uint32_t &k1) {
    isHit = false; k0 = 0u; k1 = 0u;
    if (!on) return;
    if (SRC == 0) {
        const float4 h = kzLoadStream(hit + item);
        if (h.x < KZ_INF) {
            const float4 q = reinterpret_cast<const float4 *>(shade + __float_as_uint(h.w))[6];
            isHit = true; k0 = __float_as_uint(q.x); k1 = __float_as_uint(q.z);
        }
    } else {
        k0 = kzLoadStream(keys + item);
        isHit = k0 != KZ_MATTE_NONE;
    }
}

// ---- one wave per pixel (S >= 64). The pixel's record is held one slot per lane: lane k < 7 has id[k] and count[k]; taken (slots in use: they are taken from 0
// upwards and never given back), other and miss are the same in every lane.
struct KzMatteWaveRec { uint32_t id, cnt, taken, other, miss; };

__device__ __forceinline__ void matteWaveLoad(const KzMatteTexel *t, uint32_t lane, KzMatteWaveRec &r) {
    const bool slot = lane < KZ_MATTE_SLOTS;
    r.id = slot ? t->id[lane] : 0u; r.cnt = slot ? t->count[lane] : 0u;
    r.taken = (uint32_t)__popcll(__ballot(slot && r.cnt != 0u));
    r.other = t->other; r.miss = t->miss;
}
__device__ __forceinline__ void matteWaveStore(KzMatteTexel *t, uint32_t lane, const KzMatteWaveRec &r) {
    if (lane < KZ_MATTE_SLOTS) { t->id[lane] = r.id; t->count[lane] = r.cnt; }
    if (lane == 0u) { t->other = r.other; t->miss = r.miss; }
}
// One chunk of up to 64 consecutive samples, lane = sample (`on`: the lane has one - the lanes beyond S of the tail chunk are out of every ballot). The distinct keys
// of the chunk are served in ascending order of the first lane that holds them, which is the order in which the samples would have met them one by one - so "the
// lowest free slot at the first sample" holds by construction. Every lane of the wave runs this (the loops around it are wave-uniform): the ballots are whole.
// The key being served is read with v_readlane from the lane the ballot names - not with readfirstlane under a branch of the unserved lanes, whose value would
// depend on where the compiler leaves the instruction relative to that branch.
__device__ __forceinline__ void matteWaveCount(uint32_t lane, bool on, bool isHit, uint32_t key, KzMatteWaveRec &r) {
    r.miss += (uint32_t)__popcll(__ballot(on && !isHit));
    unsigned long long todo = __ballot(on && isHit);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
        const unsigned long long same = __ballot(on && isHit && key == k) | (1ull << first);      // (| first: the loop ends whatever the compiler makes of the ballot)
        const uint32_t n = (uint32_t)__popcll(same & todo);
        todo &= ~same;
        const bool mine = lane < r.taken && r.id == k;
        if (__ballot(mine)) { if (mine) r.cnt += n; }
        else if (r.taken < KZ_MATTE_SLOTS) { if (lane == r.taken) { r.id = k; r.cnt = n; } ++r.taken; }
        else r.other += n;
    }
}

// SRC 0: t0 the mesh table, t1 the BSDF-row table (either may be null: the key is off); SRC 1: t0 alone. A wave owns whole pixels: pixel p of the pass for
// p = wave, wave + nWaves, ...; the records it touches are those of pixList[p], at y * width + x < width * height.
template <int SRC>
__global__ __launch_bounds__(KZ_BLOCK) void kz_matte_accumulate(const KzTriShade *__restrict__ shade, const float4 *__restrict__ hit, const uint32_t *__restrict__ keys,
                                                                const uint32_t *__restrict__ pixList, uint32_t nPix, uint32_t S, uint32_t width,
                                                                KzMatteTexel *__restrict__ t0, KzMatteTexel *__restrict__ t1) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (provably the same in every lane of the wave)
    const uint32_t nWaves = gridDim.x * (KZ_BLOCK / 64u);
    const bool two = SRC == 0 && t1 != nullptr;
    for (uint32_t p = blockIdx.x * (KZ_BLOCK / 64u) + wave; p < nPix; p += nWaves) {
        const uint32_t px = framePixelOf(pixList[p], width);
        KzMatteWaveRec r0 = {0u, 0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u, 0u};
        if (t0) matteWaveLoad(t0 + px, lane, r0);
        if (two) matteWaveLoad(t1 + px, lane, r1);
        for (uint32_t base = 0; base < S; base += 64u) {
            const uint32_t s = base + lane;
            const bool on = s < S;
            bool isHit; uint32_t k0, k1;
            matteItemKeys<SRC>(shade, hit, keys, p * S + s, on, isHit, k0, k1);
            if (t0) matteWaveCount(lane, on, isHit, k0, r0);
            if (two) matteWaveCount(lane, on, isHit, k1, r1);
        }
        if (t0) matteWaveStore(t0 + px, lane, r0);
        if (two) matteWaveStore(t1 + px, lane, r1);
    }
}

// ---- one lane per pixel (S < 64: a 1-4-spp interactive frame does not serialise 16-64 pixels inside one wave). The record lives in the lane's registers; every
// loop over the slots is unrolled, so no index into it is a run-time value.
struct KzMatteRegs { uint32_t id[KZ_MATTE_SLOTS], cnt[KZ_MATTE_SLOTS], other, miss; };

__device__ __forceinline__ void matteLoad(const KzMatteTexel *t, KzMatteRegs &r) {
    const uint4 *q = reinterpret_cast<const uint4 *>(t);
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    r.id[0] = a.x; r.id[1] = a.y; r.id[2] = a.z; r.id[3] = a.w; r.id[4] = b.x; r.id[5] = b.y; r.id[6] = b.z;
    r.cnt[0] = b.w; r.cnt[1] = c.x; r.cnt[2] = c.y; r.cnt[3] = c.z; r.cnt[4] = c.w; r.cnt[5] = d.x; r.cnt[6] = d.y;
    r.other = d.z; r.miss = d.w;
}
__device__ __forceinline__ void matteStore(KzMatteTexel *t, const KzMatteRegs &r) {
    uint4 *q = reinterpret_cast<uint4 *>(t);
    q[0] = make_uint4(r.id[0], r.id[1], r.id[2], r.id[3]); q[1] = make_uint4(r.id[4], r.id[5], r.id[6], r.cnt[0]);
    q[2] = make_uint4(r.cnt[1], r.cnt[2], r.cnt[3], r.cnt[4]); q[3] = make_uint4(r.cnt[5], r.cnt[6], r.other, r.miss);
}
// The rule for one sample: the slots are taken from 0 upwards, so the first free one ends the search. Written as selects over every slot - no branch whose arm
// names one slot - so that the record stays in registers: with an early exit per slot the compiler turned the chain into an indexed update of an array in scratch.
__device__ __forceinline__ void matteCount(KzMatteRegs &r, bool isHit, uint32_t k) {
    bool open = isHit;                                  // the sample still looks for its slot
#pragma unroll
    for (int j = 0; j < KZ_MATTE_SLOTS; ++j) {
        const bool isFree = r.cnt[j] == 0u;
        const bool take = open && (isFree || r.id[j] == k);
        r.id[j] = (take && isFree) ? k : r.id[j];
        r.cnt[j] += take ? 1u : 0u;
        open = open && !take;
    }
    r.other += open ? 1u : 0u;
    r.miss += isHit ? 0u : 1u;
}

template <int SRC>
__global__ __launch_bounds__(KZ_BLOCK) void kz_matte_accumulate_lane(const KzTriShade *__restrict__ shade, const float4 *__restrict__ hit, const uint32_t *__restrict__ keys,
                                                                     const uint32_t *__restrict__ pixList, uint32_t nPix, uint32_t S, uint32_t width,
                                                                     KzMatteTexel *__restrict__ t0, KzMatteTexel *__restrict__ t1) {
    const bool two = SRC == 0 && t1 != nullptr;
    for (uint32_t p = blockIdx.x * KZ_BLOCK + threadIdx.x; p < nPix; p += gridDim.x * KZ_BLOCK) {
        const uint32_t px = framePixelOf(pixList[p], width);
        KzMatteRegs r0 = {}, r1 = {};
        if (t0) matteLoad(t0 + px, r0);
        if (two) matteLoad(t1 + px, r1);
        for (uint32_t s = 0; s < S; ++s) {
            bool isHit; uint32_t k0, k1;
            matteItemKeys<SRC>(shade, hit, keys, p * S + s, true, isHit, k0, k1);
            if (t0) matteCount(r0, isHit, k0);
            if (two) matteCount(r1, isHit, k1);
        }
        if (t0) matteStore(t0 + px, r0);
        if (two) matteStore(t1 + px, r1);
    }
}

// ---- what reads a table: one lane per frame pixel, i < nPixels = width * height
__device__ __forceinline__ bool matteBefore(uint32_t ca, uint32_t ia, uint32_t cb, uint32_t ib) { return ca > cb || (ca == cb && ia < ib); }      // count descending, ties to the lower id

// The record with its slots ranked - count descending, ties to the lower id, free slots (count 0, id 0) last - through the 16 compare-exchanges of a 7-entry
// sorting network.
__global__ __launch_bounds__(KZ_BLOCK) void kz_matte_rank_kernel(const KzMatteTexel *__restrict__ table, size_t nPixels, KzMatteTexel *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (i >= nPixels) return;
    KzMatteRegs r; matteLoad(table + i, r);
#define KZ_MATTE_CX(a, b) { if (matteBefore(r.cnt[b], r.id[b], r.cnt[a], r.id[a])) { const uint32_t c_ = r.cnt[a], i_ = r.id[a]; r.cnt[a] = r.cnt[b]; r.id[a] = r.id[b]; r.cnt[b] = c_; r.id[b] = i_; } }
    KZ_MATTE_CX(0, 6) KZ_MATTE_CX(2, 3) KZ_MATTE_CX(4, 5)
    KZ_MATTE_CX(0, 2) KZ_MATTE_CX(1, 4) KZ_MATTE_CX(3, 6)
    KZ_MATTE_CX(0, 1) KZ_MATTE_CX(2, 5) KZ_MATTE_CX(3, 4)
    KZ_MATTE_CX(1, 2) KZ_MATTE_CX(4, 6)
    KZ_MATTE_CX(2, 3) KZ_MATTE_CX(4, 5)
    KZ_MATTE_CX(1, 2) KZ_MATTE_CX(3, 4) KZ_MATTE_CX(5, 6)
#undef KZ_MATTE_CX
    matteStore(out + i, r);
}

// One id's coverage: (float)count / (float)total, one IEEE division; 0 where the id has no slot or the pixel no samples.
__global__ __launch_bounds__(KZ_BLOCK) void kz_matte_layer_kernel(const KzMatteTexel *__restrict__ table, size_t nPixels, uint32_t id, float *__restrict__ coverage) {
    const size_t i = (size_t)blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (i >= nPixels) return;
    KzMatteRegs r; matteLoad(table + i, r);
    uint32_t total = r.other + r.miss, count = 0u;
#pragma unroll
    for (int j = 0; j < KZ_MATTE_SLOTS; ++j) { total += r.cnt[j]; if (r.cnt[j] != 0u && r.id[j] == id) count = r.cnt[j]; }
    coverage[i] = total ? (float)count / (float)total : 0.0f;          // (a correctly rounded division: hipcc's default for fp32; both operands and the quotient are normal or 0)
}

// The id with the largest count, ties to the lower id; KZ_MATTE_NONE where miss is at least that count or the pixel has no samples.
__global__ __launch_bounds__(KZ_BLOCK) void kz_matte_top_kernel(const KzMatteTexel *__restrict__ table, size_t nPixels, uint32_t *__restrict__ ids) {
    const size_t i = (size_t)blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (i >= nPixels) return;
    KzMatteRegs r; matteLoad(table + i, r);
    uint32_t bestCnt = 0u, bestId = KZ_MATTE_NONE;
#pragma unroll
    for (int j = 0; j < KZ_MATTE_SLOTS; ++j) if (r.cnt[j] != 0u && matteBefore(r.cnt[j], r.id[j], bestCnt, bestId)) { bestCnt = r.cnt[j]; bestId = r.id[j]; }
    ids[i] = (bestCnt == 0u || r.miss >= bestCnt) ? KZ_MATTE_NONE : bestId;
}
