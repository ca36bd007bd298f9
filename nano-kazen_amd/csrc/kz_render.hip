// kz_render.hip - the device side of kz_render / kz_render_tiles: the launch code of a pass (wfPass: the wavefront pipeline of kz_wavefront.h - camera rays by
// pixel beams, persistent BVH4 traversal with Moeller-Trumbore leaf tests, post-intersection, BSDF eval + sample, MIS next-event estimation with the
// invisible-light walk-through, Russian roulette - and the reference-shaped megakernel below), the tables that pick the kernels, and renderOn:
// plan (kz_plan.cpp) -> make room (kz_arena.cpp) -> launch -> film (kz_film.hip). The replicas a pass runs on are kz_replica.hip's.
// Reference region replaced: src/kazen/renderer.cpp:85-133 and everything it calls.
//
// Execution model (wave64): one lane = one (pixel, sample) path; items are ordered pixel-major so the lanes of a wave share a pixel neighbourhood (coherent
// camera rays, shared top-of-tree node packets in L1 / L2). Per-lane traversal stacks live in LDS ([entry][lane]: conflict-free columns). No MFMA: this is
// branchy pointer chasing, bound by VALU issue and the CU's L1 gather rate, not a contraction.
#include <hip/hip_runtime.h>

#include "kz_devfn.h"
#include "kz_wavefront.h"
#include "kz_integrators.h"
#include "kz_aov.h"
#include "kz_state.h"
#include "../../include/kazen_mi355x_variance.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

// a1/a2 renderBlock + renderSample (renderer.cpp:20-69): item = pixLinear * S + sampleOffset
template <bool STATS, int EXT>
__global__ __launch_bounds__(KZ_BLOCK) void kz_path_megakernel(KzParams P, KzDevTables T, const uint32_t *__restrict__ pixList,
                                                               uint32_t nItems, uint32_t S, uint32_t sampleBegin, const uint32_t *__restrict__ itemSample,
                                                               float *__restrict__ outJx, float *__restrict__ outJy, float *__restrict__ outR,
                                                               float *__restrict__ outG, float *__restrict__ outB,
                                                               unsigned long long *__restrict__ stats) {
    __shared__ uint32_t s_stack[KZ_STACK_DEPTH * KZ_BLOCK];
    const uint32_t item = blockIdx.x * KZ_BLOCK + threadIdx.x;
    Counters cn = {0, 0, 0, 0, 0, 0};
    if (item < nItems) {
        const uint32_t pl = item / S, so = item - pl * S;
        int px, py; pixelOf(pixList[pl], px, py);
        Sampler smp; float jx, jy; V3 ro, rd; float mint, maxt;
        cameraSample(P, T, px, py, itemSample ? itemSample[item] : sampleBegin + so, smp, jx, jy, ro, rd, mint, maxt);
        V3 L = pathLi<STATS, EXT>(P, T, smp, ro, rd, mint, maxt, s_stack + threadIdx.x, cn);
        outJx[item] = jx; outJy[item] = jy; outR[item] = L.x; outG[item] = L.y; outB[item] = L.z;
        if (STATS) {
            bool valid = L.x >= 0 && L.y >= 0 && L.z >= 0 && isfinite(L.x) && isfinite(L.y) && isfinite(L.z);
            if (!valid) cn.dropped++;
        }
    }
    if (STATS) statsFlush(stats, cn, item < nItems ? 1u : 0u);
}

// KzTuning -> the kernels' KzTune. Zero = the library default. (The KZ_* environment overrides of ABI v2 / v3 are gone: nothing in the
// library reads the environment.) dev0 .. dev5 selected the kernels of rejected experiments, which are gone: the values that did are
// refused loudly instead of ignored.
static int resolveTune(const KzTuning &t, KzTune &r) {
    auto pick = [](int a, int d) { return a > 0 ? a : d; };
    r = KzTune{};
    r.refill = pick(t.refill, 0); r.postpone = pick(t.postpone, 24); r.batch = pick(t.batch, 0);                      // 0: the default per ray kind (wfPass)
    r.travBlocksPerCU = std::min(8, pick(t.traceBlocksPerCU, KZ_TRACE_WAVES)); r.shadeBlocksPerCU = std::min(16, pick(t.shadeBlocksPerCU, 0));
    r.ldsStack = pick(t.ldsStack, 16);
    r.packet = pick(t.packetPrimary, 0); r.filmGather = pick(t.filmGather, 0);
    if (t.dev0 || t.dev1 > 0 || t.dev2 > 0 || t.dev3 > 1 || t.dev4 > 0 || t.dev5 > 0)
        return kz_fail(KZ_ERR_UNSUPPORTED, "KzTuning.dev0 .. dev5 are reserved: the kernels of rejected experiments they selected (LAB_NOTES 4) have been removed");
    r.ovf = nullptr; r.ovfStride = 0;
    return KZ_OK;
}

static int stageMark(PassCtx &c, hipStream_t stream, int kind) {
    if (c.stageUsed == c.stageEv.size()) { Event e; if (const int rc = e.ensure()) return rc; c.stageEv.push_back(std::move(e)); c.stageKind.push_back(0); }
    c.stageKind[c.stageUsed] = kind;
    HIP_TRY(hipEventRecord(c.stageEv[c.stageUsed++], stream));
    return KZ_OK;
}

// Path state per (pixel, sample) item of a pass in flight: 8 float4 + uint4 + 3 queue words (wavefront) + 5 sample floats.
static constexpr size_t KZ_STATE_BYTES_PER_ITEM = 8 * sizeof(float4) + sizeof(uint4) + 3 * sizeof(uint32_t);
static constexpr size_t KZ_SAMPLE_BYTES_PER_ITEM = 5 * sizeof(float);

// The kernels' pointers of a context (or of a view of it, a pass in halves) into the arena's arrays, from item `off` on; the counters are the context's (view's) own.
static void ctxPoint(PassCtx &c, const KzArena &A, size_t off) {
    KzWf W{};
    W.rayA.p = A.array<float4>(0) + off; W.rayB.p = A.array<float4>(1) + off; W.hit.p = A.array<float4>(2) + off; W.thr.p = A.array<float4>(3) + off;
    W.misc.p = A.array<float4>(4) + off; W.shA.p = A.array<float4>(5) + off; W.shB.p = A.array<float4>(6) + off; W.shL.p = A.array<float4>(7) + off;
    W.smp = A.array<uint4>(8) + off;
    for (int q = 0; q < 3; ++q) W.queue[q] = A.array<uint32_t>(9 + q) + off;
    W.counts = c.counts;
    c.wf = W;
    for (int k = 0; k < 5; ++k) c.plane[k] = A.array<float>(12 + k) + off;
}

// ---- buffers of one pass context. The path-state arrays and the sample planes live in the context's arena (kz_arena.cpp), which GROWS on a side
// thread: `want` items are asked for, the call returns as soon as `minItems` are there and the arena has stopped making quick progress (graceMs; < 0: wait
// for everything), and tells how many items a pass may use now (*usable, never more than `want`). Nothing is left half-allocated on failure. ----
static int ctxEnsure(PassCtx &c, size_t want, size_t minItems, double graceMs, hipStream_t stream, size_t *usable) {
    if (!c.counts) { if (const int rc = c.counts.alloc(KzCounts::kWords)) return rc; }
    KzArena &A = *c.arena;
    if (A.wouldReallocate(want)) HIP_TRY(hipDeviceSynchronize());      // (a small context outgrown, or a pass beyond the reserved ranges: what is there is given up first)
#ifdef KZ_EXPERIMENTS
    if (g_failAlloc > 0) { A.failCountdown.store(g_failAlloc); g_failAlloc = 0; }      // (kz_debug_fail_alloc counts the arena's physical allocations as this thread's)
#endif
    size_t got = 0;
    const int rc = A.request(want, minItems, graceMs, &got);
#ifdef KZ_EXPERIMENTS
    // what the call did not use up stays armed ON THE ARENA while its growth thread is still mapping levels (the thread is where the allocations of a growing
    // context happen: ADVICE r05 - the count used to be taken back here, so a failure injected beyond the first levels never fired)
    { std::lock_guard<std::mutex> g(A.m); if (!A.busy) g_failAlloc = A.failCountdown.exchange(0); }
#endif
    if (rc) return rc;
    ctxPoint(c, A, 0);
    *usable = std::min(got, want);
    return KZ_OK;
}

// kz_wf_trace instantiations by (mode, stats): the launch code picks from this table instead of a ladder of macros
static decltype(&kz_wf_trace<0, false>) traceFn(int mode, bool stats, bool late) {
    // the bounces behind kz_wf_compact (wfMis): the instantiations that take their per-path arrays from the device (modes 0 / 2 / 4: what a bounce loop launches)
    if (late) {
        constexpr int L = KZ_MODE_LATE;
        static const decltype(&kz_wf_trace<0, false>) ltab[5][2] = {{kz_wf_trace<L, false>, kz_wf_trace<L, true>}, {nullptr, nullptr},
                                            {kz_wf_trace<L + 2, false>, kz_wf_trace<L + 2, true>}, {nullptr, nullptr}, {kz_wf_trace<L + 4, false>, kz_wf_trace<L + 4, true>}};
#ifdef KZ_EXPERIMENTS
        if (mode == 4 && !g_kzShadowOrder.load(std::memory_order_relaxed)) return stats ? kz_wf_trace<L + 5, true> : kz_wf_trace<L + 5, false>;
#endif
        return ltab[mode][stats ? 1 : 0];
    }
    static const decltype(&kz_wf_trace<0, false>) tab[5][2] = {{kz_wf_trace<0, false>, kz_wf_trace<0, true>}, {kz_wf_trace<1, false>, kz_wf_trace<1, true>},
                                        {kz_wf_trace<2, false>, kz_wf_trace<2, true>}, {nullptr, nullptr}, {kz_wf_trace<4, false>, kz_wf_trace<4, true>}};
#ifdef KZ_EXPERIMENTS
    // kz_debug_shadow_order(0): the any-hit shadow launches in the closest-hit child order (mode 5, a development build's instantiation)
    if (mode == 4 && !g_kzShadowOrder.load(std::memory_order_relaxed)) return stats ? kz_wf_trace<5, true> : kz_wf_trace<5, false>;
#endif
    return tab[mode][stats ? 1 : 0];
}
// ... and the camera-ray kernels by (stats, fix): FIX = the scene has an invisible light, whose first hits are queued for the walk-through
static decltype(&kz_wf_trace_list<false, false>) listFn(bool stats, bool fix) {
    static const decltype(&kz_wf_trace_list<false, false>) tab[2][2] = {{kz_wf_trace_list<false, false>, kz_wf_trace_list<false, true>}, {kz_wf_trace_list<true, false>, kz_wf_trace_list<true, true>}};
    return tab[stats ? 1 : 0][fix ? 1 : 0];
}
static decltype(&kz_wf_trace_packet<false, false>) packetFn(bool stats, bool fix) {
    static const decltype(&kz_wf_trace_packet<false, false>) tab[2][2] = {{kz_wf_trace_packet<false, false>, kz_wf_trace_packet<false, true>}, {kz_wf_trace_packet<true, false>, kz_wf_trace_packet<true, true>}};
    return tab[stats ? 1 : 0][fix ? 1 : 0];
}
// The shade kernels are compiled for what the scene's BSDF rows need (KzParams::bsdfExt): nothing beyond diffuse / kiss (0), other models only (KZ_X_MODELS), or
// `all` the integrator knows - KZ_X_ALL for path_mis (textures, normal maps), KZ_X_MATS for path_mats (no normal maps). The tables below are indexed by that value.
static int extSel(int bsdfExt, int all) { return bsdfExt == 0 ? 0 : (bsdfExt == KZ_X_MODELS ? KZ_X_MODELS : all); }
static int extCol(int ext) { return ext == 0 ? 0 : (ext == KZ_X_MODELS ? 1 : 2); }
typedef decltype(&kz_wf_shade<false, 0>) KzShadeFn;
static KzShadeFn shadeFn(bool stats, int ext, bool late = false) {      // ext: 0 / KZ_X_MODELS / KZ_X_ALL; late: the bounces behind kz_wf_compact (wfMis)
    static const KzShadeFn tab[2][3] = {{kz_wf_shade<false, 0>, kz_wf_shade<false, KZ_X_MODELS>, kz_wf_shade<false, KZ_X_ALL>}, {kz_wf_shade<true, 0>, kz_wf_shade<true, KZ_X_MODELS>, kz_wf_shade<true, KZ_X_ALL>}};
    constexpr int L = KZ_X_LATE;
    static const KzShadeFn ltab[2][3] = {{kz_wf_shade<false, L>, kz_wf_shade<false, L | KZ_X_MODELS>, kz_wf_shade<false, L | KZ_X_ALL>}, {kz_wf_shade<true, L>, kz_wf_shade<true, L | KZ_X_MODELS>, kz_wf_shade<true, L | KZ_X_ALL>}};
    return (late ? ltab : tab)[stats ? 1 : 0][extCol(ext)];
}
typedef decltype(&kz_wf_mats<0>) KzMatsFn;
static KzMatsFn matsFn(int ext) {                    // ext: 0 / KZ_X_MODELS / KZ_X_MATS
    static const KzMatsFn tab[3] = {kz_wf_mats<0>, kz_wf_mats<KZ_X_MODELS>, kz_wf_mats<KZ_X_MATS>};
    return tab[extCol(ext)];
}
// ... and the reference-shaped megakernels (pipeline 1, kz_render_samples), which have no "other models only" variant
typedef decltype(&kz_path_megakernel<false, 0>) KzMegaFn;
static KzMegaFn megaFn(bool stats, int ext) {        // ext: 0 / KZ_X_ALL
    static const KzMegaFn tab[2][2] = {{kz_path_megakernel<false, 0>, kz_path_megakernel<false, KZ_X_ALL>}, {kz_path_megakernel<true, 0>, kz_path_megakernel<true, KZ_X_ALL>}};
    return tab[stats ? 1 : 0][ext ? 1 : 0];
}
typedef decltype(&kz_integrator_megakernel<KZ_INTEGRATOR_NORMALS, 0>) KzIntegratorMegaFn;
static KzIntegratorMegaFn integratorMegaFn(int integrator, int ext) {      // normals / ao / path_mats; ext: 0 / KZ_X_MATS
    static const KzIntegratorMegaFn tab[3][2] = {{kz_integrator_megakernel<KZ_INTEGRATOR_NORMALS, 0>, kz_integrator_megakernel<KZ_INTEGRATOR_NORMALS, KZ_X_MATS>},
                                                 {kz_integrator_megakernel<KZ_INTEGRATOR_AO, 0>, kz_integrator_megakernel<KZ_INTEGRATOR_AO, KZ_X_MATS>},
                                                 {kz_integrator_megakernel<KZ_INTEGRATOR_PATH_MATS, 0>, kz_integrator_megakernel<KZ_INTEGRATOR_PATH_MATS, KZ_X_MATS>}};
    return tab[integrator == KZ_INTEGRATOR_NORMALS ? 0 : (integrator == KZ_INTEGRATOR_AO ? 1 : 2)][ext ? 1 : 0];
}

// Beam lists for pixels [p0, p0 + n) of the current pixel list: launched on `stream` (the call's stream) unless that range of this list has been
// handed to the kernel before; the kernel itself skips pixels that already have a list (from another tile set or chunk). evBeam / beamSeq tell the
// pass streams what to wait for.
static int ensureBeamBuffers(KzScene *scene, KzDeviceState *ds, hipStream_t stream) {
    const KzParams &P = scene->prm;
    const size_t framePix = (size_t)P.width * P.height;
    int rc;
    if ((rc = ds->evBeam.ensure(hipEventDisableTiming))) return rc;
    if (!ds->beamEntries || !ds->beamCount) {
        if (!ds->beamEntries && (rc = ds->beamEntries.alloc(framePix * KZ_BEAM_CAP))) return rc;
        if (!ds->beamCount && (rc = ds->beamCount.alloc(framePix))) return rc;
        HIP_TRY(hipMemsetAsync(ds->beamCount, 0xFF, framePix * sizeof(uint2), stream));       // every pixel: KZ_BEAM_UNBUILT
        ds->beamDone.clear(); ds->beamDoneGen = ds->tileGen;
    }
    return KZ_OK;
}
static int ensureBeams(KzScene *scene, KzDeviceState *ds, hipStream_t stream, uint32_t p0, uint32_t n) {
    const KzParams &P = scene->prm;
    { const int rc_ = ensureBeamBuffers(scene, ds, stream); if (rc_) return rc_; }
    if (ds->beamDoneGen != ds->tileGen) { ds->beamDone.clear(); ds->beamDoneGen = ds->tileGen; }
    for (const auto &r : ds->beamDone) if (r.first <= p0 && p0 + n <= r.first + r.second) return KZ_OK;
    const int LS = std::max(1, std::min(P.stackBound4, KZ_BEAM_STACK));      // a beam whose open set would grow beyond this leaves the rest unexplored (t_valid)
    const dim3 gBeam((n + KZ_BLOCK - 1) / KZ_BLOCK);
    const size_t beamLds = (size_t)2 * LS * KZ_BLOCK * sizeof(uint32_t);
    hipLaunchKernelGGL(kz_wf_beam, gBeam, dim3(KZ_BLOCK), beamLds, stream, P, ds->T, (const uint32_t *)(ds->pixList + p0), n, LS, ds->beamEntries, ds->beamCount);
    if (ds->statsOn) hipLaunchKernelGGL(kz_wf_beam_count, gBeam, dim3(KZ_BLOCK), 0, stream, (const uint2 *)ds->beamCount, (const uint32_t *)(ds->pixList + p0), P.width, n, ds->stats + 24);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ds->evBeam, stream));
    ++ds->beamSeq;
    ds->beamDone.emplace_back(p0, n);
    return KZ_OK;
}

// The launch shape of the persistent traversal kernels on a scene: the grids, the per-lane stack's split between LDS and the global overflow area, the
// batch of the packet kernel. ONE statement of it for every caller - the passes (wfPass, ensureOverflow) and the ray-level entry of the development surface
// (kz_trace_rays_wf), which exists to run the very launches a render makes on a caller's rays.
#define KZ_PACKET_BATCH 8                  // packets a wave of the packet kernel claims per reservation
static unsigned travGridBlocks(const KzDeviceState *ds, const KzTune &tune) { return (unsigned)(ds->numCU * tune.travBlocksPerCU); }
static unsigned packetGridBlocks(const KzDeviceState *ds) { return (unsigned)(ds->numCU * 8); }      // the packet kernel is compiled for 8 waves per SIMD whatever KZ_TRACE_WAVES is
static bool packetFits(const KzParams &P) { return P.stackBound4 <= 128; }                            // its stack is two VGPRs: 128 entries
struct TraceShape {
    int ldsStack;            // entries per lane in LDS: tune.ldsStack clamped to [2, the builder's worst case]
    size_t traceLds;         // bytes of dynamic LDS per workgroup: + one scratch slot per lane (branch-free pushes)
    uint32_t ovfStride;      // words per overflow row: one per thread of the grid
    size_t ovfRows, ovfPart; // rows, and words, one launch's stacks may spill into: the rest of the worst case (known from the builder)
};
static TraceShape traceShape(const KzParams &P, unsigned gridBlocks, int ldsStackAsked) {
    TraceShape s;
    const int stackBound = std::max(P.stackBound4, 2);
    s.ldsStack = std::max(2, std::min(ldsStackAsked, stackBound));
    s.traceLds = (size_t)(s.ldsStack + 1) * KZ_BLOCK * sizeof(uint32_t);
    s.ovfStride = (uint32_t)((size_t)gridBlocks * KZ_BLOCK);
    s.ovfRows = (size_t)std::max(1, stackBound - s.ldsStack);
    s.ovfPart = (size_t)s.ovfStride * s.ovfRows;
    return s;
}
// One kz_wf_trace launch: mode 0 / 1 / 2 / 4 on queue q (nullptr: identity) of *cptr (nullptr: cimm) entries, with the defaults a tuning leaves open.
static void launchTrace(int mode, bool stats, dim3 grid, size_t traceLds, hipStream_t on, const KzParams &P, const KzDevTables &T, const KzWf &W, const uint32_t *q, const uint32_t *cptr,
                        uint32_t cimm, uint32_t *head, KzTune t, uint32_t *qb, uint32_t *cb, const KzWfLate *sel = nullptr) {
    if (t.batch <= 0) t.batch = 128;                 // (the least a wave reserves per global atomic: kz_wf_trace asks for more while much is left)
    // idle lanes are refilled once fewer than this many are busy. A refill of the shadow kernel is the dearer one (the invisible-light test of every new
    // ray), so it waits for more idle lanes: same-call sweep, shadow stage 21.7 / 20.9 / 20.9 ms at 40 / 32 / 28 on C3, 20.3 / 20.0 / 20.3 on C4; the
    // closest-hit kernel 32.85 / 33.3 / 34.2 on C4
    if (t.refill <= 0) t.refill = (mode == 2 || mode == 4) ? 32 : 40;
    hipLaunchKernelGGL(traceFn(mode, stats, sel != nullptr), grid, dim3(KZ_BLOCK), traceLds, on, P, T, W, q, cptr, cimm, head, t, qb, cb, sel);      // (sel: the per-path arrays are the ones *sel names - wfMis, behind kz_wf_compact)
}
// The shadow rays of queue q: with P.shadowFast the any-hit kernel without the walk-through machinery; the (rare) rays whose segment crosses an
// invisible-light triangle go to litQ and are walked through by the general kernel. Without it the general kernel takes everything.
// trace(mode, q, cptr, cimm, head, qb, cb) launches.
template <class Trace>
static void shadowLaunches(const KzParams &P, Trace &&trace, const uint32_t *q, const uint32_t *cptr, uint32_t cimm, uint32_t *head, uint32_t *litQ, uint32_t *litCount, uint32_t *litHead) {
    if (P.shadowFast) {
        trace(4, q, cptr, cimm, head, litQ, litCount);
        if (P.anyInvisibleLight) trace(2, (const uint32_t *)litQ, (const uint32_t *)litCount, 0u, litHead, (uint32_t *)nullptr, (uint32_t *)nullptr);
    } else trace(2, q, cptr, cimm, head, (uint32_t *)nullptr, (uint32_t *)nullptr);
}

// The global overflow area of the traversal stacks (entries beyond tune.ldsStack per lane, sized from the builder's worst-case bound) of one pass context.
static int ensureOverflow(KzScene *scene, KzDeviceState *ds, PassCtx &c, const KzTune &tune, hipStream_t stream) {
    const size_t needOvf = traceShape(scene->prm, travGridBlocks(ds, tune), tune.ldsStack).ovfPart * 3;      // (x 3: part 0 the pass's own stream, part 1 spare, part 2 the shadow kernels of a small pass on the side stream, wfPass)
    if (needOvf <= c.ovf.cap()) return KZ_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    return c.ovf.regrow(needOvf);
}

// The dense set of a pass: a second, small set of the per-path arrays for the late bounces of a path_mis pass (kz_wavefront.h kz_wf_compact; wfMis). It costs no
// memory: it lies INSIDE the pass's own `hit` array, 16 B per item, which is dead from shade(2)'s last read on if the late bounces move out - their closest-hit
// launches store into the dense set's hit records - and is not touched at all if they stay (kz_wf_compact decides before it writes; the shadow rays of bounce 2,
// which may still run beside it, read shA / shB / shL and the shadow queue). An entry is the seven records every bounce needs (ray A / B, hit, throughput, shadow
// A / B / L), misc and the sampler words where the kernels keep them, and the origin word: 116 - 148 B, so the set holds 16 / 116 = 13.8 % (lean kernels,
// pmj02bn: C4) to 10.8 % of the pass's items. Measured with kz_debug_trace on passes of 1920 x 1080 x 64 items of the two scenes whose late bounces weigh most
// (profiles/r20a_compact/README.md): shade(2) queues 9.0 % of C4's items for bounce 3 (11.92 M of 132.7 M) and 10.4 % of C3's (13.86 M; lean, independent:
// 12.1 % fit). A pass whose survivors do not fit goes on in its own arrays (decided on the device).
// What the late launches read from the device - which arrays, and the origins - is the pass's one KzWfLate, in the counter block (KzCounts::kLate).
#define KZ_DENSE_BOUNCE 3                  // the bounce in front of which the compaction runs: the first one that plays the roulette
struct DenseSet { KzWf D; uint32_t *origin; uint32_t cap; int withMisc, withSampler; };
static DenseSet denseSetOf(const KzParams &P, const KzWf &W, uint32_t items) {
    DenseSet s;
    s.withMisc = (P.bsdfExt || P.regularization) ? 1 : 0;      // (kz_wf_shade's `compact` state has no misc record)
    s.withSampler = P.samplerType == KZ_SAMPLER_PMJ02BN ? 0 : 1;      // (pmj02bn has no sampler record: wfLoadSampler)
    const size_t rec = 7 * sizeof(float4) + sizeof(uint32_t) + (s.withMisc ? sizeof(float4) : 0) + (s.withSampler ? sizeof(uint4) : 0);
    const size_t n = s.cap = (uint32_t)((size_t)items * sizeof(float4) / rec);
    float4 *f = W.hit.p;
    s.D = W;                               // (the queues, the counters, the sample sums and the statistics are the pass's)
    s.D.rayA.p = f; s.D.rayB.p = f + n; s.D.hit.p = f + 2 * n; s.D.thr.p = f + 3 * n; s.D.shA.p = f + 4 * n; s.D.shB.p = f + 5 * n; s.D.shL.p = f + 6 * n;
    f += 7 * n;
    s.D.misc.p = f; if (s.withMisc) f += n;                    // (a record the kernels do not keep gets no room, and nobody follows its pointer)
    s.D.smp = (uint4 *)f; if (s.withSampler) f += n;
    s.origin = (uint32_t *)f;
    return s;
}

// What the launches of one wfPass share: the stream, the kernels' arguments, the grids.
struct WfLaunch {
    KzDeviceState *ds; PassCtx &c; hipStream_t stream;
    KzParams P; KzDevTables Tsh; KzWf W; KzTune tune;
    const uint32_t *pixList; uint32_t items, Sp, sBegin; bool st;      // st: the counters run
    dim3 blk, gItems, gTrav, gShade, gPacket;
    size_t traceLds, ovfPart;
    bool dense = false;                                                // this pass compacts its survivors in front of the first roulette bounce (wfPass: path_mis with such a bounce to come)
    const KzWfLate *sel = nullptr;                                     // set by wfMis behind kz_wf_compact: the launches from there on take their per-path arrays from *sel
    int mark(int kind) { return stageMark(c, stream, kind); }
    // mode 0 / 1 / 2 / 4 of kz_wf_trace on queue q (nullptr: identity) of *cptr (nullptr: cimm) entries
    void trace(int mode, const uint32_t *q, const uint32_t *cptr, uint32_t cimm, uint32_t *head, uint32_t *qb, uint32_t *cb, hipStream_t on = nullptr) const {
        KzTune t = tune;
        const bool side = on != nullptr;                 // (a launch beside the pass's own stream walks its own part of the overflow area)
        if (side) t.ovf = tune.ovf + 2 * ovfPart; else on = stream;
        launchTrace(mode, st, gTrav, traceLds, on, P, ds->T, W, q, cptr, cimm, head, t, qb, cb, sel);
    }
};

// camera rays: pixel beams + per-sample triangle tests (kz_wf_beam / kz_wf_trace_list), the wave-level packet traversal
// (kz_wf_trace_packet) for what the beams cannot take, or the per-lane kernel on request; then the walk-through of first hits on an invisible light
static int wfCamera(WfLaunch &L, bool beams) {
    const KzParams &P = L.P; const KzWf &W = L.W; KzDeviceState *ds = L.ds; hipStream_t stream = L.stream;
    uint32_t *cam = W.counts + KzCounts::kCamera, *fixCount = cam + KzCounts::kPaths;      // (fixCount: first hits on an invisible light, in W.queue[2])
    const bool packet = L.tune.packet != 1 && packetFits(P), fix = P.anyInvisibleLight != 0;
    if (packet && beams) {
        // (the lists of this pass's pixels were handed to kz_wf_beam on the call's stream - ensureBeams - and this stream has waited for it)
        uint32_t *fbQ = W.queue[0], *fbCount = W.counts + KzCounts::kFallback, *fbHead = fbCount + 1;      // rays of pixels whose list overflowed: the packet kernel's
        hipLaunchKernelGGL(listFn(L.st, fix), L.gItems, L.blk, 0, stream, P, ds->T, W, L.pixList, L.items, L.Sp, (const uint2 *)ds->beamEntries, (const uint2 *)ds->beamCount,
                           fbQ, fbCount, W.queue[2], fixCount);
        hipLaunchKernelGGL(packetFn(L.st, fix), L.gPacket, L.blk, 0, stream, P, ds->T, W, (const uint32_t *)fbQ, (const uint32_t *)fbCount, 0u, fbHead, KZ_PACKET_BATCH, W.queue[2], fixCount);
    } else if (packet) {
        // (scenes with an invisible light: the epilogue queues the first hits on such a light for the walk-through launch below)
        hipLaunchKernelGGL(packetFn(L.st, fix), L.gPacket, L.blk, 0, stream, P, ds->T, W, (const uint32_t *)nullptr, (const uint32_t *)nullptr, L.items, cam + KzCounts::kBounceHead, KZ_PACKET_BATCH, W.queue[2], fixCount);
    } else {
        L.trace(0, nullptr, nullptr, L.items, cam + KzCounts::kBounceHead, nullptr, nullptr);
        if (fix) hipLaunchKernelGGL(kz_wf_primary_fix, L.gShade, L.blk, 0, stream, P, ds->T, W, L.items, W.queue[2], fixCount);
    }
    if (fix) L.trace(1, W.queue[2], fixCount, 0u, cam + KzCounts::kShadowHead, nullptr, nullptr);      // H6 walk-through of the first hit
    return L.mark(5);
}

// The feature films' stage of a pass (kazen_mi355x_aov.h), between the camera stage and the first shade / ao / mats launch: every item's first-hit record sits at
// its own slot of W.hit, and the shadow arrays shA / shB / shL are DEAD there - the camera stage's walk-through has consumed the rays it kept in shA / shB, and
// the next writers are the shade kernel (every slot it queues: kz_wavefront.h wfShade) and kz_wf_ao, each before its shadow kernel reads. Each array holds 16 B per
// item = room for the three float planes of one feature, so the planes alias them: albedo in shA, normal in shB, depth in shL (a view of a pass in halves points
// into its own part of every array, so the alias stays inside the view). No per-item array is added and the sample planes r / g / b are not touched.
// kz_wf_aov's variant follows P.bsdfExt as the shade kernel's does. Then one kz_film_taps<.., true> launch per enabled AOV into that AOV's own tap sums.
// ORDER: tap sums are read-modify-write per pixel and a pixel's samples must arrive in ascending sample order; with passes in flight the pass before this one,
// on another stream, touches the same pixels. The AOV stages have an event chain of their own (evAov: recorded behind a pass's AOV tap launches, waited for by
// the next pass's) - waiting for evFilm[prev], which is recorded at the END of the pass before, would serialise the passes.
// The film stage of a pass's pixels [pixList, +nPix) on `pst`: the picture's tap launch and, with the second-moment film switched on (kazen_mi355x_variance.h), that
// film's directly behind it - the same stream, pixel list and sample planes, inside the same evFilm chain - or the one launch that feeds both. Switch off: the
// picture's launch alone, as before the switch existed.
#define KZ_VARIANCE_DEFAULT_ONE_PASS 1      // what KZ_VARIANCE_ON means: the faster of the two forms on a C4 pass (2.74 against 2.94 ms of film stage)
static int filmStages(KzScene *scene, KzDeviceState *ds, hipStream_t pst, const uint32_t *pixList, uint32_t nPix, uint32_t Sp, const float *const plane[5], hipEvent_t waitFilm, int lanes) {
    const int mode = scene->varianceMode;
    if (!mode) return kzFilmStage(scene, ds, ds->picture(), false, pst, pixList, nPix, Sp, plane, waitFilm, lanes);
    const bool onePass = (mode == KZ_VARIANCE_ONE_PASS || (mode == KZ_VARIANCE_ON && KZ_VARIANCE_DEFAULT_ONE_PASS)) && kzFilmMomentOnePassOk(scene->prm);
    if (!onePass) if (const int rc = kzFilmStage(scene, ds, ds->picture(), false, pst, pixList, nPix, Sp, plane, waitFilm, lanes)) return rc;
    return kzFilmStageMoment(scene, ds, ds->picture(), ds->moment(), onePass, pst, pixList, nPix, Sp, plane, waitFilm);
}
static int filmLanes(const KzTune &tune) { return tune.filmGather == 3 ? 1 : 0; }      // kzFilmStage's lanesPerPixel: KzTuning.filmGather = 3 asks for one lane per pixel
typedef decltype(&kz_wf_aov<0>) KzAovFn;
static KzAovFn aovFn(int ext) {                      // ext: 0 / KZ_X_MODELS / KZ_X_ALL
    static const KzAovFn tab[3] = {kz_wf_aov<0>, kz_wf_aov<KZ_X_MODELS>, kz_wf_aov<KZ_X_ALL>};
    return tab[extCol(ext)];
}
static int wfAov(KzScene *scene, WfLaunch &L, hipEvent_t waitAov, hipEvent_t recordAov) {
    const KzWf &W = L.W; hipStream_t stream = L.stream;
    static_assert(sizeof(float4) >= 3 * sizeof(float), "a shadow array holds three float planes per item");
    const KzAovPlanes A = {{(float *)W.shA.p, (float *)W.shB.p, (float *)W.shL.p}, (size_t)L.items};
    const dim3 grid(std::min(L.gItems.x, (unsigned)(L.ds->numCU * 8)));
    hipLaunchKernelGGL(aovFn(extSel(L.P.bsdfExt, KZ_X_ALL)), grid, L.blk, 0, stream, L.ds->T, W, L.items, scene->aovMask, A);
    HIP_TRY(hipGetLastError());
    if (waitAov) HIP_TRY(hipStreamWaitEvent(stream, waitAov, 0));
    for (int f = 0; f < 3; ++f) {                       // one kz_film_taps<.., true> launch per enabled AOV, in ascending order
        if (!(scene->aovMask & (1u << f))) continue;
        KzFilm &film = L.ds->aov(f);
        if (!film.sums) return kz_fail(KZ_ERR_STATE, "the tap sums of AOV %u are not there", 1u << f);
        const float *const plane[5] = {W.outJx, W.outJy, A.p[f], A.p[f] + A.stride, A.p[f] + 2 * A.stride};
        if (const int rc = kzFilmStage(scene, L.ds, film, true, stream, L.pixList, L.items / L.Sp, L.Sp, plane, nullptr, filmLanes(L.tune))) return rc;
    }
    if (recordAov) HIP_TRY(hipEventRecord(recordAov, stream));
    return L.mark(4);                                   // (the stage clock books the AOV launches under "film")
}
// The ID mattes' stage of a pass (kazen_mi355x_matte.h; kz_matte.hip), in the same place and for the same reason: the first-hit records are at their own slots of
// W.hit. It adds no per-item state and reads nothing the AOV stage writes. ORDER: a pixel's record is read-modify-write and its samples are counted in ascending
// order, so with passes in flight the stage has an event chain of its own (evMatte), exactly as evAov - not evAov's events: that stage may be off.
static int wfMatte(KzScene *scene, WfLaunch &L, hipEvent_t waitMatte, hipEvent_t recordMatte) {
    if (const int rc = kzMatteStage(scene, L.ds, L.stream, L.W.hit.p, L.pixList, L.items / L.Sp, L.Sp, waitMatte, recordMatte)) return rc;
    return L.mark(4);                                   // (booked under "film" too)
}

//   path_mats  { kz_wf_mats(iter) -> kz_wf_trace<0> } until the path queue is empty or 512 bounces are done; the host reads the survivor count back
//              after every 4th bounce (one stream synchronisation per 4 bounces), so a pass launches 2 + 2 x (bounces rounded up to 4) kernels after the camera's.
static int wfMats(WfLaunch &L) {
    int rc;
    const KzParams &P = L.P; const KzWf &W = L.W; hipStream_t stream = L.stream;
    const KzMatsFn mats = matsFn(extSel(P.bsdfExt, KZ_X_MATS));
    const uint32_t *cur = nullptr, *curCount = nullptr;
    for (int iter = 0; iter < P.maxDepth; ++iter) {
        uint32_t *nextQ = W.queue[iter & 1], *nextCount = W.counts + KzCounts::quad(iter);
        hipLaunchKernelGGL(mats, L.gShade, L.blk, 0, stream, P, L.ds->T, W, L.pixList, L.Sp, L.sBegin, iter, cur, curCount, cur ? 0u : L.items, nextQ, nextCount);
        if ((rc = L.mark(2))) return rc;
        if (iter == P.maxDepth - 1) break;                    // (the ray of the last bounce is not traced: H15)
        if ((iter & 3) == 3) {                                // the queue runs dry long before the cap: stop launching when it has
            uint32_t left = 0;
            HIP_TRY(hipMemcpyAsync(&left, nextCount, sizeof left, hipMemcpyDeviceToHost, stream)); HIP_TRY(hipStreamSynchronize(stream));
            if (left == 0) break;
        }
        L.trace(0, nextQ, nextCount, 0u, nextCount + KzCounts::kBounceHead, nullptr, nullptr);
        if ((rc = L.mark(1))) return rc;
        cur = nextQ; curCount = nextCount;
    }
    return KZ_OK;
}

// path_mis: one shade kernel per bounce, then its shadow rays and its closest-hit rays, `beside` as the planner decided (kz_plan.h); the same film either way
static int wfMis(WfLaunch &L, bool beside) {
    int rc;
    const KzParams &P = L.P; const KzWf &W = L.W; PassCtx &c = L.c; hipStream_t stream = L.stream;
    L.ds->lastInfo.shadowBeside = beside ? 1u : 0u;      // (what the last pass did: kz_last_pass_info)
    if (beside && ((rc = c.side.ensure(hipStreamNonBlocking)) || (rc = c.evFork.ensure(hipEventDisableTiming)) || (rc = c.evJoin.ensure(hipEventDisableTiming)))) return rc;
    const KzShadeFn shade = shadeFn(L.st, extSel(P.bsdfExt, KZ_X_ALL));
    const KzShadeFn shadeLate = shadeFn(L.st, extSel(P.bsdfExt, KZ_X_ALL), true);
    const uint32_t *cur = nullptr, *curCount = nullptr;
    for (int iter = 0; iter < P.maxDepth; ++iter) {
        // one kernel per bounce: the path queues ping-pong (W.queue[iter & 1] is written, the other one read)
        uint32_t *nextQ = W.queue[iter & 1], *nextCount = W.counts + KzCounts::quad(iter), *shQ = W.queue[2], *shCount = nextCount + KzCounts::kShadows;
        hipLaunchKernelGGL(L.sel ? shadeLate : shade, L.gShade, L.blk, 0, stream, P, L.Tsh, W, L.pixList, L.Sp, L.sBegin, iter, cur, curCount, L.items, nextQ, nextCount, shQ, shCount, L.sel);
        const bool needExtend = iter < P.maxDepth - 1 || P.bgPresent;
        if ((rc = L.mark(2))) return rc;
        // `beside`: this bounce's shadow rays go to the context's side stream and run beside its closest-hit rays; the next shade
        // waits for both. (What the two kernels write is disjoint: the shadow kernels add to the sample sums and use the path queue the shade has just
        // consumed; the closest-hit kernel stores hit records and reads the other path queue.)
        hipStream_t shOn = nullptr;
        if (beside && needExtend) { HIP_TRY(hipEventRecord(c.evFork, stream)); HIP_TRY(hipStreamWaitEvent(c.side, c.evFork, 0)); shOn = c.side; }
        if (P.nLights > 0) {
            // (the queue of the rays that cross an invisible-light triangle is the ping-pong path queue this bounce's shade has just consumed)
            uint32_t *litQ = W.queue[(iter & 1) ^ 1], *litCount = W.counts + KzCounts::lit(iter), *litHead = litCount + 1;
            shadowLaunches(P, [&](int mode, const uint32_t *q, const uint32_t *cptr, uint32_t cimm, uint32_t *head, uint32_t *qb, uint32_t *cb) { L.trace(mode, q, cptr, cimm, head, qb, cb, shOn); },
                           shQ, shCount, 0u, nextCount + KzCounts::kShadowHead, litQ, litCount, litHead);
        }
        if (shOn) HIP_TRY(hipEventRecord(c.evJoin, c.side));
        if ((rc = L.mark(3))) return rc;
        if (iter == KZ_DENSE_BOUNCE - 1 && L.dense) {
            // Once per pass, in front of the first roulette bounce: the survivors' state goes to the pass's dense set (kz_wf_compact) and every launch from
            // here on takes its per-path arrays from the device - the dense set, or the pass's own when the survivors did not fit. (The shadow rays of this
            // bounce, which may still be running beside, read shA / shB / shL and the shadow queue of the pass's own arrays: nothing the kernel touches.)
            // The stage clock books it under "shade".
            const DenseSet ds_ = denseSetOf(P, W, L.items);
            hipLaunchKernelGGL(kz_wf_compact, L.gShade, L.blk, 0, stream, W, ds_.D, ds_.origin, ds_.cap, ds_.withMisc, ds_.withSampler, nextQ, (const uint32_t *)nextCount, (KzWfLate *)(W.counts + KzCounts::kLate));
            L.sel = (const KzWfLate *)(W.counts + KzCounts::kLate);
            if ((rc = L.mark(2))) return rc;
        }
        if (needExtend) {
            L.trace(0, nextQ, nextCount, 0u, nextCount + KzCounts::kBounceHead, nullptr, nullptr);
            if (shOn) HIP_TRY(hipStreamWaitEvent(stream, c.evJoin, 0));          // (the stage clock then shows the pair under "trace_bounce" and nothing under "trace_shadow")
            if ((rc = L.mark(1))) return rc;
        }
        cur = nextQ; curCount = nextCount;
    }
    if (P.bgPresent) {
        if (L.sel) hipLaunchKernelGGL(kz_wf_final_late, L.gShade, L.blk, 0, stream, P, L.ds->T, L.sel, cur, curCount);
        else hipLaunchKernelGGL(kz_wf_final, L.gShade, L.blk, 0, stream, P, L.ds->T, W, cur, curCount);
    }
#ifdef KZ_EXPERIMENTS
    // kz_debug_trace: how many paths each bounce queued for the next one (a host read of the counters: the pass is waited for) - what the dense set's share is chosen from
    if (g_kzTrace.load(std::memory_order_relaxed)) {
        uint32_t h[KzCounts::kLitBase];
        HIP_TRY(hipMemcpyAsync(h, W.counts, sizeof h, hipMemcpyDeviceToHost, stream)); HIP_TRY(hipStreamSynchronize(stream));
        std::string line;
        for (int iter = 0; iter < std::min(P.maxDepth, 8); ++iter) line += " " + std::to_string(h[KzCounts::quad(iter) + KzCounts::kPaths]);
        const uint32_t late = P.maxDepth >= KZ_DENSE_BOUNCE ? h[KzCounts::quad(KZ_DENSE_BOUNCE - 1) + KzCounts::kPaths] : 0u;
        KZ_TRACE("path_mis pass of %u items: paths queued by shade(0 ..):%s; late bounces %s (%u paths, dense set of %u)", L.items, line.c_str(),
                 !L.sel ? "in the pass's arrays: no compaction" : late <= denseSetOf(P, W, L.items).cap ? "compacted" : "in the pass's arrays: the dense set is too small", late, L.sel ? denseSetOf(P, W, L.items).cap : 0u);
    }
#endif
    return KZ_OK;
}

// One pass of the wavefront pipeline over `items` = nPixPass x Sp (pixel, sample) items: pixels pixList[0 .. nPixPass), sample indices
// [sBegin, sBegin + Sp). Every launch goes to `stream`; queue counts stay on the device. All four integrators share the camera stage (generate, beams + list
// kernel, packet or per-lane traversal, first-hit walk-through); then path_mis runs its bounce loop and normals / ao / path_mats their tail (kz_integrators.h).
// The three others see a copy of the parameters that names no invisible light: none of them walks through a light (H6 is path_mis's alone), so a first hit
// on such a light is kept and an occlusion ray is blocked by it.
static int wfPass(KzScene *scene, KzDeviceState *ds, PassCtx &c, hipStream_t stream, const uint32_t *pixList, uint32_t sBegin, uint32_t Sp, uint32_t items, KzTune tune, bool beams, bool beside,
                  hipEvent_t waitAov = nullptr, hipEvent_t recordAov = nullptr, hipEvent_t waitMatte = nullptr, hipEvent_t recordMatte = nullptr) {
    int rc;
    WfLaunch L{ds, c, stream};
    const bool mis = scene->prm.integrator == KZ_INTEGRATOR_PATH_MIS;
    KzParams &P = L.P = scene->prm;
    if (!mis) { P.anyInvisibleLight = 0; P.nIlTris = 0; P.shadowFast = 1; }
    // The shade kernels' tables: the roulette-ahead test as the scene has it - but not while the counters run: they state the work of the reference's loop
    // (tests/test_gpu_parity.py bounds rays and shaded hits from below against the oracle's), so a counted render traces the rays the test would skip.
    // (A development build can switch the test off, or on for counted renders too: kz_debug_rr_ahead.)
    L.Tsh = ds->T;
    if (ds->statsOn) L.Tsh.nEmTris = KZ_EM_OFF;
#ifdef KZ_EXPERIMENTS
    { const int mode = g_kzRrAhead.load(std::memory_order_relaxed);
      if (mode == 0) L.Tsh.nEmTris = KZ_EM_OFF; else if (mode == 2) L.Tsh.nEmTris = ds->T.nEmTris; }
#endif
    KzWf &W = L.W = c.wf;
    W.outJx = c.plane[0]; W.outJy = c.plane[1]; W.outR = c.plane[2]; W.outG = c.plane[3]; W.outB = c.plane[4]; W.stats = ds->stats;
    L.pixList = pixList; L.items = items; L.Sp = Sp; L.sBegin = sBegin; L.st = ds->statsOn;
    // shade: the lean variant runs 4 workgroups per CU at once (its launch bounds), so the default grid is exactly those, each looping over
    // its share: with 6 per CU the kernel ran 1.5 rounds, the second with half the CUs idle (same-call sweep, profiles/r02h_shade: shade alone
    // 24.1 ms at 6, 23.0 at 4, 22.6 at 8, 22.3 at 12 - and with two passes in flight the small grid leaves the most room for the other pass:
    // 1246 Msamples/s at 4 against 1214-1218 at 6 / 8 / 12). The EXT variant (3 resident) shows no preference on C3 and stays at 6. The kernels of the
    // other integrators run 8 per CU.
    const int shadeBlocks = tune.shadeBlocksPerCU > 0 ? tune.shadeBlocksPerCU : !mis ? 8 : (P.bsdfExt ? 6 : KZ_SHADE_WAVES);
    L.blk = dim3(KZ_BLOCK); L.gItems = dim3((items + KZ_BLOCK - 1) / KZ_BLOCK);
    L.gTrav = dim3(travGridBlocks(ds, tune)); L.gShade = dim3((unsigned)(ds->numCU * shadeBlocks));
    L.gPacket = dim3(packetGridBlocks(ds));
    // stack: tune.ldsStack entries per lane in LDS, the rest of the worst case (known from the builder) in a global overflow area
    const TraceShape shape = traceShape(P, L.gTrav.x, tune.ldsStack);
    tune.ldsStack = shape.ldsStack;
    L.traceLds = shape.traceLds;
    if ((rc = ensureOverflow(scene, ds, c, tune, stream))) return rc;
    L.dense = mis && P.maxDepth > KZ_DENSE_BOUNCE;
#ifdef KZ_EXPERIMENTS
    if (!g_kzCompactLate.load(std::memory_order_relaxed)) L.dense = false;      // kz_debug_compact_late(0): every bounce in the pass's own arrays
#endif
    tune.ovf = c.ovf; tune.ovfStride = shape.ovfStride;
    L.tune = tune; L.ovfPart = shape.ovfPart;
    c.stageUsed = 0;
    HIP_TRY(hipMemsetAsync(W.counts, 0, KzCounts::bytes(), stream));
    if ((rc = L.mark(-1))) return rc;
    hipLaunchKernelGGL(kz_wf_generate, L.gItems, L.blk, 0, stream, P, ds->T, W, pixList, items, Sp, sBegin);
    if ((rc = L.mark(0))) return rc;
    if (mis && P.maxDepth <= 0 && !scene->aovMask && !scene->matteMask) return KZ_OK;           // Li returns 0 before the loop contributes anything
    if ((rc = wfCamera(L, beams))) return rc;
    if (scene->aovMask && (rc = wfAov(scene, L, waitAov, recordAov))) return rc;
    if (scene->matteMask && (rc = wfMatte(scene, L, waitMatte, recordMatte))) return rc;
    if (mis && P.maxDepth <= 0) return KZ_OK;           // (the camera stage ran for the feature films and the mattes alone)
    if (P.integrator == KZ_INTEGRATOR_NORMALS) {
        //   normals    kz_wf_normals                                                    (no bounce state)
        hipLaunchKernelGGL(kz_wf_normals, L.gShade, L.blk, 0, stream, P, ds->T, W, items);
        rc = L.mark(2);
    } else if (P.integrator == KZ_INTEGRATOR_AO) {
        //   ao         kz_wf_ao -> kz_wf_trace<4> on the occlusion rays                 (any hit, every triangle blocks)
        uint32_t *quad = W.counts + KzCounts::quad(0), *shQ = W.queue[2], *shCount = quad + KzCounts::kShadows;
        hipLaunchKernelGGL(kz_wf_ao, L.gShade, L.blk, 0, stream, P, ds->T, W, pixList, Sp, sBegin, items, shQ, shCount);
        if ((rc = L.mark(2))) return rc;
        L.trace(4, shQ, shCount, 0u, quad + KzCounts::kShadowHead, nullptr, nullptr);
        rc = L.mark(3);
    } else rc = mis ? wfMis(L, beside) : wfMats(L);
    if (rc) return rc;
    if (L.st) hipLaunchKernelGGL(kz_wf_count, L.gItems, L.blk, 0, stream, W, items);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

// ---- kz_render / kz_render_tiles on one replica: plan (kz_plan.cpp: pure arithmetic, tabulated by tests/test_plan_cpu.py) -> make room -> launch ----
// The planner's input. The pass contexts never take more than the caller's limit; without one, not more than 3/4 of the device and not more than what is free now
// plus what this replica already holds for the purpose (another process or replica may own the rest).
static int planIn(KzDeviceState *ds, const KzRenderOpts *opts, int pipeline, uint32_t s0, uint32_t s1, KzPlanIn &in) {
    in.pipeline = pipeline; in.nPix = ds->nPix; in.s0 = s0; in.s1 = s1;
    in.passItems = opts->passItems; in.passesInFlight = opts->passesInFlight; in.sppPerPass = opts->tune.sppPerPass;
    in.perItem = (pipeline == 2 ? KZ_STATE_BYTES_PER_ITEM : 0) + KZ_SAMPLE_BYTES_PER_ITEM;
    in.limit = opts->maxStateBytes;
    if (!in.limit) {
        size_t freeB = 0, totalB = 0;
        const size_t held = ds->ctxBytes() + kzCtxPoolBytes(ds->device);          // what this replica's contexts and the device's idle pooled contexts hold (the beam lists - one per frame pixel, 264 B each - and the film's tap sums are the replica's, not part of this budget)
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && totalB > 0) in.limit = std::min(totalB / 4 * 3, freeB + held - std::min(freeB + held, KzArena::kRuntimeReserve + ((size_t)256 << 20)));      // (what the arena will not map anyway: its reserve for the HIP runtime)
        else in.limit = (size_t)32 << 30;
        if (in.limit == 0) return kz_fail(KZ_ERR_OOM, "the device has %.2f GB free and this replica holds no pass context: nothing is left for path state beyond the %.2f GB a context leaves to the HIP runtime's own allocations",
                                          freeB / 1e9, (KzArena::kRuntimeReserve + ((size_t)256 << 20)) / 1e9);
    }
    const KzTileDealer *dealer = opts->dealer;
    in.dealer = dealer != nullptr;
    if (dealer) { in.takers = dealer->takers; in.dealerBatchTiles = dealer->batchTiles; in.nTiles = (uint32_t)ds->curTiles.size(); in.tilePixOffset = ds->tilePixOffset.data(); }
    // (what the first context was last ASKED to hold, not what it holds: a context that is still growing - or growing slowly - earns the same as a complete one;
    //  a fresh replica takes the pool's largest context and goes on from what that holds)
    in.heldBefore = ds->ctx[0] ? std::max(ds->ctx[0]->wanted, ds->ctx[0]->items()) : kzCtxPoolMaxItems(ds->device);
    return KZ_OK;
}

// Memory this call does not use is given back when the call needs it: contexts beyond nCtx, what the device's pool holds idle, and - under a
// limit below what an earlier call grew them to - the tails of the contexts it does use (a growth thread still mapping towards an earlier, larger
// target is told the new one first: ADVICE r05)
static int makeRoom(KzDeviceState *ds, int nCtx, size_t need, size_t perItem, size_t limit) {
    const size_t perCtx = need * perItem;
    size_t keep = 0;
    for (int i = 0; i < nCtx; ++i) { PassCtx &c = ds->ctxAt(i); if (c.arena) c.arena->lowerTarget(need); keep += std::max(c.bytes(), perCtx); }      // (taken from the device's pool here, with whatever they hold)
    for (int i = KZ_MAX_PASSES_IN_FLIGHT - 1; i >= nCtx; --i) {
        if (!ds->ctx[i] || !ds->ctx[i]->bytes()) continue;
        if (keep + ds->ctx[i]->bytes() > limit) { HIP_TRY(hipDeviceSynchronize()); ds->ctx[i]->release(); } else keep += ds->ctx[i]->bytes();
    }
    if (keep + kzCtxPoolBytes(ds->device) > limit) (void)kzCtxPoolTrim(ds->device, limit > keep ? limit - keep : 0);
    if (keep > limit)
        for (int i = 0; i < nCtx; ++i) if (ds->ctx[i] && ds->ctx[i]->bytes() > perCtx) {
            HIP_TRY(hipDeviceSynchronize());
            // (a context that has grown into mapped levels cannot hold fewer than one of them - 1.5 GB -: under a cap below that it starts over as a small one)
            if (need <= KzArena::kSmallMax) ds->ctx[i]->arena->releaseAll(); else ds->ctx[i]->arena->shrinkTo(need);
            ds->ctx[i]->trimAux();                                                             // (a pooled context may carry another frame's overflow stacks)
        }
    return KZ_OK;
}

// Different priorities put streams on different hardware queues whatever other streams the process has created (streams of one
// priority share a small round-robin pool of queues and two of them may end up serialised on one): the pass streams cycle
// through the priority levels the device has.
static int passStreams(KzDeviceState *ds, int streamPriority, int nCtx) {
    int prLeast = 0, prGreatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest));
    const int mode = streamPriority > 0 ? streamPriority : 3;
    if (mode != ds->streamMode) {                                  // another policy than the streams were made with: make them again
        HIP_TRY(hipDeviceSynchronize());
        for (Stream &st : ds->passStream) st.reset();
        ds->streamMode = mode;
    }
    const int nPr = std::max(1, prLeast - prGreatest + 1);
    for (int i = 0; i < nCtx; ++i) {
        const int pr = mode == 1 ? (prLeast + prGreatest) / 2 : mode == 2 ? ((i & 1) ? prGreatest : prLeast) : prLeast - (i % nPr);
        if (const int rc = ds->evFilm[i].ensure(hipEventDisableTiming)) return rc;
        if (const int rc = ds->passStream[i].ensure(hipStreamNonBlocking, pr)) return rc;
    }
    return ds->evFork.ensure(hipEventDisableTiming);
}

// The passes of one call: what they share (the call's arguments and its plan) and what one leaves for the next and for the call's summary.
struct PassRun {
    KzScene *scene; KzDeviceState *ds; const KzRenderOpts *opts;
    int pipeline; hipStream_t stream; KzTune tune; bool beams;
    KzPlan pl;
    uint32_t pass = 0;
    bool inFlight[KZ_MAX_PASSES_IN_FLIGHT] = {};      // evFilm[i] of a context that has not run a pass in this call must not be waited for: inFlight marks the ones that have
    size_t firstPassItems = 0, largestPassItems = 0, lastAvail = 0;      // lastAvail: what the context of the last pass held when that pass was planned
    int ctxIndex() const { return pl.multi ? (int)(pass % (uint32_t)pl.nCtx) : 0; }
    hipStream_t streamOf(int ci) const { return pl.multi ? ds->passStream[ci] : stream; }
};

// the context the next pass runs in, with what a pass may use of it now
static int nextCtx(PassRun &r, size_t *usable) {
    KzDeviceState *ds = r.ds; const KzPlan &pl = r.pl;
    const int ci = r.ctxIndex();
    // While the context is still growing the host must not plan the whole job on what is mapped NOW (it queues passes a thousand times faster than
    // the device runs them): it stays one pass ahead - pass k + 1 is planned when pass k - 1 has finished, with what has been mapped by then.
    if (pl.grow && !r.opts->dealer && r.lastAvail < pl.need && r.pass >= 2) HIP_TRY(hipEventSynchronize(ds->events[r.pass - 2].b));
    // Back-pressure of dynamic dealing: the host takes the next batch only when the context it needs has finished its previous pass, so a device
    // holds at most nCtx passes - never the whole frame - and a slower device simply comes back to the counter less often.
    if (r.opts->dealer && r.inFlight[ci]) HIP_TRY(hipEventSynchronize(ds->evFilm[ci]));
    const int rc = ctxEnsure(ds->ctxAt(ci), pl.need, pl.minStart, pl.graceMs, r.streamOf(ci), usable);
    r.lastAvail = *usable;
    KZ_TRACE("pass %u: context %d holds %zu M items", r.pass, ci, *usable >> 20);
    return rc;
}

// How this pass runs (kz_plan.h): the planner's answer, after the replica's four timed passes have been read if the answer depends on them.
static int passMode(PassRun &r, size_t items, uint32_t nPixPass, KzPassAnswer &a) {
    KzDeviceState *ds = r.ds; const KzParams &P = r.scene->prm;
    KzPassQuery q;
    q.items = items; q.nPixPass = nPixPass; q.shadowBeside = r.opts->shadowBeside; q.passHalves = r.opts->passHalves; q.pipeline = r.pipeline;
    q.multi = r.pl.multi; q.dealer = r.opts->dealer != nullptr; q.statsOn = ds->statsOn;
    q.mis = P.integrator == KZ_INTEGRATOR_PATH_MIS; q.nLights = P.nLights; q.maxDepth = P.maxDepth;
    KzPassMode &m = ds->passMode;
    if (kzPassModeDue(m, q)) {
        float ms[4];
        HIP_TRY(hipEventSynchronize(ds->evProbe[3][1]));
        for (int k = 0; k < 4; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], ds->evProbe[k][0], ds->evProbe[k][1]));
        kzPassModeSettle(m, ms);
        KZ_TRACE("large passes of %zu items: %.2f / %.2f ms one stream, %.2f ms beside, %.2f ms as halves -> mode %d", m.items[0], m.ms[0], m.ms[3], m.ms[1], m.ms[2], m.kept);
    }
    a = kzPassModeAsk(m, q);
    return KZ_OK;
}

// The pass as two halves: pixels [0, nA) of the pass in the first part of every array on `pst`, pixels [nA, nPixPass) behind them on the context's second stream.
static int launchHalves(PassRun &r, PassCtx &c, hipStream_t pst, EventPair &ep, const uint32_t *pixList, uint32_t nPixPass, uint32_t s, uint32_t Sp, const KzPassAnswer &how) {
    int rc;
    KzScene *scene = r.scene; KzDeviceState *ds = r.ds;
    const uint32_t nA = how.firstHalfPixels, nB = nPixPass - nA;
    const size_t itemsA = (size_t)nA * Sp, itemsB = (size_t)nB * Sp;
    PassCtx &va = *c.view[0], &vb = *c.view[1];
    ctxPoint(va, *c.arena, 0); ctxPoint(vb, *c.arena, itemsA);
    const int lanes = filmLanes(r.tune);
    HIP_TRY(hipEventRecord(c.evHalfFork, pst)); HIP_TRY(hipStreamWaitEvent(c.halfStream, c.evHalfFork, 0));
    if ((rc = wfPass(scene, ds, va, pst, pixList, s, Sp, (uint32_t)itemsA, r.tune, r.beams, how.beside[0]))) return rc;
    if ((rc = wfPass(scene, ds, vb, c.halfStream, pixList + nA, s, Sp, (uint32_t)itemsB, r.tune, r.beams, how.beside[1]))) return rc;
    ds->lastInfo.shadowBeside = 2u;                                   // (kz_last_pass_info: the last pass ran as halves)
    // the halves' pixels are disjoint, so are their tap sums: the two film stages need no order between them
    if ((rc = filmStages(scene, ds, pst, pixList, nA, Sp, va.plane, nullptr, lanes))) return rc;
    if ((rc = filmStages(scene, ds, c.halfStream, pixList + nA, nB, Sp, vb.plane, nullptr, lanes))) return rc;
    if ((rc = stageMark(va, pst, 4))) return rc;
    HIP_TRY(hipEventRecord(c.evHalfJoin, c.halfStream)); HIP_TRY(hipStreamWaitEvent(pst, c.evHalfJoin, 0));
    HIP_TRY(hipEventRecord(ep.b, pst)); HIP_TRY(hipGetLastError());
    ds->lastStageCtx = &va;                                           // (the stage clock of a pass in halves is its first half's)
    return KZ_OK;
}

// The pass on one stream: the wavefront pipeline, or the reference-shaped megakernel of the scene's integrator.
static int launchWhole(PassRun &r, PassCtx &c, int ci, hipStream_t pst, EventPair &ep, const uint32_t *pixList, uint32_t nPixPass, uint32_t s, uint32_t Sp, bool beside) {
    int rc;
    KzScene *scene = r.scene; KzDeviceState *ds = r.ds; const KzParams &P = scene->prm;
    const uint32_t items = (uint32_t)((size_t)nPixPass * Sp);
    if (r.pipeline == 2) {
        // (feature films, passes in flight: this pass's AOV tap launches go behind those of the pass before it, on another stream - wfAov)
        hipEvent_t waitAov = nullptr, recordAov = nullptr;
        if (scene->aovMask && r.pl.multi) {
            if ((rc = ds->evAov[ci].ensure(hipEventDisableTiming))) return rc;
            recordAov = ds->evAov[ci];
            if (r.pass > 0) waitAov = ds->evAov[(ci + r.pl.nCtx - 1) % r.pl.nCtx];
        }
        hipEvent_t waitMatte = nullptr, recordMatte = nullptr;      // (ID mattes: the same chain, with events of its own)
        if (scene->matteMask && r.pl.multi) {
            if ((rc = ds->evMatte[ci].ensure(hipEventDisableTiming))) return rc;
            recordMatte = ds->evMatte[ci];
            if (r.pass > 0) waitMatte = ds->evMatte[(ci + r.pl.nCtx - 1) % r.pl.nCtx];
        }
        if ((rc = wfPass(scene, ds, c, pst, pixList, s, Sp, items, r.tune, r.beams, beside, waitAov, recordAov, waitMatte, recordMatte))) return rc;
    }
    else {
        const dim3 grid((items + KZ_BLOCK - 1) / KZ_BLOCK), blk(KZ_BLOCK);
        float *sJx = c.plane[0], *sJy = c.plane[1], *sR = c.plane[2], *sG = c.plane[3], *sB = c.plane[4];
        const bool mats = P.integrator == KZ_INTEGRATOR_PATH_MATS;
        if (P.integrator == KZ_INTEGRATOR_NORMALS || P.integrator == KZ_INTEGRATOR_AO || mats)      // (normals / ao read no BSDF row)
            hipLaunchKernelGGL(integratorMegaFn(P.integrator, mats && P.bsdfExt ? KZ_X_MATS : 0), grid, blk, 0, pst, P, ds->T, pixList, items, Sp, s, (const uint32_t *)nullptr, sJx, sJy, sR, sG, sB);
        else
            hipLaunchKernelGGL(megaFn(ds->statsOn, P.bsdfExt ? KZ_X_ALL : 0), grid, blk, 0, pst, P, ds->T, pixList, items, Sp, s, (const uint32_t *)nullptr, sJx, sJy, sR, sG, sB, ds->stats);
    }
    HIP_TRY(hipEventRecord(ep.b, pst)); HIP_TRY(hipGetLastError());
    // the film stage adds this pass's samples to the running tap sums of its pixels, behind the film stage of the pass before it (another stream's)
    const int prev = (ci + r.pl.nCtx - 1) % r.pl.nCtx;
    if ((rc = filmStages(scene, ds, pst, pixList, nPixPass, Sp, c.plane, (r.pl.multi && r.pass > 0) ? ds->evFilm[prev] : nullptr, filmLanes(r.tune)))) return rc;
    return r.pipeline == 2 ? stageMark(c, pst, 4) : KZ_OK;
}

// one pass: pixels [p0, p0 + nPixPass) of the pixel list x sample indices [s, s + Sp), in the context nextCtx has prepared
static int onePass(PassRun &r, uint32_t p0, uint32_t nPixPass, uint32_t s, uint32_t Sp) {
    int rc;
    KzDeviceState *ds = r.ds;
    const uint32_t *pixList = ds->pixList + p0;
    const size_t items = (size_t)nPixPass * Sp;
    const int ci = r.ctxIndex();
    PassCtx &c = ds->ctxAt(ci);
    hipStream_t pst = r.streamOf(ci);
    if (items > c.items()) return kz_fail(KZ_ERR_STATE, "pass of %zu items planned on a context that holds %zu", items, c.items());      // (the planner's invariant, kz_plan.h: never a write beyond what is mapped)
    if (!r.firstPassItems) r.firstPassItems = items;
    r.largestPassItems = std::max(r.largestPassItems, items);
    if (r.beams) {
        if ((rc = ensureBeams(r.scene, ds, r.stream, p0, nPixPass))) return rc;
        if (pst != r.stream && c.beamSeen != ds->beamSeq) { HIP_TRY(hipStreamWaitEvent(pst, ds->evBeam, 0)); c.beamSeen = ds->beamSeq; }
    }
    if (ds->eventsUsed == ds->events.size()) { EventPair ep; if ((rc = ep.a.ensure()) || (rc = ep.b.ensure())) return rc; ds->events.push_back(std::move(ep)); }
    EventPair &ep = ds->events[ds->eventsUsed++];
    HIP_TRY(hipEventRecord(ep.a, pst));
    KzPassAnswer how;
    if ((rc = passMode(r, items, nPixPass, how))) return rc;
    if (how.halves) {                                                       // (what the halves need - a second stream, per view counters and overflow stacks - is made before the clock of a timed pass starts)
        if ((rc = c.halfStream.ensure(hipStreamNonBlocking)) || (rc = c.evHalfFork.ensure(hipEventDisableTiming)) || (rc = c.evHalfJoin.ensure(hipEventDisableTiming))) return rc;
        for (int h = 0; h < 2; ++h) {
            if (!c.view[h]) c.view[h].reset(new PassCtx());
            if (!c.view[h]->counts && (rc = c.view[h]->counts.alloc(KzCounts::kWords))) return rc;
            if ((rc = ensureOverflow(r.scene, ds, *c.view[h], r.tune, h ? c.halfStream : pst))) return rc;
        }
    }
    const int probe = how.probe;
    if (probe >= 0) {
        for (int k = 0; k < 2; ++k) if ((rc = ds->evProbe[probe][k].ensure())) return rc;
        HIP_TRY(hipEventRecord(ds->evProbe[probe][0], pst));
    }
    ds->lastStageCtx = nullptr;
    if (how.halves) rc = launchHalves(r, c, pst, ep, pixList, nPixPass, s, Sp, how);
    else rc = launchWhole(r, c, ci, pst, ep, pixList, nPixPass, s, Sp, how.beside[0]);
    if (rc) return rc;
    if (probe >= 0) { HIP_TRY(hipEventRecord(ds->evProbe[probe][1], pst)); ds->passMode.record(probe, items); }      // (film stage included, the same for all three)
    if (r.pl.multi || r.opts->dealer) { HIP_TRY(hipEventRecord(ds->evFilm[ci], pst)); r.inFlight[ci] = true; }      // (a dealer paces itself on this event even with one context)
    ds->lastCtx = ci; ++r.pass;
    return KZ_OK;
}

static int renderOn(KzScene *scene, KzDeviceState *ds, const KzRenderOpts *opts) {
    int rc;
    const KzParams &P = scene->prm;
    if (opts->pipeline < 0 || opts->pipeline > 2) return kz_fail(KZ_ERR_INVALID_ARG, "pipeline %d (0 = default, 1 = megakernel, 2 = wavefront)", opts->pipeline);
    if (opts->passesInFlight < 0 || opts->passesInFlight > KZ_MAX_PASSES_IN_FLIGHT)
        return kz_fail(KZ_ERR_INVALID_ARG, "passesInFlight %d (0 = default, 1 .. %d)", opts->passesInFlight, KZ_MAX_PASSES_IN_FLIGHT);
    if (opts->shadowBeside < 0 || opts->shadowBeside > 2) return kz_fail(KZ_ERR_INVALID_ARG, "shadowBeside %d (0 = default, 1 = never, 2 = always)", opts->shadowBeside);
    if (opts->passHalves < 0 || opts->passHalves > 2) return kz_fail(KZ_ERR_INVALID_ARG, "passHalves %d (0 = default, 1 = never, 2 = always)", opts->passHalves);
    PassRun r{scene, ds, opts};
    const int pipeline = r.pipeline = opts->pipeline ? opts->pipeline : 2;
    if (pipeline == 1 && (rc = kzEnsureBvh2(scene, ds))) return rc;
    uint32_t s0 = opts->sampleBegin, s1 = opts->sampleEnd;
    if (s0 == 0 && s1 == 0) s1 = P.sampleCount;
    if (s0 >= s1 || s1 > P.sampleCount) return kz_fail(KZ_ERR_INVALID_ARG, "sample range [%u,%u) outside [0,%u)", s0, s1, P.sampleCount);
    hipStream_t stream = r.stream = (hipStream_t)opts->stream;
    // a call is ordered behind the previous call on this replica WHATEVER stream that one was given: it clears or extends the tap sums the previous call's last
    // kernels read (a caller that alternates streams used to be ordered only when the tile set changed)
    if (ds->evCallB && stream != ds->lastStream) HIP_TRY(hipStreamWaitEvent(stream, ds->evCallB, 0));
    ds->lastStream = stream;
    KzTune &tune = r.tune;
    if ((rc = resolveTune(opts->tune, tune))) return rc;
    if (tune.filmGather != 0 && tune.filmGather != 3) return kz_fail(KZ_ERR_UNSUPPORTED, "KzTuning.filmGather %d: the staged gather kernel of round 1 is gone (round 6: the film is resolved from running tap sums for every filter); 0 = default, 3 = one lane per pixel", tune.filmGather);
    if ((rc = prepareTiles(scene, ds, opts->tiles, opts->nTiles, stream))) return rc;
    // the films: the picture's running tap sums (kz_film.hip), then those of the enabled feature films (kazen_mi355x_aov.h) in ascending order - part of the replica,
    // outside the pass contexts' budget, cleared unless the call accumulates
    if ((rc = kzFilmEnsure(scene, ds->picture(), ds->filmPixels, opts->accumulate != 0, stream))) return rc;
    for (int f = 0; f < 3; ++f) if ((scene->aovMask & (1u << f)) && (rc = kzFilmEnsure(scene, ds->aov(f), ds->filmPixels, opts->accumulate != 0, stream))) return rc;
    // the ID-matte tables (kazen_mi355x_matte.h): outside the budget too, cleared unless the call accumulates
    if (scene->matteMask && (rc = kzMatteEnsure(scene, ds, opts->accumulate != 0, s1 - s0, stream))) return rc;
    // ... and the second-moment film's (kazen_mi355x_variance.h). What each of the two films has been given since it was last zeroed is counted per pixel.
    if (!opts->accumulate) { ds->pictureSamples = 0; ds->adValid = false; }      // (... and the block records of an adaptive call describe a film that is gone)
    if (scene->varianceMode) {
        if (!ds->moment().sums || !opts->accumulate) ds->momentSamples = 0;
        if ((rc = kzFilmEnsure(scene, ds->moment(), ds->filmPixels, opts->accumulate != 0, stream))) return rc;
    }
    const KzTileDealer *dealer = opts->dealer;
    if (dealer) {
        if (!dealer->counter || (dealer->takenCap && (!dealer->taken || !dealer->nTaken))) return kz_fail(KZ_ERR_INVALID_ARG, "KzTileDealer: null counter / taken buffer");
        if (pipeline != 2) return kz_fail(KZ_ERR_UNSUPPORTED, "dynamic tile dealing needs the wavefront pipeline");
        if (dealer->nTaken) *dealer->nTaken = 0;
    }
    // ---- plan
    KzPlanIn in;
    if ((rc = planIn(ds, opts, pipeline, s0, s1, in))) return rc;
    KzPlan &pl = r.pl;
    { std::string why; if ((rc = kzPlanCall(in, pl, why))) return kz_fail(rc, "%s", why.c_str()); }
    const int nCtx = pl.nCtx; const bool multi = pl.multi;
    const uint32_t nTilesSet = (uint32_t)ds->curTiles.size(), batchTiles = pl.batchTiles;
    if (dealer && !kzDealerAgree(dealer, batchTiles, nTilesSet))
        return kz_fail(KZ_ERR_INVALID_ARG, "KzTileDealer: this taker resolved batches of %u tiles of a list of %u, another taker of the same counter resolved something else "
                                           "(all takers must pass the same tile list, sample range, pass options and `takers`)", batchTiles, nTilesSet);
    // camera rays by pixel beams: a pinhole camera with an affine sample map, a stack that fits LDS twice, unless the caller asks otherwise
    const bool beams = r.beams = pipeline == 2 && P.beamOk && tune.packet != 1 && tune.packet != 2 && P.maxDepth > 0;
    r.lastAvail = pl.need;
    // ---- make room
    if ((rc = makeRoom(ds, nCtx, pl.need, in.perItem, in.limit))) return rc;
    if ((rc = ds->evCallA.ensure()) || (rc = ds->evCallB.ensure())) return rc;
    if (multi && (rc = passStreams(ds, opts->tune.streamPriority, nCtx))) return rc;
    if (dealer && (rc = ds->evFilm[0].ensure(hipEventDisableTiming))) return rc;
    ds->eventsUsed = 0;
    HIP_TRY(hipEventRecord(ds->evCallA, stream));
    if (multi) {
        HIP_TRY(hipEventRecord(ds->evFork, stream));
        for (int i = 0; i < nCtx; ++i) HIP_TRY(hipStreamWaitEvent(ds->passStream[i], ds->evFork, 0));
    }
    // Everything ELSE the call allocates is allocated now, before the first context is asked to grow: behind a wipe the growth thread takes whatever
    // clean memory there is the moment it appears, and a hipMalloc of this thread issued after that waits for the wipe like any other (round 5: the beam
    // lists, allocated inside the first pass, held the first call of a job for seconds while its context was already 80 GB large).
    if (pl.autoShape) for (int i = 0; i < nCtx; ++i) ds->ctxAt(i).wanted = pl.need;
    KZ_TRACE("renderOn: %u pixels x samples [%u, %u), target pass %zu items (%u px x %u spp), limit %.1f GB, %d context(s)", ds->nPix, s0, s1, pl.need, pl.pixPerPass, pl.S, in.limit / 1e9, nCtx);
    if (beams && (rc = ensureBeamBuffers(scene, ds, stream))) return rc;
    if (pipeline == 2) for (int i = 0; i < nCtx; ++i) if ((rc = ensureOverflow(scene, ds, ds->ctxAt(i), tune, r.streamOf(i)))) return rc;
    KZ_TRACE("renderOn: beam / overflow buffers there");
    // ---- launch: kzPlanRun walks the schedule, one context and one pass at a time
    auto next = [&r](size_t *usable) { return nextCtx(r, usable); };
    auto one = [&r](uint32_t p0, uint32_t nPixPass, uint32_t s, uint32_t Sp) { return onePass(r, p0, nPixPass, s, Sp); };
    // A call that fails in the middle (an allocation of a later pass, typically) leaves NOTHING running: passes it has already launched on the internal streams - pass
    // streams, a context's side streams - are not joined into `stream` on this path, and their film stages would add to tap sums that the next call has meanwhile
    // cleared (found by injecting allocation failures under two passes in flight: the next film carried the failed call's first pass, scripts/dev/fail_sweep.py).
    auto failed = [&](int code) -> int { (void)hipDeviceSynchronize(); return code; };
    if (!dealer) { if ((rc = kzPlanRun(pl, 0u, ds->nPix, s0, s1, next, one))) return failed(rc); }
    else {
        // BlockGenerator::next (block.cpp:117-148): batches of the tile list from the shared counter (it may live in memory shared between processes)
        for (uint32_t tb, te; kzDealerTake(dealer, batchTiles, nTilesSet, tb, te);)
            if ((rc = kzPlanRun(pl, ds->tilePixOffset[tb], ds->tilePixOffset[te], s0, s1, next, one))) return failed(rc);
    }
    if (multi)                                                         // join: everything after this call on `stream` sees the film
        for (int i = 0; i < nCtx; ++i) if (r.inFlight[i]) HIP_TRY(hipStreamWaitEvent(stream, ds->evFilm[i], 0));
    if ((rc = kzFilmResolve(scene, ds->picture(), stream))) return rc;          // the film texels from the tap sums: once per call
    ds->pictureSamples += s1 - s0;
    if (scene->varianceMode) ds->momentSamples += s1 - s0;
    HIP_TRY(hipEventRecord(ds->evCallB, stream));
    // what the call leaves for kz_last_pass_info / kz_last_grow_note
    ds->lastDual = multi;
    ds->lastInfo.passes = r.pass; ds->lastInfo.passesInFlight = (uint32_t)nCtx; ds->lastInfo.itemsPerPass = pl.need; ds->lastInfo.sppPerPass = pl.S;
    ds->lastInfo.pixels = ds->nPix; ds->lastInfo.stateBytes = ds->ctxBytes(); ds->lastInfo.pixelsPerPass = pl.pixPerPass;
    ds->lastInfo.firstPassItems = r.firstPassItems; ds->lastInfo.largestPassItems = r.largestPassItems;
    ds->growNote.clear();
    for (int i = 0; i < nCtx; ++i) if (ds->ctx[i] && ds->ctx[i]->arena) { std::lock_guard<std::mutex> g(ds->ctx[i]->arena->m); if (ds->ctx[i]->arena->growthFailed) ds->growNote = ds->ctx[i]->arena->errMsg; }
    return KZ_OK;
}

// opts->device addresses a replica by HIP device index; a scene resident on ONE device is addressed by any zero-initialised opts
int kzRenderReplica(KzScene *scene, const KzRenderOpts *opts, KzDeviceState **out) {
    int rc;
    if ((rc = findReplica(scene, opts->device, out))) {
        KzReplicaSet *rs = scene ? replicaSet(scene) : nullptr;
        bool single = false;
        if (rs) { std::lock_guard<std::mutex> g(rs->m); single = rs->v.size() == 1 && opts->device == 0; }
        if (!single || (rc = findReplica(scene, -1, out))) return rc;
    }
    return KZ_OK;
}
int kzRenderOn(KzScene *scene, KzDeviceState *ds, const KzRenderOpts *opts) { return renderOn(scene, ds, opts); }

extern "C" {

int kz_render(KzScene *scene, const KzRenderOpts *opts) {
    if (!opts) return kz_fail(KZ_ERR_INVALID_ARG, "null opts");
    KzDeviceState *ds; int rc;
    if ((rc = kzAovRefuse(scene, opts, "kz_render")) || (rc = kzVarianceRefuse(scene, opts, "kz_render")) || (rc = kzMatteRefuse(scene, opts, "kz_render"))) return rc;
    if ((rc = kzRenderReplica(scene, opts, &ds))) return rc;
    return renderOn(scene, ds, opts);
}

int kz_render_tiles(KzScene *scene, const KzRenderOpts *opts, const KzTile *tiles, uint32_t nTiles, int device, float *film, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = kzAovRefuse(scene, opts, "kz_render_tiles")) || (rc = kzVarianceRefuse(scene, opts, "kz_render_tiles")) || (rc = kzMatteRefuse(scene, opts, "kz_render_tiles"))) return rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const size_t full = ds->filmPixels * 4;
    const bool packedOut = opts && opts->packedOutput;
    if (opts && opts->dealer && film) return kz_fail(KZ_ERR_INVALID_ARG, "kz_render_tiles with a dealer hands back no film: download the batches it took (KzTileDealer.taken) with kz_film_download_tiles");
    if (film) {
        // what the buffer receives is SAID by opts->packedOutput, never inferred from its size (a full tiling with a border-less filter packs to exactly the film's size)
        if (packedOut) {
            if ((rc = checkTiles(scene->prm, tiles, nTiles))) return rc;
            const size_t packed = packedFloats(scene->prm, tiles, nTiles);
            if (!nTiles || nFloats != packed) return kz_fail(KZ_ERR_INVALID_ARG, "packedOutput: the buffer must hold the tiles' packed rects (%zu floats, kz_tiles_packed_floats), got %zu", packed, nFloats);
        } else if (nFloats != full) return kz_fail(KZ_ERR_INVALID_ARG, "film buffer must hold the whole film (%zu floats; set opts->packedOutput for the tiles' packed rects), got %zu", full, nFloats);
    }
    KzRenderOpts o{};
    if (opts) o = *opts;
    o.tiles = tiles; o.nTiles = nTiles; o.device = device;
    if ((rc = renderOn(scene, ds, &o))) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)o.stream));
    if (film && !packedOut) HIP_TRY(hipMemcpy(film, ds->picture().texels, nFloats * sizeof(float), hipMemcpyDeviceToHost));
    else if (film) return downloadTiles(scene, ds, ds->picture(), tiles, nTiles, film, nFloats, (hipStream_t)o.stream);
    return KZ_OK;
}

// What the per-sample entry points share: n > 0 samples (pixel x, y and sample index) checked against the scene, the megakernels' BVH2 made sure of, and the
// pixels (packed as a pixel list) and indices uploaded into dP / dI.
static int uploadSamples(KzScene *scene, KzDeviceState *ds, uint32_t n, const int32_t *pxy, const uint32_t *idx, const float *out, DevBuf<uint32_t> &dP, DevBuf<uint32_t> &dI) {
    int rc;
    if (!pxy || !idx || !out) return kz_fail(KZ_ERR_INVALID_ARG, "null buffer");
    if ((rc = kzEnsureBvh2(scene, ds))) return rc;
    const KzParams &P = scene->prm;
    std::vector<uint32_t> pl(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (pxy[2 * i] < 0 || pxy[2 * i] >= P.width || pxy[2 * i + 1] < 0 || pxy[2 * i + 1] >= P.height || idx[i] >= P.sampleCount)
            return kz_fail(KZ_ERR_INVALID_ARG, "sample %u: pixel (%d,%d) index %u out of range", i, pxy[2 * i], pxy[2 * i + 1], idx[i]);
        pl[i] = (uint32_t)pxy[2 * i] | ((uint32_t)pxy[2 * i + 1] << 16);
    }
    if ((rc = dP.alloc(n)) || (rc = dI.alloc(n)) || (rc = dP.upload(pl.data(), n)) || (rc = dI.upload(idx, n))) return rc;
    return KZ_OK;
}

// Radiance of explicit (pixel, sample index) pairs without touching the film: out = n x (sx, sy, r, g, b).
int kz_render_samples(KzScene *scene, uint32_t n, const int32_t *pxy, const uint32_t *idx, float *out) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (n == 0) return KZ_OK;
    DevBuf<uint32_t> dP, dI; DevBuf<float> dOut;
    if ((rc = uploadSamples(scene, ds, n, pxy, idx, out, dP, dI))) return rc;
    const KzParams &P = scene->prm;
    if ((rc = dOut.alloc((size_t)n * 5))) return rc;
    float *dO = dOut;
    const dim3 gS((n + KZ_BLOCK - 1) / KZ_BLOCK);
    // one kernel per integrator serves every scene here: the variant for everything its BSDF rows may need (normals / ao read no BSDF row; path_mats has no normal maps)
    if (P.integrator == KZ_INTEGRATOR_NORMALS || P.integrator == KZ_INTEGRATOR_AO || P.integrator == KZ_INTEGRATOR_PATH_MATS)
        hipLaunchKernelGGL(integratorMegaFn(P.integrator, KZ_X_MATS), gS, dim3(KZ_BLOCK), 0, 0, P, ds->T, dP.get(), n, 1u, 0u, dI.get(),
                           dO, dO + n, dO + 2 * (size_t)n, dO + 3 * (size_t)n, dO + 4 * (size_t)n);
    else hipLaunchKernelGGL(megaFn(false, KZ_X_ALL), gS, dim3(KZ_BLOCK), 0, 0, P, ds->T, dP.get(), n, 1u, 0u, dI.get(),
                            dO, dO + n, dO + 2 * (size_t)n, dO + 3 * (size_t)n, dO + 4 * (size_t)n, ds->stats.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> h((size_t)n * 5);
    if ((rc = dOut.download(h.data(), h.size()))) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        out[5 * i] = (float)pxy[2 * i] + h[i]; out[5 * i + 1] = (float)pxy[2 * i + 1] + h[n + i];
        out[5 * i + 2] = h[2 * (size_t)n + i]; out[5 * i + 3] = h[3 * (size_t)n + i]; out[5 * i + 4] = h[4 * (size_t)n + i];
    }
    return KZ_OK;
}

// The features of single samples (kazen_mi355x_aov.h): the test surface of the feature films, shaped like kz_render_samples
int kz_aov_samples(KzScene *scene, uint32_t n, const int32_t *pxy, const uint32_t *idx, float *out) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (n == 0) return KZ_OK;
    DevBuf<uint32_t> dP, dI; DevBuf<float> dOut;
    if ((rc = uploadSamples(scene, ds, n, pxy, idx, out, dP, dI))) return rc;
    const KzParams &P = scene->prm;
    if ((rc = dOut.alloc((size_t)n * 10))) return rc;
    hipLaunchKernelGGL(kz_aov_samples_kernel, dim3((n + KZ_BLOCK - 1) / KZ_BLOCK), dim3(KZ_BLOCK), 0, 0, P, ds->T, dP.get(), dI.get(), n,
                       P.integrator == KZ_INTEGRATOR_PATH_MIS ? 1 : 0, dOut.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = dOut.download(out, (size_t)n * 10))) return rc;
    for (uint32_t i = 0; i < n; ++i) { out[10 * (size_t)i] += (float)pxy[2 * i]; out[10 * (size_t)i + 1] += (float)pxy[2 * i + 1]; }      // sample position = pixel + jitter
    return KZ_OK;
}

// The product traversal launches on a caller's rays (kazen_mi355x_dev.h): the kernels come from the tables the passes pick from (traceFn, packetFn), their
// grids, LDS size, stack split and overflow stride from the functions the passes call (traceShape, launchTrace, shadowLaunches) - what runs here is what a
// render runs, on rays a render rarely or never makes. The path state is the call's own: only the arrays these kernels touch.
int kz_trace_rays_wf(KzScene *scene, const KzTraceWfOpts *opts, uint32_t nSlots, const float *o, const float *d, const float *tmin, const float *tmax,
                     const uint32_t *queue, uint32_t nQueue, const float *pending, KzTraceWfHit *hits, float *sums, KzTraceWfInfo *info) {
    KzDeviceState *ds; int rc;
    if (info) memset(info, 0, sizeof *info);
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!opts) return kz_fail(KZ_ERR_INVALID_ARG, "null options");
    if (opts->kernel < 0 || opts->kernel > 3) return kz_fail(KZ_ERR_INVALID_ARG, "kernel %d (0 per-lane closest hit, 1 packet, 2 walk-through ray, 3 shadow test)", opts->kernel);
    const KzParams &P = scene->prm;
    if (opts->kernel == 1 && !packetFits(P)) return kz_fail(KZ_ERR_INVALID_ARG, "the packet kernel's stack holds 128 entries and this scene's tree may need %d: a render takes the per-lane kernel", P.stackBound4);
    if (opts->gridBlocks < 0 || opts->gridBlocks > (int)packetGridBlocks(ds) || opts->packetBatch < 0 || opts->ldsStack > 63)
        return kz_fail(KZ_ERR_INVALID_ARG, "gridBlocks %d (0 .. %u), packetBatch %d (>= 0) or ldsStack %d (<= 63) out of range", opts->gridBlocks, packetGridBlocks(ds), opts->packetBatch, opts->ldsStack);
    const uint32_t count = queue ? nQueue : nSlots;
    if (nSlots == 0 || count == 0) return KZ_OK;
    if (!o || !d || !tmin || !tmax || !hits || !sums || (opts->kernel == 3 && !pending)) return kz_fail(KZ_ERR_INVALID_ARG, "null ray, hit, sum or pending-radiance buffer");
    // (the child keys of a node order as unsigned integers only for entry distances with a clear sign bit, and a render never passes anything else: -0.0 is refused too)
    for (uint32_t i = 0; i < nSlots; ++i) if (!(tmin[i] >= 0.f) || std::signbit(tmin[i])) return kz_fail(KZ_ERR_INVALID_ARG, "slot %u: tmin %g (negative or NaN)", i, (double)tmin[i]);
    if (queue) {
        if (nQueue > nSlots) return kz_fail(KZ_ERR_INVALID_ARG, "%u queue entries for %u slots: one would repeat", nQueue, nSlots);
        std::vector<uint8_t> seen(nSlots, 0);
        for (uint32_t i = 0; i < nQueue; ++i) {
            if (queue[i] >= nSlots) return kz_fail(KZ_ERR_INVALID_ARG, "queue entry %u names slot %u of %u", i, queue[i], nSlots);
            if (seen[queue[i]]) return kz_fail(KZ_ERR_INVALID_ARG, "queue entry %u repeats slot %u", i, queue[i]);
            seen[queue[i]] = 1;
        }
    }
    KzTuning asked{};
    asked.refill = opts->refill; asked.postpone = opts->postpone; asked.batch = opts->batch; asked.ldsStack = opts->ldsStack;
    KzTune tune;
    if ((rc = resolveTune(asked, tune))) return rc;
    const bool packet = opts->kernel == 1, st = opts->stats != 0;
    const unsigned gridBlocks = opts->gridBlocks > 0 ? (unsigned)opts->gridBlocks : (packet ? packetGridBlocks(ds) : travGridBlocks(ds, tune));
    const TraceShape shape = traceShape(P, gridBlocks, tune.ldsStack);
    tune.ldsStack = shape.ldsStack;

    // ---- the call's own path state: rays both as a path's ray (rayA / rayB) and as a shadow / walk-through ray (shA / shB), hit records, pending radiance, sums
    const size_t n = nSlots;
    std::vector<float4> a(n), b(n), sa(n), sb(n), sl(n), h(n);
    std::vector<float> planes(3 * n);
    for (size_t i = 0; i < n; ++i) {
        a[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], tmin[i]); b[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], tmax[i]);
        sa[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], tmax[i]); sb[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], tmin[i]);
        sl[i] = pending ? make_float4(pending[3 * i], pending[3 * i + 1], pending[3 * i + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        float gidBits; memcpy(&gidBits, &hits[i].gid, 4);
        h[i] = make_float4(hits[i].t, hits[i].u, hits[i].v, gidBits);
        for (int k = 0; k < 3; ++k) planes[k * n + i] = sums[3 * i + k];
    }
    DevBuf<float4> dA, dB, dSA, dSB, dSL, dH; DevBuf<float> dPl; DevBuf<uint32_t> dQ, dQB, dCounts, dOvf; DevBuf<unsigned long long> dStats;
    // the overflow area of ONE launch at a time (the launches below run one after another on one stream) and, behind it, one guard row: words no stack may reach
    const size_t ovfWords = shape.ovfPart + shape.ovfStride;
    if ((rc = dA.alloc(n)) || (rc = dB.alloc(n)) || (rc = dSA.alloc(n)) || (rc = dSB.alloc(n)) || (rc = dSL.alloc(n)) || (rc = dH.alloc(n)) || (rc = dPl.alloc(3 * n)) ||
        (rc = dQ.alloc(count)) || (rc = dQB.alloc(count)) || (rc = dCounts.alloc(16)) || (rc = dStats.alloc(32)) || (rc = dOvf.alloc(ovfWords))) return rc;
    if ((rc = dA.upload(a.data(), n)) || (rc = dB.upload(b.data(), n)) || (rc = dSA.upload(sa.data(), n)) || (rc = dSB.upload(sb.data(), n)) || (rc = dSL.upload(sl.data(), n)) ||
        (rc = dH.upload(h.data(), n)) || (rc = dPl.upload(planes.data(), 3 * n)) || (queue && (rc = dQ.upload(queue, count)))) return rc;
    // counter words: 0 the queue's count, 1 .. 3 the work heads of up to three launches, 4 / 5 queueB's count and head, 6 the packet kernel's first hits on an invisible light
    uint32_t cw[16] = {count};
    if ((rc = dCounts.upload(cw, 16))) return rc;
    HIP_TRY(hipMemset(dStats, 0, dStats.bytes()));
    HIP_TRY(hipMemset(dOvf, 0xFF, dOvf.bytes()));
    KzWf W{};
    W.rayA.p = dA; W.rayB.p = dB; W.hit.p = dH; W.shA.p = dSA; W.shB.p = dSB; W.shL.p = dSL;
    W.outR = dPl; W.outG = W.outR + n; W.outB = W.outG + n; W.counts = dCounts; W.stats = dStats;
    tune.ovf = dOvf; tune.ovfStride = shape.ovfStride;
    uint32_t *c = W.counts;
    const uint32_t *q = queue ? dQ.get() : nullptr, *cptr = queue ? c : nullptr;      // (a queue's count is read on the device, as a pass's are; the identity queue's travels as an argument, as the camera rays' does)
    const uint32_t cimm = queue ? 0u : count;
    hipStream_t stream = nullptr;
    auto trace = [&](int mode, const uint32_t *q_, const uint32_t *cptr_, uint32_t cimm_, uint32_t *head, uint32_t *qb, uint32_t *cb) {
        launchTrace(mode, st, dim3(gridBlocks), shape.traceLds, stream, P, ds->T, W, q_, cptr_, cimm_, head, tune, qb, cb);
    };
    if (opts->kernel == 0) trace(0, q, cptr, cimm, c + 1, nullptr, nullptr);
    else if (packet) hipLaunchKernelGGL(packetFn(st, P.anyInvisibleLight != 0), dim3(gridBlocks), dim3(KZ_BLOCK), 0, stream, P, ds->T, W, q, cptr, cimm, c + 1,
                                        opts->packetBatch > 0 ? opts->packetBatch : KZ_PACKET_BATCH, dQB.get(), c + 6);
    else if (opts->kernel == 2) trace(1, q, cptr, cimm, c + 1, nullptr, nullptr);
    else shadowLaunches(P, trace, q, cptr, cimm, c + 1, dQB.get(), c + 4, c + 5);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long stats[32];
    if ((rc = dH.download(h.data(), n)) || (rc = dPl.download(planes.data(), 3 * n)) || (rc = dCounts.download(cw, 16)) || (rc = dStats.download(stats, 32))) return rc;
    std::vector<uint32_t> ovf(packet ? 0 : ovfWords);
    if (!packet && (rc = dOvf.download(ovf.data(), ovfWords))) return rc;
    size_t touched = 0;                                         // overflow rows a stack reached (the guard row included)
    for (size_t w = ovf.size(); w > 0; --w) if (ovf[w - 1] != 0xFFFFFFFFu) { touched = (w - 1) / shape.ovfStride + 1; break; }
    if (touched > shape.ovfRows) return kz_fail(KZ_ERR_STATE, "a traversal stack spilled past the %zu overflow rows of the launch (LDS entries %d, the builder's bound %d)", shape.ovfRows, shape.ldsStack, P.stackBound4);
    for (size_t i = 0; i < n; ++i) {
        KzTraceWfHit &r = hits[i];
        r.t = h[i].x; r.u = h[i].y; r.v = h[i].z; memcpy(&r.gid, &h[i].w, 4);
        const bool known = r.t < KZ_INF && (size_t)r.gid < scene->shade.size();      // (mesh and primitive of a triangle never change: the host's shading records name them)
        r.mesh = known ? (int32_t)scene->shade[r.gid].mesh : -1; r.prim = known ? (int32_t)scene->shade[r.gid].prim : -1;
        for (int k = 0; k < 3; ++k) sums[3 * i + k] = planes[k * n + i];
    }
    if (info) {
        info->rays = stats[1]; info->nodeVisits = stats[2]; info->triTests = stats[3];
        info->nQueueB = opts->kernel == 3 ? cw[4] : 0; info->nFirstHitsOnInvisibleLight = packet ? cw[6] : 0;
        info->gridBlocks = gridBlocks; info->ldsStack = (uint32_t)shape.ldsStack; info->stackBound = (uint32_t)std::max(P.stackBound4, 0);
        info->ovfRows = packet ? 0 : (uint32_t)shape.ovfRows; info->ovfRowsTouched = (uint32_t)touched; info->shadowFast = (uint32_t)P.shadowFast;
    }
    return KZ_OK;
}

} // extern "C"
