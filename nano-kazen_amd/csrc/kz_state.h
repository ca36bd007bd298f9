// kz_state.h - what the translation units of the device library share (not part of the ABI): the path-state arrays of the wavefront pipeline,
// the per-pass contexts, the per-device replica state, error / allocation helpers, and the few host functions that cross a unit boundary.
//   kz_render.hip   a pass: every path kernel (kz_wavefront.h, the megakernel) and the tables that pick them, pass contexts' buffers, wfPass, renderOn, kz_render*
//   kz_replica.hip  replicas: lifetime + upload, tile sets (prepareTiles), the queries that only read replica state (kz_last_*, kz_pass_mode_info, kz_sync*, stats)
//   kz_refit.hip    device side of the edits of a resident scene (kz_refit.h)
//   kz_film.hip     film reconstruction kernels + their launchers, each taking the film (kz_film.h: KzFilm, the picture or a feature film) it works on, tile packing /
//                   download, the kz_film_* entry points and those of kazen_mi355x_aov.h that only touch replica state
//   kz_film_moment.hip  the tap kernels of the second-moment film (include/kazen_mi355x_variance.h) and their launcher, kzFilmStageMoment
//   kz_denoise.hip  the a-trous denoiser of include/kazen_mi355x_denoise.h and its variance-guided form (include/kazen_mi355x_variance.h): their kernels, the
//                   replica's denoise buffers, kz_denoise* and kz_denoise_variance* entry points
//   kz_motion.hip   include/kazen_mi355x_motion.h beyond the denoiser's unit: the id kernel (which mesh every frame pixel shows) and the host-only row table
//   kz_matte.hip    include_ext/kazen_mi355x_matte.h: the ID-matte tables, the stage of a pass that feeds them (kernels: kz_matte.h), their readers and entry points
//   kz_adaptive.hip the classification stage of include_ext/kazen_mi355x_adaptive.h (kernel: kz_adaptive.h), its launcher and the test surface kz_adaptive_classify_films;
//                   kz_adaptive_host.cpp (host code only): the rule's options, schedule and tile lists, the driver kz_render_adaptive and the readers of its records
//   kz_responsive.hip  the two kernels of include/kazen_mi355x_responsive.h (the fast history and the clamp) and their launcher; the entry points: kz_denoise.hip
//   (kz_history.h   the history prepare stage of the temporal, motion and responsive calls, one body: its three kernels are instances in the two units above)
//   kz_multi.cpp    tile dealing, host merge of tile rects, kz_render_multi (host code only)
//   kz_debug.hip    function-level query kernels and known-answer entry points of include/kazen_mi355x_dev.h
// Every device buffer, pinned buffer, event and stream named below is a member of one of the four move-only owners of kz_own.h (DevBuf, PinnedBuf, Event, Stream).
#pragma once
#include <hip/hip_runtime.h>
#include "kz_internal.h"
#include "kz_film.h"
#include "kz_plan.h"
#include "../../include/kazen_mi355x_motion.h"
#include "../../include_ext/kazen_mi355x_matte.h"
#include "../../include_ext/kazen_mi355x_adaptive.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// Path state in HBM: one array per field (SoA; 16-B records, coalesced for the stages that sweep all slots). Round 3 measured one 64-B line per
// path instead and rejected it (profiles/r03h_state_layout): the stages that sweep every slot lost, shade did not move.
template <class Tp> struct KzField {
    Tp *p;
    __device__ __forceinline__ Tp &operator[](uint32_t i) const { return p[(size_t)i]; }
};
struct KzWf {
    KzField<float4> rayA, rayB;    // o.xyz tmin | d.xyz tmax
    KzField<float4> hit;           // t u v gid(bits) - the shading record of the triangle; t = +inf: miss
    KzField<float4> thr;           // throughput.xyz eta (compact state, see kz_wf_shade: throughput.xyz bsdfPdf)
    KzField<float4> misc;          // bsdfPdf accumulatedRoughness discrete(EDiscrete) -
    uint4 *smp;                    // pcg32 state (.x,.y) + dimension index (.z); the pcg32 stream id is recomputed from the pixel
    KzField<float4> shA, shB, shL; // shadow (or walk-through) ray o.xyz tmax | d.xyz tmin | pending radiance
    uint32_t *queue[3];            // two ping-pong path queues + the shadow queue
    uint32_t *counts;              // queue counters, zeroed per pass (KzCounts below)
    float *outJx, *outJy, *outR, *outG, *outB;
    unsigned long long *stats;
};
// What the launches behind kz_wf_compact (kz_wavefront.h; wfMis) read from the device: the per-path arrays they run on - the context's dense set, or the pass's own -
// and the pass slot each entry of them came from (null: a slot is its own origin). KzWf itself stays as it is: the kernels of the early bounces take it by value.
struct KzWfLate { KzWf W; const uint32_t *orig; };

// The queue counters of a pass (PassCtx::counts; the kernels receive pointers into the block, the launch code alone knows its layout).
//   lower half  one quad per stage: [kPaths] entries of the path queue the stage wrote, [kShadows] entries of its shadow queue, [kBounceHead] / [kShadowHead] the work
//               heads of the persistent traversal kernels that drain the two. Quad 0 is the camera stage's - word 0 the first hits on an invisible light (queued for
//               the walk-through), word 2 the head of the per-lane / packet camera rays, word 3 the head of the walk-through -, bounce b of a loop has quad b + 1
//               (ao, which has one bounce, therefore counts its occlusion rays in word 5 and drains them through word 7).
//   upper half  one pair per bounce: the shadow rays that cross an invisible-light triangle (count, head of their walk-through), pair b + 1 for bounce b;
//               the last 8 words: the camera rays of pixels whose beam list overflowed (count, head of the packet kernel that takes them); the 64 words in front
//               of them: the pass's KzWfLate, which kz_wf_compact writes and the launches behind it read (wfMis) - it rides here so that a context has no
//               allocation of its own for it.
struct KzCounts {
    enum : uint32_t { kQuads = 520, kWords = 8 * kQuads, kLitBase = 4 * kQuads, kFallback = kWords - 8, kLate = kFallback - 64 };
    enum : uint32_t { kPaths = 0, kShadows = 1, kBounceHead = 2, kShadowHead = 3 };
    static constexpr uint32_t kCamera = 0;                                             // the camera stage's quad
    static constexpr uint32_t quad(int bounce) { return 4u * (uint32_t)(bounce + 1); }
    static constexpr uint32_t lit(int bounce) { return kLitBase + 2u * (uint32_t)(bounce + 1); }
    static constexpr size_t bytes() { return kWords * sizeof(uint32_t); }
};
static_assert(KzCounts::quad(KZ_PATH_MATS_MAX_DEPTH - 1) + 4 <= KzCounts::kLitBase && KzCounts::quad(KZ_PATH_MIS_MAX_DEPTH - 1) + 4 <= KzCounts::kLitBase, "the deepest bounce's quad stays in the lower half");
static_assert(KzCounts::lit(KZ_PATH_MIS_MAX_DEPTH - 1) + 2 <= KzCounts::kLate, "the deepest bounce's lit pair stays below the late record and the fallback pair");
static_assert(sizeof(KzWfLate) <= (KzCounts::kFallback - KzCounts::kLate) * sizeof(uint32_t) && KzCounts::kLate % 2 == 0, "the late record fits in front of the fallback pair, 8-byte aligned");

struct KzTune { int refill, postpone, batch, travBlocksPerCU, shadeBlocksPerCU, ldsStack, packet, filmGather;
                uint32_t *ovf; uint32_t ovfStride; };


#ifndef KZ_BEAM_CAP
#define KZ_BEAM_CAP 32                // leaves per pixel list (16 / 24 / 48 measured in r03o: 32 stays)
#endif

struct KzTileRect { int32_t x0, y0, w, h; uint32_t offset; };
struct KzTileDesc { int32_t x0, y0, w, h; uint32_t pixOffset; };      // a tile of the current set and the position of its first pixel in the pixel list

// kz_debug_trace (kazen_mi355x_dev.h, development builds): a timeline of the allocation / growth / pass-planning events of the calling process on stderr
#ifdef KZ_EXPERIMENTS
extern std::atomic<int> g_kzTrace;
void kzTraceLine(const char *fmt, ...);
#define KZ_TRACE(...) do { if (g_kzTrace.load(std::memory_order_relaxed)) kzTraceLine(__VA_ARGS__); } while (0)
int kzPhysicalDevice(int logical);            // kz_debug_alias_devices: the HIP device behind the index a replica is addressed by
extern thread_local int g_failAlloc;          // kz_debug_fail_alloc (kz_replica.hip): kzMalloc counts it down, ctxEnsure (kz_render.hip) hands it to a growing arena
extern std::atomic<int> g_kzRrAhead;          // kz_debug_rr_ahead (kz_debug.hip): 0 = the shade kernels trace every bounce ray, as before the roulette-ahead test
extern std::atomic<int> g_kzShadowOrder;      // kz_debug_shadow_order (kz_debug.hip): 0 = the any-hit shadow launches descend in closest-hit order (kz_wf_trace<5>), as before the overlap order
extern std::atomic<int> g_kzCompactLate;      // kz_debug_compact_late (kz_debug.hip): 0 = path_mis passes keep every bounce on the pass's own slots, as before the late-bounce compaction
#else
#define KZ_TRACE(...) do { } while (0)
static inline int kzPhysicalDevice(int logical) { return logical; }
#endif
int kzLogicalDeviceCount();                   // kz_arena.cpp: devices the library presents (= hipGetDeviceCount unless a development build aliases them)
int kzUseDevice(int device);                  // kz_replica.hip: range check + hipSetDevice of the device behind a caller's index

struct EventPair { Event a, b; };
// The path-state memory of one pass context (kz_arena.cpp). Up to 2^23 items: hipMalloc arrays of the size asked for. Beyond: one reserved virtual range
// per array, physical memory mapped into them in levels of 2^23 items on a side thread; `mapped` items of EVERY array are usable at any moment, and only
// ever more (until shrinkTo / releaseAll, which the owner calls on an idle device).
struct KzArena {
    static constexpr int kArrays = 17;        // rayA rayB hit thr misc shA shB shL | smp | queue 0 1 2 | jx jy r g b
    size_t levelItems = (size_t)1 << 23;      // items of one level, fixed while the ranges are reserved (every chunk of an array has the same size): 2^23 (128 MB chunks for the
                                              // 16-B arrays, 32 MB for the 4-B ones) for a context asked to hold up to 2^27 items, 2^25 (512 / 128 MB) for a larger one
    static constexpr size_t kSmallMax = (size_t)1 << 23;
    static constexpr size_t kRuntimeReserve = (size_t)2 << 30;     // bytes a growing context leaves free for the HIP runtime's own device allocations (growOneLevel)
    int device;
    size_t capItems = 0;                      // items the virtual ranges (one per array) are reserved for; 0: no reservation (a small or empty context)
    size_t smallItems = 0;                    // items of the hipMalloc arrays of a small context
    char *base[kArrays]; size_t elem[kArrays];
    struct Level { size_t firstItem, items; hipMemGenericAllocationHandle_t h[kArrays]; int mappedArrays; };
    std::vector<Level> levels;
    std::atomic<size_t> mapped{0};
    std::mutex m; std::condition_variable cvProgress; std::thread th;
    bool stop = false, busy = false, growthFailed = false; size_t target = 0;
    std::atomic<int> failCountdown{0};        // kz_debug_fail_alloc (development builds): the nth physical allocation from now on fails
    bool injectedFailure() {
#ifdef KZ_EXPERIMENTS
        int fc = failCountdown.load();
        return fc > 0 && failCountdown.compare_exchange_strong(fc, fc - 1) && fc == 1;
#else
        return false;
#endif
    }
    int err = 0; std::string errMsg;
    std::chrono::steady_clock::time_point lastProgress;
    explicit KzArena(int dev);
    ~KzArena();
    KzArena(const KzArena &) = delete; KzArena &operator=(const KzArena &) = delete;
    static size_t bytesPerItem();
    size_t bytes() const { return mapped.load() * bytesPerItem(); }
    bool wouldReallocate(size_t items) const;
    int request(size_t items, size_t minItems, double graceMs, size_t *got);
    void shrinkTo(size_t items);
    void lowerTarget(size_t items);
    void releaseAll();
    template <class Tp> Tp *array(int a) const { return (Tp *)base[a]; }
private:
    int reserve(size_t cap, size_t firstTarget); int requestSmall(size_t items, size_t *got); void freeSmall();
    void growLoop(); bool growOneLevel(size_t first); void dropLevels(size_t keepLevels); void stopThread();
};
// path state + sample records + stage events of one pass in flight
struct PassCtx {
    std::unique_ptr<KzArena> arena;                              // the path-state arrays and the five sample planes (jx | jy | r | g | b)
    KzWf wf{};                                                   // (pointers into the arena, set by ctxEnsure)
    float *plane[5] = {};                                        // the five sample planes jx | jy | r | g | b (each its own range of the arena)
    DevBuf<uint32_t> counts;                                     // queue counters of a pass (KzCounts)
    DevBuf<uint32_t> ovf;                                        // the global overflow area of the traversal stacks (ensureOverflow)
    Stream side; Event evFork, evJoin;                           // small passes: the shadow rays of a bounce beside its closest-hit rays (wfPass)
    // A pass run as two HALVES of its pixels side by side (renderOn: KzRenderOpts::passHalves): two views of this context's arrays - the first and the second part
    // of every array - each with its own counters, overflow stacks, side stream and stage clock, the second on a stream of its own. A view owns no arena.
    std::unique_ptr<PassCtx> view[2]; Stream halfStream; Event evHalfFork, evHalfJoin;
    size_t wanted = 0;                                           // items the last call with the default schedule asked this context to hold (kz_render.hip: `earned`)
    uint64_t beamSeen = 0;                                       // the last beam-list build (KzDeviceState::beamSeq) this context's stream has waited for
    std::vector<Event> stageEv; std::vector<int> stageKind; size_t stageUsed = 0;
    size_t items() const { return arena ? arena->mapped.load() : 0; }
    size_t bytes() const { return (arena ? arena->bytes() : 0) + ovf.bytes() + (view[0] ? view[0]->bytes() : 0) + (view[1] ? view[1]->bytes() : 0); }
    // gives the memory back (the context stays usable: it grows again on demand); the caller has synchronised the device
    void release() {
        if (arena) arena->shrinkTo(0);
        wf = KzWf{}; for (float *&q : plane) q = nullptr; wanted = 0;
        ovf.free();
        for (auto &v : view) if (v) v->release();
    }
    // buffers sized for another frame (a pooled context): given back when a call is short of memory (the caller has synchronised the device)
    void trimAux() {
        ovf.free();
        for (auto &v : view) if (v) v->trimAux();
    }
    // (a context that goes - kzCtxPoolTrim, on an idle device - takes its views, buffers, streams, events and arena with it: the members' destructors)
};
// Pass contexts live in a per-device pool between replicas (kz_arena.cpp): a replica takes them on first use and hands them back when it goes.
PassCtx *kzCtxAcquire(int device);
void kzCtxRelease(int device, PassCtx *c);
size_t kzCtxPoolBytes(int device);
size_t kzCtxPoolMaxItems(int device);
size_t kzCtxPoolTrim(int device, size_t keepBytes);
size_t kzCtxPoolTrimPhysical(int hipDevice);      // every idle pooled context that lives on that HIP device (kzMalloc's answer to an out-of-memory)
struct KzDeviceState {
    int device = -1;                                             // the index the caller addresses this replica by
    int hipDevice = -1;                                          // the HIP device it lives on (the same number, unless a development build aliases devices: kz_debug_alias_devices)
    KzDevTables T{};                                             // what the kernels take by value: filled from the tables' owners below
    DevBuf<KzNode> noNodes, bvh2;                                // T.nodes: a placeholder until the BVH2 goes up on first use (kzEnsureBvh2; bvh2Resident)
    DevBuf<KzNode4> nodes4; DevBuf<KzTri> tris, ilTris, emTris; DevBuf<KzTriShade> shade; DevBuf<KzMeshRow> meshes; DevBuf<KzBSDF> bsdfs; DevBuf<KzLightRow> lights;
    DevBuf<float> cdf, pmj, bn, pixelSamples, filter; DevBuf<KzPcgJump> jump;
    DevBuf<KzTexProg> texProgs; DevBuf<KzTexOp> texOps; DevBuf<KzImageRow> images; DevBuf<uint8_t> texels;
    bool bvh2Resident = false;
    // The films (kz_film.h): [0] the picture - its texels there from the upload, its sums from the first render -, [1 + f] the feature film of AOV f (kazen_mi355x_aov.h:
    // 0 albedo, 1 normal, 2 depth), there from the first render with the AOV enabled. filmPixels: the texels of each. evAov[i]: the AOV tap launches of the pass last
    // run in context i (the chain passes in flight order their AOV stages by, wfPass)
    // [4] the second-moment film (kazen_mi355x_variance.h): (w r^2, w g^2, w b^2, w) of the samples the picture receives, there from the first render with the switch on.
    // pictureSamples / momentSamples: samples per pixel the two films have been given since each was last zeroed (the sum of sampleEnd - sampleBegin over renders).
    KzFilm films[5]; size_t filmPixels = 0; Event evAov[KZ_MAX_PASSES_IN_FLIGHT];
    uint32_t pictureSamples = 0, momentSamples = 0;
    KzFilm &picture() { return films[0]; }
    KzFilm &aov(int f) { return films[1 + f]; }
    KzFilm &moment() { return films[4]; }
    size_t aovBytes() const { return films[1].bytes() + films[2].bytes() + films[3].bytes(); }
    // ID mattes (kazen_mi355x_matte.h; kz_matte.hip): per enabled key - [0] mesh, [1] BSDF row - one 64-B record per FRAME pixel, there from the first render with the
    // key, outside the budget, freed when the key leaves the scene's mask. matteSamples: samples per pixel counted since the table was last zeroed (an upper bound:
    // the sum of sampleEnd - sampleBegin over renders). evMatte[i]: the matte stage of the pass last run in context i (a chain of its own, as evAov).
    DevBuf<KzMatteTexel> matte[2]; uint64_t matteSamples[2] = {}; Event evMatte[KZ_MAX_PASSES_IN_FLIGHT];
    size_t matteBytes() const { return matte[0].bytes() + matte[1].bytes(); }
    DevBuf<uint8_t> srgb;                                        // staging raster of kz_film_to_srgb8 / kz_denoise_to_srgb8 (allocated on first use)
    // The denoiser (kazen_mi355x_denoise.h; kz_denoise.hip), allocated by the first kz_denoise outside the pass contexts' budget: frame-sized planes without an
    // apron - the colour plane (e.rgb, valid) twice, the iterations ping-pong between the two; (n.xyz, z); (a.rgb, -) - and the result, laid out like the film.
    // dnValid: dnOut holds the result of a kz_denoise (a snapshot: renders, clears and edits leave it alone).
    DevBuf<float4> dnColor[2], dnNormalZ, dnAlbedo, dnOut; bool dnValid = false;
    size_t dnBytes() const { return dnColor[0].bytes() + dnColor[1].bytes() + dnNormalZ.bytes() + dnAlbedo.bytes() + dnOut.bytes(); }
    // The temporal history (kazen_mi355x_temporal.h), allocated by the first kz_denoise_temporal, outside the budget too: per frame pixel (e.rgb, v) | (n.xyz, z) | N in
    // three planes, twice - a call reads copy tpCur and writes the other. tpFrames: calls folded into it since it started (0: nothing stored); tpO / tpInv: the view it
    // was stored with; tpDemod: whether its colours are demodulated; tpEdits: the scene's geometryEdits then (another value now: stale).
    DevBuf<float4> tpE[2], tpG[2]; DevBuf<float> tpN[2]; int tpCur = 0; uint32_t tpFrames = 0; bool tpDemod = false; uint64_t tpEdits = 0; float tpO[3] = {}, tpInv[9] = {};
    size_t tpBytes() const { size_t b = 0; for (int k = 0; k < 2; ++k) b += tpE[k].bytes() + tpG[k].bytes() + tpN[k].bytes(); return b; }
    // Motion vectors (kazen_mi355x_motion.h). tpBaseEdits / tpXf: the scene's baseEdits and its meshes' matrices (16 floats each) when the history was stored -
    // every call that stores a history records them. mtIds: the mesh id of every frame pixel (kz_motion_ids_kernel, kz_motion.hip), mtRows: the row table of the
    // last kz_denoise_motion that needed one; both allocated on first use, outside the budget, freed by kz_temporal_reset. mtCounts: static / moved / untracked
    // meshes of the last kz_denoise_motion.
    uint64_t tpBaseEdits = 0; std::vector<float> tpXf;
    DevBuf<uint32_t> mtIds; DevBuf<KzMotionRow> mtRows; uint32_t mtCounts[3] = {};
    size_t mtBytes() const { return mtIds.bytes() + mtRows.bytes(); }
    // The fast history (kazen_mi355x_responsive.h): per frame pixel (f.rgb, vf), twice - copy k goes with the history's copy k -, allocated by the first
    // kz_denoise_responsive, outside the budget, freed by kz_temporal_reset. tpStore counts the stores of the history, whichever call made them; rsStore: the store the
    // fast plane was written with (0: none) - another value than tpStore: the plane counts as absent.
    DevBuf<float4> rsF[2]; uint64_t tpStore = 0, rsStore = 0;
    size_t rsBytes() const { return rsF[0].bytes() + rsF[1].bytes(); }
    DevBuf<float4> packDev; DevBuf<KzTileRect> rectsDev;         // kz_film_download_tiles: packed tile rects + their table
    PinnedBuf<float4> packHost;                                  // pinned staging of the same (D2H at link rate)
    // The tile set: pixList = its pixels (tile after tile, 8x8 blocks row-major inside a tile, row-major inside a block), written on the device from the
    // tile descriptors (kz_tiles_expand).
    DevBuf<uint32_t> pixList; uint32_t nPix = 0;
    DevBuf<KzTileDesc> tileDev; PinnedBuf<KzTileDesc> tileHost; Event evTiles;
    std::vector<KzTile> curTiles; std::vector<uint32_t> tilePixOffset;      // tilePixOffset[t]: first list position of tile t (+ the total at the end)
    bool tilesValid = false; uint64_t tileGen = 0;                          // tileGen: bumped whenever the pixel list changes
    DevBuf<unsigned long long> stats; bool statsOn = false;
    hipStream_t lastStream = nullptr;
    int numCU = 256; size_t totalMem = 0;
    PassCtx *ctx[KZ_MAX_PASSES_IN_FLIGHT] = {};                  // taken from the device's pool on first use (ctxAt), handed back by releaseReplica
    PassCtx &ctxAt(int i) { if (!ctx[i]) ctx[i] = kzCtxAcquire(device); return *ctx[i]; }
    std::vector<EventPair> events; size_t eventsUsed = 0;
    Stream passStream[KZ_MAX_PASSES_IN_FLIGHT]; Event evFork, evFilm[KZ_MAX_PASSES_IN_FLIGHT], evCallA, evCallB;
    // LARGE passes with KzRenderOpts::shadowBeside = passHalves = 0: the replica times four passes of one size (evProbe: their first and last event), then keeps
    // the fastest way for its scene (kz_plan.h KzPassMode: the policy and what it has measured).
    Event evProbe[4][2]; KzPassMode passMode;
    int lastCtx = 0; bool lastDual = false; int streamMode = 0;
    PassCtx *lastStageCtx = nullptr;                             // whose stage clock kz_last_stage_ms reads (a view, when the last pass ran as halves)
    // Beam lists (kz_wf_beam), one per pixel of the FRAME, built at most once per pixel and replica - the camera belongs to the scene - whatever tile
    // sets and pixel chunks the pixel is rendered in. They are built on the call's stream (evBeam / beamSeq: the passes wait for the latest build);
    // beamDone remembers the ranges of the CURRENT pixel list that have been handed to the kernel (it skips pixels that already have a list).
    DevBuf<uint2> beamEntries, beamCount; Event evBeam; uint64_t beamSeq = 0;
    std::vector<std::pair<uint32_t, uint32_t>> beamDone; uint64_t beamDoneGen = 0;
    size_t beamBytes() const { return beamCount.cap() * (KZ_BEAM_CAP + 1) * sizeof(uint2); }
    size_t ctxBytes() const { size_t b = 0; for (const PassCtx *c : ctx) if (c) b += c->bytes(); return b; }
    KzPassInfo lastInfo{}; std::string growNote;
    // Edits (kz_refit.hip): the triangles' vertex indices and the BVH4 slot map, uploaded on the replica's first kz_scene_set_vertices (with the BVH2, which the
    // refit keeps resident), a staging area for the vertex data of a batch, and the refit's absolute box padding. editBytes(): what they hold.
    DevBuf<uint32_t> editTriVtx, editSlotSrc; DevBuf<float> editPad, editStage;
    // kz_scene_set_transforms: per mesh its base V (then N) on this replica, there from the replica's first transform of the mesh (kz_scene_set_vertices keeps it current);
    // the flag kz_edit_xform raises for a non-finite position. kz_scene_set_lights: T.ilTris re-allocated once to hold the 64 rows a visibility toggle may need.
    std::vector<DevBuf<float>> editBase; DevBuf<uint32_t> editFlag; bool ilTrisRoomy = false;
    // Adaptive sampling (kazen_mi355x_adaptive.h; kz_adaptive_host.cpp): one record per block of the frame and the byte per block a round's test leaves for the host
    // (read back through adActiveHost), there from the replica's first kz_render_adaptive, outside the budget. adValid: the records are those of a finished adaptive
    // call and nothing has cleared the film since (renderOn without accumulate and kzFilmClear lower it); adBlock / adNbx: the block edge and blocks per row they were
    // made with; adInfo: that call's summary.
    DevBuf<KzAdaptiveBlock> adRec; DevBuf<uint8_t> adActive; PinnedBuf<uint8_t> adActiveHost; bool adValid = false; uint32_t adBlock = 0, adNbx = 0; KzAdaptiveInfo adInfo{};
    Event adEv[4]; float adStageMs[3] = {};                          // the stage clock of a round (moment resolve | classification | read-back) and its sums over the last call's rounds
    size_t adBytes() const { return adRec.bytes() + adActive.bytes(); }
    size_t editBytes() const {
        size_t b = editTriVtx.bytes() + editSlotSrc.bytes() + editPad.bytes() + editStage.bytes() + editFlag.bytes() + (ilTrisRoomy ? ilTris.bytes() : 0);
        for (const DevBuf<float> &e : editBase) b += e.bytes();
        return b;
    }
};
struct KzReplicaSet { std::mutex m; std::vector<KzDeviceState *> v; };

static inline KzReplicaSet *replicaSet(const KzScene *scene) { return (KzReplicaSet *)scene->dev; }
// kz_replica.hip
int findReplica(const KzScene *scene, int device, KzDeviceState **out);
int kzEnsureBvh2(KzScene *scene, KzDeviceState *ds);                                                      // the BVH2 table, on first use
// kz_motion.hip
int kzMotionIds(KzScene *scene, KzDeviceState *ds);                                                       // ds->mtIds: the mesh id of every frame pixel of the scene as it stands (returns with the device idle)
// kz_matte.hip: the tables of the enabled keys before the passes of a call, every table zeroed, and the matte stage of one pass (items nPix x S, pixel-major, first hits at `hit`)
int kzMatteEnsure(KzScene *scene, KzDeviceState *ds, bool accumulate, uint32_t nSamples, hipStream_t stream);
int kzMatteClear(KzDeviceState *ds, hipStream_t stream);
int kzMatteStage(KzScene *scene, KzDeviceState *ds, hipStream_t stream, const float4 *hit, const uint32_t *pixList, uint32_t nPix, uint32_t S, hipEvent_t wait, hipEvent_t record);
int kzEmitterUpload(KzScene *scene, KzDeviceState *ds);                                                   // the emitter triangles, their count and box (upload and every edit of a light)
int prepareTiles(KzScene *scene, KzDeviceState *ds, const KzTile *tiles, uint32_t nTiles, hipStream_t stream);      // makes `tiles` the replica's tile set
static inline int requireDevice(KzScene *scene, KzDeviceState **out) { return findReplica(scene, -1, out); }
// kz_render.hip: the replica a render call's opts->device addresses (a scene resident on ONE device is addressed by any zero-initialised opts), and the render of one
// call on it - kz_render is the two in a row; kz_render_adaptive (kz_adaptive_host.cpp) renders every round through the second
int kzRenderReplica(KzScene *scene, const KzRenderOpts *opts, KzDeviceState **out);
int kzRenderOn(KzScene *scene, KzDeviceState *ds, const KzRenderOpts *opts);
// kz_adaptive_host.cpp: the rule's numbers from a caller's options, defaults filled in (sceneSamples 0: no scene - maxSamples stays as given, 0 = no cap known); a bad
// field: KZ_ERR_INVALID_ARG under `call`'s name. kz_adaptive.hip: the test of one round on `stream` - film and moment resolved, rec and active one entry per block.
struct KzAdaptiveRule { float threshold, thr2, floor; uint32_t minSamples, maxSamples, step, block, permille; };
int kzAdaptiveResolve(const KzAdaptiveOpts *aopts, uint32_t sceneSamples, const char *call, KzAdaptiveRule *rule);
int kzAdaptiveClassify(const float4 *film, const float4 *moment, int32_t width, int32_t height, int32_t border, const KzAdaptiveRule &rule, const uint32_t *blockSamples, uint32_t nAll,
                       KzAdaptiveBlock *rec, uint8_t *active, hipStream_t stream);
// kz_film.hip
size_t packedFloats(const KzParams &P, const KzTile *tiles, uint32_t nTiles);
int checkTiles(const KzParams &P, const KzTile *tiles, uint32_t nTiles);
int downloadTiles(KzScene *scene, KzDeviceState *ds, KzFilm &film, const KzTile *tiles, uint32_t nTiles, float *packed, size_t nFloats, hipStream_t stream);      // the rects of `film`
// The film machine (kz_film.hip), each function for the film it is handed: kzFilmEnsure before the passes of a call (KzFilm::ensure with the scene's geometry), kzFilmStage
// after every pass (ImageBlock::put for the pass's sample records - five planes jx | jy | r | g | b - into the film's running tap sums, launched on `pst` behind `waitFilm`;
// isSigned: a feature film's values, which may be negative), kzFilmResolve once per call and wherever a feature film is read (the texels from the sums).
#define KZ_TAPS_CHUNK1 8                     // samples per staging round with one lane per pixel (32-B pieces of every sample row; round 2's kernel)
#define KZ_TAPS_CHUNK 16                     // ... with several lanes per pixel: 64-B pieces = whole HBM sectors (profiles/r05h_film_taps)
#define KZ_FILM_GRID 64                      // the canonical tile grid of the resolve = kz_deal_tiles' default tile: the film of one device equals the host merge of its tiles' rects bit for bit
int kzFilmEnsure(KzScene *scene, KzFilm &film, size_t filmPixels, bool accumulate, hipStream_t stream);
int kzFilmClear(KzDeviceState *ds, hipStream_t stream);          // every film of the replica: the picture's sums and texels, then each feature film's
int kzFilmStage(KzScene *scene, KzDeviceState *ds, KzFilm &film, bool isSigned, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *const plane[5], hipEvent_t waitFilm, int lanesPerPixel);
int kzFilmResolve(KzScene *scene, KzFilm &film, hipStream_t stream);
// The second-moment film's stage of a pass, on the picture's stream with its pixel list and sample planes: behind the picture's tap launch (onePass = false), or in
// its place, feeding both films from one read of the planes (onePass = true, filters kzFilmMomentOnePassOk accepts; waits for `waitFilm` as kzFilmStage does)
bool kzFilmMomentOnePassOk(const KzParams &P);
int kzFilmStageMoment(KzScene *scene, KzDeviceState *ds, KzFilm &picture, KzFilm &moment, bool onePass, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *const plane[5], hipEvent_t waitFilm);
// The float planes a pass's features go to: three per feature (p[0] albedo, p[1] normal, p[2] depth replicated), `stride` floats apart. They alias the shadow
// arrays of the pass context (wfAov, kz_render.hip), which are dead between the camera stage and the first shade / ao / mats launch.
struct KzAovPlanes { float *p[3]; size_t stride; };
// The 8-bit sRGB raster of a film-shaped device buffer of the replica (kz_film_srgb8 on ds->lastStream, through ds->srgb): kz_film_to_srgb8 and kz_denoise_to_srgb8
int kzFilmSrgb8(KzScene *scene, KzDeviceState *ds, const float4 *film, uint8_t *rgb8, size_t nBytes);
