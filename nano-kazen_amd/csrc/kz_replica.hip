// kz_replica.hip - replicas: one device state per GPU a scene is resident on. Their lifetime and upload (kz_scene_upload / kz_scene_evict), every device
// allocation of the library (kzMalloc), the tile set of a call (prepareTiles: kz_tiles_expand writes the pixel list on the device), and the entry points that
// only read what a replica holds: kz_last_*, kz_pass_mode_info, kz_sync*, the counters. What RUNS on a replica - a pass - is kz_render.hip.
#include <hip/hip_runtime.h>

#include "kz_state.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>

// Every device allocation of the library goes through here. Out of memory: the idle pass contexts of the device's pool (up to 3/4 of the card, parked there by
// replicas that have gone) are given back and the allocation is tried once more - tables, film and beam lists of the NEXT scene must not fail because the
// last one's path state is still mapped. (Development builds: kz_debug_fail_alloc makes the nth allocation of the calling thread fail.)
#ifdef KZ_EXPERIMENTS
thread_local int g_failAlloc = 0;
// kz_debug_fail_device: a countdown per (logical) device, handed to whichever thread addresses that device's replica next (findReplica) - so that a test can fail an
// allocation inside ONE device thread of kz_render_multi, which no caller's thread-local countdown reaches
static std::atomic<int> g_failDevice[64];
#endif
// Makes the device a caller addresses by `device` current, for the entry points that take a device index and no scene.
int kzUseDevice(int device) {
    const int n = kzLogicalDeviceCount();
    if (device < 0 || device >= n) return kz_fail(n ? KZ_ERR_INVALID_ARG : KZ_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(kzPhysicalDevice(device)));
    return KZ_OK;
}
hipError_t kzMalloc(void **p, size_t bytes) {
    *p = nullptr;
#ifdef KZ_EXPERIMENTS
    if (g_failAlloc > 0 && --g_failAlloc == 0) return hipErrorOutOfMemory;
#endif
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && kzCtxPoolTrimPhysical(dev) > 0) e = hipMalloc(p, bytes);
    }
    return e;
}

// A device table for `v` in its owner (a valid dummy of at least 256 bytes when it is empty, so kernels never see null); not yet filled unless empty.
template <class Tp> static int allocVec(DevBuf<Tp> &buf, const std::vector<Tp> &v, const Tp **out) {
    *out = nullptr;
    if (const int rc = buf.alloc(v.empty() ? (256 + sizeof(Tp) - 1) / sizeof(Tp) : v.size())) return rc;
    if (v.empty()) HIP_TRY(hipMemset(buf, 0, buf.bytes()));
    *out = buf;
    return KZ_OK;
}
template <class Tp> static int uploadVec(DevBuf<Tp> &buf, const std::vector<Tp> &v, const Tp **out) {
    if (const int rc = allocVec(buf, v, out)) return rc;
    return v.empty() ? KZ_OK : buf.upload(v.data(), v.size());
}

// The emitter triangles of the roulette-ahead test (kz_host.cpp kzEmitterTris) on one replica: room for KZ_EM_MAX rows + the header row from the start, so
// that an edit only copies; the count and the box travel in the kernel argument. The caller has made the replica's device current.
int kzEmitterUpload(KzScene *scene, KzDeviceState *ds) {
    if (!ds->emTris) {
        if (const int rc = ds->emTris.alloc(KZ_EM_MAX + 1)) return rc;
        HIP_TRY(hipMemset(ds->emTris, 0, ds->emTris.bytes()));
        ds->T.emTris = ds->emTris;
    }
    if (!scene->emTris.empty() && scene->emTris.size() <= KZ_EM_MAX + 1)
        if (const int rc = ds->emTris.upload(scene->emTris.data(), scene->emTris.size())) return rc;
    ds->T.nEmTris = scene->nEmTris;
    for (int a = 0; a < 3; ++a) { ds->T.emLo[a] = scene->emLo[a]; ds->T.emHi[a] = scene->emHi[a]; }
    return KZ_OK;
}

// The replica goes, and with it everything its members own (kz_own.h); its pass contexts go back to the device's pool, memory and all.
static void releaseReplica(KzDeviceState *ds) {
    (void)hipSetDevice(ds->hipDevice);
    (void)hipDeviceSynchronize();
    for (PassCtx *&c : ds->ctx) if (c) { kzCtxRelease(ds->device, c); c = nullptr; }
    delete ds;
}

void kz_device_init(KzScene *scene) { scene->dev = new KzReplicaSet(); }

void kz_device_release(KzScene *scene) {
    KzReplicaSet *rs = replicaSet(scene);
    if (!rs) return;
    for (KzDeviceState *ds : rs->v) releaseReplica(ds);
    delete rs;
    scene->dev = nullptr;
}

int findReplica(const KzScene *scene, int device, KzDeviceState **out) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "null scene");
    KzReplicaSet *rs = replicaSet(scene);
    KzDeviceState *ds = nullptr;
    if (rs) {
        std::lock_guard<std::mutex> g(rs->m);
        if (device < 0) ds = rs->v.empty() ? nullptr : rs->v.front();
        else for (KzDeviceState *d : rs->v) if (d->device == device) { ds = d; break; }
    }
    if (!ds) {
        if (device < 0 || !rs || rs->v.empty()) return kz_fail(KZ_ERR_STATE, "scene is not on a device: call kz_scene_upload first");
        return kz_fail(KZ_ERR_STATE, "scene is not resident on device %d: call kz_scene_upload(scene, %d) first", device, device);
    }
    hipError_t e = hipSetDevice(ds->hipDevice);
    if (e != hipSuccess) return kz_fail(KZ_ERR_HIP, "hipSetDevice(%d): %s", ds->hipDevice, hipGetErrorString(e));
#ifdef KZ_EXPERIMENTS
    { const int n = g_failDevice[ds->device & 63].exchange(0); if (n > 0) g_failAlloc = n; }
#endif
    *out = ds;
    return KZ_OK;
}

static int uploadReplica(KzScene *scene, KzDeviceState *ds) {
    int rc;
    KZ_TRACE("upload: start (%.1f MB of tables)", (scene->nodes.size() * sizeof(scene->nodes[0]) + scene->nodes4.size() * sizeof(scene->nodes4[0]) + scene->tris.size() * sizeof(scene->tris[0]) + scene->shade.size() * sizeof(scene->shade[0])) / 1e6);
    // The four large tables (C4: 248 MB; their allocations first, in this thread, so that a failure is this call's) travel side by side: a pageable copy is
    // a chain of host memcpys into the runtime's pinned staging buffers and DMA transfers out of them, one chain per calling thread - one thread per table in
    // flight took the upload of C4 from 45 to 36 ms (profiles/r05d_cold_job; finer pieces over eight threads change nothing - round 6: ~32 ms of an upload are
    // fixed costs of a process's first allocations, the 8 MB scene of the reference's own file takes as long -; the FIRST process on a freshly leased box spends 170 ms here either way: the
    // first transfers of a box wake something up that no later process pays for)
    {
        struct Job { const void *src; void *dst; size_t bytes; hipError_t err; };
        Job jobs[4] = {};
        auto prep = [&](auto &buf, auto &vec, auto **out, Job &j) -> int {
            const int rc_ = allocVec(buf, vec, out);
            j.src = vec.empty() ? nullptr : (const void *)vec.data(); j.dst = (void *)*out; j.bytes = buf.bytes();
            return rc_;
        };
        // (the BVH2 - C4: 62 MB of the 248 - serves the reference-shaped megakernel, kz_trace_rays and kz_render_samples only: it goes up on the first of those
        //  calls, kzEnsureBvh2; a one-frame job through the wavefront pipeline never pays for it)
        static const std::vector<KzNode> noNodes;
        if ((rc = prep(ds->noNodes, noNodes, &ds->T.nodes, jobs[0]))) return rc;
        if ((rc = prep(ds->nodes4, scene->nodes4, &ds->T.nodes4, jobs[1]))) return rc;
        if ((rc = prep(ds->tris, scene->tris, &ds->T.tris, jobs[2]))) return rc;
        if ((rc = prep(ds->shade, scene->shade, &ds->T.shade, jobs[3]))) return rc;
        std::vector<std::thread> th;
        const int dev = ds->hipDevice;
        for (Job &j : jobs) if (j.src && j.bytes >= ((size_t)4 << 20)) th.emplace_back([&j, dev] { j.err = hipSetDevice(dev); if (j.err == hipSuccess) j.err = hipMemcpy(j.dst, j.src, j.bytes, hipMemcpyHostToDevice); });
        for (Job &j : jobs) if (j.src && j.bytes < ((size_t)4 << 20)) j.err = hipMemcpy(j.dst, j.src, j.bytes, hipMemcpyHostToDevice);
        for (std::thread &t : th) t.join();
        for (Job &j : jobs) if (j.err != hipSuccess) return kz_fail(KZ_ERR_HIP, "upload of a scene table (%zu bytes) failed: %s", j.bytes, hipGetErrorString(j.err));
    }
    KZ_TRACE("upload: nodes, nodes4, tris, shade there");
    if ((rc = uploadVec(ds->meshes, scene->meshRows, &ds->T.meshes)) || (rc = uploadVec(ds->bsdfs, scene->bsdfs, &ds->T.bsdfs)) || (rc = uploadVec(ds->lights, scene->lightRows, &ds->T.lights)) ||
        (rc = uploadVec(ds->cdf, scene->cdf, &ds->T.cdf)) || (rc = uploadVec(ds->pmj, scene->pmj, &ds->T.pmj)) || (rc = uploadVec(ds->bn, scene->bn, &ds->T.bn)) ||
        (rc = uploadVec(ds->pixelSamples, scene->pixelSamples, &ds->T.pixelSamples)) || (rc = uploadVec(ds->jump, scene->jump, &ds->T.jump))) return rc;
    std::vector<float> ft(scene->filter, scene->filter + KZ_FILTER_RESOLUTION + 1);
    if ((rc = uploadVec(ds->filter, ft, &ds->T.filter))) return rc;
    if ((rc = uploadVec(ds->ilTris, scene->ilTris, &ds->T.ilTris))) return rc;
    if ((rc = kzEmitterUpload(scene, ds))) return rc;
    if ((rc = uploadVec(ds->texProgs, scene->texProgs, &ds->T.texProgs)) || (rc = uploadVec(ds->texOps, scene->texOps, &ds->T.texOps)) ||
        (rc = uploadVec(ds->images, scene->images, &ds->T.images)) || (rc = uploadVec(ds->texels, scene->texels, &ds->T.texels))) return rc;
    ds->T.texPow2 = scene->texPow2;
    const KzParams &P = scene->prm;
    ds->filmPixels = (size_t)(P.width + 2 * P.border) * (size_t)(P.height + 2 * P.border);
    KZ_TRACE("upload: small tables there");
    if ((rc = ds->picture().texels.alloc(ds->filmPixels))) return rc;      // (the picture's sums: its first render)
    HIP_TRY(hipMemset(ds->picture().texels, 0, ds->filmPixels * sizeof(float4)));
    if ((rc = ds->stats.alloc(32))) return rc;                         // 8 counters of KzStats + 16 lane statistics of the -DKZ_LANESTAT development build + 3 beam-list counters
    HIP_TRY(hipMemset(ds->stats, 0, 32 * sizeof(unsigned long long)));
    { hipDeviceProp_t prop; HIP_TRY(hipGetDeviceProperties(&prop, ds->hipDevice)); ds->numCU = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; ds->totalMem = prop.totalGlobalMem; }
    KZ_TRACE("upload: film + counters there");
    HIP_TRY(hipDeviceSynchronize());
    KZ_TRACE("upload: done");
    return KZ_OK;
}

// The BVH2 table of a replica, on first use (see uploadReplica). The caller has made the replica's device current.
int kzEnsureBvh2(KzScene *scene, KzDeviceState *ds) {
    if (ds->bvh2Resident || scene->nodes.empty()) return KZ_OK;
    kzHostSync(scene);                                  // (the host BVH2 follows the last edit before it goes up)
    int rc;
    if ((rc = ds->bvh2.alloc(scene->nodes.size()))) return rc;
    if ((rc = ds->bvh2.upload(scene->nodes.data(), scene->nodes.size()))) return rc;      // (blocking, behind everything queued on the device: a rare call)
    ds->T.nodes = ds->bvh2;
    ds->bvh2Resident = true;
    return KZ_OK;
}

// The pixel list of a tile set (tile after tile; 8x8 blocks row-major inside a tile, row-major inside a block: a wave of 64 list entries is an 8x8
// block of the image), written on the device from the tile descriptors: one thread per list entry finds its tile by bisection over the tiles' first positions.
__global__ __launch_bounds__(256) void kz_tiles_expand(const KzTileDesc *__restrict__ tiles, uint32_t nTiles, uint32_t nPix, int width,
                                                       uint32_t *__restrict__ pixList) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nPix) return;
    uint32_t lo = 0, hi = nTiles;                          // the last tile whose pixOffset <= i
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tiles[mid].pixOffset <= i) lo = mid; else hi = mid; }
    const KzTileDesc t = tiles[lo];
    const uint32_t local = i - t.pixOffset, w = (uint32_t)t.w, h = (uint32_t)t.h;
    const uint32_t r = local / (8u * w), rem = local - r * 8u * w, hb = min(8u, h - 8u * r);       // block row r holds hb rows of the tile
    const uint32_t c = rem / (8u * hb), rem2 = rem - c * 8u * hb, wb = min(8u, w - 8u * c);        // block c of that row is wb pixels wide
    const uint32_t yl = rem2 / wb, xl = rem2 - yl * wb;
    const uint32_t x = (uint32_t)t.x0 + 8u * c + xl, y = (uint32_t)t.y0 + 8u * r + yl;
    pixList[i] = x | (y << 16);
}

// Makes `tiles` the replica's tile set. Nothing here waits for the device: the descriptors go up through the call's stream, behind the end of the
// previous call (evCallB), and the expansion kernel runs there - a change of tile set costs a few microseconds of host time and ~30 us of device
// time, where it used to synchronise every stream, build the list on the host and copy it with a blocking pageable copy.
int prepareTiles(KzScene *scene, KzDeviceState *ds, const KzTile *tiles, uint32_t nTiles, hipStream_t stream) {
    const KzParams &P = scene->prm;
    KzTile whole = {0, 0, P.width, P.height};
    if (!tiles || nTiles == 0) { tiles = &whole; nTiles = 1; }
    bool same = ds->tilesValid && ds->curTiles.size() == nTiles && std::memcmp(ds->curTiles.data(), tiles, nTiles * sizeof(KzTile)) == 0;
    if (same) return KZ_OK;
    // bounds, then overlaps: tiles on the 8-px grid (every tile the library deals) are marked on a coarse occupancy map, others compared pairwise
    std::vector<KzTileDesc> desc(nTiles);
    std::vector<uint32_t> offs(nTiles + 1);
    bool grid = true;
    uint64_t total = 0;
    if (const int rc = checkTiles(P, tiles, nTiles)) return rc;
    for (uint32_t t = 0; t < nTiles; ++t) {
        const KzTile &tl = tiles[t];
        if ((tl.x0 & 7) || (tl.y0 & 7) || ((tl.w & 7) && tl.x0 + tl.w != P.width) || ((tl.h & 7) && tl.y0 + tl.h != P.height)) grid = false;
        desc[t] = KzTileDesc{tl.x0, tl.y0, tl.w, tl.h, (uint32_t)total};
        offs[t] = (uint32_t)total;
        total += (uint64_t)tl.w * (uint64_t)tl.h;
    }
    offs[nTiles] = (uint32_t)total;
    if (total > (uint64_t)P.width * (uint64_t)P.height) return kz_fail(KZ_ERR_INVALID_ARG, "tiles overlap (%llu pixels in a %dx%d image)", (unsigned long long)total, P.width, P.height);
    if (grid) {
        const int gw = (P.width + 7) / 8, gh = (P.height + 7) / 8;
        std::vector<uint8_t> occ((size_t)gw * gh, 0);
        for (uint32_t t = 0; t < nTiles; ++t) {
            const KzTile &tl = tiles[t];
            for (int gy = tl.y0 / 8; gy < (tl.y0 + tl.h + 7) / 8; ++gy)
                for (int gx = tl.x0 / 8; gx < (tl.x0 + tl.w + 7) / 8; ++gx) {
                    uint8_t &o = occ[(size_t)gy * gw + gx];
                    if (o) return kz_fail(KZ_ERR_INVALID_ARG, "tiles overlap at pixel (%d,%d)", gx * 8, gy * 8);
                    o = 1;
                }
        }
    } else {
        for (uint32_t a = 0; a < nTiles; ++a) for (uint32_t b2 = a + 1; b2 < nTiles; ++b2) {
            const KzTile &A = tiles[a], &B = tiles[b2];
            if (A.x0 < B.x0 + B.w && B.x0 < A.x0 + A.w && A.y0 < B.y0 + B.h && B.y0 < A.y0 + A.h)
                return kz_fail(KZ_ERR_INVALID_ARG, "tiles overlap at pixel (%d,%d)", std::max(A.x0, B.x0), std::max(A.y0, B.y0));
        }
    }
    const size_t framePix = (size_t)P.width * P.height;
    if (ds->pixList.cap() < framePix || ds->tileDev.cap() < nTiles) {          // first use (or a longer tile list than ever before): allocate
        HIP_TRY(hipDeviceSynchronize());
        int rc;
        if (ds->pixList.cap() < framePix && (rc = ds->pixList.regrow(framePix))) return rc;
        if (ds->tileDev.cap() < nTiles && (rc = ds->tileDev.regrow(std::max<size_t>(nTiles, 4096)))) return rc;
    }
    ds->tilesValid = false;
    if (ds->evCallB) HIP_TRY(hipStreamWaitEvent(stream, ds->evCallB, 0));        // behind everything the previous call (on whatever stream) queued
    // the descriptors travel through a pinned buffer of the replica (the copy of the previous tile set has left it: evTiles)
    if (ds->tileHost.cap() < nTiles) {
        if (ds->evTiles) HIP_TRY(hipEventSynchronize(ds->evTiles));
        if (const int rc = ds->tileHost.regrow(std::max<size_t>(nTiles, 4096))) return rc;
    }
    if (!ds->evTiles) { if (const int rc = ds->evTiles.ensure(hipEventDisableTiming)) return rc; }
    else HIP_TRY(hipEventSynchronize(ds->evTiles));
    std::memcpy(ds->tileHost, desc.data(), nTiles * sizeof(KzTileDesc));
    HIP_TRY(hipMemcpyAsync(ds->tileDev, ds->tileHost, nTiles * sizeof(KzTileDesc), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ds->evTiles, stream));
    hipLaunchKernelGGL(kz_tiles_expand, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const KzTileDesc *)ds->tileDev.get(), nTiles, (uint32_t)total, P.width, ds->pixList);
    HIP_TRY(hipGetLastError());
    ds->nPix = (uint32_t)total;
    ds->curTiles.assign(tiles, tiles + nTiles);
    ds->tilePixOffset = std::move(offs);
    ds->tilesValid = true; ++ds->tileGen;
    return KZ_OK;
}

extern "C" {

#ifdef KZ_EXPERIMENTS
void kz_debug_fail_alloc(int nth) { g_failAlloc = nth > 0 ? nth : 0; }
void kz_debug_fail_device(int device, int nth) { g_failDevice[device & 63].store(nth > 0 ? nth : 0); }
#endif

int kz_device_count(void) { return kzLogicalDeviceCount(); }

int kz_device_mem_info(int device, uint64_t *freeBytes, uint64_t *totalBytes) {
    if (const int rc = kzUseDevice(device)) return rc;
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (freeBytes) *freeBytes = f;
    if (totalBytes) *totalBytes = t;
    return KZ_OK;
}

int kz_scene_upload(KzScene *scene, int device) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "null scene");
    const int n = kzLogicalDeviceCount();
    if (n <= 0) return kz_fail(KZ_ERR_NO_DEVICE, "no HIP device visible (the product path has no CPU fallback)");
    if (device < 0 || device >= n) return kz_fail(KZ_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, n);
    KzReplicaSet *rs = replicaSet(scene);
    {
        std::lock_guard<std::mutex> g(rs->m);
        for (KzDeviceState *d : rs->v) if (d->device == device) return KZ_OK;       // already resident
    }
    KZ_TRACE("kz_scene_upload(%d)", device);
    HIP_TRY(hipSetDevice(kzPhysicalDevice(device)));
    KZ_TRACE("upload: hipSetDevice done");
    kzHostSync(scene);                                  // (the tables follow the last edit before they go up)
    KzDeviceState *ds = new KzDeviceState();
    ds->device = device; ds->hipDevice = kzPhysicalDevice(device);
    const int rc = uploadReplica(scene, ds);
    if (rc) { releaseReplica(ds); return rc; }
    std::lock_guard<std::mutex> g(rs->m);
    for (KzDeviceState *d : rs->v) if (d->device == device) { releaseReplica(ds); return KZ_OK; }     // lost a race for the same device
    rs->v.push_back(ds);
    return KZ_OK;
}

int kz_scene_evict(KzScene *scene, int device) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "null scene");
    KzReplicaSet *rs = replicaSet(scene);
    std::vector<KzDeviceState *> gone;
    {
        std::lock_guard<std::mutex> g(rs->m);
        for (size_t i = 0; i < rs->v.size();) {
            if (device < 0 || rs->v[i]->device == device) { gone.push_back(rs->v[i]); rs->v.erase(rs->v.begin() + i); } else ++i;
        }
    }
    if (gone.empty() && device >= 0) return kz_fail(KZ_ERR_STATE, "scene is not resident on device %d", device);
    for (KzDeviceState *d : gone) releaseReplica(d);
    return KZ_OK;
}

int kz_scene_devices(const KzScene *scene, int32_t *devices, uint32_t cap, uint32_t *count) {
    if (!scene || !count) return kz_fail(KZ_ERR_INVALID_ARG, "null argument");
    KzReplicaSet *rs = replicaSet(scene);
    std::lock_guard<std::mutex> g(rs->m);
    *count = (uint32_t)rs->v.size();
    for (uint32_t i = 0; i < *count && i < cap && devices; ++i) devices[i] = rs->v[i]->device;
    return KZ_OK;
}

// Device time of the stages of the LAST pass of the last kz_render (wavefront pipeline), from hipEvents on the launch stream:
// out[0] generate, [1] closest-hit traversal of the BOUNCE rays (the kz_wf_trace<0> launches), [2] shade, [3] shadow traversal, [4] film,
// [5] camera rays (kz_wf_beam when the lists are rebuilt, kz_wf_trace_list, kz_wf_trace_packet, the first-hit walk-through).
int kz_last_stage_ms(KzScene *scene, float *out6) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!out6) return kz_fail(KZ_ERR_INVALID_ARG, "null out");
    for (int i = 0; i < 6; ++i) out6[i] = 0.f;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    const PassCtx &c = ds->lastStageCtx ? *ds->lastStageCtx : ds->ctxAt(ds->lastCtx);
    for (size_t i = 1; i < c.stageUsed; ++i) {
        float t = 0; HIP_TRY(hipEventElapsedTime(&t, c.stageEv[i - 1], c.stageEv[i]));
        const int k = c.stageKind[i];
        if (k >= 0 && k < 6) out6[k] += t;
    }
    return KZ_OK;
}

// Why the pass context of the last kz_render stopped growing short of its target, if it did ("" otherwise): the call itself succeeds on what there is.
int kz_last_grow_note(KzScene *scene, char *buf, size_t cap) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!buf || !cap) return kz_fail(KZ_ERR_INVALID_ARG, "null buffer");
    std::snprintf(buf, cap, "%s", ds->growNote.c_str());
    return KZ_OK;
}

int kz_last_pass_info(KzScene *scene, KzPassInfo *out) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!out) return kz_fail(KZ_ERR_INVALID_ARG, "null out");
    *out = ds->lastInfo;
    out->contextItems = ds->ctx[0] ? ds->ctx[0]->items() : 0;
    return KZ_OK;
}

// What the replica on `device` (-1: the primary one) has measured about its large passes (kz_plan.h KzPassMode: KzRenderOpts::shadowBeside / passHalves at 0).
int kz_pass_mode_info(KzScene *scene, int device, KzPassModeInfo *out) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!out) return kz_fail(KZ_ERR_INVALID_ARG, "null out");
    *out = KzPassModeInfo{};
    const KzPassMode &m = ds->passMode;
    out->kept = m.kept; out->timedPasses = (uint32_t)m.launched; out->items = m.items[0];
    if (m.kept >= 0) { out->msOneStream[0] = m.ms[0]; out->msOneStream[1] = m.ms[3]; out->msShadowBeside = m.ms[1]; out->msHalves = m.ms[2]; }
    return KZ_OK;
}

int kz_sync_on(KzScene *scene, int device) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    return KZ_OK;
}
int kz_sync(KzScene *scene) { return kz_sync_on(scene, -1); }

int kz_last_kernel_ms(KzScene *scene, float *ms) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!ms) return kz_fail(KZ_ERR_INVALID_ARG, "null ms");
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    if (ds->lastDual && ds->lastInfo.passes) {          // passes overlap: the per-pass figure is the span of the call over its passes (film included)
        float t = 0; HIP_TRY(hipEventElapsedTime(&t, ds->evCallA, ds->evCallB));
        *ms = t / (float)ds->lastInfo.passes;
        return KZ_OK;
    }
    double tot = 0;
    for (size_t i = 0; i < ds->eventsUsed; ++i) { float t = 0; HIP_TRY(hipEventElapsedTime(&t, ds->events[i].a, ds->events[i].b)); tot += t; }
    *ms = ds->eventsUsed ? (float)(tot / ds->eventsUsed) : 0.f;
    return KZ_OK;
}

int kz_set_stats(KzScene *scene, int enable) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    ds->statsOn = enable != 0;
    return KZ_OK;
}

int kz_get_stats(KzScene *scene, KzStats *out, int reset) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    if (!out) return kz_fail(KZ_ERR_INVALID_ARG, "null out");
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    unsigned long long h[8];
    HIP_TRY(hipMemcpy(h, ds->stats, sizeof h, hipMemcpyDeviceToHost));
    { unsigned long long b[3]; HIP_TRY(hipMemcpy(b, ds->stats + 24, sizeof b, hipMemcpyDeviceToHost)); out->beamPixels = b[0]; out->beamListEntries = b[1]; out->beamCompletePixels = b[2];
      if (reset) HIP_TRY(hipMemset(ds->stats + 24, 0, sizeof b)); }
    out->samples = h[0]; out->rays = h[1]; out->nodeVisits = h[2]; out->triTests = h[3]; out->shadedHits = h[4]; out->lightSamples = h[5]; out->droppedSamples = h[6];
#ifdef KZ_LANESTAT
    {
        unsigned long long ls[16];
        HIP_TRY(hipMemcpy(ls, ds->stats + 8, sizeof ls, hipMemcpyDeviceToHost));
        for (int m = 0; m < 2; ++m) {
            const unsigned long long *a = ls + 8 * m;
            std::fprintf(stderr, "lanestat %s: node iters %llu  active/iter %.2f  inner/iter %.2f | leaf phases %llu  lanes/phase %.2f  tri iters/phase %.2f | refills %llu  lanes/refill %.2f\n",
                         m ? "shadow " : "closest", a[0], a[0] ? (double)a[1] / a[0] : 0.0, a[0] ? (double)a[2] / a[0] : 0.0, a[3], a[3] ? (double)a[4] / a[3] : 0.0,
                         a[3] ? (double)a[7] / a[3] : 0.0, a[5], a[5] ? (double)a[6] / a[5] : 0.0);
        }
        if (reset) HIP_TRY(hipMemset(ds->stats + 8, 0, sizeof ls));
    }
#endif
#ifdef KZ_TRACESTAT
    {
        unsigned long long ts[10];
        HIP_TRY(hipMemcpy(ts, ds->stats + 8, sizeof ts, hipMemcpyDeviceToHost));
        for (int m = 0; m < 2; ++m) {
            const unsigned long long *a = ts + 4 * m; const double tot = (double)(a[0] + a[1] + a[2] + a[3]);
            std::fprintf(stderr, "tracestat %s: refill %.2f %%  node phase %.2f %%  leaf phase (+ pop / finish) %.2f %% (triangle loop alone %.2f %%)  loop %.2f %%\n", m ? "shadow " : "closest",
                         tot > 0 ? 100.0 * a[0] / tot : 0.0, tot > 0 ? 100.0 * a[1] / tot : 0.0, tot > 0 ? 100.0 * a[2] / tot : 0.0, tot > 0 ? 100.0 * ts[8 + m] / tot : 0.0, tot > 0 ? 100.0 * a[3] / tot : 0.0);
        }
        if (reset) HIP_TRY(hipMemset(ds->stats + 8, 0, sizeof ts));
    }
#endif
#ifdef KZ_SHADESTAT
    {
        unsigned long long ss[14]; double tot = 0;
        HIP_TRY(hipMemcpy(ss, ds->stats + 8, sizeof ss, hipMemcpyDeviceToHost));
        static const char *nm[14] = {"passA: rest (emitter, classification, roulette)", "compact+barrier", "B:loads+setup", "B:light draws+sample", "B:eval+pdf+shadow stores", "B:bsdf draws", "B:bsdf sample", "B:next-ray stores",
                                     "barrier+staging+flush", "loop head", "passA: queue+hit+ray loads", "passA: shading record arrives", "passA: postIntersect", "-"};
        for (int k = 0; k < 14; ++k) tot += (double)ss[k];
        for (int k = 0; k < 14; ++k) std::fprintf(stderr, "shadestat %-48s %6.2f %%\n", nm[k], tot > 0 ? 100.0 * (double)ss[k] / tot : 0.0);
        if (reset) HIP_TRY(hipMemset(ds->stats + 8, 0, sizeof ss));
    }
#endif
    if (reset) HIP_TRY(hipMemset(ds->stats, 0, sizeof h));
    return KZ_OK;
}

} // extern "C"
