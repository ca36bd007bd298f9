// kz_matte.hip - include_ext/kazen_mi355x_matte.h: the ID-matte tables of a replica (KzDeviceState::matte), the stage of a pass that feeds them (kzMatteStage, launched by
// wfPass where wfAov is launched), what reads them (rank, layer, top) and the test surface kz_matte_accumulate_items. The kernels are kz_matte.h's; this unit is
// compiled as the render units are (build.sh DEVICE_UNITS).
#include "kz_state.h"
#include "kz_matte.h"

#include <algorithm>
#include <cstring>
#include <vector>

static int matteKeyIndex(uint32_t key) { return key == KZ_MATTE_MESH ? 0 : 1; }
static unsigned matteBlocks(const KzDeviceState *ds, size_t units) { return (unsigned)std::max<size_t>(1, std::min<size_t>((units + KZ_BLOCK - 1) / KZ_BLOCK, (size_t)ds->numCU * 8)); }

// SRC 0 / 1 x the two forms. lanes: one lane per pixel (S < 64 in a render), else one wave per pixel.
template <int SRC>
static int matteLaunch(const KzDeviceState *ds, hipStream_t stream, bool lanes, const KzTriShade *shade, const float4 *hit, const uint32_t *keys, const uint32_t *pixList,
                       uint32_t nPix, uint32_t S, uint32_t width, KzMatteTexel *t0, KzMatteTexel *t1) {
    if (lanes) hipLaunchKernelGGL(kz_matte_accumulate_lane<SRC>, dim3(matteBlocks(ds, nPix)), dim3(KZ_BLOCK), 0, stream, shade, hit, keys, pixList, nPix, S, width, t0, t1);
    else hipLaunchKernelGGL(kz_matte_accumulate<SRC>, dim3(matteBlocks(ds, (size_t)nPix * 64)), dim3(KZ_BLOCK), 0, stream, shade, hit, keys, pixList, nPix, S, width, t0, t1);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

// Before the passes of a call: the table of every enabled key is there - allocated, zeroed, by the first render with the key; zeroed again unless the call
// accumulates - and the call's nSamples samples per pixel fit the 32-bit counts.
int kzMatteEnsure(KzScene *scene, KzDeviceState *ds, bool accumulate, uint32_t nSamples, hipStream_t stream) {
    int rc;
    const size_t nPixels = (size_t)scene->prm.width * (size_t)scene->prm.height;
    for (int k = 0; k < 2; ++k) {
        if (!(scene->matteMask & (1u << k))) continue;
        DevBuf<KzMatteTexel> &t = ds->matte[k];
        const bool fresh = t.cap() != nPixels;
        if (fresh) {
            if (t.cap()) HIP_TRY(hipDeviceSynchronize());
            if ((rc = t.regrow(nPixels))) return rc;
        }
        if (fresh || !accumulate) { HIP_TRY(hipMemsetAsync(t.get(), 0, t.bytes(), stream)); ds->matteSamples[k] = 0; }
        if (ds->matteSamples[k] + nSamples > 0xFFFFFFFFull)
            return kz_fail(KZ_ERR_STATE, "kz_render: %u more samples would take a pixel of the mattes past 2^32 - 1 samples (%llu counted since the last clear)", nSamples, (unsigned long long)ds->matteSamples[k]);
        ds->matteSamples[k] += nSamples;
    }
    return KZ_OK;
}

int kzMatteClear(KzDeviceState *ds, hipStream_t stream) {
    for (int k = 0; k < 2; ++k) {
        if (ds->matte[k]) HIP_TRY(hipMemsetAsync(ds->matte[k].get(), 0, ds->matte[k].bytes(), stream));
        ds->matteSamples[k] = 0;
    }
    return KZ_OK;
}

// The matte stage of a pass on `stream`, behind its camera stage: items nPix x S, pixel-major, their first-hit records at `hit`. The kernel reads and writes the
// records of the pass's pixels, and their samples must arrive in ascending order: with passes in flight it waits for the matte stage of the pass before it
// (`wait`, another stream's) and leaves `record` for the next one.
int kzMatteStage(KzScene *scene, KzDeviceState *ds, hipStream_t stream, const float4 *hit, const uint32_t *pixList, uint32_t nPix, uint32_t S, hipEvent_t wait, hipEvent_t record) {
    KzMatteTexel *t0 = (scene->matteMask & KZ_MATTE_MESH) ? ds->matte[0].get() : nullptr, *t1 = (scene->matteMask & KZ_MATTE_BSDF) ? ds->matte[1].get() : nullptr;
    if (((scene->matteMask & KZ_MATTE_MESH) && !t0) || ((scene->matteMask & KZ_MATTE_BSDF) && !t1)) return kz_fail(KZ_ERR_STATE, "the matte tables (mask %u) are not there", scene->matteMask);
    if (wait) HIP_TRY(hipStreamWaitEvent(stream, wait, 0));
    if (const int rc = matteLaunch<0>(ds, stream, S < 64u, ds->T.shade, hit, nullptr, pixList, nPix, S, (uint32_t)scene->prm.width, t0, t1)) return rc;
    if (record) HIP_TRY(hipEventRecord(record, stream));
    return KZ_OK;
}

// What the three readers share: the key is exactly one enabled bit, the replica, the buffer's size, the key's table (there from the first render with the key),
// the wait for the replica's queued work.
static int matteTable(KzScene *scene, int device, uint32_t key, const void *out, size_t nPixels, const char *call, KzDeviceState **dsOut, const KzMatteTexel **table) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null scene", call);
    if ((key != KZ_MATTE_MESH && key != KZ_MATTE_BSDF) || !(scene->matteMask & key))
        return kz_fail(KZ_ERR_INVALID_ARG, "%s: key %u must be exactly one enabled matte key (the scene's mask is %u)", call, key, scene->matteMask);
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const size_t want = (size_t)scene->prm.width * (size_t)scene->prm.height;
    if (!out || nPixels != want) return kz_fail(KZ_ERR_INVALID_ARG, "%s: the buffer must hold %zu entries (width x height)", call, want);
    const DevBuf<KzMatteTexel> &t = ds->matte[matteKeyIndex(key)];
    if (!t || t.cap() != want) return kz_fail(KZ_ERR_STATE, "%s: nothing has been rendered on this replica with matte key %u enabled", call, key);
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    *dsOut = ds; *table = t.get();
    return KZ_OK;
}

extern "C" {

int kz_scene_set_mattes(KzScene *scene, uint32_t mask) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_mattes: null scene");
    if (mask & ~KZ_MATTE_ALL) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_mattes: mask %u has bits outside KZ_MATTE_ALL (%u)", mask, KZ_MATTE_ALL);
    KzReplicaSet *rs = replicaSet(scene);
    std::vector<KzDeviceState *> v;
    if (rs) { std::lock_guard<std::mutex> g(rs->m); v = rs->v; }
    for (KzDeviceState *ds : v) {                                      // queued work finishes with the tables it was launched with
        HIP_TRY(hipSetDevice(ds->hipDevice));
        HIP_TRY(hipDeviceSynchronize());
        for (int k = 0; k < 2; ++k) if (scene->matteMask & ~mask & (1u << k)) { ds->matte[k].free(); ds->matteSamples[k] = 0; }
    }
    scene->matteMask = mask;
    return KZ_OK;
}
int kz_scene_mattes(const KzScene *scene, uint32_t *mask) {
    if (!scene || !mask) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_mattes: null argument");
    *mask = scene->matteMask;
    return KZ_OK;
}

int kz_matte_download_on(KzScene *scene, int device, uint32_t key, KzMatteTexel *out, size_t nPixels) {
    KzDeviceState *ds; const KzMatteTexel *table; int rc;
    if ((rc = matteTable(scene, device, key, out, nPixels, "kz_matte_download", &ds, &table))) return rc;
    DevBuf<KzMatteTexel> ranked;
    if ((rc = ranked.alloc(nPixels))) return rc;
    hipLaunchKernelGGL(kz_matte_rank_kernel, dim3((unsigned)((nPixels + KZ_BLOCK - 1) / KZ_BLOCK)), dim3(KZ_BLOCK), 0, ds->lastStream, table, nPixels, ranked.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    return ranked.download(out, nPixels);
}
int kz_matte_download(KzScene *scene, uint32_t key, KzMatteTexel *out, size_t nPixels) { return kz_matte_download_on(scene, -1, key, out, nPixels); }

int kz_matte_layer(KzScene *scene, int device, uint32_t key, uint32_t id, float *coverage, size_t nPixels) {
    if (id == KZ_MATTE_NONE) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_layer: id 0xFFFFFFFF is KZ_MATTE_NONE, not an id");
    KzDeviceState *ds; const KzMatteTexel *table; int rc;
    if ((rc = matteTable(scene, device, key, coverage, nPixels, "kz_matte_layer", &ds, &table))) return rc;
    DevBuf<float> plane;
    if ((rc = plane.alloc(nPixels))) return rc;
    hipLaunchKernelGGL(kz_matte_layer_kernel, dim3((unsigned)((nPixels + KZ_BLOCK - 1) / KZ_BLOCK)), dim3(KZ_BLOCK), 0, ds->lastStream, table, nPixels, id, plane.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    return plane.download(coverage, nPixels);
}

int kz_matte_top(KzScene *scene, int device, uint32_t key, uint32_t *ids, size_t nPixels) {
    KzDeviceState *ds; const KzMatteTexel *table; int rc;
    if ((rc = matteTable(scene, device, key, ids, nPixels, "kz_matte_top", &ds, &table))) return rc;
    DevBuf<uint32_t> plane;
    if ((rc = plane.alloc(nPixels))) return rc;
    hipLaunchKernelGGL(kz_matte_top_kernel, dim3((unsigned)((nPixels + KZ_BLOCK - 1) / KZ_BLOCK)), dim3(KZ_BLOCK), 0, ds->lastStream, table, nPixels, plane.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    return plane.download(ids, nPixels);
}

int kz_matte_info(KzScene *scene, int device, uint64_t *bytes) {
    KzDeviceState *ds; int rc;
    if (!bytes) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_info: null bytes");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    *bytes = ds->matteBytes();
    return KZ_OK;
}

int kz_matte_accumulate_items(KzScene *scene, int device, const uint32_t *keys, uint32_t nPix, uint32_t S, const uint32_t *pixList, KzMatteTexel *tablesInOut, uint32_t form) {
    if (!scene || !keys || !pixList || !tablesInOut) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items: null argument");
    if (!nPix || !S || (uint64_t)nPix * S > 0xFFFFFFFFull || form > 2u) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items: %u pixels x %u samples (both > 0, the product below 2^32), form %u (0 .. 2)", nPix, S, form);
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const uint32_t width = (uint32_t)scene->prm.width, height = (uint32_t)scene->prm.height;
    const size_t nPixels = (size_t)width * height;
    // the caller's records into a frame-sized table, at the place a render keeps them; every index the kernel forms is checked here
    std::vector<KzMatteTexel> frame(nPixels);
    std::memset(frame.data(), 0, nPixels * sizeof(KzMatteTexel));
    std::vector<uint8_t> seen(nPixels, 0);
    for (uint32_t p = 0; p < nPix; ++p) {
        const uint32_t x = pixList[p] & 0xffffu, y = pixList[p] >> 16;
        if (x >= width || y >= height) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items: pixel %u (%u, %u) outside the %u x %u frame", p, x, y, width, height);
        const size_t at = (size_t)y * width + x;
        if (seen[at]) return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items: pixel %u (%u, %u) is listed twice", p, x, y);
        seen[at] = 1;
        const KzMatteTexel &t = tablesInOut[p];
        uint64_t total = (uint64_t)t.other + t.miss + S;
        bool freeSeen = false;
        for (int k = 0; k < KZ_MATTE_SLOTS; ++k) {
            total += t.count[k];
            if (t.count[k] == 0) freeSeen = true;
            if ((t.count[k] != 0 && (freeSeen || t.id[k] == KZ_MATTE_NONE)) || (t.count[k] == 0 && t.id[k] != 0))
                return kz_fail(KZ_ERR_INVALID_ARG, "kz_matte_accumulate_items: record %u: slots are taken from 0 upwards, a free slot is all zero and 0xFFFFFFFF is no id", p);
        }
        if (total > 0xFFFFFFFFull) return kz_fail(KZ_ERR_STATE, "kz_matte_accumulate_items: record %u would pass 2^32 - 1 samples", p);
        frame[at] = t;
    }
    DevBuf<KzMatteTexel> dT; DevBuf<uint32_t> dK, dP;
    const size_t items = (size_t)nPix * S;
    if ((rc = dT.alloc(nPixels)) || (rc = dK.alloc(items)) || (rc = dP.alloc(nPix)) || (rc = dT.upload(frame.data(), nPixels)) || (rc = dK.upload(keys, items)) || (rc = dP.upload(pixList, nPix))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const bool lanes = form == 1u || (form == 0u && S < 64u);
    if ((rc = matteLaunch<1>(ds, nullptr, lanes, nullptr, nullptr, dK.get(), dP.get(), nPix, S, width, dT.get(), nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = dT.download(frame.data(), nPixels))) return rc;
    for (uint32_t p = 0; p < nPix; ++p) tablesInOut[p] = frame[(size_t)(pixList[p] >> 16) * width + (pixList[p] & 0xffffu)];
    return KZ_OK;
}

} // extern "C"
