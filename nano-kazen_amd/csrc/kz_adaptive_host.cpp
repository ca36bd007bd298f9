// kz_adaptive_host.cpp - include_ext/kazen_mi355x_adaptive.h on the host: the rule's options (kzAdaptiveResolve), the two pure functions kz_adaptive_schedule and
// kz_adaptive_tiles - they touch no HIP symbol, as kz_plan.cpp does not -, the driver kz_render_adaptive and the readers of the records it leaves on a replica.
// The driver owns no pass loop: every round is one render of kz_render's own internal entry (kzRenderOn, kz_render.hip) with a sample range, a tile list and
// `accumulate`; between two rounds it resolves the second-moment film, runs the classification stage (kz_adaptive.hip) and reads one byte per block back.
#include "kz_state.h"

#include <cmath>
#include <cstring>
#include <vector>

int kzAdaptiveResolve(const KzAdaptiveOpts *aopts, uint32_t sceneSamples, const char *call, KzAdaptiveRule *rule) {
    if (!aopts) return kz_fail(KZ_ERR_INVALID_ARG, "%s: NULL KzAdaptiveOpts (threshold has no default)", call);
    const KzAdaptiveOpts &o = *aopts;
    if (!std::isfinite(o.threshold) || !(o.threshold > 0.0f)) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.threshold %g (finite and > 0; it has no default)", call, (double)o.threshold);
    if (!std::isfinite(o.floor) || o.floor < 0.0f) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.floor %g (finite and >= 0; 0 = 0.01)", call, (double)o.floor);
    if (sceneSamples && o.maxSamples > sceneSamples)
        return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.maxSamples %u is larger than the scene's sample count %u", call, o.maxSamples, sceneSamples);
    if (o.block != 0 && o.block != 8 && o.block != 16 && o.block != 32 && o.block != 64) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.block %u (8, 16, 32 or 64; 0 = 16)", call, o.block);
    if (o.outlierPermille > 999u) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.outlierPermille %u (0 .. 999)", call, o.outlierPermille);
    if (o.flags) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzAdaptiveOpts.flags %u (must be 0)", call, o.flags);
    rule->threshold = o.threshold;
    rule->thr2 = o.threshold * o.threshold;
    rule->floor = o.floor == 0.0f ? 0.01f : o.floor;
    rule->maxSamples = o.maxSamples ? o.maxSamples : sceneSamples;
    const uint32_t minDefault = rule->maxSamples && rule->maxSamples < 16u ? rule->maxSamples : 16u;
    rule->minSamples = o.minSamples ? o.minSamples : minDefault;
    if (rule->maxSamples && rule->minSamples > rule->maxSamples) rule->minSamples = rule->maxSamples;          // n_0 = min(minSamples, maxSamples)
    rule->step = o.step;
    rule->block = o.block ? o.block : 16u;
    rule->permille = o.outlierPermille;
    return KZ_OK;
}

// the end of the round after one that ended at n (< maxSamples)
static uint32_t adaptiveNext(const KzAdaptiveRule &r, uint32_t n) {
    const uint64_t next = r.step ? (uint64_t)n + r.step : 2ull * n;
    return next < r.maxSamples ? (uint32_t)next : r.maxSamples;
}

// The tile list of `active` (kz_adaptive_tiles' definition); tiles past `cap` are counted, not written.
static uint32_t adaptiveTiles(int32_t width, int32_t height, uint32_t block, const uint8_t *active, KzTile *out, uint32_t cap) {
    const int32_t e = (int32_t)block, nbx = (width + e - 1) / e, nby = (height + e - 1) / e;
    uint32_t n = 0;
    for (int32_t by = 0; by < nby; ++by)
        for (int32_t bx = 0; bx < nbx;) {
            if (!active[(size_t)by * nbx + bx]) { ++bx; continue; }
            int32_t end = bx + 1;
            while (end < nbx && active[(size_t)by * nbx + end]) ++end;
            if (n < cap) {
                const int32_t x0 = bx * e, y0 = by * e, x1 = end * e < width ? end * e : width, y1 = y0 + e < height ? y0 + e : height;
                out[n] = KzTile{x0, y0, x1 - x0, y1 - y0};
            }
            ++n; bx = end;
        }
    return n;
}

// Pixels of block b of a frame cut into nbx blocks per row.
static uint64_t blockPixels(int32_t width, int32_t height, uint32_t block, uint32_t nbx, uint32_t b) {
    const int32_t e = (int32_t)block, x0 = (int32_t)(b % nbx) * e, y0 = (int32_t)(b / nbx) * e;
    return (uint64_t)((x0 + e < width ? e : width - x0)) * (uint64_t)((y0 + e < height ? e : height - y0));
}

// The records of a finished adaptive call of the replica on `device`, on the host.
static int adaptiveRecords(const char *call, KzScene *scene, int device, KzDeviceState **dsOut, std::vector<KzAdaptiveBlock> *rec) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null scene", call);
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (!ds->adValid || !ds->adRec)
        return kz_fail(KZ_ERR_STATE, "%s: the replica holds no block records: none before its first kz_render_adaptive, none after kz_film_clear or a render without accumulate", call);
    *dsOut = ds;
    if (rec) { rec->resize(ds->adInfo.blocks); if ((rc = ds->adRec.download(rec->data(), rec->size()))) return rc; }
    return KZ_OK;
}

extern "C" {

int kz_adaptive_schedule(const KzAdaptiveOpts *aopts, uint32_t sceneSamples, uint32_t *bounds, uint32_t cap, uint32_t *count) {
    if (!count || (cap && !bounds)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_schedule: null count or bounds");
    if (!sceneSamples) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_schedule: sceneSamples 0");
    KzAdaptiveRule r; int rc;
    if ((rc = kzAdaptiveResolve(aopts, sceneSamples, "kz_adaptive_schedule", &r))) return rc;
    uint32_t k = 0;
    for (uint32_t n = r.minSamples;; n = adaptiveNext(r, n)) {
        if (k < cap) bounds[k] = n;
        ++k;
        if (n == r.maxSamples) break;
    }
    *count = k;
    return KZ_OK;
}

int kz_adaptive_tiles(int32_t width, int32_t height, uint32_t block, const uint8_t *active, KzTile *out, uint32_t cap, uint32_t *count) {
    if (!active || !count || (cap && !out)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_tiles: null active, count or out");
    if (width < 1 || height < 1) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_tiles: a frame of %d x %d", width, height);
    if (block != 8 && block != 16 && block != 32 && block != 64) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_tiles: block %u (8, 16, 32 or 64)", block);
    *count = adaptiveTiles(width, height, block, active, out, cap);
    return KZ_OK;
}

int kz_render_adaptive(KzScene *scene, const KzRenderOpts *opts, const KzAdaptiveOpts *aopts, KzAdaptiveInfo *out) {
    static const char *call = "kz_render_adaptive";
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null scene", call);
    if (!opts) return kz_fail(KZ_ERR_INVALID_ARG, "%s: NULL KzRenderOpts", call);
    const KzParams &P = scene->prm;
    KzAdaptiveRule rule; int rc;
    if ((rc = kzAdaptiveResolve(aopts, P.sampleCount, call, &rule))) return rc;
    if (opts->sampleBegin || opts->sampleEnd)
        return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzRenderOpts.sampleBegin / sampleEnd [%u,%u) must be 0: the call owns the sample range (KzAdaptiveOpts.minSamples / maxSamples)", call, opts->sampleBegin, opts->sampleEnd);
    if (opts->tiles || opts->nTiles) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzRenderOpts.tiles must be NULL: the call renders the whole frame and owns the tile lists of its rounds", call);
    if (opts->accumulate) return kz_fail(KZ_ERR_INVALID_ARG, "%s: KzRenderOpts.accumulate must be 0: the call starts from a cleared film", call);
    if (opts->pipeline == 1) return kz_fail(KZ_ERR_UNSUPPORTED, "%s: KzRenderOpts.pipeline = 1 (the megakernel pipeline feeds no second-moment film)", call);
    if (opts->dealer) return kz_fail(KZ_ERR_UNSUPPORTED, "%s: a KzTileDealer (KzRenderOpts.dealer): the call deals its own tiles", call);
    if (opts->packedOutput) return kz_fail(KZ_ERR_UNSUPPORTED, "%s: KzRenderOpts.packedOutput = 1", call);
    if (!scene->varianceMode) return kz_fail(KZ_ERR_STATE, "%s: the second-moment film is switched off: kz_scene_set_variance(scene, 1) first", call);
    KzDeviceState *ds;
    if ((rc = kzRenderReplica(scene, opts, &ds))) return rc;

    const uint32_t e = rule.block, nbx = ((uint32_t)P.width + e - 1) / e, nby = ((uint32_t)P.height + e - 1) / e, nBlocks = nbx * nby;
    hipStream_t stream = (hipStream_t)opts->stream;
    ds->adValid = false;
    if (ds->adRec.cap() != nBlocks) {                                 // first call, or another block edge than last time
        HIP_TRY(hipDeviceSynchronize());
        if ((rc = ds->adRec.regrow(nBlocks)) || (rc = ds->adActive.regrow(nBlocks)) || (rc = ds->adActiveHost.regrow(nBlocks))) return rc;
    }
    for (Event &ev : ds->adEv) if ((rc = ev.ensure())) return rc;
    for (float &ms : ds->adStageMs) ms = 0.f;
    std::vector<KzTile> tiles;
    KzRenderOpts o = *opts;
    uint32_t rounds = 0, nPrev = 0, n = rule.minSamples;
    for (;;) {
        o.sampleBegin = nPrev; o.sampleEnd = n;
        o.accumulate = rounds ? 1 : 0;
        o.tiles = rounds ? tiles.data() : nullptr; o.nTiles = rounds ? (uint32_t)tiles.size() : 0u;
        if ((rc = kzRenderOn(scene, ds, &o))) return rc;              // (ends with the picture's resolve)
        if (!rounds) HIP_TRY(hipMemsetAsync(ds->adRec.get(), 0, ds->adRec.bytes(), stream));
        HIP_TRY(hipEventRecord(ds->adEv[0], stream));
        if ((rc = kzFilmResolve(scene, ds->moment(), stream))) return rc;
        HIP_TRY(hipEventRecord(ds->adEv[1], stream));
        if ((rc = kzAdaptiveClassify(ds->picture().texels, ds->moment().texels, P.width, P.height, P.border, rule, nullptr, n, ds->adRec, ds->adActive, stream))) return rc;
        HIP_TRY(hipEventRecord(ds->adEv[2], stream));
        HIP_TRY(hipMemcpyAsync(ds->adActiveHost.get(), ds->adActive.get(), nBlocks, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ds->adEv[3], stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int k = 0; k < 3; ++k) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, ds->adEv[k], ds->adEv[k + 1])); ds->adStageMs[k] += ms; }
        ++rounds;
        if (n == rule.maxSamples) break;
        tiles.resize(nBlocks);
        tiles.resize(adaptiveTiles(P.width, P.height, e, ds->adActiveHost.get(), tiles.data(), nBlocks));
        if (tiles.empty()) break;
        nPrev = n; n = adaptiveNext(rule, n);
    }
    std::vector<KzAdaptiveBlock> rec(nBlocks);
    if ((rc = ds->adRec.download(rec.data(), nBlocks))) return rc;
    KzAdaptiveInfo info{};
    info.rounds = rounds; info.blocks = nBlocks; info.bytes = ds->adBytes();
    for (uint32_t b = 0; b < nBlocks; ++b) {
        if (rec[b].flags & KZ_ADAPTIVE_CONVERGED) ++info.converged;
        if (rec[b].flags & KZ_ADAPTIVE_AT_CAP) ++info.atCap;
        info.samples += (uint64_t)rec[b].samples * blockPixels(P.width, P.height, e, nbx, b);
    }
    ds->adInfo = info; ds->adBlock = e; ds->adNbx = nbx; ds->adValid = true;
    if (out) *out = info;
    return KZ_OK;
}

int kz_adaptive_blocks(KzScene *scene, int device, KzAdaptiveBlock *out, size_t nBlocks) {
    KzDeviceState *ds; int rc;
    if ((rc = adaptiveRecords("kz_adaptive_blocks", scene, device, &ds, nullptr))) return rc;
    if (!out || nBlocks != ds->adInfo.blocks) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_blocks: the buffer must hold %u records, got %zu", ds->adInfo.blocks, nBlocks);
    return ds->adRec.download(out, nBlocks);
}

int kz_adaptive_counts(KzScene *scene, int device, uint32_t *samplesPerPixel, size_t nPixels) {
    KzDeviceState *ds; int rc; std::vector<KzAdaptiveBlock> rec;
    if ((rc = adaptiveRecords("kz_adaptive_counts", scene, device, &ds, &rec))) return rc;
    const KzParams &P = scene->prm;
    if (!samplesPerPixel || nPixels != (size_t)P.width * (size_t)P.height) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_counts: the plane must hold %d x %d counts, got %zu", P.width, P.height, nPixels);
    for (int32_t y = 0; y < P.height; ++y)
        for (int32_t x = 0; x < P.width; ++x)
            samplesPerPixel[(size_t)y * P.width + x] = rec[(size_t)((uint32_t)y / ds->adBlock) * ds->adNbx + (uint32_t)x / ds->adBlock].samples;
    return KZ_OK;
}

int kz_adaptive_stage_ms(KzScene *scene, int device, float *out3) {
    KzDeviceState *ds; int rc;
    if (!out3) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_stage_ms: null out");
    if ((rc = adaptiveRecords("kz_adaptive_stage_ms", scene, device, &ds, nullptr))) return rc;
    for (int k = 0; k < 3; ++k) out3[k] = ds->adStageMs[k];
    return KZ_OK;
}

int kz_adaptive_info(KzScene *scene, int device, KzAdaptiveInfo *out) {
    KzDeviceState *ds; int rc;
    if (!out) return kz_fail(KZ_ERR_INVALID_ARG, "kz_adaptive_info: null out");
    if ((rc = adaptiveRecords("kz_adaptive_info", scene, device, &ds, nullptr))) return rc;
    *out = ds->adInfo;
    return KZ_OK;
}

} // extern "C"
