/* kazen_mi355x_adaptive.h - adaptive sampling: one call that renders the frame in rounds and stops sampling the blocks of it whose relative standard error, measured
 * from the picture's film and the second-moment film of kazen_mi355x_variance.h, has fallen below a threshold. It is built from pieces that exist: the second-moment
 * film (the same bits for any split of the sample range over calls), the film's per-pixel running tap sums (a pixel that has been given the samples [0, n_p) has
 * well-defined bits whatever its neighbours received) and kz_render's tile lists with `accumulate`. No path kernel knows about it.
 *
 * THE RULE (tests/cpu_ref/kz_adaptive_ref.cpp restates it in plain C++; the device's records have its bits).
 *
 * SCHEDULE. n_0 = min(minSamples, maxSamples). After a round that ends at n the next one ends at min(maxSamples, step ? n + step : 2 n). Round 0 renders the sample
 * indices [0, n_0) of the whole frame into a cleared film; round r renders [n_(r-1), n_r) on the blocks that are still active, accumulating. The call ends when no
 * block is active or n == maxSamples. Every pixel therefore holds a prefix [0, n_p) of its own sample sequence.
 *
 * PIXEL TEST, after every round, the last included, on the resolved picture texel T and moment texel M of frame pixel (x, y) - the texels at (x + b, y + b). All fp32,
 * one rounding per operation, no contraction, nothing flushed to zero, in the order written; n is the sample count of the pixel's block:
 *   the pixel is valid iff T.w != 0
 *   c_k = T.k / T.w                      s_k = M.w != 0 ? M.k / M.w : 0                   k = r, g, b
 *   d_k = s_k - c_k * c_k                var_k = d_k > 0 ? d_k : 0
 *   v = ((var_r + var_g) + var_b) / (float)n
 *   m = (c_r + c_g) + c_b                a = (m > 0 ? m : 0) + floor
 *   the pixel is NOISY iff v > (threshold * threshold) * (a * a)
 * The comparison is strict; there is no square root and no division beyond those written; a NaN compares false, so such a pixel is not noisy.
 *
 * BLOCK TEST. The frame is cut into blocks of `block` x `block` pixels from its top left corner, row-major, the blocks of the right and bottom edge clipped to the
 * frame. `valid` and `noisy` are integer counts over a block's frame pixels (no reduction order enters). A block is CONVERGED iff
 * (uint64)noisy * 1000 <= (uint64)outlierPermille * valid. A converged block gets KZ_ADAPTIVE_CONVERGED, is never sampled or tested again in that call, and keeps the
 * record it converged with. A block that fails the test at n == maxSamples gets KZ_ADAPTIVE_AT_CAP.
 * KNOWN APPROXIMATION: a texel near a block border mixes, through the reconstruction filter, samples of neighbouring blocks that hold other counts - but it is
 * tested with its own block's n.
 *
 * TILE LIST OF A ROUND (kz_adaptive_tiles). Block rows from top to bottom; within a row every maximal run of horizontally adjacent active blocks is one tile; no
 * vertical merging; edge blocks clipped to the frame. (The film's bits do not depend on the tiles' shape: the function is pinned so that it can be tested.)
 *
 * THE CALL BLOCKS: after every round one byte per block is read back, and the next round's tile list is built from them on the host.
 * AOVs, mattes and the motion ids ride along exactly as over a sequence of kz_render calls with tile lists; the replica's sample counts of the picture and of the
 * moment film (kz_variance_info) end at the last round's n, as that sequence would leave them. For kz_denoise_variance, KzVarianceOpts.samples (or the replica's
 * count) is then an UPPER BOUND of what a pixel received; a denoiser that reads per-pixel counts is not part of this header.
 *
 * LIFECYCLE. The block records (16 x blocks bytes) and the flags read back after a round (1 x blocks bytes) live on the replica, outside KzRenderOpts.maxStateBytes:
 * allocated by the replica's first adaptive call, rewritten by each later one, invalidated (KZ_ERR_STATE on read) by kz_film_clear[_on] and by any plain render with
 * accumulate = 0, freed with the replica.
 *
 * ABI v6: no existing struct grows and no existing call changes. (The header sits in include_ext/, beside include/: the set of files in include/ is pinned.) */
#ifndef KAZEN_MI355X_ADAPTIVE_H
#define KAZEN_MI355X_ADAPTIVE_H
#include "../include/kazen_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_ADAPTIVE_CONVERGED 1u   /* the block passed the test and was not sampled again */
#define KZ_ADAPTIVE_AT_CAP    2u   /* samples == maxSamples and the last test still failed */

typedef struct KzAdaptiveOpts {    /* 32 bytes */
    float    threshold;        /* bound on the relative standard error; finite and > 0; no default (0: KZ_ERR_INVALID_ARG) */
    float    floor;            /* added to a pixel's brightness before the comparison; finite, >= 0; 0 = default 0.01 */
    uint32_t minSamples;       /* samples every pixel gets before the first test; 0 = min(16, maxSamples) */
    uint32_t maxSamples;       /* cap per pixel; 0 = the scene's sample count (kz_scene_sample_count); larger than it: KZ_ERR_INVALID_ARG */
    uint32_t step;             /* samples per later round; 0 = double the count (n -> 2n) */
    uint32_t block;            /* block edge in pixels: 8, 16, 32 or 64; 0 = 16 */
    uint32_t outlierPermille;  /* 0 .. 999: share of a block's valid pixels that may stay noisy; 0 = none */
    uint32_t flags;            /* must be 0 */
} KzAdaptiveOpts;

typedef struct KzAdaptiveBlock { uint32_t samples, noisy, valid, flags; } KzAdaptiveBlock;   /* 16 bytes, row-major blocks, edge blocks clipped */

typedef struct KzAdaptiveInfo {
    uint32_t rounds, blocks, converged, atCap;
    uint64_t samples;          /* sum over frame pixels of the samples they received */
    uint64_t bytes;            /* what the feature holds on the replica: the block records and the flags read back after a round, 17 x blocks */
} KzAdaptiveInfo;

/* Renders the scene's frame adaptively on the replica opts->device addresses (as kz_render resolves it) and returns when the last round is done and tested.
 * Checked before any replica is looked up, each with a message that names the field - KZ_ERR_INVALID_ARG: NULL options, a bad KzAdaptiveOpts field, opts->sampleBegin
 * or opts->sampleEnd non-zero, opts->tiles non-NULL, opts->accumulate non-zero; KZ_ERR_UNSUPPORTED: opts->pipeline = 1, opts->dealer, opts->packedOutput;
 * KZ_ERR_STATE: the second-moment film is switched off (kz_scene_set_variance(scene, 1) first). Every other KzRenderOpts field means what it means to kz_render. */
int kz_render_adaptive(KzScene *scene, const KzRenderOpts *opts, const KzAdaptiveOpts *aopts, KzAdaptiveInfo *out /* may be NULL */);
/* What the last adaptive call on that replica (-1: the primary one) left: the records (nBlocks must be its block count), the records expanded to a width x height
 * plane of samples per pixel, and the summary. Before the first adaptive call and after the records were invalidated: KZ_ERR_STATE. */
int kz_adaptive_blocks(KzScene *scene, int device, KzAdaptiveBlock *out, size_t nBlocks);
int kz_adaptive_counts(KzScene *scene, int device, uint32_t *samplesPerPixel, size_t nPixels);
int kz_adaptive_info(KzScene *scene, int device, KzAdaptiveInfo *out);
/* Device time, in milliseconds, of what that call ran between its renders, summed over its rounds: out3[0] the second-moment film's resolve (the picture's is part
 * of the round's render, as in kz_render), [1] the classification stage, [2] the read-back of the blocks' bytes. For measurements (scripts/adaptive_rates.py). */
int kz_adaptive_stage_ms(KzScene *scene, int device, float *out3);

/* The test surface (no scene), like kz_denoise_variance_films: the product kernel on caller-supplied host films of (height + 2 border) x (width + 2 border) x 4
 * floats. blockSamples: n of every block, row-major; a block whose entry is 0 is skipped and its record is all zeros. aopts->maxSamples = 0 here means that no cap
 * is known: no record gets KZ_ADAPTIVE_AT_CAP. out: one record per block. */
int kz_adaptive_classify_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment,
                               const uint32_t *blockSamples, const KzAdaptiveOpts *aopts, KzAdaptiveBlock *out);

/* Pure host functions, no GPU. kz_adaptive_schedule: the ends n_0 < n_1 < ... = maxSamples of the rounds of a call that converges nowhere, for a scene of
 * sceneSamples samples per pixel (> 0); *count receives their number, bounds (may be NULL when cap is 0) the first min(cap, *count) of them. Bad options:
 * KZ_ERR_INVALID_ARG. kz_adaptive_tiles: the tile list of the blocks whose byte in `active` (row-major, one per block) is non-zero; *count receives the number of
 * tiles, out (may be NULL when cap is 0) the first min(cap, *count). */
int kz_adaptive_schedule(const KzAdaptiveOpts *aopts, uint32_t sceneSamples, uint32_t *bounds, uint32_t cap, uint32_t *count);
int kz_adaptive_tiles(int32_t width, int32_t height, uint32_t block, const uint8_t *active, KzTile *out, uint32_t cap, uint32_t *count);

#ifdef __cplusplus
}
#endif
#endif
