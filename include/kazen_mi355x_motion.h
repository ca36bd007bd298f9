/* kazen_mi355x_motion.h - motion vectors for the temporal stage of the denoiser (kazen_mi355x_temporal.h): the history kept across kz_scene_set_transforms. For a
 * caller who drags a mesh every frame: a transform is a matrix per mesh that maps the mesh's base data to the world and does not compose with earlier ones
 * (kazen_mi355x_edit.h), so a surface point X of mesh m was at H_m C_m^-1 X when the history was stored - C_m the mesh's matrix now, H_m the one then. What this adds
 * is that map per mesh (KzMotionRow) and which mesh each frame pixel shows (the id plane). It lifts the second limitation kazen_mi355x_temporal.h lists, "No motion
 * vectors", for kz_scene_set_transforms; kz_scene_set_vertices still restarts the history.
 *
 * THE STAGE is kazen_mi355x_temporal.h's, with three changes (tests/cpu_ref/kz_motion_ref.cpp restates it in plain C++; the device's result has its bits). All fp32,
 * one rounding per operation, no contraction, nothing flushed to zero, in the order written. For a valid pixel p with z > 0, X as that header forms it
 * (X_k = o_k + d_k * r) and m = ids(p):
 *   m is a miss (KZ_MOTION_MISS), or rows[m] is KZ_MOTION_STATIC:  nothing changes - the pixel goes through that header's arithmetic bit for bit
 *   rows[m] is KZ_MOTION_UNTRACKED:  p takes no history: (e_cur, v_cur, N = 1)
 *   otherwise, with d = rows[m].d and n = rows[m].n:
 *       Xp_k = ((d[4k] * X.x + d[4k + 1] * X.y) + d[4k + 2] * X.z) + d[4k + 3]                 (k = 0, 1, 2)
 *       q_k = Xp_k - o'_k  takes the place of X_k - o'_k everywhere: in P, sx, sy and zp
 *       n'_k = (n[3k] * n(p).x + n[3k + 1] * n(p).y) + n[3k + 2] * n(p).z  takes the place of n(p) in the taps' normal test
 * Everything behind the taps is unchanged: the blend, the stored history (e, v, n(p), z(p), N) - the normal as the film has it, not n' - and the filter.
 * A background that a mover reveals reprojects onto where the mover was; the history's depth there is the mover's, so the depth test rejects the tap: disocclusion
 * needs no test of its own.
 *
 * What this is not (the limitations):
 *   - Under a non-uniform scale n' has another length than the history's normal: the normal test is approximate there.
 *   - Shadows and reflections of a moved mesh LAG like any lighting change (kazen_mi355x_temporal.h); kz_temporal_reset is the remedy.
 *   - kz_scene_set_vertices (per-vertex deformation) still makes every replica's history stale.
 *   - The id is that of the pixel CENTRE's ray through the lens centre, the depth a filter-weighted mean: where the two disagree, at silhouettes, the pixel is left
 *     to the depth and normal tests.
 *
 * ABI v6: no existing struct grows and no existing call changes. */
#ifndef KAZEN_MI355X_MOTION_H
#define KAZEN_MI355X_MOTION_H
#include "kazen_mi355x_temporal.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_MOTION_STATIC 1u             /* the mesh has not moved: the kernel skips the multiply, so identity is exact by construction */
#define KZ_MOTION_UNTRACKED 2u          /* the motion is not affine (or not finite): pixels on the mesh take no history */
#define KZ_MOTION_MISS 0xFFFFFFFFu      /* an id: the pixel's ray hits nothing */

typedef struct KzMotionRow {            /* 96 bytes: where a point of the mesh was when the history was stored */
    float d[12];                        /* row-major 3 x 4: the affine map H C^-1, formed in double and narrowed once */
    float n[9];                         /* row-major 3 x 3: the inverse transpose of d's linear part, formed the same way, not rescaled */
    uint32_t flags;                     /* 0, KZ_MOTION_STATIC or KZ_MOTION_UNTRACKED; with either flag d and n are the identity and are not read */
    uint32_t reserved[2];               /* 0 */
} KzMotionRow;

/* The rows of nMeshes meshes, on the host alone (no device, no scene). cur / prev: per mesh its object-to-world matrix now and when the history was stored, 16 floats
 * each, row-major; either pointer NULL: every matrix of that side is the identity. Per mesh, in this order: an entry of either matrix that is not finite ->
 * KZ_MOTION_UNTRACKED; the two matrices bitwise equal -> KZ_MOTION_STATIC; a last row other than 0 0 0 1 in either, a linear part of either whose determinant is 0
 * or not finite, an entry of d or n that is not finite after narrowing -> KZ_MOTION_UNTRACKED. KZ_ERR_INVALID_ARG: rows NULL with nMeshes > 0. */
int kz_motion_rows(const float *cur, const float *prev, uint32_t nMeshes, KzMotionRow *rows);

/* Per frame pixel, row-major, the index of the mesh of the first hit the scene's integrator shades (KZ_MOTION_MISS: none): the scene's own camera ray for the film
 * position (x + 1/2, y + 1/2) through the lens centre; for path_mis the hit behind the walk-through of an invisible light. n must be width x height. Both the test
 * surface of the id kernel and a picking query. The id plane - width x height x 4 bytes, with the row table outside KzRenderOpts.maxStateBytes - is allocated by the
 * first call that needs it, freed by kz_temporal_reset and with the replica. */
int kz_motion_ids(KzScene *scene, int device, uint32_t *ids, size_t n);

/* kz_denoise_temporal with the motion stage: the rows are those of the scene's matrices now and of the ones the replica's history was stored with, the ids this
 * frame's. It writes the buffers kz_denoise writes and reads and writes kz_denoise_temporal's history: kz_denoise_download, kz_denoise_to_srgb8, kz_temporal_info,
 * kz_temporal_reset and kz_temporal_download serve it unchanged, and the two calls may be mixed on one history (every call that stores a history records the
 * matrices it was stored with). Its refusals are kz_denoise_temporal's, under its own name. The history is stale - the call starts afresh - only after a
 * kz_scene_set_vertices or when the frame size changed; kz_denoise_temporal keeps its own rule. When no mesh has moved since the history was stored the call IS
 * kz_denoise_temporal: no id is computed. */
int kz_denoise_motion(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts);

/* The test surface: kz_denoise_temporal_films plus the id plane (width x height), the row table and its length. ids and rows must be non-NULL (rows may be NULL when
 * nRows is 0); an id at or beyond nRows other than KZ_MOTION_MISS, row flags outside the two bits or both bits at once: KZ_ERR_INVALID_ARG, checked on the host
 * before anything is launched. */
int kz_denoise_motion_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal,
                            const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current,
                            const KzTemporalView *previous, const float *historyIn, const uint32_t *ids, const KzMotionRow *rows, uint32_t nRows, float *out,
                            float *historyOut, float *outVariance);

/* bytes: what the id plane and the row table hold on that replica (0 before the first call that needs them and after kz_temporal_reset). counts[3]: the meshes that
 * were static, moved and untracked in the replica's last kz_denoise_motion (zeros before it and after a reset). Either pointer may be NULL, not both. */
int kz_motion_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif
