/* kazen_mi355x_temporal.h - the temporal half of the variance-guided denoiser (kazen_mi355x_variance.h; Schied et al., "Spatiotemporal Variance-Guided Filtering",
 * HPG 2017): a per-replica HISTORY of the denoiser's input - colour, variance, normal, depth and a count per frame pixel - that is reprojected into the current
 * view, blended with this frame's values and stored again, in front of the unchanged variance-guided filter. For a caller who moves the camera every frame
 * (kz_scene_set_camera) and renders a few samples per pixel per frame.
 *
 * THE STAGE is defined by this arithmetic (tests/cpu_ref/kz_temporal_ref.cpp restates it in plain C++; the device's result has its bits). All fp32, one rounding
 * per operation, no contraction, nothing flushed to zero, in the order written; max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b; division and sqrt are IEEE.
 *
 *   per frame pixel p = (x, y):  c, a, n, z, s, am, valid(p), n_s = (float)samples as kazen_mi355x_variance.h defines them (its `n` is n_s here); the normal film
 *   absent from the guides: n = 0. e_cur = c / am when demodulating, else c; v_cur = that header's v_0.
 *   views: (o, a, u, v) of the current view, (o', inv') of the view the history was stored with (KzTemporalView)
 *   reprojection, for valid p with z > 0:
 *       fx = (float)x + 0.5f, fy = (float)y + 0.5f
 *       d_k = (a_k + fx * u_k) + fy * v_k,  len = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z),  r = z / len,  X_k = o_k + d_k * r
 *       q_k = X_k - o'_k,  P_i = (inv'[3i] * q.x + inv'[3i + 1] * q.y) + inv'[3i + 2] * q.z   (i = 0, 1, 2);   no history for p unless P_2 > 0
 *       sx = P_0 / P_2 - 0.5f, sy = P_1 / P_2 - 0.5f;   no history unless sx >= -1 && sx < (float)width && sy >= -1 && sy < (float)height (a NaN fails)
 *       x0 = floor(sx), y0 = floor(sy), tx = sx - x0, ty = sy - y0,  zp = sqrt((q.x * q.x + q.y * q.y) + q.z * q.z)
 *   four taps, j = 0, 1 (outer), i = 0, 1 (inner), t = (x0 + i, y0 + j):  b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty); a tap is skipped when it is outside
 *   the frame, when N_h(t) == 0, when |z_h(t) - zp| > depthTolerance * max(zp, 1e-20f), or when |n_h(t) - n(p)|^2 > normalTolerance * normalTolerance
 *   (|d|^2 = (d.x * d.x + d.y * d.y) + d.z * d.z; the product of the tolerances is formed once); otherwise
 *       Wb += b,  E_k += b * e_h(t)_k,  V += b * v_h(t),  M += b * N_h(t)
 *   history exists iff Wb > 1e-3f:  e_h = E / Wb, v_h = V / Wb, N_h = M / Wb
 *   with history:     Nn = min(N_h + 1.0f, (float)maxHistory), al = 1.0f / Nn, om = 1.0f - al
 *                     e_k = om * e_h,k + al * e_cur,k,   v = (om * om) * v_h + (al * al) * v_cur,   N = Nn
 *   without (z == 0, nothing stored, a stale history, maxHistory = 1 included):  e = e_cur, v = v_cur, N = 1
 *   a pixel that is not valid: N = 0, every other history float 0; it takes no part.
 *   The new history is (e, v, n(p), z(p), N) with the current view: the values BEFORE the spatial filter, so it does not depend on the filter's options.
 *   Then e_0 = e, v_0 = v, and the iterations, the remodulation and the result of kazen_mi355x_variance.h follow unchanged; outVariance is v_last, as there.
 * With no history, and with maxHistory = 1 whatever the history holds, the result has kz_denoise_variance's bits at the same options.
 *
 * What this is not (the limitations):
 *   - N counts CALLS, not samples: frames of different sample counts weigh the same.
 *   - No motion vectors: kz_scene_set_vertices and kz_scene_set_transforms mark every replica's history stale - the next call starts afresh (frames = 1) in the
 *     buffers it has. Camera, material and light edits keep the history: a changed light or material LAGS in the picture by up to the history's length;
 *     kz_temporal_reset is the remedy.
 *   - A thin-lens camera is taken as the pinhole through its lens centre, although its depth film measures from the lens sample: out-of-focus regions misregister
 *     by up to the circle of confusion.
 *   - The history lives on one replica; nothing is exchanged between devices or with host-merged films.
 *
 * ABI v6: no existing struct grows and no existing call changes. */
#ifndef KAZEN_MI355X_TEMPORAL_H
#define KAZEN_MI355X_TEMPORAL_H
#include "kazen_mi355x_variance.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct KzTemporalView {         /* 96 bytes: a pinhole view as the stage reads it */
    float o[3], a[3], u[3], v[3];       /* origin; the direction through the point (sx, sy) of the frame, in pixels, is a + sx * u + sy * v (not normalised) */
    float inv[9];                       /* row-major inverse of the matrix with the columns (u, v, a): inv * (X - o) = (sx * l, sy * l, l) */
    float reserved[3];                  /* 0 */
} KzTemporalView;

typedef struct KzTemporalOpts {         /* 32 bytes; a zero field means its default; NULL means all defaults */
    float depthTolerance;               /* finite and > 0; default 0.05 (relative to the reprojected distance) */
    float normalTolerance;              /* finite and > 0; default 0.5 (|n_h - n| of the films' values, which are not normalised) */
    uint32_t maxHistory;                /* 1 .. 65535; default 32; 1 = never blend */
    uint32_t flags;                     /* must be 0 */
    uint32_t reserved[4];               /* must be 0 */
} KzTemporalOpts;

/* The view of a camera, on the host alone (no device, no scene): o, a, u, v are the words the renderer derives for a pinhole camera whose pixel -> direction map is
 * affine (double arithmetic narrowed once), inv a double 3 x 3 inverse narrowed once. A thin-lens camera gives the pinhole through its lens centre. A camera whose
 * map is not affine (a sampleToCamera with a perspective row that depends on the sample position, a toWorld that is not affine), an unsupported type or a singular
 * matrix (u, v, a): KZ_ERR_UNSUPPORTED with a message. */
int kz_temporal_view(const KzCamera *camera, KzTemporalView *view);

/* kz_denoise_variance with the temporal stage in front, into the buffers kz_denoise writes: kz_denoise_download, kz_denoise_to_srgb8, kz_denoise_info and
 * kz_denoise_release serve it unchanged. The current view is that of the scene's current camera; the previous one is kept with the history. Bad options are
 * KZ_ERR_INVALID_ARG, checked before the replica is looked up: what kz_denoise_variance refuses, a KzDenoiseOpts.guides that leaves out KZ_AOV_DEPTH (the
 * reprojection reads the depth film), a tolerance that is not finite or is negative, maxHistory > 65535, flag bits, a non-zero reserved word.
 * KZ_ERR_STATE, with the numbers in the message: KZ_AOV_DEPTH is not in the scene's mask; kz_denoise_variance's refusals (the switch off, no samples, the two
 * films' counts differ); the call's demodulation (albedo among the guides and KZ_DENOISE_NO_DEMODULATE unset) differs from the history's - kz_temporal_reset first.
 * KZ_ERR_UNSUPPORTED: the scene's camera has no view (kz_temporal_view).
 * The history - 2 x width x height x 36 bytes, two copies because a pixel's taps read arbitrary neighbours while it writes its own - is allocated by the first
 * call, outside KzRenderOpts.maxStateBytes, freed by kz_temporal_reset and with the replica, and left alone by kz_denoise_release. */
int kz_denoise_temporal(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts);

/* Bytes of the history buffers of that replica and the number of calls folded into the history since it last started; both 0 before the first call and after a
 * reset. Either pointer may be NULL, not both. */
int kz_temporal_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *frames);

/* Frees the history of that replica: the next kz_denoise_temporal starts afresh. */
int kz_temporal_reset(KzScene *scene, int device);

/* The history in the interchange format: width x height x 12 floats, per pixel (e.r, e.g, e.b, v), (n.x, n.y, n.z, z), (N, 0, 0, 0). KZ_ERR_STATE before the first
 * call and after a reset. */
int kz_temporal_download(KzScene *scene, int device, float *history, size_t nFloats);

/* The test surface, like kz_denoise_variance_films: the same device code on caller-supplied host data. `depth` must be non-NULL; vopts->samples must be stated;
 * `current` must be non-NULL; historyIn (interchange format) NULL means no history, otherwise `previous` is the view it was stored with; historyOut (interchange
 * format) and outVariance may be NULL. */
int kz_denoise_temporal_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo,
                              const float *normal, const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts,
                              const KzTemporalView *current, const KzTemporalView *previous, const float *historyIn, float *out, float *historyOut,
                              float *outVariance);

#ifdef __cplusplus
}
#endif
#endif
