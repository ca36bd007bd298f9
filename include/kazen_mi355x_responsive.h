/* kazen_mi355x_responsive.h - a FAST history beside the denoiser's long one (kazen_mi355x_temporal.h, kazen_mi355x_motion.h), and the long history clamped to it where
 * the light on a surface has changed. For a caller who edits a lamp or a material, or drags a mesh whose shadow sweeps the floor: the depth and normal tests of the
 * taps cannot see a change of LIGHTING, so the long history (up to maxHistory = 32 calls) smears it over as many frames. What this adds is a test on the colour itself,
 * the "fast history clamping" of ReLAX-style denoisers: a second history of a few calls, built from the same taps; after the blend the long history's colour is
 * clamped to the fast history's local mean +- k sigma, and where the clamp bites the pixel falls back to the fast history's count and variance - it re-converges in a
 * few frames while the rest of the picture keeps its 32. It lifts the limitation both headers list, "a changed light or material LAGS by up to maxHistory calls;
 * kz_temporal_reset is the remedy", without throwing the picture's history away because of one lamp.
 *
 * THE STAGE (tests/cpu_ref/kz_responsive_ref.cpp restates it in plain C++; the device's result has its bits). All fp32, one rounding per operation, no contraction,
 * nothing flushed to zero, in the order written; comparisons as written (a NaN fails them). fastHistory, clampSigma and radius: KzResponsiveOpts' with the defaults in.
 *
 * Pass A, per valid pixel p: kazen_mi355x_motion.h's stage up to its (e, v, N), called (e_l, v_l, N_l) here. At every tap t that stage counts (weight b, the sum of
 * the counted b: Wb), with the history's record (e_h, v_h) and the fast plane's (f_h, vf_h) at t, it also accumulates
 *       F_k += b * f_h(t)_k   (k = r, g, b)        VF += b * vf_h(t)
 *   with the fast plane ABSENT: f_h(t) = e_h(t) and vf_h(t) = v_h(t).
 *   with history (the pixel blended: Wb > 1e-3):
 *       f_h,k = F_k / Wb, vf_h = VF / Wb
 *       Nf = min(N_l, (float)fastHistory)                                  (N_l < fh ? N_l : fh)
 *       af = 1.0f / Nf, of = 1.0f - af
 *       f_k = of * f_h,k + af * e_cur,k
 *       vf = (of * of) * vf_h + (af * af) * v_cur
 *   without history:  f = e_cur, vf = v_cur, Nf = 1
 *   a pixel that is not valid: four zeros.
 *
 * Pass B, per valid pixel p, only if N_l > (float)fastHistory and KZ_RESPONSIVE_CLAMP_OFF is unset. r = radius:
 *   window: dy = -r..r outer, dx = -r..r inner, q = p + (dx, dy) inside the frame and valid
 *   first loop:   cnt += 1.0f, S_k += f(q)_k;  then m_k = S_k / cnt
 *   second loop, the same order:  t = f(q)_k - m_k, D_k += t * t;  then
 *       sd_k = sqrt(D_k / cnt), w_k = clampSigma * sd_k, lo_k = m_k - w_k, hi_k = m_k + w_k
 *       c_k = e_l,k < lo_k ? lo_k : (e_l,k > hi_k ? hi_k : e_l,k)
 *   if c_k != e_l,k for any k:  (e, v, N) = (c, vf(p), Nf(p))  with Nf(p) = min(N_l, (float)fastHistory) as in pass A
 *   otherwise:                  (e, v, N) = (e_l, v_l, N_l)
 *   pixels that fail the condition keep (e_l, v_l, N_l).
 *
 * The new history is (e, v, n(p), z(p), N) after pass B; the fast plane is (f, vf); (e, v) then enter kazen_mi355x_variance.h's filter unchanged.
 *
 * Identities, each bit for bit:
 *   1. with KZ_RESPONSIVE_CLAMP_OFF the picture, the history and v_last are kz_denoise_motion's;
 *   2. with no history, and in every call while N_l <= fastHistory everywhere, the result is kz_denoise_motion's - in the first call kz_denoise_variance's: a first
 *      frame is never clamped;
 *   3. with the fast plane absent and fastHistory >= maxHistory, f == e_l and vf == v_l at every valid pixel.
 *
 * What this is not (the limitations):
 *   - The window does not respect depth or normal edges: a window across one only has a larger sigma, which WIDENS the bounds there. It does not always widen them
 *     enough: a pixel that is alone among n window texels of another colour lies k sigma from their mean only if k >= sqrt(n - 1) (2.8 for 3 x 3, 4.9 for 5 x 5), so
 *     a lone highlight or the corner of a lamp is pulled towards its surroundings at the default k = 2 (DESIGN.md 4i has what that costs).
 *   - A clamped pixel takes the fast history's variance although its colour is a bound of the window, not the fast history's own colour.
 *   - Noise larger than the change hides the change: sigma is the fast history's spatial spread, noise included, and a change within k sigma is not seen.
 *   - There are no gradient samples: A-SVGF's temporal gradient re-renders samples with the previous frame's seeds inside the path kernels and would see a change
 *     of any size; nothing here touches a render kernel.
 *
 * ABI v6: no existing struct grows and no existing call changes. A process that never calls an entry point below launches and allocates what it did before. */
#ifndef KAZEN_MI355X_RESPONSIVE_H
#define KAZEN_MI355X_RESPONSIVE_H
#include "kazen_mi355x_motion.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_RESPONSIVE_CLAMP_OFF 1u      /* maintain the fast history, never clamp */

typedef struct KzResponsiveOpts {       /* 32 bytes; a zero field means its default; NULL means all defaults */
    uint32_t fastHistory;               /* 1 .. 65535 calls the fast history blends over; default 2 */
    float    clampSigma;                /* finite and > 0: the k of mean +- k sigma; default 2.0 */
    uint32_t radius;                    /* 1 or 2: the window is (2 radius + 1)^2; default 1 */
    uint32_t flags;                     /* 0 or KZ_RESPONSIVE_CLAMP_OFF */
    uint32_t reserved[4];               /* must be 0 */
} KzResponsiveOpts;

/* kz_denoise_motion with the stage above. It writes the buffers kz_denoise writes and reads and writes kz_denoise_temporal's history: kz_denoise_download,
 * kz_denoise_to_srgb8, kz_temporal_info and kz_temporal_download serve it unchanged. Its refusals are kz_denoise_motion's, under its own name; in addition
 * KZ_ERR_INVALID_ARG, checked before the replica is looked up: fastHistory > 65535, a clampSigma that is not finite or is negative, a radius above 2, flag bits
 * outside KZ_RESPONSIVE_CLAMP_OFF, a non-zero reserved word.
 * The fast plane - 2 x width x height x 16 bytes, two copies for the reason the history has two - is allocated by the first call, outside
 * KzRenderOpts.maxStateBytes, and freed by kz_temporal_reset and with the replica. The calls may be mixed on one history: the replica records which store of the
 * history its fast plane belongs to, and when the last history was stored by kz_denoise_temporal or kz_denoise_motion the fast plane counts as ABSENT (a stale
 * history is not read at all). */
int kz_denoise_responsive(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzResponsiveOpts *ropts);

/* The test surface: kz_denoise_motion_films plus the options above and the fast plane in and out, width x height x 4 floats each: (f.r, f.g, f.b, vf) per pixel.
 * fastIn NULL with a history: the fast plane is absent; fastIn without a history (historyIn NULL, or maxHistory = 1) is ignored; fastOut may be NULL. */
int kz_denoise_responsive_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo, const float *normal,
                                const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, const KzTemporalOpts *topts, const KzTemporalView *current,
                                const KzTemporalView *previous, const float *historyIn, const uint32_t *ids, const KzMotionRow *rows, uint32_t nRows, float *out,
                                float *historyOut, float *outVariance, const KzResponsiveOpts *ropts, const float *fastIn, float *fastOut);

/* The fast plane that goes with the replica's history: width x height x 4 floats, (f.r, f.g, f.b, vf) per pixel, zeros where the pixel is not valid. KZ_ERR_STATE
 * before the first kz_denoise_responsive, after a kz_temporal_reset, and while the history was last stored by another call (the plane is absent then). */
int kz_responsive_download(KzScene *scene, int device, float *fast, size_t nFloats);

/* bytes: what the fast planes hold on that replica (0 before the first call and after kz_temporal_reset). */
int kz_responsive_info(KzScene *scene, int device, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
