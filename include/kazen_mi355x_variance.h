/* kazen_mi355x_variance.h - a second-moment film beside the picture's, and the a-trous denoiser of kazen_mi355x_denoise.h with a colour tolerance that follows
 * the variance that film measures (the variance guidance of Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017, without its temporal half).
 *
 * THE SECOND-MOMENT FILM. While the switch is on, every render keeps one more film per replica, made by the machine that makes the picture's: running tap sums of
 * (w r^2, w g^2, w b^2, w), where (r, g, b) is the sample the picture's film receives and w the picture's filter weight for that tap. Validity is Color3f::isValid
 * of the SAMPLE: a sample the picture skips is skipped here, a square that overflows is added as computed - so the film's w channel has the picture's bits.
 * The film is the same bits for any pass size, chunking, passes in flight, halves, and any split of the sample range over calls; it is cleared by kz_film_clear[_on]
 * and by a render with accumulate = 0, accumulated otherwise, left alone by the kz_scene_set_* edit calls, resolved where it is read. Its texels are allocated by
 * the first render that needs them, outside KzRenderOpts.maxStateBytes: taps^2 x width x height x 16 bytes of sums + (height + 2b) x (width + 2b) x 16 of texels.
 * With the switch off (the default) a render launches and allocates exactly what it did before this header existed.
 * While the switch is on, what AOVs refuse is refused with KZ_ERR_UNSUPPORTED: KzRenderOpts.pipeline = 1, kz_render_multi, a KzTileDealer,
 * KzRenderOpts.packedOutput = 1 and kz_film_download_tiles.
 * A replica counts the samples per pixel the picture's film and this film have each been given since they were last zeroed: the sum of sampleEnd - sampleBegin
 * over renders.
 *
 * THE VARIANCE-GUIDED FILTER is kz_denoise's definition (kazen_mi355x_denoise.h) with the following added; everything not mentioned is unchanged. All fp32, one
 * rounding per operation, no contraction, nothing flushed to zero, in the order written; max(a, b) is a > b ? a : b.
 *
 *   s = value of the moment film (w != 0 ? xyz / w : 0),  c, a, am as before,  n = (float)samples
 *   var_k = max(s_k - c_k * c_k, 0) / n                                                       k = r, g, b
 *   v_0 = (var_r / (am_r * am_r) + var_g / (am_g * am_g)) + var_b / (am_b * am_b)             when demodulating, else (var_r + var_g) + var_b
 *   iteration i, valid pixel p:
 *       gn = 0, gd = 0; for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = p + (dx, dy) (unit spacing at every iteration) inside the frame and valid:
 *           gn += (k[dy + 1] * k[dx + 1]) * v_i(q), gd += k[dy + 1] * k[dx + 1]               k = {1/4, 1/2, 1/4}
 *       g   = gn / gd
 *       kv  = 1.0f / ((sigmaVariance * sigmaVariance) * g + 1e-12f)
 *       kcv = max(kc_i, kv)                                                                   the tolerance is the smaller of the fixed one and the variance's
 *       per tap as before with  arg = ((dc * kcv + dn * kn) + dz * kz) + da * ka              (KZ_DENOISE_NO_GUIDES: arg = dc * kcv)
 *       additionally  nv += (wgt * wgt) * v_i(q)
 *       e_{i+1}(p) = num / den,   v_{i+1}(p) = nv / (den * den)
 *   A pixel that is not valid neither gives nor receives, in e and in v.
 * The result has the bits of a plain C++ restatement (tests/cpu_ref/kz_variance_ref.cpp). With a moment film so large that kv stays below every kc_i, the colours
 * are kz_denoise's at the same KzDenoiseOpts, bit for bit.
 *
 * ABI v6: no existing struct grows and no existing call changes. */
#ifndef KAZEN_MI355X_VARIANCE_H
#define KAZEN_MI355X_VARIANCE_H
#include "kazen_mi355x_denoise.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_VARIANCE_OFF          0
#define KZ_VARIANCE_ON           1      /* the faster of the two ways to feed the film (measured: DESIGN.md 4f) */
#define KZ_VARIANCE_TWO_LAUNCHES 2      /* the film's own tap launch directly behind the picture's */
#define KZ_VARIANCE_ONE_PASS     3      /* one tap launch that reads the samples once and feeds both films (filters of up to 5 taps per axis; wider: two launches) */

/* Switches the second-moment film of every later render of the scene, on every replica: KZ_VARIANCE_OFF / KZ_VARIANCE_ON; the two other values name the way the
 * film is fed (the same bits either way; they exist to be timed against each other). Other values: KZ_ERR_INVALID_ARG. Waits for the work earlier calls enqueued on
 * the scene's replicas. Off frees the film on every replica and returns them to the state of a scene that never had it. A film that is switched on starts at zero at
 * the next render and covers ONLY THE SAMPLES RENDERED FROM THEN ON: a caller that accumulates clears the film (kz_film_clear) when it switches the film on, or
 * kz_denoise_variance refuses the pair. */
int kz_scene_set_variance(KzScene *scene, int32_t mode);
int kz_scene_variance(const KzScene *scene, int32_t *mode);

/* The second-moment film of the replica on `device` (-1: the primary one), resolved as the picture's is: (h + 2b) x (w + 2b) x 4 floats = (w r^2, w g^2, w b^2, w).
 * Switched on but nothing rendered yet: zeros. Switched off: KZ_ERR_STATE. */
int kz_variance_download(KzScene *scene, int device, float *film, size_t nFloats);

/* Bytes the film's sums and texels hold on that replica (0 before the first render with the switch on and after switching off) and the samples per pixel it has been
 * given since it was last zeroed. Either pointer may be NULL, not both. */
int kz_variance_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *samples);

typedef struct KzVarianceOpts {         /* 16 bytes; a zero field means its default; NULL means all defaults */
    float sigmaVariance;                /* finite and > 0; default 3.0 */
    uint32_t samples;                   /* n of the definition; 0 = the replica's count. A caller who rendered different counts into different tiles states it */
    uint32_t flags;                     /* must be 0 */
    uint32_t reserved;                  /* must be 0 */
} KzVarianceOpts;

/* kz_denoise_on with the variance-guided tolerance, into the buffers kz_denoise writes: kz_denoise_download, kz_denoise_to_srgb8, kz_denoise_info and
 * kz_denoise_release serve both calls, and the call needs no buffer beyond kz_denoise's. `device` -1: the primary replica. In this call the default of
 * KzDenoiseOpts.sigmaColor is 2.0; every other default is kz_denoise's. Bad KzDenoiseOpts are refused as kz_denoise refuses them; a sigmaVariance that is not
 * finite or is negative, flag bits and a non-zero `reserved` of KzVarianceOpts are KZ_ERR_INVALID_ARG - all checked before the replica is looked up.
 * KZ_ERR_STATE, with the numbers in the message: the switch is off; `samples` resolves to 0; the picture's and the moment film's sample counts differ (a film
 * switched on late without a clear). */
int kz_denoise_variance(KzScene *scene, int device, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts);

/* The test surface, like kz_denoise_films: the same device code on caller-supplied host films; `moment` has the picture's layout, vopts->samples must be stated
 * (0: KZ_ERR_STATE). outVariance (may be NULL) receives v_last of every frame pixel, width x height floats, 0 where the pixel is not valid. */
int kz_denoise_variance_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const float *albedo,
                              const float *normal, const float *depth, const KzDenoiseOpts *opts, const KzVarianceOpts *vopts, float *out, float *outVariance);

#ifdef __cplusplus
}
#endif
#endif
