/* kazen_mi355x_denoise.h - the picture denoised on the device, guided by its feature films (kazen_mi355x_aov.h): an edge-avoiding a-trous wavelet filter
 * (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010 - the spatial filter SVGF uses).
 * The reference renderer has no denoiser: the filter is DEFINED BY THE ARITHMETIC BELOW (csrc/kz_denoise.h states it once for the device), and the result
 * has the bits of a plain C++ restatement of it (tests/cpu_ref/kz_denoise_ref.cpp), subnormal weights included.
 *
 * A pure function of four films of the layout (h + 2b) x (w + 2b) float4 = (value * w, w): the picture's and the albedo, normal and depth films.
 * All arithmetic is fp32, one rounding per operation, no contraction, nothing flushed to zero; "a > b ? a : b" is written max(a, b).
 *
 *   per frame pixel p and film:  value = w != 0 ? xyz / w : 0   ->   c (picture), a (albedo), n (normal, not renormalised), z = depth.x
 *   valid(p): the picture's w != 0. A guide that is absent (not enabled, not among `guides`, a null film) is all zeros.
 *   demodulation, iff albedo is among the guides used and KZ_DENOISE_NO_DEMODULATE is not set (KZ_DENOISE_NO_GUIDES does not switch it off):
 *       am = max(a, 1e-3f) per channel, e_0 = c / am, result = e_last * am;     otherwise e_0 = c, result = e_last.
 *   iteration i = 0 .. iterations - 1, step s = 2^i, h = {1/16, 1/4, 3/8, 1/4, 1/16}; for every valid p:
 *       num = (0, 0, 0), den = 0
 *       for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner): q = p + s * (dx, dy); skipped when q is outside the frame or not valid
 *           |v|^2 = (v.x * v.x + v.y * v.y) + v.z * v.z
 *           dc = |e_i(q) - e_i(p)|^2, dn = |n(q) - n(p)|^2, da = |a(q) - a(p)|^2
 *           m = max(max(z_p, z_q), 1e-20f), t = (z_q - z_p) / m, dz = t * t
 *           arg = ((dc * kc_i + dn * kn) + dz * kz) + da * ka       k = 1.0f / (sigma * sigma); for kc_i: sigma = sigmaColor * 2^-i (Dammertz' halving)
 *           wgt = (h[dy + 2] * h[dx + 2]) * kzExp(-arg)             kzExp: exp as csrc/kz_crmath.h defines it (double arithmetic, one narrowing)
 *           num.k += wgt * e_i(q).k for k = r, g, b;  den += wgt
 *       e_{i+1}(p) = num / den                                       (the centre tap alone makes den >= 9/64)
 *   With KZ_DENOISE_NO_GUIDES, arg = dc * kc_i. A pixel that is not valid neither gives nor receives.
 *
 * The result has the film's layout: (r, g, b, 1) in a frame pixel that is valid, (0, 0, 0, 0) in the apron and in pixels that are not - so
 * kz_film_to_rgb, the writers of output.py and the device's sRGB raster take it as they take a film.
 *
 * ABI v6: no existing struct grows and no existing call changes. */
#ifndef KAZEN_MI355X_DENOISE_H
#define KAZEN_MI355X_DENOISE_H
#include "kazen_mi355x_aov.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_DENOISE_NO_DEMODULATE 1u
#define KZ_DENOISE_NO_GUIDES     2u
#define KZ_DENOISE_MAX_ITERATIONS 8u

typedef struct KzDenoiseOpts {          /* 32 bytes; a zero field means its default; NULL means all defaults */
    uint32_t iterations;                /* 1..8, default 5: iteration i uses tap spacing 2^i */
    uint32_t guides;                    /* KZ_AOV_* bits to guide by; 0 = every AOV in the scene's mask. Must be a subset of it */
    uint32_t flags;                     /* 1 = KZ_DENOISE_NO_DEMODULATE, 2 = KZ_DENOISE_NO_GUIDES (colour weights only); other bits refused */
    uint32_t reserved;                  /* must be 0 */
    float sigmaColor, sigmaNormal, sigmaDepth, sigmaAlbedo;   /* finite and > 0; defaults 1.0, 0.3, 0.1, 0.1 */
} KzDenoiseOpts;

/* Denoises the picture of the primary replica / of the replica on `device`: waits for the replica's queued work, resolves the enabled guide films on the
 * device (a guide that is enabled but was never rendered counts as zeros, as in kz_aov_download), filters, and returns with the result in a buffer the
 * replica owns. Reads the picture's film and the AOV sums and writes neither. The result is a SNAPSHOT: later renders, clears and edits leave it alone until
 * the next kz_denoise. Works on the replica's own film, also one a static kz_render_tiles rendered (pixels no sample reached have weight 0 and stay out);
 * a host-merged multi-device film is not denoised. Bad options - iterations above 8, a sigma that is not finite and > 0, unknown flag bits, a non-zero
 * `reserved`, `guides` outside the scene's mask - are KZ_ERR_INVALID_ARG, checked before the replica is looked up; a scene on no device: KZ_ERR_STATE.
 * Buffers (allocated on first use, outside KzRenderOpts.maxStateBytes): 4 x width x height x 16 bytes of planes + (height + 2b) x (width + 2b) x 16 for the result. */
int kz_denoise(KzScene *scene, const KzDenoiseOpts *opts);
int kz_denoise_on(KzScene *scene, int device, const KzDenoiseOpts *opts);

/* The last result of that replica (device -1: the primary one): the (h + 2b) x (w + 2b) x 4 floats / the 8-bit sRGB raster kz_film_to_srgb8 would make of
 * them (width x height x 3 bytes, tone-mapped on the device). Before any kz_denoise (or after kz_denoise_release): KZ_ERR_STATE. */
int kz_denoise_download(KzScene *scene, int device, float *film, size_t nFloats);
int kz_denoise_to_srgb8(KzScene *scene, int device, uint8_t *rgb8, size_t nBytes);

/* Bytes the denoiser's buffers hold on that replica (0 before the first kz_denoise and after a release) / gives them back. */
int kz_denoise_info(KzScene *scene, int device, uint64_t *bytes);
int kz_denoise_release(KzScene *scene, int device);

/* The test surface, like kz_aov_samples: the same device code on caller-supplied host films of (height + 2 border) x (width + 2 border) float4 each; needs a
 * device, no scene. albedo / normal / depth may be NULL (an absent guide contributes no term); opts->guides: 0 = every film given, else a subset of them. */
int kz_denoise_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *albedo,
                     const float *normal, const float *depth, const KzDenoiseOpts *opts, float *out);

#ifdef __cplusplus
}
#endif
#endif
