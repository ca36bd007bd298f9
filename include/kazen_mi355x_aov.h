/* kazen_mi355x_aov.h - feature films beside the picture: first-hit albedo, shading normal and depth of every sample, filtered into films of
 * their own by the machine that makes the picture's film (the same filter, taps and block-relative weights, the same canonical resolve, the
 * same layout (h + 2b) x (w + 2b) float4 = (value * w, w)). What a denoiser or a compositor asks a path tracer for beside a noisy picture.
 *
 * A feature is a function of the FIRST HIT THE SCENE'S INTEGRATOR SHADES, on the sample's own camera ray (pixel jitter, aperture draw and all):
 * for path_mis the hit behind an invisible light the camera ray walks through (integrator.cpp:214-219), for normals / ao / path_mats the first
 * hit itself, even on such a light. A miss contributes 0 in every channel, with its filter weight; the background is never consulted.
 *
 *   KZ_AOV_ALBEDO  the hit's BSDF row: `albedo` of diffuse / ggx / roughplastic, `baseColor` of kazenstandard, each through its texture at the
 *                  hit's uv when the row has one; (1, 1, 1) for mirror, dielectric, roughdielectric and roughconductor; a normalmap row gives its
 *                  nested row's value; a mesh without a BSDF the default row's. An emitter is a surface like any other: its row, not its radiance.
 *   KZ_AOV_NORMAL  the world-space shading normal as post-intersection leaves it: SIGNED, not flipped toward the camera (a film of normals holds
 *                  negative values; the film keeps them). A normalmap row gives the perturbed frame's normal.
 *   KZ_AOV_DEPTH   the distance t of that hit along its ray, replicated into r = g = b. LIMITATION: for a sample that was walked through an invisible
 *                  light, t is measured from the restart origin behind the light (the hit record holds it so), not from the camera.
 *
 * An AOV film is the same bits for any pass size, chunking, passes in flight, halves, and any split of the sample range over calls, like the picture.
 * The AOV films follow the picture's film: cleared by kz_film_clear / kz_film_clear_on and by a render with accumulate = 0, accumulated otherwise, left
 * alone by the kz_scene_set_* edit calls. With the mask 0 (the default) a render launches exactly what it launched before this header existed.
 *
 * While the mask is non-zero these are refused with KZ_ERR_UNSUPPORTED: KzRenderOpts.pipeline = 1, kz_render_multi, a KzTileDealer,
 * KzRenderOpts.packedOutput = 1 and kz_film_download_tiles (the tile-rect gather of AOV films is not built). kz_render and a static
 * kz_render_tiles on one replica work. */
#ifndef KAZEN_MI355X_AOV_H
#define KAZEN_MI355X_AOV_H
#include "kazen_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_AOV_ALBEDO 1u
#define KZ_AOV_NORMAL 2u
#define KZ_AOV_DEPTH  4u
#define KZ_AOV_ALL    7u

/* Selects the features every later render of the scene produces, on every replica. Waits for the work earlier calls enqueued on the scene's
 * replicas. Bits outside KZ_AOV_ALL: KZ_ERR_INVALID_ARG. An AOV that leaves the mask frees its sums and its film on every replica; one that
 * enters starts at zero at the next render and covers ONLY THE SAMPLES RENDERED FROM THEN ON: a caller that accumulates should clear the film
 * (kz_film_clear) when it enables an AOV, or the picture and the feature hold different sample sets. Mask 0 returns the replicas to the
 * state of a scene that never had AOVs. */
int kz_scene_set_aovs(KzScene *scene, uint32_t mask);
int kz_scene_aovs(const KzScene *scene, uint32_t *mask);

/* The film of one AOV (`aov`: exactly one enabled bit, else KZ_ERR_INVALID_ARG) of the primary replica / of the replica on `device`: its tap sums
 * are resolved as the picture's are and the (h + 2b) x (w + 2b) x 4 floats copied out. kz_film_to_rgb turns such a film into values. */
int kz_aov_download(KzScene *scene, uint32_t aov, float *film, size_t nFloats);
int kz_aov_download_on(KzScene *scene, int device, uint32_t aov, float *film, size_t nFloats);

/* Bytes the AOV tap sums and films hold on the replica on `device` (-1: the primary one): 0 with the mask 0. Per enabled AOV that has been
 * rendered: taps^2 x width x height x 16 for the sums + (height + 2b) x (width + 2b) x 16 for the film. */
int kz_aov_info(KzScene *scene, int device, uint64_t *bytes);

/* The features of single samples, shaped like kz_render_samples: pxy = n x (pixel x, y), idx = n sample indices; out = n x 10 floats:
 * sample position x, y | albedo r g b | normal x y z | depth | hit (1, or 0 with every feature 0). One lane per sample through the BVH2,
 * whatever the mask is. */
int kz_aov_samples(KzScene *scene, uint32_t n, const int32_t *pxy, const uint32_t *idx, float *out);

#ifdef __cplusplus
}
#endif
#endif
