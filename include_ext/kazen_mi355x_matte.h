/* kazen_mi355x_matte.h - ID mattes beside the picture: per frame pixel a short list of (id, sample count) that tells a compositor WHICH object or material the
 * pixel shows, and how much of it, so that one mesh or one material can be isolated or regraded without a new render. The feature films of kazen_mi355x_aov.h say
 * what surface a pixel shows (albedo, normal, depth); this says whose.
 *
 * THE KEY of a sample is taken from the first hit the scene's integrator shades - the feature films' own definition: for path_mis the hit behind the walk-through of
 * an invisible light, for normals, ao and path_mats the first hit itself. KZ_MATTE_MESH: the index of the hit triangle's mesh; KZ_MATTE_BSDF: the BSDF row of that
 * mesh (a normalmap row counts as itself, not as the row it wraps; a mesh that names no BSDF has the default diffuse, whose row is KzSceneDesc.nBsdfs, the one behind
 * the description's rows). A sample that hits nothing has no key: it is a miss.
 *
 * THE RULE (tests/cpu_ref/kz_matte_ref.cpp restates it in plain C++; the device's tables have its bits). Per enabled key every replica keeps one KzMatteTexel per
 * frame pixel. A pixel's samples are counted in the order they are rendered - call after call, ascending sample index within a call:
 *   a miss adds 1 to `miss`;
 *   a key that already has a slot adds 1 to that slot's count;
 *   a key without a slot takes the lowest free slot (count 1);
 *   once all KZ_MATTE_SLOTS slots are taken every other key adds 1 to `other`. Nothing is ever evicted.
 * A slot is free while its count is 0. The counts are integers, so a table depends on the pixel's sample sequence alone: the same bits for any pass size and
 * chunking, passes in flight, passes in halves and any ascending split of the sample range over accumulating calls.
 * COVERAGE of an id in a pixel is count / (sum of the counts + other + miss): the pixel's own samples, each with weight 1. Deviation from Cryptomatte practice: no
 * reconstruction filter - a sample counts for the pixel it was drawn in and for no neighbour. Name hashes, manifests and EXR channel packing are the caller's.
 *
 * LIFECYCLE. A key's table (64 x width x height bytes, outside KzRenderOpts.maxStateBytes) is allocated, zeroed, by the replica's first render with the key enabled;
 * cleared by kz_film_clear[_on] and by a render with accumulate = 0; left alone by the kz_scene_set_* edits of kazen_mi355x_edit.h (topology is fixed: ids keep
 * their meaning); freed on every replica when the key leaves the mask - a key that enters again starts from zero. Pixels no sample has reached are all zeros.
 * A render that would take a pixel past 2^32 - 1 samples since the last clear: KZ_ERR_STATE.
 * While the mask is non-zero the calls the feature films refuse are refused (KZ_ERR_UNSUPPORTED): KzRenderOpts.pipeline = 1, kz_render_multi, a KzTileDealer,
 * KzRenderOpts.packedOutput = 1 and kz_film_download_tiles. kz_render and a static kz_render_tiles work. With the mask 0 a render does what it did without this header.
 *
 * ABI v6: no existing struct grows and no existing call changes. (The header sits in include_ext/, beside include/: the set of files in include/ is pinned.) */
#ifndef KAZEN_MI355X_MATTE_H
#define KAZEN_MI355X_MATTE_H
#include "../include/kazen_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

#define KZ_MATTE_MESH 1u                /* key: the index of the hit triangle's mesh */
#define KZ_MATTE_BSDF 2u                /* key: the BSDF row of the hit triangle's mesh */
#define KZ_MATTE_ALL 3u
#define KZ_MATTE_SLOTS 7
#define KZ_MATTE_NONE 0xFFFFFFFFu       /* not an id: a miss in a key plane (kz_matte_accumulate_items), "no id" in kz_matte_top's plane (= KZ_MOTION_MISS) */

typedef struct KzMatteTexel {           /* 64 bytes */
    uint32_t id[KZ_MATTE_SLOTS];        /* the key of slot k; meaningful while count[k] > 0 */
    uint32_t count[KZ_MATTE_SLOTS];     /* samples counted for it; 0: the slot is free (its id is 0) */
    uint32_t other;                     /* samples whose key found every slot taken */
    uint32_t miss;                      /* samples without a hit */
} KzMatteTexel;

/* mask: any of KZ_MATTE_MESH | KZ_MATTE_BSDF; 0 switches the mattes off. A bit outside KZ_MATTE_ALL: KZ_ERR_INVALID_ARG. Waits for the work queued on every replica. */
int kz_scene_set_mattes(KzScene *scene, uint32_t mask);
int kz_scene_mattes(const KzScene *scene, uint32_t *mask);

/* The table of one key (exactly one enabled bit, else KZ_ERR_INVALID_ARG), width x height records, row-major, RANKED: the slots by count descending, ties to the
 * lower id, free slots last. The replica's own table keeps its slot order. nPixels must be width x height. Before the replica's first render with the key:
 * KZ_ERR_STATE. kz_matte_download addresses the scene's only replica. */
int kz_matte_download(KzScene *scene, uint32_t key, KzMatteTexel *out, size_t nPixels);
int kz_matte_download_on(KzScene *scene, int device, uint32_t key, KzMatteTexel *out, size_t nPixels);

/* One id's coverage plane, width x height floats: (float)count / (float)total, one IEEE division; 0 where the id has no slot or the pixel no samples.
 * id = KZ_MATTE_NONE: KZ_ERR_INVALID_ARG. */
int kz_matte_layer(KzScene *scene, int device, uint32_t key, uint32_t id, float *coverage, size_t nPixels);

/* Per pixel the id with the largest count, ties to the lower id; KZ_MATTE_NONE where `miss` is at least that count or the pixel has no samples. The plane has
 * kz_motion_ids' format (kazen_mi355x_motion.h) - but its ids are counted from the samples the render drew, not traced through the pixel centre. */
int kz_matte_top(KzScene *scene, int device, uint32_t key, uint32_t *ids, size_t nPixels);

/* bytes: what the tables hold on that replica - 64 x width x height per enabled key that has been rendered. */
int kz_matte_info(KzScene *scene, int device, uint64_t *bytes);

/* The test surface: the product kernel on caller-supplied keys. keys: nPix x S words, pixel-major (item p * S + s is sample s of pixel p), KZ_MATTE_NONE = a miss.
 * pixList: nPix distinct frame pixels, x | y << 16. tablesInOut: nPix records, record p that of pixList[p] - the records the count starts from on entry (slots taken
 * from 0 upwards, free slots all zero), the UNRANKED result on return. The records travel through a frame-sized table at y * width + x, as a render's do: the scene
 * is there for the replica and the frame's size only, and its own tables are not touched. form: 0 = the kernel a render picks for S (one lane per pixel below 64
 * samples per pixel, one wave per pixel from 64 on), 1 = one lane per pixel, 2 = one wave per pixel, whatever S. */
int kz_matte_accumulate_items(KzScene *scene, int device, const uint32_t *keys, uint32_t nPix, uint32_t S, const uint32_t *pixList, KzMatteTexel *tablesInOut, uint32_t form);

#ifdef __cplusplus
}
#endif
#endif
