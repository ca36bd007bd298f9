/* kazen_mi355x_edit.h - editing a scene that already exists (and may be resident on any number of devices) without rebuilding it:
 * a new camera, new vertex positions / normals for meshes of a fixed topology (a turntable, an animation, a viewport), new material
 * rows, new light colours / intensities / visibilities, and a matrix per mesh.
 *
 * Every call waits for the work earlier kz_render* calls enqueued on the scene's replicas (it finishes with the old tables) and return
 * with the new tables in place on every replica and on the host (the next render, upload or query reads them). Like every call on one
 * scene, they are not made concurrently with renders of that scene. The film is left alone: a caller that accumulates across an edit
 * gets what it asked for. A call that fails with KZ_ERR_INVALID_ARG or KZ_ERR_UNSUPPORTED leaves the scene exactly as it was.
 * DESIGN.md "Editing a resident scene" says what a refit keeps and when to rebuild instead. */
#ifndef KAZEN_MI355X_EDIT_H
#define KAZEN_MI355X_EDIT_H
#include "kazen_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the scene's camera. Pinhole and thin lens are both allowed and the type may change; width, height and rfilter must equal
 * the scene's (films, tap sums and filter taps stay valid), else KZ_ERR_INVALID_ARG. The camera part of the render constants is
 * derived as kz_scene_create derives it (pixel beams included), and every replica's pixel-beam lists are marked unbuilt, so that the
 * next render rebuilds them. camera->sampleToCamera is borrowed for the call only. */
int kz_scene_set_camera(KzScene *scene, const KzCamera *camera);

/* One mesh's new vertex data. nV must equal the mesh's vertex count at creation; N (nV x 3) is given exactly when the mesh was
 * created with normals (NULL otherwise). Faces and UVs do not change. Host pointers, borrowed for the call only. */
typedef struct KzVertexUpdate {
    uint32_t mesh;              /* index into KzSceneDesc.meshes                                  */
    uint32_t nV;
    const float *V;             /* nV x 3 positions: every value finite                           */
    const float *N;             /* nV x 3 normals, or NULL for a mesh without normals              */
} KzVertexUpdate;

/* Replaces the vertex data of the listed meshes (each at most once per batch) and refits the whole batch once: on every replica only
 * V and N (and the few derived light rows) cross PCIe, and HIP kernels rebuild the triangle and shading records, refit the BVH2
 * bottom-up and re-quantise the BVH4 packets in place; the tree topology stays that of the build. Light CDFs, the invisible-light
 * box and kz_scene_bvh_info's sahCost (of the refit tree: a caller may rebuild once it has drifted far) follow the new positions.
 * Refused (KZ_ERR_INVALID_ARG, scene unchanged): a mesh out of range or listed twice, a wrong nV, a missing or surplus N, a
 * non-finite position. A triangle the build dropped for a non-finite vertex stays out of the tree. */
int kz_scene_set_vertices(KzScene *scene, const KzVertexUpdate *updates, uint32_t nUpdates);

/* One material row: `row` is an index into KzSceneDesc.bsdfs as given at creation (the default diffuse row that kz_scene_create appends for
 * meshes without a BSDF is not addressable). */
typedef struct KzBsdfUpdate {
    uint32_t row;
    KzBSDF bsdf;
} KzBsdfUpdate;

/* Replaces the listed BSDF rows (each at most once per batch). The batch is checked as a whole table - the scene's rows with the batch
 * applied pass the checks kz_scene_create makes (type, texture ids among the scene's existing textures, which model reads which texture,
 * alphaResolved, a normalmap's texture and nested row, no normalmap under path_mats) - and the rows are resolved as at creation (the rough
 * models' alpha). Textures, images, the mesh -> row assignment and the row count stay. Per replica only the listed rows cross PCIe
 * (128 B each); no geometry table is touched. The kernel variants a render launches follow the edited table, as for a fresh scene.
 * Refused (scene unchanged): KZ_ERR_INVALID_ARG / KZ_ERR_UNSUPPORTED as kz_scene_create refuses such a table, a row out of range or listed twice. */
int kz_scene_set_bsdfs(KzScene *scene, const KzBsdfUpdate *updates, uint32_t nUpdates);

/* One light: `light` is an index into KzSceneDesc.lights; the value applies to every mesh that named that light. */
typedef struct KzLightUpdate {
    uint32_t light;
    KzLight value;
} KzLightUpdate;

/* Replaces colour, intensity and primaryVisibility of the listed lights (each at most once per batch). Which meshes emit does not change:
 * the light count, the CDFs and the shading records stay. The invisible-light triangles and their box (the exact any-hit shadow test)
 * follow the new visibilities. Values are taken as kz_scene_create takes them (a non-finite radiance is not refused: the film drops such
 * samples). Per replica the light rows and the invisible-light triangles cross PCIe; pixel-beam lists stay built.
 * Refused (KZ_ERR_INVALID_ARG, scene unchanged): a light out of range or listed twice. */
int kz_scene_set_lights(KzScene *scene, const KzLightUpdate *updates, uint32_t nUpdates);

/* One mesh's object-to-world matrix, row-major like KzCamera.toWorld. */
typedef struct KzTransformUpdate {
    uint32_t mesh;              /* index into KzSceneDesc.meshes                                  */
    float toWorld[16];          /* every entry finite                                             */
} KzTransformUpdate;

/* Places the listed meshes (each at most once per batch) by a matrix and refits the batch once, as kz_scene_set_vertices does. A mesh's
 * BASE DATA is the V / N that kz_scene_create or its last kz_scene_set_vertices gave it; the matrix maps base data to the rendered
 * positions and normals and does NOT compose with an earlier transform of that mesh (the same call twice is idempotent);
 * kz_scene_set_vertices replaces a mesh's base data and drops its transform. The arithmetic is the scene loaders' (kz_xform.h): a point
 * is four float dot products and three divisions by w, a normal the inverse transpose of the upper 3x3 (formed in double, unchanged when
 * the determinant is 0), narrowed once and normalised. Per replica a mesh's base V / N cross PCIe on its first transform there and stay;
 * after that a transform sends its matrix alone and a HIP kernel (kz_edit_xform) forms the vertices.
 * Refused (KZ_ERR_INVALID_ARG, scene unchanged): a mesh out of range or listed twice, a non-finite matrix entry, a non-finite transformed
 * position (w = 0 somewhere). */
int kz_scene_set_transforms(KzScene *scene, const KzTransformUpdate *updates, uint32_t nUpdates);

#ifdef __cplusplus
}
#endif
#endif
