/* kazen_mi355x_edit.h - editing a scene that already exists (and may be resident on any number of devices) without rebuilding it:
 * a new camera, and new vertex positions / normals for meshes of a fixed topology (a turntable, an animation, a viewport).
 *
 * Both calls wait for the work earlier kz_render* calls enqueued on the scene's replicas (it finishes with the old tables) and return
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

#ifdef __cplusplus
}
#endif
#endif
