// kz_internal.h — host-side scene object and the flat device tables of the MI355X path-tracing core.
// Not part of the ABI (that is include/kazen_mi355x.h).
#pragma once
#include "../../include/kazen_mi355x_dev.h"
#include "../../include/kazen_mi355x_edit.h"
#include "../../include/kazen_mi355x_aov.h"

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#define KZ_STACK_DEPTH 32        // per-lane traversal stack entries (LDS); the builder caps the tree depth to this
#define KZ_MAX_LEAF 4            // triangles per leaf
#define KZ_MAX_FILTER_TAPS 9     // candidates per axis the film kernel supports (filter radius <= 4)
#define KZ_PATH_MIS_MAX_DEPTH 512    // the deepest path_mis loop a scene may ask for (kz_scene_create clamps to it)
#define KZ_PATH_MATS_MAX_DEPTH 512   // bounces of a path_mats path at most (the reference has no cap: LAB_NOTES H15)
#define KZ_EM_MAX 64             // emitter triangles the roulette-ahead test of kz_wf_shade takes (one per lane of a wave)
#define KZ_EM_OFF 0xFFFFFFFFu    // KzDevTables::nEmTris of a scene without that test (more triangles, a background, another integrator)

// ---- device formats (DESIGN.md "data layout in HBM") ---------------------------------------------
// BVH2 node, 64 B, four 16-B quads -> four global_load_dwordx4 per lane:
//   q0 = lo0.x lo0.y lo0.z hi0.x | q1 = hi0.y hi0.z lo1.x lo1.y | q2 = lo1.z hi1.x hi1.y hi1.z | q3 = child0 child1 - -
// child: bit31 set -> leaf, bits[30:3] = first triangle, bits[2:0] = count-1; else node index.
struct KzNode { float q[12]; uint32_t child[2]; uint32_t pad[2]; };
static_assert(sizeof(KzNode) == 64, "node packet must be 64 B");

// BVH4 node with 8-bit quantised child boxes, 64 B (the wavefront traversal kernels use this tree; the megakernel and
// kz_trace_rays keep the BVH2): one packet fetch tests FOUR children, which halves both the number of per-lane 16-B
// gathers and the length of the dependent-load chain (and, per ray, the instructions spent on loop control and stack traffic:
// the traversal is VALU-issue-bound on MI355X).
//   q0 = p.x p.y p.z | 2^ex (float)                                        child box = p + q * 2^e per axis
//   q1 = qlo.x[4] qlo.y[4] qlo.z[4] qhi.x[4]   (4 x u8 per word, child i in byte i)
//   q2 = qhi.y[4] qhi.z[4] | 2^ey 2^ez (floats)
//   q3 = child[4] (same encoding as KzNode::child; an empty slot has qlo = 255, qhi = 0)
// Quantisation rounds outward against the SAME float expression the kernel evaluates, so the boxes stay conservative.
struct KzNode4 { float p[3]; float scaleX; uint32_t qlo[3]; uint32_t qhi[3]; float scaleY, scaleZ; uint32_t child[4]; };      // scale = 2^e per axis, as floats (the node step multiplies them by 1/d: no exponent unpacking)
static_assert(sizeof(KzNode4) == 64, "BVH4 packet must be 64 B");

// Leaf triangle in Moeller-Trumbore form, 48 B, three quads: p0.xyz e1.x | e1.y e1.z e2.x e2.y | e2.z mesh prim gid
struct KzTri { float p0[3]; float e1[3]; float e2[3]; uint32_t mesh, prim, gid; };
static_assert(sizeof(KzTri) == 48, "leaf triangle must be 48 B");

// Shading record per triangle (indexed by gid), 112 B, seven quads: p0 p1 p2 n0 n1 n2 uv0 uv1 uv2 | mesh prim bsdf lightFlags.
// One hop replaces the reference's F -> V/N/UV double gather (accel.cpp:133-136,167-169), and the last quad the leaf-triangle -> mesh row
// hops (geomID -> mesh -> getBSDF / getLight / hasNormals): a hit record names the gid, everything shading needs hangs off this record.
// lightFlags = (light row + 1) << 2 | mesh flags (bit0 hasN, bit1 hasUV); light row -1 = not an emitter.
struct KzTriShade { float p[9]; float n[9]; float uv[6]; uint32_t mesh, prim, bsdf, lightFlags; };
static_assert(sizeof(KzTriShade) == 112, "shading record must be 112 B");

// Per-mesh row, 32 B.
struct KzMeshRow {
    int32_t bsdf;          // index into bsdfs (never -1 on device: the default diffuse is materialised)
    int32_t light;         // index into lightRows or -1
    uint32_t flags;        // bit0 hasN, bit1 hasUV
    uint32_t triOffset;    // gid of face 0
    uint32_t nF;
    uint32_t pad[3];
};
// Per-light row (Scene::m_lights order, scene.cpp:42-46), 48 B.
struct KzLightRow {
    float radiance[3];     // intensity * color (light.cpp:13)
    int32_t primaryVisibility;
    uint32_t mesh;
    uint32_t triOffset;    // gid of the light mesh's face 0
    uint32_t nF;
    uint32_t cdfOffset;    // into cdf[] (nF+1 floats, dpdf.h)
    float normalization;   // DiscretePDF::m_normalization = Mesh::pdf() (mesh.h:165-168)
    uint32_t hasN;         // the light mesh has vertex normals (Mesh::sample interpolates them, mesh.cpp:122-128)
    uint32_t pad[2];
};
// Flattened texture trees (texture.cpp): every KzTexture root becomes a postfix program over a small operand stack,
// so the device needs no recursion. 32 B per op.
enum { KZ_TOP_CONST = 0, KZ_TOP_IMAGE = 1, KZ_TOP_RAMP = 2, KZ_TOP_BLEND = 3 };
struct KzTexOp {
    uint32_t op;           // KZ_TOP_*
    uint32_t a;            // IMAGE: image row; BLEND: KZ_BLEND_*
    float f0, f1, f2;      // CONST: colour; IMAGE: f0 = scale, f1 = bits(texel offset / 16), f2 = bits((width - 1) | (height - 1) << 16) - the image row, so that a lookup
                           //   loads the op and then the texels, nothing in between; RAMP: f0 = min, f1 = max
    uint32_t b;            // IMAGE: bit 0 = srgb, bits 1..7 = KZ_TEXFILTER_*, bits 8..15 = channels, bits 16..23 = KZ_PIXEL_*
    uint32_t pad[2];
};
static_assert(sizeof(KzTexOp) == 32, "texture op must be 32 B");
struct KzTexProg { uint32_t start, count; };      // count: low half = ops, high half = the operand stack depth the program needs
struct KzImageRow { uint64_t offset; int32_t width, height, channels, format; };   // offset in bytes into the texel blob, 16-B aligned
static_assert(sizeof(KzBSDF) == 128, "BSDF row must be 128 B");

// pcg32 jump-ahead pair for advance(sampleIndex * 65536): state' = mult*state + inc*plus (pcg32.h:145-166 is
// linear in `inc`, so the pair is pixel independent and tabulated once per sample index).
struct KzPcgJump { uint64_t mult, plus; };

// Render constants, passed to kernels by value.
struct KzParams {
    // camera (camera.cpp:35-91)
    float s2c[16];
    float c2w[16];
    float invW, invH, nearClip, farClip;
    int32_t width, height, border;
    // integrator (integrator.cpp:187-193)
    int32_t maxDepth; float traceBias; int32_t regularization; float accumulatedRoughness;
    // sampler
    int32_t samplerType; uint32_t sampleCount; uint64_t seed; int32_t pixelTileSize;
    int32_t resX, resY;                  // stratified resolution / correlated m_resolution
    int32_t sppPow2; float invSpp;       // sampleCount is a power of two: x / sampleCount == x * invSpp bit for bit (no underflow: x >= 2^-17 or 0)
    int32_t cameraType; float apertureRadius, focusDistance;
    // lights / background
    uint32_t nLights; float lightPickPdf;
    float lightPickScale;                // nLights when that is a power of two (x / lightPickPdf == x * nLights bit for bit), else 0
    int32_t bgPresent; float bgRadiance[3];          // constant background: intensity * colour
    int32_t bgImage; float bgIntensity;             // environment map: row of `images` (-1: none) and the intensity it is scaled by
    int32_t bgFilter;                               // KZ_TEXFILTER_* of that lookup (the nested texture's `filter`)
    int32_t integrator;                             // KZ_INTEGRATOR_* (in what was this row's padding word: the path_mis kernels' arguments keep their layout)
    // film (block.cpp:13-21)
    float filterRadius, lookupFactor; int32_t tapLo, tapHi;
    uint32_t rootRef;
    uint32_t rootRef4; int32_t stackBound4;     // BVH4 root and the worst-case traversal stack depth
    // shadow rays: invisible-light triangles (lightPrimaryVisibility == false) are few; their box + list make the
    // any-hit form of the shadow test exact (kz_devfn.h shadowOccluded)
    int32_t shadowFast; uint32_t nIlTris; float ilLo[3], ilHi[3];
    int32_t anyInvisibleLight; int32_t stackDepth;
    uint32_t ilGidLo, ilGidSpan;         // every triangle of an invisible light has gid - ilGidLo <= ilGidSpan (a prefilter: other triangles may too)
    // pixel beams of a pinhole camera whose sample -> near-plane map is affine (kz_wf_beam): nearP(sx, sy) = beamA + sx * beamU + sy * beamV in WORLD
    // axes (the 3x3 of c2w applied), apex beamO
    int32_t beamOk; float beamO[3], beamA[3], beamU[3], beamV[3];
    int32_t bsdfExt;                     // bit mask (kz_devfn.h KZ_X_*) of what the BSDF rows need beyond constant diffuse / kazenstandard: 1 other models, 2 texture-backed
                                         // parameters, normal maps (selects the larger kernel variants)
};

// Device pointers (all HBM-resident after kz_scene_upload).
struct KzDevTables {
    const KzNode *nodes;
    const KzNode4 *nodes4;
    const KzTri *tris;
    const KzTriShade *shade;
    const KzMeshRow *meshes;
    const KzBSDF *bsdfs;
    const KzLightRow *lights;
    const float *cdf;
    const float *pmj;           // [5][65536][2]: the table entries as the floats GetPMJ02BNSample returns, (float)(u32 * 0x1p-32) (pmj02table.h:28-29), converted once on the host
    const float *bn;            // [48][128][128]: BlueNoise()'s value / 65535.f (bluenoise.h:16-23), divided once on the host (same IEEE division)
    const float *pixelSamples;  // pmj02bn pixel table (sampler.cpp:291-309), 2 floats per entry
    const KzPcgJump *jump;      // [sampleCount]
    const float *filter;        // [33]
    const KzTri *ilTris;        // invisible-light triangles (<= 64) for the exact any-hit shadow test
    const KzTexProg *texProgs;  // [nTextures]
    const KzTexOp *texOps;
    const KzImageRow *images;
    const uint8_t *texels;
    uint32_t texPow2;           // every image has power-of-two sides: the periodic wrap of a texel coordinate is a mask (kz_scene_create)
    // Roulette ahead (kz_wavefront.h wfShadeSurvivor): the triangles of every light mesh, visible or not, and their padded box. A path whose next roulette draw
    // ends it keeps its bounce ray only if the ray hits one of them. (The render constants would be the place for the count and the box, but sizeof(KzParams)
    // and its offsets are pinned by the edit tests: they travel here, in the kernel argument next to the pointer.)
    uint32_t nEmTris = KZ_EM_OFF;   // rows of emTris (<= KZ_EM_MAX), or KZ_EM_OFF
    const KzTri *emTris;
    float emLo[3], emHi[3];
};

// A mesh's object-to-world matrix as kz_scene_set_transforms applies it (kz_xform.h): the matrix (row-major) and, formed once on the host in double, the nine
// cofactors of the 4x4 that make up the upper 3x3 of its inverse (before the division by the determinant) and the determinant.
struct KzXform {
    float m[16];
    double c[9];            // inv[0] inv[4] inv[8] | inv[1] inv[5] inv[9] | inv[2] inv[6] inv[10] of the cofactor inverse
    double det;
};

struct KzScene {
    // flattened host tables
    std::vector<KzNode> nodes;
    std::vector<KzNode4> nodes4;
    std::vector<KzTri> tris;
    std::vector<KzTriShade> shade;
    std::vector<KzMeshRow> meshRows;
    std::vector<KzBSDF> bsdfs;
    std::vector<KzLightRow> lightRows;
    std::vector<float> cdf;
    std::vector<float> pmj;             // 2 floats per entry
    std::vector<float> bn;
    std::vector<float> pixelSamples;
    std::vector<KzPcgJump> jump;
    std::vector<KzTri> ilTris;
    // emitter triangles (kzEmitterTris): nEmTris rows, then ONE header row - p0 = emLo, e1 = emHi, mesh = nEmTris - so that kz_scene_table shows the count and the box too
    std::vector<KzTri> emTris; uint32_t nEmTris = KZ_EM_OFF; float emLo[3] = {0, 0, 0}, emHi[3] = {0, 0, 0};
    std::vector<KzTexProg> texProgs;
    std::vector<KzTexOp> texOps;
    std::vector<KzImageRow> images;
    std::vector<uint8_t> texels;
    float filter[KZ_FILTER_RESOLUTION + 1];
    KzParams prm;
    uint32_t texPow2 = 1;               // every image of the scene has power-of-two sides
    KzBvhInfo bvh;
    // editing (include/kazen_mi355x_edit.h, kz_edit.cpp): what a refit needs beyond the flat tables, and how far the host tables lag behind the last edit
    KzFilter rfilter;                   // the film's filter as created (an edited camera must keep it)
    std::vector<uint32_t> triVtx;       // 3 per gid: the face's vertex indices within its mesh
    std::vector<uint32_t> meshNV;       // vertex count of every mesh at creation
    std::vector<uint32_t> slotSrc;      // 4 per BVH4 packet: 2 x BVH2 node + child of the box each slot is quantised from (0xFFFFFFFF: empty slot)
    std::vector<uint32_t> levelStart;   // the BVH2 nodes of depth d are [levelStart[d], levelStart[d + 1]) (breadth-first numbering; filled by the first edit)
    std::vector<std::vector<float>> pendV, pendN;   // per mesh: positions / normals an edit has set that the host's shading records do not hold yet
    // what kz_scene_set_bsdfs / _lights / _transforms need (kz_edit.cpp)
    uint32_t nDescBsdfs = 0, nDescLights = 0;       // rows of KzSceneDesc.bsdfs / .lights as given (bsdfs may hold the default diffuse row behind them)
    std::vector<uint32_t> lightDesc;    // per light row: the index into KzSceneDesc.lights its mesh named
    std::vector<std::vector<float>> baseV, baseN;   // per mesh: its base data (the V / N of creation or of the last kz_scene_set_vertices), held from its first transform on
    std::vector<KzXform> pendX;         // per mesh: the transform the host's shading records do not follow yet (pendXOn[m]); applied to baseV / baseN by kzHostSync
    std::vector<uint8_t> pendXOn;
    bool hostStale = false;             // tris, nodes, nodes4 and bvh.sahCost do not follow the last edit yet (kzHostSync brings them up to date)
    uint32_t aovMask = 0;               // KZ_AOV_* feature films every render of the scene produces beside the picture (kazen_mi355x_aov.h; kz_scene_set_aovs)
    uint32_t matteMask = 0;             // KZ_MATTE_* ID-matte tables every render of the scene feeds beside the picture (kazen_mi355x_matte.h; kz_scene_set_mattes)
    int32_t varianceMode = 0;           // KZ_VARIANCE_*: every render keeps a second-moment film beside the picture's (kazen_mi355x_variance.h; kz_scene_set_variance)
    uint64_t geometryEdits = 0;         // kz_scene_set_vertices / kz_scene_set_transforms calls that changed something: a replica's temporal history (kazen_mi355x_temporal.h) older than the last one is stale
    // motion vectors (kazen_mi355x_motion.h): per mesh its object-to-world matrix as it stands, 16 floats each - the identity until the mesh's first
    // kz_scene_set_transforms and again after a kz_scene_set_vertices of it (pendX only holds what the host tables lag behind) - and the number of
    // kz_scene_set_vertices calls that changed something: kz_denoise_motion's history is stale only when that one moved on
    std::vector<float> meshXf; uint64_t baseEdits = 0;
    std::mutex editMutex;              // guards the lazy host refit (kzHostSync may be reached from several device threads of kz_render_multi)
    // device replicas, one per GPU the scene is resident on (KzReplicaSet, owned by kz_render.hip; created with the scene)
    void *dev = nullptr;
};

// scene->meshXf, sized: identities for every mesh no transform has placed yet
static inline std::vector<float> &kzMeshXf(KzScene *sc) {
    const size_t n = 16 * sc->meshRows.size();
    if (sc->meshXf.size() != n) { sc->meshXf.assign(n, 0.f); for (size_t m = 0; m < n; m += 16) for (int k = 0; k < 16; k += 5) sc->meshXf[m + k] = 1.f; }
    return sc->meshXf;
}

// kz_bvh.cpp
struct KzBuildTri { float v[3][3]; uint32_t mesh, prim, gid; };
int kz_build_bvh(const std::vector<KzBuildTri> &in, std::vector<KzNode> &nodes, std::vector<KzTri> &tris,
                 uint32_t &rootRef, KzBvhInfo &info, std::string &err);
int kz_collapse_bvh4(const std::vector<KzNode> &nodes, uint32_t rootRef, std::vector<KzNode4> &out, uint32_t &rootRef4, int &stackBound,
                     std::vector<uint32_t> *slotSrc = nullptr);

// kz_multi.cpp: what a scene with feature films enabled refuses (kazen_mi355x_aov.h) - of a render's options the megakernel pipeline, a dealer and packed tile rects
// (kzAovRefuse), and every call that is the tile-rect gather itself (kzAovRefuseGather). KZ_OK for a scene without AOVs.
int kzAovRefuse(const KzScene *scene, const KzRenderOpts *opts, const char *call);
int kzAovRefuseGather(const KzScene *scene, const char *call);
// ... and the same refusals while the second-moment film is switched on (kazen_mi355x_variance.h). KZ_OK with the switch off.
int kzVarianceRefuse(const KzScene *scene, const KzRenderOpts *opts, const char *call);
int kzVarianceRefuseGather(const KzScene *scene, const char *call);
// ... and while ID mattes are enabled (kazen_mi355x_matte.h). KZ_OK with the mask 0.
int kzMatteRefuse(const KzScene *scene, const KzRenderOpts *opts, const char *call);
int kzMatteRefuseGather(const KzScene *scene, const char *call);
// kz_host.cpp
int kz_fail(int code, const char *fmt, ...);
int kzFailedIn(const char *call, int code);                             // the last error with "<call>: " in front: a shared check's refusal as an edit reports it
int kzCameraParams(const KzCamera &c, KzParams &p);                     // the camera part of KzParams (pixel beams included)
bool kzPinholeWords(const KzParams &p, float O[3], float A[3], float U[3], float V[3]);      // the affine pixel -> near-plane map of p.s2c / p.c2w, whatever the camera's type; false: there is none
// ... what kz_scene_create and the edits of kz_edit.cpp both form, each stated once
KzTri kzLeafTri(const KzTriShade &s, uint32_t gid);                     // the leaf-triangle form of a shading record
void kzMeshToShade(KzScene *sc, uint32_t m, const float *V, const float *N);                          // mesh m's shading records (p, n) from its vertex data through triVtx
void kzShadeToMesh(const KzScene *sc, uint32_t m, std::vector<float> &V, std::vector<float> &N);      // the inverse: vertex data out of the shading records
void kzLightRowValue(KzLightRow &lr, const KzLight &kl);                // a light row's radiance and primaryVisibility
void kzLightCdf(const KzTriShade *shade, uint32_t nF, std::vector<float> &t, float &normalization);   // a light mesh's area CDF (t[0] = 0, nF + 1 entries)
void kzLightTables(KzScene *sc);                                        // every table derived from the lights: ilTris, ilLo / ilHi, ilGid*, shadowFast; emTris, nEmTris, emLo / emHi
int kzCheckBsdfs(const KzBSDF *rows, uint32_t n, uint32_t nTextures, int32_t integrator);   // the checks of a whole BSDF row table (kz_scene_create, kz_scene_set_bsdfs)
void kzResolveBsdf(KzBSDF &b);                                          // a row as the kernels read it (the rough models' alpha)
int32_t kzBsdfExt(const std::vector<KzBSDF> &rows);                     // KzParams::bsdfExt of a row table

// kz_edit.cpp: the host tables follow every edit before anything reads them (uploads, BVH2 paths, kz_scene_bvh_info, kz_scene_table)
void kzHostSync(KzScene *scene);
// kz_refit.hip: the device side of an edit, on every replica of the scene
int kzEditWait(KzScene *scene);                                        // the work earlier calls enqueued has finished
int kzEditPrepare(KzScene *scene);                                     // BVH2, triangle vertex indices and slot map resident (once per replica)
int kzEditBeamsUnbuilt(KzScene *scene);                                // every replica's pixel-beam lists marked unbuilt
int kzEditVertices(KzScene *scene, const KzVertexUpdate *u, uint32_t n, const std::vector<uint32_t> &lightRows);   // upload + refit + derived rows
int kzEditBsdfRows(KzScene *scene, const uint32_t *rows, uint32_t n, bool extChanged);   // the listed rows of scene->bsdfs go up; the large-pass probe starts over when bsdfExt changed
int kzEditLightRows(KzScene *scene);                                   // light rows + invisible-light triangles go up
struct KzXformJob { uint32_t mesh; const KzXform *x; };
int kzEditReplicaCount(KzScene *scene);
int kzEditXformStage(KzScene *scene, const KzXformJob *jobs, uint32_t n, int32_t *bad);   // base data resident, kz_edit_xform into the staging area; *bad = the first job whose non-finite flag a replica raised, or -1
int kzEditXformCommit(KzScene *scene, const KzXformJob *jobs, uint32_t n, const std::vector<uint32_t> &lightRows);   // refit from the staging area + derived rows

// kz_render.hip
void kz_device_init(KzScene *scene);          // empty replica set
void kz_device_release(KzScene *scene);
