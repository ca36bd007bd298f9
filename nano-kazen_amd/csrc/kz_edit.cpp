// kz_edit.cpp - host side of include/kazen_mi355x_edit.h: editing the camera and the vertex data of a scene that already exists, without
// a new build (DESIGN.md "Editing a resident scene").
//
// A refit keeps the build's tree topology and recomputes everything that depends on positions with the build's own arithmetic
// (kz_refit.h): triangle and shading records, BVH2 boxes bottom-up with an absolute padding from the updated scene's extent, BVH4
// packets re-quantised from the exact BVH2 box of the subtree each slot collapsed, light CDFs, the invisible-light box, the SAH cost.
// Every replica refits on its device (kz_refit.hip). The host copy is brought up to date LAZILY (kzHostSync), before anything reads it:
// an upload to a new device, the BVH2 paths' first upload, kz_scene_bvh_info, kz_scene_table - so that an update of a scene resident
// on one device costs no host refit. The rows the lights need (shading records of light meshes, CDFs, invisible-light triangles) are
// formed on the host at once: they are few, and the light CDF is a sequential float sum.
#include "kz_internal.h"
#include "kz_refit.h"
#include "kz_xform.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// the breadth-first levels of the BVH2 (the device refits one level per launch, deepest first)
void computeLevels(KzScene *sc) {
    if (!sc->levelStart.empty() || sc->nodes.empty()) return;
    std::vector<uint32_t> depth(sc->nodes.size(), 0);
    for (size_t h = 0; h < sc->nodes.size(); ++h)
        for (int k = 0; k < 2; ++k) { const uint32_t c = sc->nodes[h].child[k]; if (!(c & 0x80000000u)) depth[c] = depth[h] + 1; }
    sc->levelStart.push_back(0);
    for (size_t h = 1; h < depth.size(); ++h) if (depth[h] != depth[h - 1]) sc->levelStart.push_back((uint32_t)h);
    sc->levelStart.push_back((uint32_t)sc->nodes.size());
}

// gives a vector's memory back (clear() would keep it)
template <class T> void release(std::vector<T> &v) { std::vector<T>().swap(v); }

// A mesh's base data for its first transform: what an edit has set and the shading records do not hold yet (pendV / pendN), else a copy out of the shading
// records (kzShadeToMesh). The caller holds editMutex.
void captureBase(KzScene *sc, uint32_t m) {
    const size_t nMeshes = sc->meshRows.size();
    if (sc->baseV.size() != nMeshes) { sc->baseV.resize(nMeshes); sc->baseN.resize(nMeshes); sc->pendX.resize(nMeshes); sc->pendXOn.assign(nMeshes, 0); }
    if (sc->pendV.size() != nMeshes) { sc->pendV.resize(nMeshes); sc->pendN.resize(nMeshes); }
    if (!sc->baseV[m].empty() || !sc->meshNV[m]) return;
    if (!sc->pendV[m].empty()) { sc->baseV[m] = sc->pendV[m]; sc->baseN[m] = sc->pendN[m]; return; }
    kzShadeToMesh(sc, m, sc->baseV[m], sc->baseN[m]);
}

// What a batch of edits names, for batchIndex's texts: one of them, how the scene came by them, several of them.
struct BatchNoun { const char *one, *has, *many; };
const BatchNoun MESHES = {"mesh", "has", "meshes"}, BSDF_ROWS = {"row", "was created with", "BSDF rows"}, LIGHTS = {"light", "was created with", "lights"};
// Update i of `call`'s batch names `index` of the scene's `count`: in range, and not named by an earlier update of the batch (seen: one byte per index, marked here).
int batchIndex(const char *call, const BatchNoun &w, uint32_t i, uint32_t index, uint32_t count, std::vector<uint8_t> &seen) {
    if (index >= count) return kz_fail(KZ_ERR_INVALID_ARG, "%s: update %u names %s %u, the scene %s %u %s", call, i, w.one, index, w.has, count, w.many);
    if (seen[index]) return kz_fail(KZ_ERR_INVALID_ARG, "%s: %s %u is listed twice in one batch", call, w.one, index);
    seen[index] = 1;
    return KZ_OK;
}

// base data of mesh m under x (kz_xform.h); false when a transformed coordinate is not finite
bool transformMesh(const KzScene *sc, uint32_t m, const KzXform &x, std::vector<float> &V, std::vector<float> &N) {
    const std::vector<float> &bV = sc->baseV[m], &bN = sc->baseN[m];
    V.resize(bV.size()); N.resize(bN.size());
    bool fin = true;
    for (size_t i = 0; i < bV.size(); i += 3) { kzXfPoint(x, &bV[i], &V[i]); fin = fin && kzFinite(V[i]) && kzFinite(V[i + 1]) && kzFinite(V[i + 2]); }
    for (size_t i = 0; i < bN.size(); i += 3) kzXfNormal(x, &bN[i], &N[i]);
    return fin;
}

// the rows a light mesh's new positions move: its shading records, its CDF (the caller brings the tables derived from the lights up to date once per batch: kzLightTables)
void applyLightMesh(KzScene *sc, uint32_t m, const float *V, const float *N) {
    kzMeshToShade(sc, m, V, N);
    KzLightRow &lr = sc->lightRows[(size_t)sc->meshRows[m].light];
    std::vector<float> t;
    kzLightCdf(&sc->shade[lr.triOffset], lr.nF, t, lr.normalization);
    std::copy(t.begin(), t.end(), sc->cdf.begin() + lr.cdfOffset);
}

} // namespace

// The host refit: the same arithmetic, node by node, as the device's (kz_refit.hip) and the build's (kz_bvh.cpp).
void kzHostSync(KzScene *sc) {
    std::lock_guard<std::mutex> g(sc->editMutex);
    if (!sc->hostStale) return;
    for (size_t m = 0; m < sc->pendV.size(); ++m) {
        if (sc->pendV[m].empty()) continue;
        kzMeshToShade(sc, (uint32_t)m, sc->pendV[m].data(), sc->pendN[m].empty() ? nullptr : sc->pendN[m].data());
        release(sc->pendV[m]); release(sc->pendN[m]);
    }
    for (size_t m = 0; m < sc->pendXOn.size(); ++m) {   // (kz_scene_set_transforms of a mesh that is no light: its base data under the matrix, by the arithmetic the replicas used)
        if (!sc->pendXOn[m]) continue;
        std::vector<float> V, N;
        transformMesh(sc, (uint32_t)m, sc->pendX[m], V, N);
        kzMeshToShade(sc, (uint32_t)m, V.data(), N.empty() ? nullptr : N.data());
        sc->pendXOn[m] = 0;
    }
    for (KzTri &t : sc->tris) t = kzLeafTri(sc->shade[t.gid], t.gid);      // (mesh and prim are the shading record's, as the build took them)
    const size_t N = sc->nodes.size();
    if (N) {
        std::vector<KzBox> exact(2 * N);                // unpadded child boxes, children before parents (breadth-first numbering)
        for (size_t h = N; h-- > 0;)
            for (int k = 0; k < 2; ++k) {
                const uint32_t c = sc->nodes[h].child[k];
                if (c & 0x80000000u) kzLeafBox(exact[2 * h + k], sc->tris.data(), sc->shade.data(), c);
                else { exact[2 * h + k] = exact[2 * (size_t)c]; kzBoxGrow(exact[2 * h + k], exact[2 * (size_t)c + 1]); }
            }
        KzBox root = exact[0]; kzBoxGrow(root, exact[1]);
        const float absPad = kzAbsPad(root);
        double sah = 0.0;                               // (kz_bvh.cpp: the same sum in the same order)
        for (size_t h = 0; h < N; ++h)
            for (int k = 0; k < 2; ++k) {
                const uint32_t c = sc->nodes[h].child[k];
                sah += (double)kzBoxArea(exact[2 * h + k]) * (double)((c & 0x80000000u) ? (c & 7u) + 1u : 1u);
                KzBox b = exact[2 * h + k]; kzPadBox(b, absPad); kzSetNodeBox(sc->nodes[h].q, k, b);
            }
        const float rootArea = kzBoxArea(root);
        sc->bvh.sahCost = rootArea > 0 ? (float)(sah / rootArea) : 0.f;
        for (size_t h = 0; h < sc->nodes4.size(); ++h) {
            KzBox cb[4]; int n = 0;
            for (int i = 0; i < 4; ++i) { const uint32_t s = sc->slotSrc[4 * h + i]; if (s == 0xFFFFFFFFu) break; kzNodeBox(sc->nodes[s >> 1].q, (int)(s & 1u), cb[n++]); }
            kzQuantiseNode4(sc->nodes4[h], cb, n);
        }
    }
    sc->hostStale = false;
}

extern "C" {

int kz_scene_set_camera(KzScene *sc, const KzCamera *c) {
    if (!sc || !c) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_camera: null argument");
    if (c->width != sc->prm.width || c->height != sc->prm.height)
        return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_camera: image size %dx%d differs from the scene's %dx%d (films and filter taps are sized for it)",
                       c->width, c->height, sc->prm.width, sc->prm.height);
    if (std::memcmp(&c->rfilter, &sc->rfilter, sizeof(KzFilter)) != 0)
        return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_camera: rfilter differs from the scene's (type %d radius %g; the film's filter taps are built for it)",
                       sc->rfilter.type, sc->rfilter.radius);
    KzParams np = sc->prm;
    int rc = kzCameraParams(*c, np);
    if (rc != KZ_OK) return rc;
    if ((rc = kzEditWait(sc)) != KZ_OK) return rc;
    sc->prm = np;
    return kzEditBeamsUnbuilt(sc);
}

int kz_scene_set_vertices(KzScene *sc, const KzVertexUpdate *u, uint32_t n) {
    if (!sc || (n && !u)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: null argument");
    const uint32_t nMeshes = (uint32_t)sc->meshRows.size();
    std::vector<uint8_t> seen(nMeshes, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const KzVertexUpdate &x = u[i];
        if (int rc = batchIndex("kz_scene_set_vertices", MESHES, i, x.mesh, nMeshes, seen)) return rc;
        if (x.nV != sc->meshNV[x.mesh]) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: mesh %u has %u vertices, the update gives %u (the topology is fixed)", x.mesh, sc->meshNV[x.mesh], x.nV);
        if (!x.V) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: mesh %u: V is null", x.mesh);
        const bool hasN = (sc->meshRows[x.mesh].flags & 1u) != 0;
        if (hasN != (x.N != nullptr))
            return kz_fail(KZ_ERR_INVALID_ARG, hasN ? "kz_scene_set_vertices: mesh %u was created with normals: the update must give N" : "kz_scene_set_vertices: mesh %u was created without normals: the update must not give N", x.mesh);
        for (size_t k = 0; k < 3 * (size_t)x.nV; ++k)
            if (!std::isfinite(x.V[k])) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: mesh %u: vertex %zu has a non-finite coordinate (%g)", x.mesh, k / 3, x.V[k]);
    }
    if (!n) return KZ_OK;
    int rc;
    if ((rc = kzEditWait(sc)) != KZ_OK) return rc;
    computeLevels(sc);
    if ((rc = kzEditPrepare(sc)) != KZ_OK) return rc;          // (the first edit of a replica: its BVH2 from the host tables, which kzHostSync has brought up to date)
    // ---- host: light meshes at once (their CDFs and the invisible-light rows need the positions), every other mesh when something reads the tables
    std::vector<uint32_t> lightRows;
    {
        std::lock_guard<std::mutex> g(sc->editMutex);
        if (sc->pendV.size() != nMeshes) { sc->pendV.resize(nMeshes); sc->pendN.resize(nMeshes); }
        for (uint32_t i = 0; i < n; ++i) {
            const KzVertexUpdate &x = u[i];
            const int32_t light = sc->meshRows[x.mesh].light;
            if (!sc->baseV.empty()) {                   // new base data: the host's copy is taken again by the mesh's next transform (every replica's follows in kzEditVertices), its transform goes
                release(sc->baseV[x.mesh]); release(sc->baseN[x.mesh]); sc->pendXOn[x.mesh] = 0;
            }
            if (light < 0) {
                sc->pendV[x.mesh].assign(x.V, x.V + 3 * (size_t)x.nV);
                if (x.N) sc->pendN[x.mesh].assign(x.N, x.N + 3 * (size_t)x.nV); else sc->pendN[x.mesh].clear();
                continue;
            }
            release(sc->pendV[x.mesh]); release(sc->pendN[x.mesh]);
            applyLightMesh(sc, x.mesh, x.V, x.N);
            lightRows.push_back((uint32_t)light);
        }
        if (!lightRows.empty()) kzLightTables(sc);
        sc->hostStale = true;
    }
    ++sc->geometryEdits;                                       // (every replica's temporal history is stale from here on: kz_denoise_temporal's ...
    ++sc->baseEdits;                                           //  ... and kz_denoise_motion's, which follows matrices, not vertices)
    {
        std::vector<float> &xf = kzMeshXf(sc);                 // new base data: the mesh's matrix is the identity again
        for (uint32_t i = 0; i < n; ++i) for (int k = 0; k < 16; ++k) xf[16 * (size_t)u[i].mesh + k] = (k % 5 == 0) ? 1.f : 0.f;
    }
    return kzEditVertices(sc, u, n, lightRows);
}

int kz_scene_set_bsdfs(KzScene *sc, const KzBsdfUpdate *u, uint32_t n) {
    if (!sc || (n && !u)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_bsdfs: null argument");
    std::vector<KzBSDF> table(sc->bsdfs.begin(), sc->bsdfs.begin() + sc->nDescBsdfs);      // the addressable rows (a default diffuse row may follow them)
    std::vector<uint8_t> seen(sc->nDescBsdfs, 0);
    std::vector<uint32_t> rows;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = batchIndex("kz_scene_set_bsdfs", BSDF_ROWS, i, u[i].row, sc->nDescBsdfs, seen)) return rc;
        table[u[i].row] = u[i].bsdf;
        rows.push_back(u[i].row);
    }
    int rc = kzCheckBsdfs(table.data(), sc->nDescBsdfs, (uint32_t)sc->texProgs.size(), sc->prm.integrator);
    if (rc != KZ_OK) return kzFailedIn("kz_scene_set_bsdfs", rc);
    if (!n) return KZ_OK;
    if ((rc = kzEditWait(sc)) != KZ_OK) return rc;
    for (uint32_t r : rows) { kzResolveBsdf(table[r]); sc->bsdfs[r] = table[r]; }
    const int32_t ext = kzBsdfExt(sc->bsdfs);           // over the whole table, default row included: a render picks its kernel variants from it per launch
    const bool extChanged = ext != sc->prm.bsdfExt;
    sc->prm.bsdfExt = ext;
    return kzEditBsdfRows(sc, rows.data(), (uint32_t)rows.size(), extChanged);
}

int kz_scene_set_lights(KzScene *sc, const KzLightUpdate *u, uint32_t n) {
    if (!sc || (n && !u)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_lights: null argument");
    std::vector<uint8_t> seen(sc->nDescLights, 0);
    std::vector<int32_t> which(sc->nDescLights, -1);       // per light of the description: the update that names it
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = batchIndex("kz_scene_set_lights", LIGHTS, i, u[i].light, sc->nDescLights, seen)) return rc;
        which[u[i].light] = (int32_t)i;
    }
    if (!n) return KZ_OK;
    int rc;
    if ((rc = kzEditWait(sc)) != KZ_OK) return rc;
    {
        std::lock_guard<std::mutex> g(sc->editMutex);
        for (size_t l = 0; l < sc->lightRows.size(); ++l) {
            const int32_t i = which[sc->lightDesc[l]];
            if (i >= 0) kzLightRowValue(sc->lightRows[l], u[i].value);
        }
        kzLightTables(sc);                          // (the shading records of light meshes follow every edit at once: nothing to sync first)
    }
    return kzEditLightRows(sc);
}

int kz_scene_set_transforms(KzScene *sc, const KzTransformUpdate *u, uint32_t n) {
    if (!sc || (n && !u)) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_transforms: null argument");
    const uint32_t nMeshes = (uint32_t)sc->meshRows.size();
    std::vector<uint8_t> seen(nMeshes, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = batchIndex("kz_scene_set_transforms", MESHES, i, u[i].mesh, nMeshes, seen)) return rc;
        for (int k = 0; k < 16; ++k)
            if (!kzFinite(u[i].toWorld[k])) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_transforms: mesh %u: matrix entry %d is not finite (%g)", u[i].mesh, k, u[i].toWorld[k]);
    }
    if (!n) return KZ_OK;
    int rc;
    if ((rc = kzEditWait(sc)) != KZ_OK) return rc;
    std::vector<KzXform> xf(n);
    std::vector<KzXformJob> jobs(n);
    for (uint32_t i = 0; i < n; ++i) { kzXformFromMatrix(u[i].toWorld, xf[i]); jobs[i] = KzXformJob{u[i].mesh, &xf[i]}; }
    // ---- nothing below changes a table before every check has passed: the host checks the light meshes (and, for a scene no replica holds, all of them),
    // every replica's kz_edit_xform the rest
    const bool resident = kzEditReplicaCount(sc) > 0;
    std::vector<std::vector<float>> lightV(n), lightN(n);
    {
        std::lock_guard<std::mutex> g(sc->editMutex);
        for (uint32_t i = 0; i < n; ++i) captureBase(sc, u[i].mesh);
        for (uint32_t i = 0; i < n; ++i) {
            const bool light = sc->meshRows[u[i].mesh].light >= 0;
            if (!light && resident) continue;
            std::vector<float> V, N;
            if (!transformMesh(sc, u[i].mesh, xf[i], V, N))
                return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_transforms: mesh %u: a transformed position is not finite (the matrix maps a vertex to w = 0 or overflows)", u[i].mesh);
            if (light) { lightV[i].swap(V); lightN[i].swap(N); }
        }
    }
    int32_t bad = -1;
    if ((rc = kzEditXformStage(sc, jobs.data(), n, &bad)) != KZ_OK) return rc;
    if (bad >= 0) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_transforms: mesh %u: a transformed position is not finite (the matrix maps a vertex to w = 0 or overflows)", u[bad].mesh);
    computeLevels(sc);
    if ((rc = kzEditPrepare(sc)) != KZ_OK) return rc;          // (as kz_scene_set_vertices: the BVH2, the vertex indices and the slot map, once per replica)
    std::vector<uint32_t> lightRows;
    {
        std::lock_guard<std::mutex> g(sc->editMutex);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t m = u[i].mesh;
            release(sc->pendV[m]); release(sc->pendN[m]);
            if (sc->meshRows[m].light < 0) { sc->pendX[m] = xf[i]; sc->pendXOn[m] = 1; continue; }
            sc->pendXOn[m] = 0;
            applyLightMesh(sc, m, lightV[i].data(), lightN[i].empty() ? nullptr : lightN[i].data());
            lightRows.push_back((uint32_t)sc->meshRows[m].light);
        }
        if (!lightRows.empty()) kzLightTables(sc);
        sc->hostStale = true;
    }
    ++sc->geometryEdits;
    {
        std::vector<float> &cur = kzMeshXf(sc);                // the meshes' matrices as they stand (kazen_mi355x_motion.h)
        for (uint32_t i = 0; i < n; ++i) std::memcpy(&cur[16 * (size_t)u[i].mesh], u[i].toWorld, 16 * sizeof(float));
    }
    return kzEditXformCommit(sc, jobs.data(), n, lightRows);
}

} // extern "C"
