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

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// the shading records of mesh m from its vertex data (kz_scene_create: p from V, n from N through the face's vertex indices)
void applyMesh(KzScene *sc, uint32_t m, const float *V, const float *N) {
    const KzMeshRow &row = sc->meshRows[m];
    for (uint32_t f = 0; f < row.nF; ++f) {
        const uint32_t g = row.triOffset + f;
        KzTriShade &s = sc->shade[g];
        for (int v = 0; v < 3; ++v) {
            const size_t i = sc->triVtx[3 * (size_t)g + v];
            for (int a = 0; a < 3; ++a) {
                s.p[3 * v + a] = V[3 * i + a];
                if (N) s.n[3 * v + a] = N[3 * i + a];
            }
        }
    }
}

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

} // namespace

// The host refit: the same arithmetic, node by node, as the device's (kz_refit.hip) and the build's (kz_bvh.cpp).
void kzHostSync(KzScene *sc) {
    std::lock_guard<std::mutex> g(sc->editMutex);
    if (!sc->hostStale) return;
    for (size_t m = 0; m < sc->pendV.size(); ++m) {
        if (sc->pendV[m].empty()) continue;
        applyMesh(sc, (uint32_t)m, sc->pendV[m].data(), sc->pendN[m].empty() ? nullptr : sc->pendN[m].data());
        std::vector<float>().swap(sc->pendV[m]); std::vector<float>().swap(sc->pendN[m]);
    }
    for (KzTri &t : sc->tris) {                         // p0, e1 = v1 - v0, e2 = v2 - v0 (kz_bvh.cpp: the leaf triangles)
        const float *p = sc->shade[t.gid].p;
        for (int a = 0; a < 3; ++a) { t.p0[a] = p[a]; t.e1[a] = p[3 + a] - p[a]; t.e2[a] = p[6 + a] - p[a]; }
    }
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
        if (x.mesh >= nMeshes) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: update %u names mesh %u, the scene has %u meshes", i, x.mesh, nMeshes);
        if (seen[x.mesh]) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_vertices: mesh %u is listed twice in one batch", x.mesh);
        seen[x.mesh] = 1;
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
            if (light < 0) {
                sc->pendV[x.mesh].assign(x.V, x.V + 3 * (size_t)x.nV);
                if (x.N) sc->pendN[x.mesh].assign(x.N, x.N + 3 * (size_t)x.nV); else sc->pendN[x.mesh].clear();
                continue;
            }
            std::vector<float>().swap(sc->pendV[x.mesh]); std::vector<float>().swap(sc->pendN[x.mesh]);
            applyMesh(sc, x.mesh, x.V, x.N);
            KzLightRow &lr = sc->lightRows[(size_t)light];
            std::vector<float> t;
            kzLightCdf(&sc->shade[lr.triOffset], lr.nF, t, lr.normalization);
            std::copy(t.begin(), t.end(), sc->cdf.begin() + lr.cdfOffset);
            lightRows.push_back((uint32_t)light);
        }
        if (!lightRows.empty()) kzInvisibleLights(sc);
        sc->hostStale = true;
    }
    return kzEditVertices(sc, u, n, lightRows);
}

} // extern "C"
