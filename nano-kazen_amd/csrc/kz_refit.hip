// kz_refit.hip - the device side of include/kazen_mi355x_edit.h (kz_edit.cpp holds the host side): on every replica of a scene, the refit of the
// triangle and shading records, the BVH2 boxes and the BVH4 packets from new vertex data, and the per-replica state an edit invalidates.
//
// Per replica and batch: V / N of the updated meshes go up (one copy each), then
//   kz_edit_shade   per face of an updated mesh: its shading record's p / n from V / N through the face's vertex indices
//   kz_edit_tris    per leaf triangle: p0, e1 = v1 - v0, e2 = v2 - v0 from its shading record
//   kz_edit_level   per BVH2 node of one breadth-first level, deepest level first: the exact (unpadded) child boxes - a leaf's from its triangles, an inner
//                   child's from the union of its own two boxes; the root also writes the absolute padding of the updated scene
//   kz_edit_pad     per BVH2 node: both boxes padded as the build pads them
//   kz_edit_quant   per BVH4 packet: re-quantised from the padded BVH2 boxes of the subtrees its slots collapsed (scene->slotSrc)
// Each kernel's result is a function of its inputs alone (no atomics, no order between threads): the refit is deterministic, and it is kz_refit.h's
// arithmetic, which the host refit and the build evaluate too. This unit is compiled WITHOUT -fgpu-flush-denormals-to-zero (build.sh): a box or an
// edge of subnormal size is then the host's to the bit.
#include <hip/hip_runtime.h>

#include "kz_state.h"
#include "kz_refit.h"
#include "kz_xform.h"

#include <algorithm>
#include <cstring>
#include <vector>

#define KZ_EDIT_BLOCK 256

__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_shade(KzTriShade *__restrict__ shade, const uint32_t *__restrict__ triVtx, uint32_t gid0, uint32_t nF,
                                                               const float *__restrict__ V, const float *__restrict__ N) {
    const uint32_t f = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (f >= nF) return;
    const size_t g = (size_t)gid0 + f;
    KzTriShade &s = shade[g];
    for (int v = 0; v < 3; ++v) {
        const size_t i = triVtx[3 * g + v];               // < the mesh's nV (kz_scene_create checked every index), and V / N hold nV x 3 floats
        for (int a = 0; a < 3; ++a) {
            s.p[3 * v + a] = V[3 * i + a];
            if (N) s.n[3 * v + a] = N[3 * i + a];
        }
    }
}

// kz_scene_set_transforms, one lane per vertex: the replica's base V / N of one mesh under its matrix (kz_xform.h) into the staging area, where kz_edit_shade reads them as it
// reads uploaded vertices. A lane whose position is not finite raises the job's flag with a plain store of 1 (every writer stores the same value: no atomic); the host
// reads the flags before anything is written to a table.
__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_xform(const float *__restrict__ baseV, const float *__restrict__ baseN, float *__restrict__ outV, float *__restrict__ outN,
                                                               uint32_t nV, KzXform x, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (i >= nV) return;                                   // (base and staging hold nV x 3 floats each: kzEditXformStage)
    const size_t o = 3 * (size_t)i;
    const float p[3] = {baseV[o], baseV[o + 1], baseV[o + 2]};
    float q[3];
    kzXfPoint(x, p, q);
    outV[o] = q[0]; outV[o + 1] = q[1]; outV[o + 2] = q[2];
    if (!kzFinite(q[0]) || !kzFinite(q[1]) || !kzFinite(q[2])) flag[0] = 1u;
    if (baseN) {
        const float n[3] = {baseN[o], baseN[o + 1], baseN[o + 2]};
        float r[3];
        kzXfNormal(x, n, r);
        outN[o] = r[0]; outN[o + 1] = r[1]; outN[o + 2] = r[2];
    }
}

__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_tris(KzTri *__restrict__ tris, const KzTriShade *__restrict__ shade, uint32_t n) {
    const uint32_t i = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (i >= n) return;
    KzTri &t = tris[i];
    const float *p = shade[t.gid].p;
    for (int a = 0; a < 3; ++a) { t.p0[a] = p[a]; t.e1[a] = __fsub_rn(p[3 + a], p[a]); t.e2[a] = __fsub_rn(p[6 + a], p[a]); }
}

__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_level(KzNode *__restrict__ nodes, const KzTri *__restrict__ tris, const KzTriShade *__restrict__ shade,
                                                               uint32_t first, uint32_t count, float *__restrict__ absPad) {
    const uint32_t i = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint32_t h = first + i;
    KzNode &nd = nodes[h];
    KzBox b[2];
    for (int k = 0; k < 2; ++k) {
        const uint32_t c = nd.child[k];
        if (c & 0x80000000u) kzLeafBox(b[k], tris, shade, c);
        else { KzBox r; kzNodeBox(nodes[c].q, 0, b[k]); kzNodeBox(nodes[c].q, 1, r); kzBoxGrow(b[k], r); }      // (the next level down: written by the previous launch)
    }
    kzSetNodeBox(nd.q, 0, b[0]); kzSetNodeBox(nd.q, 1, b[1]);
    if (h == 0) { KzBox root = b[0]; kzBoxGrow(root, b[1]); absPad[0] = kzAbsPad(root); }
}

__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_pad(KzNode *__restrict__ nodes, uint32_t n, const float *__restrict__ absPad) {
    const uint32_t h = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (h >= n) return;
    const float pad = absPad[0];
    for (int k = 0; k < 2; ++k) { KzBox b; kzNodeBox(nodes[h].q, k, b); kzPadBox(b, pad); kzSetNodeBox(nodes[h].q, k, b); }
}

__global__ __launch_bounds__(KZ_EDIT_BLOCK) void kz_edit_quant(KzNode4 *__restrict__ nodes4, uint32_t n, const KzNode *__restrict__ nodes, const uint32_t *__restrict__ slotSrc) {
    const uint32_t h = blockIdx.x * KZ_EDIT_BLOCK + threadIdx.x;
    if (h >= n) return;
    KzBox cb[4]; int cnt = 0;
    for (int i = 0; i < 4; ++i) { const uint32_t s = slotSrc[4 * (size_t)h + i]; if (s == 0xFFFFFFFFu) break; kzNodeBox(nodes[s >> 1].q, (int)(s & 1u), cb[cnt++]); }
    KzNode4 nd = nodes4[h];
    kzQuantiseNode4(nd, cb, cnt);
    nodes4[h] = nd;
}

static inline dim3 editGrid(size_t n) { return dim3((unsigned)((n + KZ_EDIT_BLOCK - 1) / KZ_EDIT_BLOCK)); }

// every replica, each with its device current, under the replica set's lock (edits are not made concurrently with renders of the scene)
template <class Fn> static int forEachReplica(KzScene *scene, Fn fn) {
    KzReplicaSet *rs = replicaSet(scene);
    std::vector<KzDeviceState *> v;
    { std::lock_guard<std::mutex> g(rs->m); v = rs->v; }
    for (KzDeviceState *ds : v) {
        HIP_TRY(hipSetDevice(ds->hipDevice));
        const int rc = fn(ds);
        if (rc != KZ_OK) return rc;
    }
    return KZ_OK;
}

int kzEditWait(KzScene *scene) {
    return forEachReplica(scene, [](KzDeviceState *) -> int { HIP_TRY(hipDeviceSynchronize()); return KZ_OK; });
}

static int beamsUnbuilt(KzDeviceState *ds) {
    if (ds->beamCount) HIP_TRY(hipMemset(ds->beamCount, 0xFF, ds->beamCount.bytes()));         // every pixel: KZ_BEAM_UNBUILT
    ds->beamDone.clear();
    return KZ_OK;
}

int kzEditBeamsUnbuilt(KzScene *scene) {
    return forEachReplica(scene, [](KzDeviceState *ds) -> int {
        const int rc = beamsUnbuilt(ds); if (rc) return rc;
        HIP_TRY(hipDeviceSynchronize());
        return KZ_OK;
    });
}

int kzEditPrepare(KzScene *scene) {
    return forEachReplica(scene, [scene](KzDeviceState *ds) -> int {
        int rc;
        if ((rc = kzEnsureBvh2(scene, ds))) return rc;
        auto up = [](const std::vector<uint32_t> &v, DevBuf<uint32_t> &buf) -> int {      // (at least 256 bytes, so the kernels never see null)
            if (buf) return KZ_OK;
            if (const int rc_ = buf.alloc(std::max<size_t>(64, v.size()))) return rc_;
            return v.empty() ? KZ_OK : buf.upload(v.data(), v.size());
        };
        if ((rc = up(scene->triVtx, ds->editTriVtx))) return rc;
        if ((rc = up(scene->slotSrc, ds->editSlotSrc))) return rc;
        return ds->editPad ? KZ_OK : ds->editPad.alloc(64);
    });
}

static int stageRoom(KzDeviceState *ds, size_t floats) {
    return ds->editStage.cap() >= floats ? KZ_OK : ds->editStage.regrow(floats);
}

// The refit of one replica behind kz_edit_shade (launched by the caller for every mesh of the batch): triangles, BVH2 levels, padding, BVH4 packets; then the rows the
// host formed for the light meshes of the batch; the pixel-beam lists are marked unbuilt. Ends with the device idle.
static int refitChain(KzScene *scene, KzDeviceState *ds, const std::vector<uint32_t> &lightRows) {
    KzTri *tris = const_cast<KzTri *>(ds->T.tris);
    KzNode *nodes = const_cast<KzNode *>(ds->T.nodes);
    if (!scene->tris.empty()) hipLaunchKernelGGL(kz_edit_tris, editGrid(scene->tris.size()), dim3(KZ_EDIT_BLOCK), 0, 0, tris, ds->T.shade, (uint32_t)scene->tris.size());
    if (!scene->nodes.empty()) {
        const std::vector<uint32_t> &L = scene->levelStart;
        for (size_t d = L.size() - 1; d-- > 0;)
            hipLaunchKernelGGL(kz_edit_level, editGrid(L[d + 1] - L[d]), dim3(KZ_EDIT_BLOCK), 0, 0, nodes, (const KzTri *)tris, ds->T.shade, L[d], L[d + 1] - L[d], ds->editPad);
        hipLaunchKernelGGL(kz_edit_pad, editGrid(scene->nodes.size()), dim3(KZ_EDIT_BLOCK), 0, 0, nodes, (uint32_t)scene->nodes.size(), (const float *)ds->editPad);
        if (!scene->nodes4.empty())
            hipLaunchKernelGGL(kz_edit_quant, editGrid(scene->nodes4.size()), dim3(KZ_EDIT_BLOCK), 0, 0, const_cast<KzNode4 *>(ds->T.nodes4), (uint32_t)scene->nodes4.size(),
                               (const KzNode *)nodes, (const uint32_t *)ds->editSlotSrc);
    }
    HIP_TRY(hipGetLastError());
    // the light rows, their CDFs and the invisible-light triangles (formed on the host: kz_edit.cpp)
    for (uint32_t l : lightRows) {
        const KzLightRow &lr = scene->lightRows[l];
        HIP_TRY(hipMemcpy(const_cast<float *>(ds->T.cdf) + lr.cdfOffset, scene->cdf.data() + lr.cdfOffset, (lr.nF + 1) * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!lightRows.empty()) {
        HIP_TRY(hipMemcpy(const_cast<KzLightRow *>(ds->T.lights), scene->lightRows.data(), scene->lightRows.size() * sizeof(KzLightRow), hipMemcpyHostToDevice));
        if (!scene->ilTris.empty()) HIP_TRY(hipMemcpy(const_cast<KzTri *>(ds->T.ilTris), scene->ilTris.data(), scene->ilTris.size() * sizeof(KzTri), hipMemcpyHostToDevice));
        const int erc = kzEmitterUpload(scene, ds); if (erc) return erc;
    }
    const int rc = beamsUnbuilt(ds); if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return KZ_OK;
}

int kzEditVertices(KzScene *scene, const KzVertexUpdate *u, uint32_t n, const std::vector<uint32_t> &lightRows) {
    size_t floats = 0;
    for (uint32_t i = 0; i < n; ++i) floats += 3 * (size_t)u[i].nV * (u[i].N ? 2 : 1);
    return forEachReplica(scene, [&](KzDeviceState *ds) -> int {
        int rc;
        if ((rc = stageRoom(ds, floats))) return rc;
        KzTriShade *shade = const_cast<KzTriShade *>(ds->T.shade);
        size_t off = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const KzVertexUpdate &x = u[i];
            const size_t k = 3 * (size_t)x.nV;
            if (!k) continue;
            float *V = ds->editStage + off, *N = x.N ? V + k : nullptr;
            HIP_TRY(hipMemcpy(V, x.V, k * sizeof(float), hipMemcpyHostToDevice));
            if (N) HIP_TRY(hipMemcpy(N, x.N, k * sizeof(float), hipMemcpyHostToDevice));
            off += N ? 2 * k : k;
            // (new base data: a replica that holds the mesh's base V / N for its transforms keeps it current, device to device)
            if (x.mesh < ds->editBase.size() && ds->editBase[x.mesh]) HIP_TRY(hipMemcpy(ds->editBase[x.mesh], V, (N ? 2 * k : k) * sizeof(float), hipMemcpyDeviceToDevice));
            const KzMeshRow &row = scene->meshRows[x.mesh];
            if (row.nF) hipLaunchKernelGGL(kz_edit_shade, editGrid(row.nF), dim3(KZ_EDIT_BLOCK), 0, 0, shade, (const uint32_t *)ds->editTriVtx, row.triOffset, row.nF, (const float *)V, (const float *)N);
        }
        return refitChain(scene, ds, lightRows);
    });
}

int kzEditReplicaCount(KzScene *scene) {
    KzReplicaSet *rs = replicaSet(scene);
    std::lock_guard<std::mutex> g(rs->m);
    return (int)rs->v.size();
}

int kzEditBsdfRows(KzScene *scene, const uint32_t *rows, uint32_t n, bool extChanged) {
    return forEachReplica(scene, [&](KzDeviceState *ds) -> int {
        for (uint32_t i = 0; i < n; ++i)                       // (rows < the table's size: kz_scene_set_bsdfs checked them against the rows of creation)
            HIP_TRY(hipMemcpy(const_cast<KzBSDF *>(ds->T.bsdfs) + rows[i], &scene->bsdfs[rows[i]], sizeof(KzBSDF), hipMemcpyHostToDevice));
        // the large-pass probe timed another shade kernel: it starts over (films are the same bits in every mode)
        if (extChanged) ds->passMode.reset();
        HIP_TRY(hipDeviceSynchronize());
        return KZ_OK;
    });
}

int kzEditLightRows(KzScene *scene) {
    return forEachReplica(scene, [&](KzDeviceState *ds) -> int {
        if (!ds->ilTrisRoomy) {                                 // a visibility toggle changes the length of the invisible-light list: room for the 64 rows it may have
            DevBuf<KzTri> roomy;
            if (const int rc = roomy.alloc(64)) return rc;
            HIP_TRY(hipMemset(roomy, 0, roomy.bytes()));
            ds->ilTris = std::move(roomy);                      // (the table of the upload is freed here: the edit has waited for the device, kzEditWait)
            ds->T.ilTris = ds->ilTris; ds->ilTrisRoomy = true;
        }
        if (!scene->lightRows.empty()) HIP_TRY(hipMemcpy(const_cast<KzLightRow *>(ds->T.lights), scene->lightRows.data(), scene->lightRows.size() * sizeof(KzLightRow), hipMemcpyHostToDevice));
        if (!scene->ilTris.empty()) HIP_TRY(hipMemcpy(const_cast<KzTri *>(ds->T.ilTris), scene->ilTris.data(), scene->ilTris.size() * sizeof(KzTri), hipMemcpyHostToDevice));
        { const int erc = kzEmitterUpload(scene, ds); if (erc) return erc; }
        HIP_TRY(hipDeviceSynchronize());
        return KZ_OK;
    });
}

// floats a job's mesh takes in the staging area (and in its base data): V, then N when the mesh has normals
static size_t xformFloats(const KzScene *scene, uint32_t mesh) { return 3 * (size_t)scene->meshNV[mesh] * ((scene->meshRows[mesh].flags & 1u) ? 2 : 1); }

int kzEditXformStage(KzScene *scene, const KzXformJob *jobs, uint32_t n, int32_t *bad) {
    *bad = -1;
    size_t floats = 0;
    for (uint32_t i = 0; i < n; ++i) floats += xformFloats(scene, jobs[i].mesh);
    std::vector<uint32_t> flags(n);
    return forEachReplica(scene, [&](KzDeviceState *ds) -> int {
        int rc;
        if ((rc = stageRoom(ds, floats))) return rc;
        if (ds->editBase.size() != scene->meshRows.size()) ds->editBase.resize(scene->meshRows.size());
        if (!ds->editFlag && (rc = ds->editFlag.alloc(4096))) return rc;
        size_t off = 0;
        for (uint32_t first = 0; first < n; first += 4096) {       // (4096 flags: a longer batch is staged in pieces; nothing but the staging area is written)
            const uint32_t cnt = std::min<uint32_t>(4096, n - first);
            HIP_TRY(hipMemset(ds->editFlag, 0, cnt * sizeof(uint32_t)));
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t m = jobs[first + j].mesh, nV = scene->meshNV[m];
                const size_t k = 3 * (size_t)nV, all = xformFloats(scene, m);
                if (!k) continue;
                if (!ds->editBase[m]) {                            // this replica's first transform of the mesh: its base V / N go up once (the host holds them: kz_edit.cpp captureBase)
                    DevBuf<float> &base = ds->editBase[m];
                    if ((rc = base.alloc(all)) || (rc = base.upload(scene->baseV[m].data(), k)) || (all > k && (rc = base.upload(scene->baseN[m].data(), k, k)))) return rc;
                }
                const float *bV = ds->editBase[m], *bN = all > k ? bV + k : nullptr;
                float *V = ds->editStage + off, *N = bN ? V + k : nullptr;
                off += all;
                hipLaunchKernelGGL(kz_edit_xform, editGrid(nV), dim3(KZ_EDIT_BLOCK), 0, 0, bV, bN, V, N, nV, *jobs[first + j].x, ds->editFlag + j);
            }
            HIP_TRY(hipGetLastError());
            if ((rc = ds->editFlag.download(flags.data() + first, cnt))) return rc;      // (blocking: behind the kernels above)
        }
        for (uint32_t i = 0; i < n; ++i) if (flags[i] && *bad < 0) *bad = (int32_t)i;
        return KZ_OK;
    });
}

int kzEditXformCommit(KzScene *scene, const KzXformJob *jobs, uint32_t n, const std::vector<uint32_t> &lightRows) {
    return forEachReplica(scene, [&](KzDeviceState *ds) -> int {
        KzTriShade *shade = const_cast<KzTriShade *>(ds->T.shade);
        size_t off = 0;
        for (uint32_t i = 0; i < n; ++i) {                         // (the staging area as kzEditXformStage laid it out)
            const uint32_t m = jobs[i].mesh;
            const size_t k = 3 * (size_t)scene->meshNV[m], all = xformFloats(scene, m);
            if (!k) continue;
            const float *V = ds->editStage + off, *N = all > k ? V + k : nullptr;
            off += all;
            const KzMeshRow &row = scene->meshRows[m];
            if (row.nF) hipLaunchKernelGGL(kz_edit_shade, editGrid(row.nF), dim3(KZ_EDIT_BLOCK), 0, 0, shade, (const uint32_t *)ds->editTriVtx, row.triOffset, row.nF, V, N);
        }
        return refitChain(scene, ds, lightRows);
    });
}

extern "C" int kz_scene_table(KzScene *scene, int device, int table, void *out, size_t cap, size_t *bytes) {
    if (!scene || !bytes) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_table: null argument");
    if (table < KZ_TABLE_NODES || table > KZ_TABLE_EM_TRIS) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_table: table %d (KZ_TABLE_NODES .. KZ_TABLE_EM_TRIS)", table);
    if (device >= 0 && table == KZ_TABLE_PARAMS) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_table: the render constants (KZ_TABLE_PARAMS) are a host table: device must be -1");
    kzHostSync(scene);
    const void *host = nullptr; size_t n = 0;
    switch (table) {
    case KZ_TABLE_NODES: host = scene->nodes.data(); n = scene->nodes.size() * sizeof(KzNode); break;
    case KZ_TABLE_NODES4: host = scene->nodes4.data(); n = scene->nodes4.size() * sizeof(KzNode4); break;
    case KZ_TABLE_TRIS: host = scene->tris.data(); n = scene->tris.size() * sizeof(KzTri); break;
    case KZ_TABLE_SHADE: host = scene->shade.data(); n = scene->shade.size() * sizeof(KzTriShade); break;
    case KZ_TABLE_CDF: host = scene->cdf.data(); n = scene->cdf.size() * sizeof(float); break;
    case KZ_TABLE_LIGHTS: host = scene->lightRows.data(); n = scene->lightRows.size() * sizeof(KzLightRow); break;
    case KZ_TABLE_IL_TRIS: host = scene->ilTris.data(); n = scene->ilTris.size() * sizeof(KzTri); break;
    case KZ_TABLE_BSDFS: host = scene->bsdfs.data(); n = scene->bsdfs.size() * sizeof(KzBSDF); break;
    case KZ_TABLE_EM_TRIS: host = scene->emTris.data(); n = scene->emTris.size() * sizeof(KzTri); break;
    default: host = &scene->prm; n = sizeof(KzParams); break;
    }
    *bytes = n;
    if (!out || !n) return KZ_OK;
    const size_t copy = std::min(cap, n);
    if (device < 0) { std::memcpy(out, host, copy); return KZ_OK; }
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const void *src = nullptr;
    switch (table) {
    case KZ_TABLE_NODES:
        if (!ds->bvh2Resident) return kz_fail(KZ_ERR_STATE, "kz_scene_table: the BVH2 of the replica on device %d is not resident (no BVH2 path or edit has used it)", device);
        src = ds->T.nodes; break;
    case KZ_TABLE_NODES4: src = ds->T.nodes4; break;
    case KZ_TABLE_TRIS: src = ds->T.tris; break;
    case KZ_TABLE_SHADE: src = ds->T.shade; break;
    case KZ_TABLE_CDF: src = ds->T.cdf; break;
    case KZ_TABLE_LIGHTS: src = ds->T.lights; break;
    case KZ_TABLE_BSDFS: src = ds->T.bsdfs; break;
    case KZ_TABLE_EM_TRIS: src = ds->T.emTris; break;
    default: src = ds->T.ilTris; break;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, copy, hipMemcpyDeviceToHost));
    return KZ_OK;
}
