// kz_motion.hip - what include/kazen_mi355x_motion.h needs beyond the denoiser's unit: the id kernel - which mesh every frame pixel shows - and the host-only row
// table. The kernel calls the path kernels' own cameraRay, closestHit, postIntersect and walk-through (kz_devfn.h), so this unit is compiled as the render units are
// (build.sh DEVICE_UNITS, with flush-to-zero): its hits are the oracle's hits. kz_dn_prepare_motion, which reads the ids, lives in the IEEE unit (kz_denoise.hip).
#include "kz_state.h"
#include "kz_devfn.h"

#include <cmath>
#include <cstring>
#include <vector>

// The lanes of a block over the frame. Primary rays are coherent in two dimensions: by default a wave is an 8 x 8 pixel tile and a block of four waves 16 x 16
// pixels; -DKZ_MOTION_TILE=0 builds the row mapping instead (a wave = 64 pixels of a row, a block four rows) for scripts/motion_rates.py to time the two side by
// side. The result does not depend on the mapping.
#ifndef KZ_MOTION_TILE
#define KZ_MOTION_TILE 1
#endif
#if KZ_MOTION_TILE
#define KZ_MOTION_BW 16
#define KZ_MOTION_BH 16
#else
#define KZ_MOTION_BW 64
#define KZ_MOTION_BH 4
#endif
static_assert(KZ_MOTION_BW * KZ_MOTION_BH == KZ_BLOCK, "a block of the id kernel is KZ_BLOCK lanes");

// renderSample up to the first shaded hit, as kz_aov_samples_kernel (kz_aov.h) has it, for the film position (x + 1/2, y + 1/2) and the lens centre - the aperture
// sample (0, 0): radius sqrtExact(0) = 0, whatever the angle - with the mesh of the hit as the only result. One lane per pixel, the BVH2 and the per-lane LDS stack
// of the reference-shaped kernels. `mis`: the scene's integrator walks through invisible lights (a miss behind one keeps the light's hit, as the integrator does).
__global__ __launch_bounds__(KZ_BLOCK) void kz_motion_ids_kernel(KzParams P, KzDevTables T, int mis, uint32_t *__restrict__ ids) {
    __shared__ uint32_t s_stack[KZ_STACK_DEPTH * KZ_BLOCK];
#if KZ_MOTION_TILE
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int x = (int)(blockIdx.x * KZ_MOTION_BW + (wave & 1u) * 8u + (lane & 7u)), y = (int)(blockIdx.y * KZ_MOTION_BH + (wave >> 1) * 8u + (lane >> 3));
#else
    const int x = (int)(blockIdx.x * KZ_MOTION_BW + (threadIdx.x & 63u)), y = (int)(blockIdx.y * KZ_MOTION_BH + (threadIdx.x >> 6));
#endif
    if (x >= P.width || y >= P.height) return;
    uint32_t *stk = s_stack + threadIdx.x;
    Counters cn = {0, 0, 0, 0, 0, 0};
    V3 ro, rd; float mint, maxt;
    cameraRay(P, (float)x + 0.5f, (float)y + 0.5f, 0.0f, 0.0f, ro, rd, mint, maxt);
    uint32_t id = KZ_MOTION_MISS;
    RawHit rh; Its its;
    if (closestHit<false>(T, P.rootRef, ro, rd, mint, maxt, rh, stk, cn)) {
        postIntersect<false>(T, rh, its);
        if (mis && isInvisibleLight(T, its.light)) {                                          // integrator.cpp:214-219 (H6): the result is ignored on a miss
            const V3 no = walkThroughOrigin(P, its, rd);
            if (closestHit<false>(T, P.rootRef, no, rd, KZ_EPSILON, KZ_INF, rh, stk, cn)) postIntersect<false>(T, rh, its);
        }
        id = its.mesh;
    }
    ids[(size_t)y * (size_t)P.width + (size_t)x] = id;                                        // x < width, y < height: < width * height
}

// ds->mtIds for the scene as it stands: the BVH2 resident and current as kz_aov_samples has it (kzEnsureBvh2; a refit keeps a resident BVH2 up to date), behind
// everything queued on the device - the streams of a replica do not wait for the null stream - and finished on return.
int kzMotionIds(KzScene *scene, KzDeviceState *ds) {
    int rc;
    if ((rc = kzEnsureBvh2(scene, ds))) return rc;
    const KzParams &P = scene->prm;
    const size_t nPix = (size_t)P.width * (size_t)P.height;
    if (ds->mtIds.cap() != nPix && (rc = ds->mtIds.regrow(nPix))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const dim3 grid((unsigned)((P.width + KZ_MOTION_BW - 1) / KZ_MOTION_BW), (unsigned)((P.height + KZ_MOTION_BH - 1) / KZ_MOTION_BH));
    hipLaunchKernelGGL(kz_motion_ids_kernel, grid, dim3(KZ_BLOCK), 0, 0, P, ds->T, P.integrator == KZ_INTEGRATOR_PATH_MIS ? 1 : 0, ds->mtIds.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return KZ_OK;
}

// ---- the rows, in double
namespace {

// the inverse of a row-major 3 x 3 by its adjugate; false: the determinant is 0 or not finite
bool mtInverse3(const double m[9], double inv[9]) {
    const double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};      // the adjugate, row-major
    const double det = m[0] * c[0] + m[1] * c[3] + m[2] * c[6];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int k = 0; k < 9; ++k) inv[k] = c[k] / det;
    return true;
}

void mtIdentity(KzMotionRow &r, uint32_t flags) {
    std::memset(&r, 0, sizeof r);
    r.d[0] = r.d[5] = r.d[10] = 1.f; r.n[0] = r.n[4] = r.n[8] = 1.f;
    r.flags = flags;
}

// one mesh: C its matrix now, H the history's (16 floats each, row-major)
void mtRow(const float *C, const float *H, KzMotionRow &r) {
    for (int k = 0; k < 16; ++k) if (!std::isfinite(C[k]) || !std::isfinite(H[k])) { mtIdentity(r, KZ_MOTION_UNTRACKED); return; }
    if (std::memcmp(C, H, 16 * sizeof(float)) == 0) { mtIdentity(r, KZ_MOTION_STATIC); return; }
    mtIdentity(r, KZ_MOTION_UNTRACKED);
    for (const float *m : {C, H}) if (m[12] != 0.f || m[13] != 0.f || m[14] != 0.f || m[15] != 1.f) return;      // not affine
    const double a[9] = {C[0], C[1], C[2], C[4], C[5], C[6], C[8], C[9], C[10]}, h[9] = {H[0], H[1], H[2], H[4], H[5], H[6], H[8], H[9], H[10]};
    double ai[9], hi[9];
    if (!mtInverse3(a, ai) || !mtInverse3(h, hi)) return;               // a singular C has no inverse; a singular H leaves the normals' map without one
    // X' = H C^-1 X: linear part L = h a^-1, translation t_H - L t_C; the normals' map is (L^-1)^T = (a h^-1)^T
    double L[9], Li[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            L[3 * i + j] = (h[3 * i] * ai[j] + h[3 * i + 1] * ai[3 + j]) + h[3 * i + 2] * ai[6 + j];
            Li[3 * i + j] = (a[3 * i] * hi[j] + a[3 * i + 1] * hi[3 + j]) + a[3 * i + 2] * hi[6 + j];
        }
    KzMotionRow out;
    mtIdentity(out, 0);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { out.d[4 * i + j] = (float)L[3 * i + j]; out.n[3 * i + j] = (float)Li[3 * j + i]; }
        out.d[4 * i + 3] = (float)((double)H[4 * i + 3] - ((L[3 * i] * (double)C[3] + L[3 * i + 1] * (double)C[7]) + L[3 * i + 2] * (double)C[11]));
    }
    for (int k = 0; k < 12; ++k) if (!std::isfinite(out.d[k])) return;
    for (int k = 0; k < 9; ++k) if (!std::isfinite(out.n[k])) return;
    r = out;
}

}  // namespace

extern "C" {

int kz_motion_rows(const float *cur, const float *prev, uint32_t nMeshes, KzMotionRow *rows) {
    if (nMeshes && !rows) return kz_fail(KZ_ERR_INVALID_ARG, "kz_motion_rows: null rows for %u meshes", nMeshes);
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (uint32_t m = 0; m < nMeshes; ++m) mtRow(cur ? cur + 16 * (size_t)m : identity, prev ? prev + 16 * (size_t)m : identity, rows[m]);
    return KZ_OK;
}

int kz_motion_ids(KzScene *scene, int device, uint32_t *ids, size_t n) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_motion_ids: null scene");
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    const size_t nPix = (size_t)scene->prm.width * (size_t)scene->prm.height;
    if (!ids || n != nPix) return kz_fail(KZ_ERR_INVALID_ARG, "kz_motion_ids: the id buffer must hold %zu words (width x height)", nPix);
    if ((rc = kzMotionIds(scene, ds))) return rc;
    return ds->mtIds.download(ids, nPix);
}

} // extern "C"
