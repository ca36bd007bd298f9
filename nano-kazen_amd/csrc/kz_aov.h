// kz_aov.h - feature films beside the picture (include/kazen_mi355x_aov.h): first-hit albedo, shading normal and depth of every sample, as functions of the
// first hit the scene's integrator shades - the record W.hit[slot] holds when the camera stage (wfCamera, kz_render.hip) returns: for path_mis after the H6
// walk-through of an invisible light, for the three others the first hit itself. Two forms, as for the integrators: the wavefront kernel kz_wf_aov that
// wfPass launches between the camera stage and the first shade / ao / mats launch, and a reference-shaped kernel (one lane = one sample, BVH2) behind
// kz_aov_samples. Sample to camera ray, hit record to RawHit and the walk-through test are the path kernels' own functions (kz_devfn.h); that those kernels'
// compiled code stays what it was is checked by scripts/device_code_diff.sh.
#pragma once
#include "kz_devfn.h"
#include "kz_wavefront.h"

// The features of one shaded hit. albedo: the hit's BSDF row - a normalmap unwrapped to its nested row - `albedo` (diffuse, ggx, roughplastic) or `baseColor`
// (kazenstandard) through its texture at its.uv exactly as resolveTextures folds it; the models without a diffuse colour (mirror, dielectric, roughdielectric,
// roughconductor) are white. An emitter is a surface like any other: its row, not its radiance. normal: its.sh.n as post-intersection leaves it (signed), or the
// perturbed frame's normal nm.pf.n of a normalmap row (nmapSetup).
template <int EXT>
__device__ __forceinline__ void aovFeatures(const KzDevTables &T, const Its &its, V3 &albedo, V3 &normal) {
    const KzBSDF *b = &T.bsdfs[its.bsdf];
    normal = its.sh.n;
    if (EXT & KZ_X_NMAP) { if (b->type == KZ_BSDF_NORMALMAP) { NMap nm; nmapSetup(T, *b, its, nm); normal = nm.pf.n; b = &T.bsdfs[b->nested]; } }
    const int32_t type = b->type;
    if ((EXT & KZ_X_MODELS) && (type == KZ_BSDF_MIRROR || type == KZ_BSDF_DIELECTRIC || type == KZ_BSDF_ROUGHDIELECTRIC || type == KZ_BSDF_ROUGHCONDUCTOR)) { albedo = mk(1.0f); return; }
    if ((EXT & KZ_X_TEX) && b->albedoTex) { albedo = texEval(T, b->albedoTex, its.uvx, its.uvy); return; }
    albedo = type == KZ_BSDF_KAZENSTANDARD ? mk(b->baseColor[0], b->baseColor[1], b->baseColor[2]) : mk(b->albedo[0], b->albedo[1], b->albedo[2]);
}

__device__ __forceinline__ void aovStore(const KzAovPlanes &A, int f, uint32_t slot, V3 v) {
    __builtin_nontemporal_store(v.x, A.p[f] + slot); __builtin_nontemporal_store(v.y, A.p[f] + A.stride + slot); __builtin_nontemporal_store(v.z, A.p[f] + 2 * A.stride + slot);
}

// Every enabled feature of every item of the pass - a miss: zeros - into the planes. Grid-stride, one lane per item, like kz_wf_normals; bound by the 112-B
// shading record it gathers per hit and the streams it reads and writes. EXT as the shade kernel's: a lean scene compiles no texture code.
template <int EXT>
__global__ __launch_bounds__(KZ_BLOCK) void kz_wf_aov(KzDevTables T, KzWf W, uint32_t nItems, uint32_t mask, KzAovPlanes A) {
    for (uint32_t slot = blockIdx.x * KZ_BLOCK + threadIdx.x; slot < nItems; slot += gridDim.x * KZ_BLOCK) {
        const float4 h = kzLoadStream(&W.hit[slot]);
        V3 albedo = mk(0.f), normal = mk(0.f); float depth = 0.f;
        if (h.x < KZ_INF) {
            const RawHit rh = rawHitOf(h);
            Its its; postIntersect<false>(T, rh, its);
            aovFeatures<EXT>(T, its, albedo, normal);
            depth = h.x;
        }
        if (mask & KZ_AOV_ALBEDO) aovStore(A, 0, slot, albedo);
        if (mask & KZ_AOV_NORMAL) aovStore(A, 1, slot, normal);
        if (mask & KZ_AOV_DEPTH) aovStore(A, 2, slot, mk(depth));
    }
}

// kz_aov_samples: renderSample up to the first shaded hit (renderer.cpp:20-33, integrator.cpp:206-219) with the megakernel's own closestHit, the path_mis
// walk-through and postIntersect; 10 floats per sample: jitter x, y | albedo | normal | depth | hit. `mis`: the scene's integrator walks through invisible lights.
__global__ __launch_bounds__(KZ_BLOCK) void kz_aov_samples_kernel(KzParams P, KzDevTables T, const uint32_t *__restrict__ pixList, const uint32_t *__restrict__ itemSample,
                                                                  uint32_t nItems, int mis, float *__restrict__ out) {
    __shared__ uint32_t s_stack[KZ_STACK_DEPTH * KZ_BLOCK];
    const uint32_t item = blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (item >= nItems) return;
    uint32_t *stk = s_stack + threadIdx.x;
    Counters cn = {0, 0, 0, 0, 0, 0};
    int px, py; pixelOf(pixList[item], px, py);
    Sampler smp; float jx, jy; V3 ro, rd; float mint, maxt;
    cameraSample(P, T, px, py, itemSample[item], smp, jx, jy, ro, rd, mint, maxt);
    V3 albedo = mk(0.f), normal = mk(0.f); float depth = 0.f, hit = 0.f;
    RawHit rh; Its its;
    if (closestHit<false>(T, P.rootRef, ro, rd, mint, maxt, rh, stk, cn)) {
        postIntersect<false>(T, rh, its);
        if (mis && isInvisibleLight(T, its.light)) {                                          // integrator.cpp:214-219 (H6): the result is ignored on a miss
            const V3 no = walkThroughOrigin(P, its, rd);
            if (closestHit<false>(T, P.rootRef, no, rd, KZ_EPSILON, KZ_INF, rh, stk, cn)) postIntersect<false>(T, rh, its);
        }
        aovFeatures<KZ_X_ALL>(T, its, albedo, normal);
        depth = its.t; hit = 1.f;
    }
    float *o = out + (size_t)item * 10;
    o[0] = jx; o[1] = jy; o[2] = albedo.x; o[3] = albedo.y; o[4] = albedo.z; o[5] = normal.x; o[6] = normal.y; o[7] = normal.z; o[8] = depth; o[9] = hit;
}
