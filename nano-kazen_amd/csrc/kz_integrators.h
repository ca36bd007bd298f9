// kz_integrators.h - the integrators other than path_mis: "normals" (integrator.cpp:11-34), "ao" (:37-71) and "path_mats" (:137-181), in the two forms
// the library has for path_mis: a reference-shaped megakernel (one lane = one sample, BVH2; pipeline 1 and kz_render_samples) and the wavefront kernels of
// the default pipeline (wfPassIntegrator in kz_render.hip launches them around the unchanged camera-ray and traversal kernels of kz_wavefront.h).
// The per-path steps these kernels have in common with the path_mis kernels and with each other - sample to camera ray, hit record to RawHit, the emitter
// term, a slot's pixel and sample index, the radiance add - are stated once, as __forceinline__ functions of kz_devfn.h and
// kz_wavefront.h. That the path_mis kernels' compiled code stays what it was is checked, not assumed: scripts/device_code_diff.sh.
#pragma once
#include "kz_devfn.h"
#include "kz_wavefront.h"

#define KZ_INV_TWOPI 0.15915494309189533577f          // common.h:35

// Warp::squareToUniformHemisphere (warp.cpp:68-79). M_PI is common.h's float literal (common.h:31-33), so 2.0f * M_PI * y is a float product,
// evaluated left to right; std::sin / std::cos of that float are the defined sequences of kz_crmath.h (LAB_NOTES H14).
__device__ __forceinline__ V3 squareToUniformHemisphere(float sx, float sy) {
    const float z = sx;
    const float tmp = sqrtExact(1.0f - z * z);
    float sinPhi, cosPhi; kzSinCos(2.0f * KZ_PI_F * sy, &sinPhi, &cosPhi);
    return mk(cosPhi * tmp, sinPhi * tmp, z);
}
// AmbientOcclusionIntegrator::Li after an unoccluded occlusion ray (integrator.cpp:58-62): shFrame.n.normalize(), point.normalize(), the cosine in the
// shading frame, then Color3f(cosTheta / M_PI) / INV_TWOPI - two float divisions (H14). The caller adds it to a zero sum, so a -0 comes out as +0.
__device__ __forceinline__ float aoValue(const Its &its, V3 dirWorld) {
    const V3 n = normalized(its.sh.n), d = normalized(dirWorld);
    const float cosTheta = dot(d, n);
    return (cosTheta / KZ_PI_F) / KZ_INV_TWOPI;
}
// The occlusion ray of `ao`: Ray3f(its.p, its.toWorld(sample)) - mint Epsilon, maxt infinite (ray.h:35-38), NOT traceBias
__device__ __forceinline__ V3 aoDirection(const Its &its, float sx, float sy) { return toWorld(its.sh, squareToUniformHemisphere(sx, sy)); }
// std::min(t.x(), 0.95f) (integrator.cpp:158): (0.95f < t.x) ? 0.95f : t.x - a NaN throughput stays NaN, as it does there
__device__ __forceinline__ float matsRoulette(float tx) { return (0.95f < tx) ? 0.95f : tx; }

// ---- megakernel form ----------------------------------------------------------------------------------------------------
template <int EXT>
__device__ V3 normalsLi(const KzParams &P, const KzDevTables &T, V3 ro, V3 rd, float mint, float maxt, uint32_t *stk) {
    Counters cn = {0, 0, 0, 0, 0, 0};
    RawHit rh; Its its;
    if (!closestHit<false>(T, P.rootRef, ro, rd, mint, maxt, rh, stk, cn)) return mk(0.f);
    postIntersect<true>(T, rh, its);
    return mk(fabsf(its.geoN.x), fabsf(its.geoN.y), fabsf(its.geoN.z));      // geoFrame.n.cwiseAbs() (integrator.cpp:27)
}
__device__ V3 aoLi(const KzParams &P, const KzDevTables &T, Sampler &smp, V3 ro, V3 rd, float mint, float maxt, uint32_t *stk) {
    Counters cn = {0, 0, 0, 0, 0, 0};
    RawHit rh; Its its;
    if (!closestHit<false>(T, P.rootRef, ro, rd, mint, maxt, rh, stk, cn)) return mk(0.f);
    postIntersect<false>(T, rh, its);
    float sx, sy; smp.next2D(P, T, sx, sy);
    const V3 dir = aoDirection(its, sx, sy);
    if (anyHit<false>(T, P.rootRef, its.p, dir, KZ_EPSILON, KZ_INF, stk, cn)) return mk(0.f);      // scene->rayIntersect(ray): every triangle blocks
    return mk(0.f) + mk(aoValue(its, dir));
}
template <int EXT>
__device__ V3 matsLi(const KzParams &P, const KzDevTables &T, Sampler &smp, V3 ro, V3 rd, float mint, float maxt, uint32_t *stk) {
    Counters cn = {0, 0, 0, 0, 0, 0};
    V3 color = mk(0.f), t = mk(1.f);
    RawHit rh; Its its;
    for (int depth = 0; depth < KZ_PATH_MATS_MAX_DEPTH; ++depth) {                                     // (H15: the reference has no cap)
        if (!closestHit<false>(T, P.rootRef, ro, rd, mint, maxt, rh, stk, cn)) break;               // a miss: no background term
        postIntersect<false>(T, rh, its);
        if (its.light >= 0 && emitterFaces(its, normalized(its.p - ro))) color = color + emitterTerm(T.lights[its.light], 1.f, t);      // AreaLight::eval, no MIS weight (integrator.cpp:151-154)
        const float probability = matsRoulette(t.x);                                                // integrator.cpp:157-162
        if (smp.next1D(P, T) >= probability) break;
        t = t / probability;
        // (the bounce from here on is kz_wf_mats's, line for line: as one function of both forms it changed that kernel's compiled code - profiles/r13a_shared_steps)
        KzBSDF bsdf = T.bsdfs[its.bsdf];
        NMap nm; surfaceSetup<EXT>(T, its, bsdf, nm);                                               // (the record's uv: textures; no normal maps, H16)
        const V3 wiLocal = toLocal(its.sh, -rd);
        float s2x, s2y; smp.next2D(P, T, s2x, s2y);                                                 // H1: next2D before next1D
        const float s1 = smp.next1D(P, T);
        V3 woLocal; bool alive, discrete, solid; float etaScale, pdfUnused;
        const V3 f = surfSample<EXT>(bsdf, nm, its, wiLocal, 0.f, s1, s2x, s2y, woLocal, alive, discrete, etaScale, pdfUnused, solid);
        t = t * f;
        if (!alive || (f.x == 0.f && f.y == 0.f && f.z == 0.f)) break;                              // zero weight ends the path (as path_mis)
        ro = its.p; rd = toWorld(its.sh, woLocal); mint = KZ_EPSILON; maxt = KZ_INF;                 // Ray3f(its.p, its.toWorld(bRec.wo))
    }
    return color;
}

// renderBlock + renderSample (renderer.cpp:20-69) over the integrator INTEG; the same item layout and outputs as kz_path_megakernel
template <int INTEG, int EXT>
__global__ __launch_bounds__(KZ_BLOCK) void kz_integrator_megakernel(KzParams P, KzDevTables T, const uint32_t *__restrict__ pixList, uint32_t nItems, uint32_t S,
                                                                     uint32_t sampleBegin, const uint32_t *__restrict__ itemSample,
                                                                     float *__restrict__ outJx, float *__restrict__ outJy, float *__restrict__ outR,
                                                                     float *__restrict__ outG, float *__restrict__ outB) {
    __shared__ uint32_t s_stack[KZ_STACK_DEPTH * KZ_BLOCK];
    const uint32_t item = blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (item >= nItems) return;
    const uint32_t pl = item / S, so = item - pl * S;
    int px, py; pixelOf(pixList[pl], px, py);
    Sampler smp; float jx, jy; V3 ro, rd; float mint, maxt;
    cameraSample(P, T, px, py, itemSample ? itemSample[item] : sampleBegin + so, smp, jx, jy, ro, rd, mint, maxt);
    V3 L;
    if (INTEG == KZ_INTEGRATOR_NORMALS) L = normalsLi<EXT>(P, T, ro, rd, mint, maxt, s_stack + threadIdx.x);
    else if (INTEG == KZ_INTEGRATOR_AO) L = aoLi(P, T, smp, ro, rd, mint, maxt, s_stack + threadIdx.x);
    else L = matsLi<EXT>(P, T, smp, ro, rd, mint, maxt, s_stack + threadIdx.x);
    outJx[item] = jx; outJy[item] = jy; outR[item] = L.x; outG[item] = L.y; outB[item] = L.z;
}

// ---- wavefront form -----------------------------------------------------------------------------------------------------
// Queue entry i of (queue, count): queue ? queue[i] : i (the camera stage leaves every item's hit record at its own slot)
__device__ __forceinline__ uint32_t wfCountOf(const uint32_t *countPtr, uint32_t countImm) { return countPtr ? *countPtr : countImm; }

// normals: |n_geo| of the camera ray's closest hit into the sample planes (generate left them at 0: a miss stays black)
__global__ __launch_bounds__(KZ_BLOCK) void kz_wf_normals(KzParams P, KzDevTables T, KzWf W, uint32_t nItems) {
    for (uint32_t slot = blockIdx.x * KZ_BLOCK + threadIdx.x; slot < nItems; slot += gridDim.x * KZ_BLOCK) {
        const float4 h = kzLoadStream(&W.hit[slot]);
        if (!(h.x < KZ_INF)) continue;
        const RawHit rh = rawHitOf(h);
        Its its; postIntersect<true>(T, rh, its);
        W.outR[slot] = fabsf(its.geoN.x); W.outG[slot] = fabsf(its.geoN.y); W.outB[slot] = fabsf(its.geoN.z);
    }
}

// ao: post-intersection, the hemisphere draw, the occlusion ray (shA / shB) and the value it carries (shL) -> the shadow queue. kz_wf_trace<4> then adds the
// value of every ray that no triangle blocks (launched with no invisible-light triangles: nothing is walked through, H6 is path_mis's alone).
__global__ __launch_bounds__(KZ_BLOCK) void kz_wf_ao(KzParams P, KzDevTables T, KzWf W, const uint32_t *__restrict__ pixList, uint32_t S, uint32_t sampleBegin,
                                                     uint32_t nItems, uint32_t *__restrict__ shQueue, uint32_t *__restrict__ shCount) {
    __shared__ uint32_t s_buf[KZ_WF_QCAP]; __shared__ uint32_t s_n, s_gb;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    WfAppender ap = {s_buf, &s_n, &s_gb, shQueue, shCount};
    for (uint32_t base = blockIdx.x * KZ_BLOCK; base < nItems; base += gridDim.x * KZ_BLOCK) {
        const uint32_t slot = base + threadIdx.x;
        bool ray = false;
        if (slot < nItems) {
            const float4 h = kzLoadStream(&W.hit[slot]);
            if (h.x < KZ_INF) {
                const RawHit rh = rawHitOf(h);
                Its its; postIntersect<false>(T, rh, its);
                int px, py; uint32_t sampleIndex; wfSampleOf(pixList, S, sampleBegin, slot, px, py, sampleIndex);
                Sampler smp; wfLoadSampler(P, W, slot, px, py, sampleIndex, smp, 4u);
                float sx, sy; smp.next2D(P, T, sx, sy);
                const V3 dir = aoDirection(its, sx, sy);
                const float v = 0.f + aoValue(its, dir);
                kzStoreStream(&W.shA[slot], make_float4(its.p.x, its.p.y, its.p.z, KZ_INF));
                kzStoreStream(&W.shB[slot], make_float4(dir.x, dir.y, dir.z, KZ_EPSILON));
                kzStoreStream(&W.shL[slot], make_float4(v, v, v, 0.f));
                ray = true;
            }
        }
        ap.push(ray, slot);
        ap.maybeFlush(false);
    }
    ap.maybeFlush(true);
}

// path_mats, one bounce: emission (no MIS weight, no primaryVisibility test), roulette on t.x, BSDF sample -> the next ray into rayA / rayB and the
// next path queue; no light sample, no shadow ray. State per path: ray, hit, throughput (thr.xyz), sampler. Every bounce draws 1 + 2 + 1 dimensions.
// (EXT: KZ_X_MODELS | KZ_X_TEX at most - kz_scene_create refuses normal maps in a path_mats scene - compiled, like kz_wf_shade's texture variant, for 3 waves)
#define KZ_X_MATS (KZ_X_MODELS | KZ_X_TEX)
template <int EXT>
__global__ __launch_bounds__(KZ_BLOCK, ((EXT & KZ_X_TEX) ? 3 : 4)) void kz_wf_mats(KzParams P, KzDevTables T, KzWf W, const uint32_t *__restrict__ pixList, uint32_t S, uint32_t sampleBegin,
                                                       int iter, const uint32_t *__restrict__ queue, const uint32_t *__restrict__ countPtr, uint32_t countImm,
                                                       uint32_t *__restrict__ outQueue, uint32_t *__restrict__ outCount) {
    __shared__ uint32_t s_buf[KZ_WF_QCAP]; __shared__ uint32_t s_n, s_gb;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    WfAppender ap = {s_buf, &s_n, &s_gb, outQueue, outCount};
    const uint32_t count = wfCountOf(countPtr, countImm);
    for (uint32_t base = blockIdx.x * KZ_BLOCK; base < count; base += gridDim.x * KZ_BLOCK) {
        const uint32_t qi = base + threadIdx.x;
        bool next = false;
        uint32_t slot = 0;
        if (qi < count) {
            slot = queue ? queue[qi] : qi;
            const float4 h = kzLoadStream(&W.hit[slot]);
            if (h.x < KZ_INF) {
                const RawHit rh = rawHitOf(h);
                Its its; postIntersect<false>(T, rh, its);
                const float4 ra = kzLoadStream(&W.rayA[slot]), rb = kzLoadStream(&W.rayB[slot]);
                const V3 ro = mk(ra.x, ra.y, ra.z), rd = mk(rb.x, rb.y, rb.z);
                V3 t = mk(1.f);
                if (iter > 0) { const float4 th = kzLoadStream(&W.thr[slot]); t = mk(th.x, th.y, th.z); }
                if (its.light >= 0) { if (emitterFaces(its, normalized(its.p - ro))) wfAddRadiance(W, slot, emitterTerm(T.lights[its.light], 1.f, t)); }      // (no MIS weight; one writer per slot)
                int px, py; uint32_t sampleIndex; wfSampleOf(pixList, S, sampleBegin, slot, px, py, sampleIndex);
                Sampler smp; wfLoadSampler(P, W, slot, px, py, sampleIndex, smp, 4u + 4u * (uint32_t)iter);
                const float probability = matsRoulette(t.x);
                if (!(smp.next1D(P, T) >= probability)) {
                    t = t / probability;
                    KzBSDF bsdf = T.bsdfs[its.bsdf];
                    NMap nm; surfaceSetup<EXT>(T, its, bsdf, nm);
                    const V3 wiLocal = toLocal(its.sh, -rd);
                    float s2x, s2y; smp.next2D(P, T, s2x, s2y);
                    const float s1 = smp.next1D(P, T);
                    V3 woLocal; bool alive, discrete, solid; float etaScale, pdfUnused;
                    const V3 f = surfSample<EXT>(bsdf, nm, its, wiLocal, 0.f, s1, s2x, s2y, woLocal, alive, discrete, etaScale, pdfUnused, solid);
                    t = t * f;
                    if (alive && !(f.x == 0.f && f.y == 0.f && f.z == 0.f)) {
                        const V3 nd = toWorld(its.sh, woLocal);
                        kzStoreStream(&W.rayA[slot], make_float4(its.p.x, its.p.y, its.p.z, KZ_EPSILON));
                        kzStoreStream(&W.rayB[slot], make_float4(nd.x, nd.y, nd.z, KZ_INF));
                        kzStoreStream(&W.thr[slot], make_float4(t.x, t.y, t.z, 1.f));
                        wfStoreSampler(P, W, slot, smp);
                        next = true;
                    }
                }
            }
        }
        ap.push(next, slot);
        ap.maybeFlush(false);
    }
    ap.maybeFlush(true);
}
