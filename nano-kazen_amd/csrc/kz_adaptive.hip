// kz_adaptive.hip - include_ext/kazen_mi355x_adaptive.h on the device: the launcher of the classification stage (kernel: kz_adaptive.h) and the test surface
// kz_adaptive_classify_films. The driver that renders the rounds, and everything of the rule that needs no device, is kz_adaptive_host.cpp. This unit keeps
// subnormals (build.sh IEEE_UNITS): the pixel test's variances and bounds compare as a plain C++ restatement's do.
#include "kz_state.h"
#include "kz_adaptive.h"

#include <vector>

// The test of one round on `stream`: one wave per block, KZ_ADAPTIVE_WAVES blocks per workgroup. The films are resolved; rec and active hold one entry per block.
int kzAdaptiveClassify(const float4 *film, const float4 *moment, int32_t width, int32_t height, int32_t border, const KzAdaptiveRule &rule, const uint32_t *blockSamples, uint32_t nAll,
                       KzAdaptiveBlock *rec, uint8_t *active, hipStream_t stream) {
    const uint32_t e = rule.block, nbx = ((uint32_t)width + e - 1) / e, nby = ((uint32_t)height + e - 1) / e;
    KzAdaptiveArgs A;
    A.film = film; A.moment = moment; A.width = width; A.height = height; A.border = border;
    A.nbx = nbx; A.nBlocks = nbx * nby; A.blockSamples = blockSamples; A.nAll = nAll;
    A.thr2 = rule.thr2; A.floor = rule.floor; A.permille = rule.permille; A.maxSamples = rule.maxSamples;
    const dim3 grid((A.nBlocks + KZ_ADAPTIVE_WAVES - 1) / KZ_ADAPTIVE_WAVES), wg(64 * KZ_ADAPTIVE_WAVES);
    switch (e) {
        case 8: hipLaunchKernelGGL(kz_adaptive_classify<8>, grid, wg, 0, stream, A, rec, active); break;
        case 16: hipLaunchKernelGGL(kz_adaptive_classify<16>, grid, wg, 0, stream, A, rec, active); break;
        case 32: hipLaunchKernelGGL(kz_adaptive_classify<32>, grid, wg, 0, stream, A, rec, active); break;
        case 64: hipLaunchKernelGGL(kz_adaptive_classify<64>, grid, wg, 0, stream, A, rec, active); break;
        default: return kz_fail(KZ_ERR_INVALID_ARG, "adaptive block edge %u (8, 16, 32 or 64)", e);
    }
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

extern "C" int kz_adaptive_classify_films(int device, int32_t width, int32_t height, int32_t border, const float *film, const float *moment, const uint32_t *blockSamples,
                                          const KzAdaptiveOpts *aopts, KzAdaptiveBlock *out) {
    static const char *call = "kz_adaptive_classify_films";
    if (!film || !moment || !blockSamples || !out) return kz_fail(KZ_ERR_INVALID_ARG, "%s: null film, moment, blockSamples or out", call);
    if (width < 1 || height < 1 || border < 0 || border > 64 || (uint64_t)(width + 2 * (int64_t)border) * (uint64_t)(height + 2 * (int64_t)border) >= (1ull << 31))
        return kz_fail(KZ_ERR_INVALID_ARG, "%s: a frame of %d x %d with border %d (at least 1 x 1, border 0 .. 64, fewer than 2^31 texels)", call, width, height, border);
    KzAdaptiveRule rule; int rc;
    if ((rc = kzAdaptiveResolve(aopts, 0u, call, &rule))) return rc;
    if ((rc = kzUseDevice(device))) return rc;
    const size_t nTexels = (size_t)(width + 2 * border) * (size_t)(height + 2 * border);
    const size_t nBlocks = (size_t)(((uint32_t)width + rule.block - 1) / rule.block) * (size_t)(((uint32_t)height + rule.block - 1) / rule.block);
    DevBuf<float4> dFilm, dMoment; DevBuf<uint32_t> dSamples; DevBuf<KzAdaptiveBlock> dRec; DevBuf<uint8_t> dActive;
    if ((rc = dFilm.alloc(nTexels)) || (rc = dFilm.upload((const float4 *)film, nTexels)) || (rc = dMoment.alloc(nTexels)) || (rc = dMoment.upload((const float4 *)moment, nTexels)) ||
        (rc = dSamples.alloc(nBlocks)) || (rc = dSamples.upload(blockSamples, nBlocks)) || (rc = dRec.alloc(nBlocks)) || (rc = dActive.alloc(nBlocks))) return rc;
    HIP_TRY(hipMemset(dRec, 0, dRec.bytes()));
    HIP_TRY(hipMemset(dActive, 0, dActive.bytes()));
    if ((rc = kzAdaptiveClassify(dFilm, dMoment, width, height, border, rule, dSamples, 0u, dRec, dActive, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return dRec.download(out, nBlocks);
}
