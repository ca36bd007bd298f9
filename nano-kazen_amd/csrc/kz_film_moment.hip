// kz_film_moment.hip - the tap kernels of the second-moment film (include/kazen_mi355x_variance.h) and their launcher. A unit of its own beside kz_film.hip: the code the
// compiler gives the picture's and the feature films' tap kernels follows what else is instantiated in their unit, and they keep the code they had
// (scripts/device_code_diff.sh). Everything else about the film - its sums, its resolve, its entry points - is kz_film.hip's, as for every other film.
#include "kz_state.h"
#include "kz_devfn.h"

// The second-moment film's kernel (kazen_mi355x_variance.h): kz_film_taps<TAPS, GROUPS, false> (kz_film.hip) restated with the values
// SQUARED behind the validity test of the SAMPLE, so `tapSums` receives (w r^2, w g^2, w b^2, w): the w channel has the picture's bits (FUSED = false, launched
// behind the picture's kernel). FUSED = true is the one-pass form: the values into `tapSums` and the squares into `tapSums2` from one read of the sample planes, each
// accumulator the sum the two launches form.
template <int TAPS, int GROUPS, bool FUSED>
__global__ __launch_bounds__(64) void kz_film_taps_moment(KzParams P, const float *__restrict__ filter, const uint32_t *__restrict__ pixList, uint32_t nPix, uint32_t S,
                                                          const float *__restrict__ inJx, const float *__restrict__ inJy, const float *__restrict__ inR,
                                                          const float *__restrict__ inG, const float *__restrict__ inB, float4 *__restrict__ tapSums, float4 *__restrict__ tapSums2, size_t framePix) {
    constexpr int PIX = 64 / GROUPS, R0 = (TAPS + GROUPS - 1) / GROUPS, CHUNK = GROUPS == 1 ? KZ_TAPS_CHUNK1 : KZ_TAPS_CHUNK;
    __shared__ float s_filter[KZ_FILTER_RESOLUTION + 1];
    __shared__ float s_in[5][CHUNK][PIX + 1];                          // [array][sample][pixel], rows padded against bank conflicts of the transposing store
    const int lane = threadIdx.x, pixLane = lane % PIX, group = lane / PIX;
    if (lane <= KZ_FILTER_RESOLUTION) s_filter[lane] = filter[lane];
    const uint32_t pl0 = blockIdx.x * (uint32_t)PIX, pl = pl0 + (uint32_t)pixLane;
    const bool havePixel = pl < nPix;
    const uint32_t pxy = havePixel ? pixList[pl] : 0u;
    const int px = (int)(pxy & 0xffffu), py = (int)(pxy >> 16);
    const int bx0 = px & ~31, by0 = py & ~31;                          // the reference block this pixel is rendered in
    const float r = P.filterRadius, lf = P.lookupFactor;
    const int ty0 = group * R0, nRowsMine = min(R0, max(0, TAPS - ty0));
    float xb[TAPS], yb[R0];                                            // block-relative film coordinates this pixel reaches through tap t
#pragma unroll
    for (int t = 0; t < TAPS; ++t) xb[t] = (float)(px + P.border - P.tapLo - t - bx0);
#pragma unroll
    for (int t = 0; t < R0; ++t) yb[t] = (float)(py + P.border - P.tapLo - (ty0 + t) - by0);
    float4 *const mine = tapSums + (size_t)py * (size_t)P.width + (size_t)px;
    float4 acc[R0 * TAPS];
#pragma unroll
    for (int ty = 0; ty < R0; ++ty)
#pragma unroll
        for (int tx = 0; tx < TAPS; ++tx)
            acc[ty * TAPS + tx] = (havePixel && ty < nRowsMine) ? mine[(size_t)((ty0 + ty) * TAPS + tx) * framePix] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 *const mine2 = FUSED ? tapSums2 + (size_t)py * (size_t)P.width + (size_t)px : nullptr;
    float4 acc2[FUSED ? R0 * TAPS : 1];
    if (FUSED) {
#pragma unroll
        for (int ty = 0; ty < R0; ++ty)
#pragma unroll
            for (int tx = 0; tx < TAPS; ++tx)
                acc2[ty * TAPS + tx] = (havePixel && ty < nRowsMine) ? mine2[(size_t)((ty0 + ty) * TAPS + tx) * framePix] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float *const in[5] = {inJx, inJy, inR, inG, inB};
    const uint32_t nRows = min((uint32_t)PIX, nPix - min(nPix, pl0));  // pixels of this wave
    for (uint32_t c0 = 0; c0 < S; c0 += CHUNK) {
        const uint32_t n = min((uint32_t)CHUNK, S - c0);
        __syncthreads();
        for (uint32_t i = lane; i < nRows * CHUNK; i += 64u) {         // consecutive lanes: consecutive samples of one pixel, then the next pixel
            const uint32_t p = i / CHUNK, k = i % CHUNK;
            if (k < n) {
                const size_t gi = (size_t)(pl0 + p) * S + c0 + k;
#pragma unroll
                for (int a = 0; a < 5; ++a) s_in[a][k][p] = in[a][gi];
            }
        }
        __syncthreads();
        if (havePixel) {
            for (uint32_t k = 0; k < n; ++k) {
                const float jx = s_in[0][k][pixLane], jy = s_in[1][k][pixLane];
                float cr = s_in[2][k][pixLane], cg = s_in[3][k][pixLane], cb = s_in[4][k][pixLane];
                const bool valid = (cr >= 0.f && cg >= 0.f && cb >= 0.f) && isfinite(cr) && isfinite(cg) && isfinite(cb);   // Color3f::isValid
                if (!valid) continue;                                  // an invalid sample carries weight 0 everywhere: adds exact zeros
                const float qr = cr * cr, qg = cg * cg, qb = cb * cb;  // (a square that overflows is added as computed)
                if (!FUSED) { cr = qr; cg = qg; cb = qb; }
                const float posx = ((float)px + jx) - 0.5f - (float)(bx0 - P.border), posy = ((float)py + jy) - 0.5f - (float)(by0 - P.border);   // block.cpp:64-67
                const float lox = ceilf(posx - r), hix = floorf(posx + r), loy = ceilf(posy - r), hiy = floorf(posy + r);                     // block.cpp:70-73
                float wx[TAPS], wy[R0];
#pragma unroll
                for (int t = 0; t < TAPS; ++t) wx[t] = !(xb[t] < lox || xb[t] > hix) ? s_filter[(int)(fabsf(xb[t] - posx) * lf)] : 0.f;          // block.cpp:77-80
#pragma unroll
                for (int t = 0; t < R0; ++t) wy[t] = (t < nRowsMine && !(yb[t] < loy || yb[t] > hiy)) ? s_filter[(int)(fabsf(yb[t] - posy) * lf)] : 0.f;
#pragma unroll
                for (int ty = 0; ty < R0; ++ty)
#pragma unroll
                    for (int tx = 0; tx < TAPS; ++tx) {
                        float4 &a = acc[ty * TAPS + tx];
                        a.x += cr * wx[tx] * wy[ty]; a.y += cg * wx[tx] * wy[ty]; a.z += cb * wx[tx] * wy[ty]; a.w += 1.0f * wx[tx] * wy[ty];     // block.cpp:84
                        if (FUSED) {
                            float4 &m = acc2[ty * TAPS + tx];
                            m.x += qr * wx[tx] * wy[ty]; m.y += qg * wx[tx] * wy[ty]; m.z += qb * wx[tx] * wy[ty]; m.w += 1.0f * wx[tx] * wy[ty];
                        }
                    }
            }
        }
    }
    if (havePixel) {
#pragma unroll
        for (int ty = 0; ty < R0; ++ty)
            if (ty < nRowsMine) {
#pragma unroll
                for (int tx = 0; tx < TAPS; ++tx) mine[(size_t)((ty0 + ty) * TAPS + tx) * framePix] = acc[ty * TAPS + tx];
                if (FUSED) {
#pragma unroll
                    for (int tx = 0; tx < TAPS; ++tx) mine2[(size_t)((ty0 + ty) * TAPS + tx) * framePix] = acc2[ty * TAPS + tx];
                }
            }
    }
}

// The second-moment film's stage of a pass (kazen_mi355x_variance.h): the same pixel list and the same five sample planes as the picture's stage, on the same stream.
// onePass = false: kz_film_taps_moment<.., false> into `moment`'s sums, directly behind the picture's tap launch; onePass = true: kz_film_taps_moment<.., true> INSTEAD of
// the picture's launch - both films' sums from one read of the planes. That form is built and timed for filters of up to 5 taps (197 VGPRs at 5 taps, no scratch, 2 waves
// per SIMD against the 4 of the two-launch kernels, and still the faster: DESIGN.md 4f); for 6 .. 9 taps it would compile without scratch too (179 .. 256 VGPRs, 2 .. 1
// waves per SIMD) but has not been timed, so those filters take the two launches. Always the default lane grouping: the sums do not depend on it.
bool kzFilmMomentOnePassOk(const KzParams &P) { return P.tapHi - P.tapLo + 1 <= 5; }
template <bool FUSED>
static int launchTapsMoment(const KzParams &P, KzDeviceState *ds, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *const plane[5], float4 *sums, float4 *sums2) {
    const int ftaps = P.tapHi - P.tapLo + 1;
    const size_t framePix = (size_t)P.width * (size_t)P.height;
#define KZ_FILM_TAPS(N, GR) hipLaunchKernelGGL((kz_film_taps_moment<N, GR, FUSED>), dim3((nPixPass + 64 / GR - 1) / (64 / GR)), dim3(64), 0, pst, P, ds->T.filter, pixList, nPixPass, Sp, plane[0], plane[1], plane[2], plane[3], plane[4], sums, sums2, framePix)
    switch (ftaps) {
        case 1: KZ_FILM_TAPS(1, 2); break; case 2: KZ_FILM_TAPS(2, 2); break; case 3: KZ_FILM_TAPS(3, 2); break; case 4: KZ_FILM_TAPS(4, 2); break; case 5: KZ_FILM_TAPS(5, 2); break;
        default:
            if constexpr (!FUSED) switch (ftaps) {
                case 6: KZ_FILM_TAPS(6, 4); break; case 7: KZ_FILM_TAPS(7, 4); break; case 8: KZ_FILM_TAPS(8, 4); break; case 9: KZ_FILM_TAPS(9, 4); break;
                default: return kz_fail(KZ_ERR_UNSUPPORTED, "film filter of %d taps per axis (at most %d)", ftaps, KZ_MAX_FILTER_TAPS);
            }
            else return kz_fail(KZ_ERR_STATE, "the one-pass tap kernel is built for filters of up to 5 taps per axis, not %d", ftaps);
    }
#undef KZ_FILM_TAPS
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}
int kzFilmStageMoment(KzScene *scene, KzDeviceState *ds, KzFilm &picture, KzFilm &moment, bool onePass, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *const plane[5], hipEvent_t waitFilm) {
    if (!moment.sums) return kz_fail(KZ_ERR_STATE, "the tap sums of the second-moment film are not there");
    if (!onePass) return launchTapsMoment<false>(scene->prm, ds, pst, pixList, nPixPass, Sp, plane, moment.sums, nullptr);
    if (waitFilm) HIP_TRY(hipStreamWaitEvent(pst, waitFilm, 0));
    return launchTapsMoment<true>(scene->prm, ds, pst, pixList, nPixPass, Sp, plane, picture.sums, moment.sums);
}
