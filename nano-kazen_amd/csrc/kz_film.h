// kz_film.h - one film of a replica: the running tap sums of every pixel of the frame, [tap][y * width + x], and the film texels resolved from them. A replica
// keeps five of identical construction - the picture, the albedo, normal and depth feature films (kazen_mi355x_aov.h) and the second-moment film
// (kazen_mi355x_variance.h) -, all fed by kz_film_taps (the last by its restatement kz_film_taps_moment, kz_film_moment.hip) and resolved by kz_film_resolve (kz_film.hip). What a film is made of arrives as plain numbers: nSums = taps x taps x the frame's pixels, nTexels = the frame's texels with
// its filter apron (KzDeviceState::filmPixels). Host code only, like kz_own.h: a plain C++ program can exercise it against stand-ins (tests/host_cpp/film_test.cpp).
#pragma once
#include "kz_own.h"

struct KzFilm {
    DevBuf<float4> sums, texels;
    // Before the passes of a call: sums and texels are there - allocated and zeroed on first use, the sums before the texels -, and sums that were there already are
    // zeroed unless the call accumulates (texels are not: the call's resolve writes every one). A failed allocation leaves the film as it was.
    int ensure(size_t nSums, size_t nTexels, bool accumulate, hipStream_t stream) {
        const bool fresh = !sums;
        int rc;
        if (fresh && (rc = sums.alloc(nSums))) return rc;
        if (!texels) {
            if ((rc = texels.alloc(nTexels))) { if (fresh) sums.free(); return rc; }      // (never sums that nothing has zeroed)
            HIP_TRY(hipMemsetAsync(texels, 0, texels.bytes(), stream));
        }
        if (fresh || !accumulate) HIP_TRY(hipMemsetAsync(sums, 0, sums.bytes(), stream));
        return KZ_OK;
    }
    int clear(hipStream_t stream) {
        if (sums) HIP_TRY(hipMemsetAsync(sums, 0, sums.bytes(), stream));
        if (texels) HIP_TRY(hipMemsetAsync(texels, 0, texels.bytes(), stream));
        return KZ_OK;
    }
    void free() { sums.free(); texels.free(); }
    size_t bytes() const { return sums.bytes() + texels.bytes(); }
};
