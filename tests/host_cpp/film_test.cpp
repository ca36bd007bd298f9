// No GPU: the film type of nano-kazen_amd/csrc/kz_film.h (KzFilm: running tap sums + the texels resolved from them) against stand-ins for kzMalloc, hipFree, hipMemset and
// hipMemsetAsync, which log every call - kind, element count (float4s), stream. A replica's four films (the picture at 0, AOV f at 1 + f) are driven through upload, renders,
// AOV mask changes, a clear and the release the way kz_replica.hip, kz_render.hip and kz_film.hip drive them, and the log is compared literally, step by step, with
// what the code before the film type did: the number, size and order of the device allocations and memsets of a call are part of what a first call of a job costs
// (renderOn: everything is allocated before the first context grows). Built with -fsanitize=address,undefined; tests/test_film_cpu.py builds and runs it.
#include "kz_film.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// ---- the stand-ins ----
struct Call {
    char kind; size_t elems; uintptr_t stream;          // 'A' kzMalloc, 'F' hipFree, 'Z' hipMemset (blocking: stream 0), 'z' hipMemsetAsync
    bool operator==(const Call &o) const { return kind == o.kind && elems == o.elems && stream == o.stream; }
};
static std::vector<Call> g_log;
struct Block { void *p; size_t bytes; };
static std::vector<Block> g_live;
static int g_failDev = 0;                               // > 0: the nth allocation from now on fails
static int g_failCode = 0;

static size_t bytesOf(const void *p) {
    for (const Block &b : g_live) if (b.p == p) return b.bytes;
    std::fprintf(stderr, "film_test.cpp: a pointer no live allocation starts at\n"); std::exit(1);
}
int kz_fail(int code, const char *, ...) { g_failCode = code; return code; }
hipError_t kzMalloc(void **p, size_t bytes) {
    *p = nullptr;
    if (g_failDev > 0 && --g_failDev == 0) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    g_live.push_back(Block{*p, bytes});
    g_log.push_back(Call{'A', bytes / sizeof(float4), 0});
    return hipSuccess;
}
extern "C" {
hipError_t hipFree(void *p) {
    g_log.push_back(Call{'F', bytesOf(p) / sizeof(float4), 0});
    for (size_t i = 0; i < g_live.size(); ++i) if (g_live[i].p == p) { g_live.erase(g_live.begin() + (long)i); break; }
    std::free(p);
    return hipSuccess;
}
// (a memset must cover its buffer exactly: every one of the library's film memsets does)
hipError_t hipMemset(void *p, int v, size_t bytes) { if (v != 0 || bytes != bytesOf(p)) std::exit(2); g_log.push_back(Call{'Z', bytes / sizeof(float4), 0}); return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t s) { if (v != 0 || bytes != bytesOf(p)) std::exit(2); g_log.push_back(Call{'z', bytes / sizeof(float4), (uintptr_t)s}); return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "film_test.cpp:%d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
// the log since the last look is exactly `want`
static bool logged(std::vector<Call> want) {
    const bool same = g_log == want;
    if (!same) { std::fprintf(stderr, "logged:"); for (const Call &c : g_log) std::fprintf(stderr, " %c %zu @%zu,", c.kind, c.elems, (size_t)c.stream); std::fprintf(stderr, "\n"); }
    g_log.clear();
    return same;
}

// ---- a replica's films, driven as the library drives them ----
// The geometry of tests/test_aov_cpu.py: a 96 x 72 frame, a filter of 5 taps per axis (gaussian r = 2), a border of 2.
static const size_t W = 96, H = 72, TAPS = 5, BORDER = 2;
static const size_t SUMS = TAPS * TAPS * W * H, TEXELS = (W + 2 * BORDER) * (H + 2 * BORDER);      // 172 800 and 7 600 float4
static_assert(SUMS == 172800 && TEXELS == 7600, "the numbers the expectations below are written with");
static const size_t FILM_BYTES = (SUMS + TEXELS) * 16;

struct Replica {
    KzFilm films[4];
    uint32_t mask = 0;
    // uploadReplica (kz_replica.hip): the picture's texels, zeroed with a blocking memset; its sums wait for the first render
    int upload() {
        if (const int rc = films[0].texels.alloc(TEXELS)) return rc;
        HIP_TRY(hipMemset(films[0].texels, 0, TEXELS * sizeof(float4)));
        return KZ_OK;
    }
    // renderOn (kz_render.hip), before the passes: the picture, then the enabled AOVs in ascending order
    int render(bool accumulate, hipStream_t s) {
        if (const int rc = films[0].ensure(SUMS, TEXELS, accumulate, s)) return rc;
        for (int f = 0; f < 3; ++f) if (mask & (1u << f)) if (const int rc = films[1 + f].ensure(SUMS, TEXELS, accumulate, s)) return rc;
        return KZ_OK;
    }
    // kz_scene_set_aovs (kz_film.hip): the films of the AOVs that leave the mask go
    void setAovs(uint32_t m) { for (int f = 0; f < 3; ++f) if (mask & ~m & (1u << f)) films[1 + f].free(); mask = m; }
    // kzFilmClear (kz_film.hip)
    int clear(hipStream_t s) { for (KzFilm &f : films) if (const int rc = f.clear(s)) return rc; return KZ_OK; }
    size_t aovBytes() const { return films[1].bytes() + films[2].bytes() + films[3].bytes(); }      // KzDeviceState::aovBytes
    size_t bytes() const { return films[0].bytes() + aovBytes(); }
};

int main() {
    const hipStream_t s1 = (hipStream_t)(uintptr_t)0x10, s2 = (hipStream_t)(uintptr_t)0x20, s3 = (hipStream_t)(uintptr_t)0x30;
    const uintptr_t S1 = 0x10, S2 = 0x20, S3 = 0x30;
    {
        Replica r;
        CHECK(r.bytes() == 0 && logged({}));
        // 1. upload. Before: uploadReplica - ds->film.alloc(filmPixels), a blocking hipMemset of it; no tap sums ("allocated by the first render, not at upload").
        CHECK(r.upload() == KZ_OK && logged({{'A', TEXELS, 0}, {'Z', TEXELS, 0}}));
        CHECK(r.films[0].bytes() == TEXELS * 16 && r.aovBytes() == 0);
        // 2. the first render. Before: kzFilmEnsureTapSums - alloc + ONE hipMemsetAsync; renderOn's own clear is skipped for fresh sums ("zeroed once, not twice").
        CHECK(r.render(false, s1) == KZ_OK && logged({{'A', SUMS, 0}, {'z', SUMS, S1}}));
        CHECK(r.films[0].bytes() == FILM_BYTES && r.aovBytes() == 0);
        // 3. a render that does not accumulate. Before: renderOn - `if (!opts->accumulate && !fresh) hipMemsetAsync(tapSums)`: sums, not texels.
        CHECK(r.render(false, s2) == KZ_OK && logged({{'z', SUMS, S2}}));
        // 4. an accumulating render: nothing.
        CHECK(r.render(true, s1) == KZ_OK && logged({}));
        CHECK(r.bytes() == FILM_BYTES);
        // 5. mask 3, then a render. Before: kz_scene_set_aovs frees what LEAVES the mask (nothing); kzAovEnsure per enabled AOV in ascending order - aovTapSums[f].alloc,
        //    aovFilm[f].alloc + its memset, then the sums' memset (`fresh || !accumulate`) - behind the picture's clear.
        r.setAovs(3);
        CHECK(logged({}) && r.aovBytes() == 0);                       // allocated on first use
        CHECK(r.render(false, s3) == KZ_OK && logged({{'z', SUMS, S3},
                                                      {'A', SUMS, 0}, {'A', TEXELS, 0}, {'z', TEXELS, S3}, {'z', SUMS, S3},
                                                      {'A', SUMS, 0}, {'A', TEXELS, 0}, {'z', TEXELS, S3}, {'z', SUMS, S3}}));
        CHECK(r.aovBytes() == 2 * FILM_BYTES && !r.films[3].sums && !r.films[3].texels);
        // 6. mask 7, then an accumulating render. Before: kzAovEnsure - the AOVs that were there are left alone, the one that entered is made (fresh sums are zeroed
        //    although the call accumulates).
        r.setAovs(7);
        CHECK(logged({}));
        CHECK(r.render(true, s1) == KZ_OK && logged({{'A', SUMS, 0}, {'A', TEXELS, 0}, {'z', TEXELS, S1}, {'z', SUMS, S1}}));
        CHECK(r.aovBytes() == 3 * (TAPS * TAPS * W * H * 16 + (H + 2 * BORDER) * (W + 2 * BORDER) * 16));      // tests/test_aov_gpu.py test_picture_untouched_and_memory
        CHECK(r.films[0].bytes() == FILM_BYTES);
        // 7. clear. Before: kzFilmClear - the picture's sums, the picture's texels, then per AOV its sums and its texels.
        CHECK(r.clear(s2) == KZ_OK && logged({{'z', SUMS, S2}, {'z', TEXELS, S2}, {'z', SUMS, S2}, {'z', TEXELS, S2}, {'z', SUMS, S2}, {'z', TEXELS, S2}, {'z', SUMS, S2}, {'z', TEXELS, S2}}));
        // 8. mask 2. Before: kzAovFree(mask & ~new) - per AOV that leaves, in ascending order, aovTapSums[f].free() then aovFilm[f].free().
        r.setAovs(2);
        CHECK(logged({{'F', SUMS, 0}, {'F', TEXELS, 0}, {'F', SUMS, 0}, {'F', TEXELS, 0}}));
        CHECK(r.aovBytes() == TAPS * TAPS * W * H * 16 + (H + 2 * BORDER) * (W + 2 * BORDER) * 16);             // the same test, after set_aovs(["normal"])
        CHECK(!r.films[1].sums && !r.films[1].texels && r.films[2].sums && r.films[2].texels && !r.films[3].sums && !r.films[3].texels);
        // (a clear passes over what is not there)
        CHECK(r.clear(s1) == KZ_OK && logged({{'z', SUMS, S1}, {'z', TEXELS, S1}, {'z', SUMS, S1}, {'z', TEXELS, S1}}));
        // 9. release: the replica goes, its owners' destructors free what is left (members in reverse order: films 3 .. 0, each its texels, then its sums)
    }
    CHECK(logged({{'F', TEXELS, 0}, {'F', SUMS, 0}, {'F', TEXELS, 0}, {'F', SUMS, 0}}) && g_live.empty());

    // ---- free() by hand, twice; bytes() of an empty film ----
    {
        KzFilm f;
        CHECK(f.bytes() == 0 && f.clear(s1) == KZ_OK && logged({}));
        CHECK(f.ensure(SUMS, TEXELS, true, s1) == KZ_OK && f.bytes() == FILM_BYTES);
        f.free(); f.free();
        CHECK(f.bytes() == 0 && !f.sums && !f.texels && g_live.empty());
        g_log.clear();
    }
    // ---- a failed allocation, at each position: the film is empty or as it was, never half-made, and usable afterwards ----
    {
        KzFilm f;                                                     // a feature film: neither sums nor texels
        g_failDev = 1;
        CHECK(f.ensure(SUMS, TEXELS, false, s1) == KZ_ERR_OOM && g_failCode == KZ_ERR_OOM && !f.sums && !f.texels && g_live.empty() && logged({}));
        g_failDev = 2;                                                // the texels: the sums made a moment ago, which nothing has zeroed, go again
        CHECK(f.ensure(SUMS, TEXELS, true, s1) == KZ_ERR_OOM && !f.sums && !f.texels && f.bytes() == 0 && g_live.empty() && logged({{'A', SUMS, 0}, {'F', SUMS, 0}}));
        CHECK(f.ensure(SUMS, TEXELS, true, s2) == KZ_OK && logged({{'A', SUMS, 0}, {'A', TEXELS, 0}, {'z', TEXELS, S2}, {'z', SUMS, S2}}));
        KzFilm p;                                                     // the picture after the upload: texels, no sums
        CHECK(p.texels.alloc(TEXELS) == KZ_OK);
        float4 *const had = p.texels;
        g_log.clear();
        g_failDev = 1;
        CHECK(p.ensure(SUMS, TEXELS, false, s1) == KZ_ERR_OOM && !p.sums && p.texels.get() == had && p.texels.cap() == TEXELS && g_live.size() == 3 && logged({}));
        CHECK(p.ensure(SUMS, TEXELS, false, s1) == KZ_OK && p.texels.get() == had && logged({{'A', SUMS, 0}, {'z', SUMS, S1}}));
    }
    CHECK(g_live.empty());
    // ... and at each of the seven allocations of a replica's first render with all three AOVs enabled: every film is whole (sums and texels) or as the upload left it
    for (int nth = 1; nth <= 8; ++nth) {
        Replica r;
        CHECK(r.upload() == KZ_OK);
        r.setAovs(7);
        g_failDev = nth;
        const int rc = r.render(false, s1);
        CHECK(rc == (nth <= 7 ? KZ_ERR_OOM : KZ_OK));
        g_failDev = 0;
        const int whole = nth / 2;                                    // films made before the failure: allocation 1 is the picture's sums, 2k and 2k + 1 are AOV k - 1's
        CHECK(r.films[0].texels && (r.films[0].sums ? whole >= 1 : whole == 0));
        for (int k = 1; k < 4; ++k) CHECK(k < whole ? (r.films[k].sums && r.films[k].texels) : (!r.films[k].sums && !r.films[k].texels));
        CHECK(g_live.size() == (size_t)(whole == 0 ? 1 : 2 * whole) && r.bytes() == (whole == 0 ? TEXELS * 16 : whole * FILM_BYTES));
        g_log.clear();
        CHECK(r.render(true, s2) == KZ_OK && r.bytes() == 4 * FILM_BYTES && g_live.size() == 8);      // the next call makes the rest
    }
    g_log.clear();
    CHECK(g_live.empty());
    std::printf("ok\n");
    return 0;
}
