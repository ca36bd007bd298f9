// No GPU: the four owners of nano-kazen_amd/csrc/kz_own.h (DevBuf, PinnedBuf, Event, Stream) against stand-ins for the handful of HIP functions they call.
// The stand-ins count what is live, remember the byte counts of the copies and can fail the nth allocation; built with -fsanitize=address,undefined, so a
// buffer freed twice or never is reported by the sanitizer as well. tests/test_own_cpu.py builds and runs it.
#include "kz_own.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

static int g_dev = 0, g_pinned = 0, g_events = 0, g_streams = 0;      // live objects
static int g_devMax = 0, g_devAllocs = 0, g_devFrees = 0, g_eventsMade = 0, g_streamsMade = 0;
static int g_failDev = 0, g_failPinned = 0;                          // > 0: the nth allocation from now on fails
static hipError_t g_failWith = hipErrorOutOfMemory;
static std::vector<size_t> g_copyBytes; static std::vector<hipMemcpyKind> g_copyKind;
static unsigned g_lastFlags = 0; static int g_lastPriority = 0;
static int g_failCode = 0; static char g_failMsg[256];

int kz_fail(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); std::vsnprintf(g_failMsg, sizeof g_failMsg, fmt, ap); va_end(ap);
    g_failCode = code;
    return code;
}
hipError_t kzMalloc(void **p, size_t bytes) {
    *p = nullptr;
    if (g_failDev > 0 && --g_failDev == 0) return g_failWith;
    *p = std::malloc(bytes ? bytes : 1);
    ++g_devAllocs; ++g_dev; if (g_dev > g_devMax) g_devMax = g_dev;
    return hipSuccess;
}
extern "C" {
hipError_t hipFree(void *p) { if (p) { std::free(p); --g_dev; ++g_devFrees; } return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) {
    *p = nullptr;
    if (g_failPinned > 0 && --g_failPinned == 0) return g_failWith;
    *p = std::malloc(bytes ? bytes : 1); ++g_pinned;
    return hipSuccess;
}
hipError_t hipHostFree(void *p) { if (p) { std::free(p); --g_pinned; } return hipSuccess; }
hipError_t hipMemcpy(void *, const void *, size_t bytes, hipMemcpyKind kind) { g_copyBytes.push_back(bytes); g_copyKind.push_back(kind); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { *e = (hipEvent_t)std::malloc(1); ++g_events; ++g_eventsMade; g_lastFlags = flags; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { std::free(e); --g_events; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { *s = (hipStream_t)std::malloc(1); ++g_streams; ++g_streamsMade; g_lastFlags = flags; g_lastPriority = 0; return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority) { *s = (hipStream_t)std::malloc(1); ++g_streams; ++g_streamsMade; g_lastFlags = flags; g_lastPriority = priority; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { std::free(s); --g_streams; return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "own_test.cpp:%d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static bool nothingLive() { return g_dev == 0 && g_pinned == 0 && g_events == 0 && g_streams == 0; }

// shaped like PassCtx (kz_state.h): buffers, a side stream with its events, two nested views, a growing list of stage events
struct Ctx {
    DevBuf<uint32_t> counts, ovf;
    Stream side; Event evFork, evJoin;
    std::unique_ptr<Ctx> view[2]; Stream halfStream; Event evHalfFork, evHalfJoin;
    std::vector<Event> stageEv;
    int fill(bool views) {
        int rc;
        if ((rc = counts.alloc(4160)) || (rc = ovf.regrow(3 * 1024)) || (rc = side.ensure(hipStreamNonBlocking)) || (rc = evFork.ensure(hipEventDisableTiming)) || (rc = evJoin.ensure(hipEventDisableTiming))) return rc;
        for (int i = 0; i < 5; ++i) { Event e; if ((rc = e.ensure())) return rc; stageEv.push_back(std::move(e)); }      // (the vector reallocates: events move)
        if (!views) return KZ_OK;
        if ((rc = halfStream.ensure(hipStreamNonBlocking)) || (rc = evHalfFork.ensure(hipEventDisableTiming)) || (rc = evHalfJoin.ensure(hipEventDisableTiming))) return rc;
        for (auto &v : view) { v.reset(new Ctx()); if ((rc = v->fill(false))) return rc; }
        return KZ_OK;
    }
};

int main() {
    struct Rec { float a[14]; };                                  // 56 bytes: no power of two
    // ---- scope exit, sizes, copies ----
    {
        DevBuf<Rec> b; PinnedBuf<float> h; Event e; Stream s;
        CHECK(!b && !b.get() && b.cap() == 0 && b.bytes() == 0 && !h && h.cap() == 0 && !e.get() && !s.get());      // all four start empty
        CHECK(b.alloc(10) == KZ_OK && b && b.cap() == 10 && b.bytes() == 560 && g_dev == 1);
        CHECK(h.alloc(7) == KZ_OK && h && h.cap() == 7 && h.bytes() == 28 && g_pinned == 1);
        Rec host[10] = {};
        CHECK(b.upload(host, 10) == KZ_OK && b.download(host, 3, 2) == KZ_OK);
        CHECK(g_copyBytes.size() == 2 && g_copyBytes[0] == 10 * sizeof(Rec) && g_copyKind[0] == hipMemcpyHostToDevice && g_copyBytes[1] == 3 * sizeof(Rec) && g_copyKind[1] == hipMemcpyDeviceToHost);
        CHECK(e.ensure(hipEventDisableTiming) == KZ_OK && e.get() && g_lastFlags == hipEventDisableTiming && g_events == 1);
        CHECK(s.ensure(hipStreamNonBlocking, -1) == KZ_OK && s.get() && g_lastFlags == hipStreamNonBlocking && g_lastPriority == -1 && g_streams == 1);
    }
    CHECK(nothingLive());
    // ---- ensure() creates once; reset() makes it again; reset() / free() twice are harmless ----
    {
        Event e; Stream s, s2;
        const int e0 = g_eventsMade, s0 = g_streamsMade;
        CHECK(e.ensure() == KZ_OK && g_lastFlags == hipEventDefault);
        const hipEvent_t he = e; const hipEvent_t again = (e.ensure(), e.ensure(hipEventDisableTiming), e.get());
        CHECK(he == again && g_eventsMade == e0 + 1);
        CHECK(s.ensure(hipStreamNonBlocking) == KZ_OK && s.ensure(hipStreamNonBlocking) == KZ_OK && s.ensure(hipStreamNonBlocking, 2) == KZ_OK && g_streamsMade == s0 + 1 && g_lastPriority == 0);
        s.reset(); s.reset(); CHECK(!s.get() && g_streams == 0);
        CHECK(s.ensure(hipStreamNonBlocking, 2) == KZ_OK && g_streamsMade == s0 + 2 && g_lastPriority == 2);      // "make them again" (passStreams)
        e.reset(); e.reset(); CHECK(!e.get() && g_events == 0);
        s2.reset();                                               // (of an empty one)
        DevBuf<int> b; PinnedBuf<int> h;
        b.free(); h.free();
        CHECK(b.alloc(3) == KZ_OK && h.alloc(3) == KZ_OK);
        const int f0 = g_devFrees;
        b.free(); b.free(); h.free(); h.free();
        CHECK(g_devFrees == f0 + 1 && !b && b.cap() == 0 && !h && h.cap() == 0 && g_dev == 0 && g_pinned == 0);
    }
    CHECK(nothingLive());
    // ---- a moved-from owner is empty and frees nothing ----
    {
        DevBuf<float> a; CHECK(a.alloc(8) == KZ_OK);
        float *p = a;
        const int f0 = g_devFrees;
        DevBuf<float> b(std::move(a));
        CHECK(!a && a.cap() == 0 && b.get() == p && b.cap() == 8 && g_dev == 1);
        { DevBuf<float> gone(std::move(a)); }                     // (an empty one goes)
        CHECK(g_devFrees == f0 && g_dev == 1);
        DevBuf<float> c; CHECK(c.alloc(2) == KZ_OK);
        c = std::move(b);                                         // what c held is freed, b is empty
        CHECK(g_devFrees == f0 + 1 && g_dev == 1 && c.get() == p && c.cap() == 8 && !b && b.cap() == 0);
        PinnedBuf<float> h1; CHECK(h1.alloc(4) == KZ_OK);
        PinnedBuf<float> h2(std::move(h1)); CHECK(!h1 && h1.cap() == 0 && h2.cap() == 4 && g_pinned == 1);
        Event e1; CHECK(e1.ensure() == KZ_OK); Event e2(std::move(e1)); CHECK(!e1.get() && e2.get() && g_events == 1);
        Event e3; CHECK(e3.ensure() == KZ_OK); e3 = std::move(e2); CHECK(!e2.get() && g_events == 1);
        Stream s1; CHECK(s1.ensure(0) == KZ_OK); Stream s2(std::move(s1)); CHECK(!s1.get() && s2.get() && g_streams == 1);
        std::vector<DevBuf<float>> v(3);                          // (KzDeviceState::editBase)
        CHECK(v[1].alloc(5) == KZ_OK); v.resize(40); CHECK(v[1].cap() == 5 && g_dev == 2);
    }
    CHECK(nothingLive());
    // ---- regrow never has two buffers live, and keeps nothing ----
    {
        DevBuf<float> b; PinnedBuf<float> h;
        CHECK(b.regrow(16) == KZ_OK && h.regrow(16) == KZ_OK);    // (of an empty one: an alloc)
        g_devMax = g_dev;
        const int a0 = g_devAllocs, f0 = g_devFrees;
        CHECK(b.regrow(1024) == KZ_OK && b.cap() == 1024 && h.regrow(64) == KZ_OK && h.cap() == 64);
        CHECK(g_devMax == 1 && g_dev == 1 && g_pinned == 1 && g_devAllocs == a0 + 1 && g_devFrees == f0 + 1);
    }
    CHECK(nothingLive());
    // ---- a failed alloc / regrow leaves the owner empty, with KZ_ALLOC's codes ----
    {
        DevBuf<Rec> b;
        g_failDev = 1; g_failWith = hipErrorOutOfMemory;
        CHECK(b.alloc(100) == KZ_ERR_OOM && g_failCode == KZ_ERR_OOM && !b && b.cap() == 0 && b.bytes() == 0 && g_dev == 0);
        CHECK(std::string(g_failMsg) == "device allocation of 5600 bytes failed: out of memory");
        CHECK(b.alloc(4) == KZ_OK);
        g_failDev = 1; g_failWith = hipErrorInvalidValue;
        CHECK(b.regrow(9) == KZ_ERR_HIP && !b && b.cap() == 0 && g_dev == 0);      // (what it held is gone: nothing is kept)
        g_failDev = 2; g_failWith = hipErrorOutOfMemory;          // the SECOND allocation from now on
        DevBuf<int> c, d;
        CHECK(c.alloc(1) == KZ_OK && d.alloc(1) == KZ_ERR_OOM && c && !d && g_dev == 1);
        PinnedBuf<int> h; CHECK(h.alloc(2) == KZ_OK);
        g_failPinned = 1;
        CHECK(h.regrow(50) == KZ_ERR_OOM && !h && h.cap() == 0 && g_pinned == 0);
        CHECK(h.alloc(50) == KZ_OK && h.cap() == 50);             // (usable again)
    }
    CHECK(nothingLive());
    // ---- an aggregate shaped like PassCtx, two nested views: everything is released exactly once ----
    {
        const int a0 = g_devAllocs, f0 = g_devFrees, e0 = g_eventsMade, s0 = g_streamsMade;
        {
            std::unique_ptr<Ctx> c(new Ctx());
            CHECK(c->fill(true) == KZ_OK);
            CHECK(g_dev == 6 && g_devAllocs == a0 + 6 && g_streams == 4 && g_events == 3 * 7 + 2);
            c->ovf.free(); c->view[0]->ovf.free();                // (trimAux: the context stays usable)
            CHECK(g_dev == 4 && c->ovf.regrow(64) == KZ_OK && g_dev == 5);
        }
        CHECK(nothingLive() && g_devFrees - f0 == g_devAllocs - a0 && g_eventsMade == e0 + 23 && g_streamsMade == s0 + 4);
        // ... and one whose making fails half way
        g_failDev = 4;
        { Ctx c; CHECK(c.fill(true) == KZ_ERR_OOM); }
        g_failDev = 0;
    }
    CHECK(nothingLive());
    std::printf("ok\n");
    return 0;
}
