// kz_own.h - the owners of the library's device resources: every device buffer, pinned host buffer, event and stream is a member or a local of one of
// the four move-only types below, and goes when its owner goes. The destructors neither set a device nor wait for it: whoever lets an owner go has made
// the device current and idle where that matters (releaseReplica, kzCtxPoolTrim, the regrow sites). The methods return the library's int status like
// everything else here. Host code only; of HIP it needs the runtime API's declarations and nothing else, so a plain C++ program can exercise it
// against stand-ins (tests/host_cpp/own_test.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include "../../include/kazen_mi355x.h"

int kz_fail(int code, const char *fmt, ...);          // kz_host.cpp
// Every device allocation of the library goes through here (kz_replica.hip: the pool's idle contexts are given back and the allocation tried once more
// when the card is full; kz_debug_fail_alloc can make the nth one fail).
hipError_t kzMalloc(void **p, size_t bytes);

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return kz_fail(KZ_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// A device buffer of cap() elements. Empty (null, cap 0) from the start, after free(), after a failed alloc / regrow and after it has been moved from.
template <class T> class DevBuf {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { free(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~DevBuf() { free(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
    void free() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    // n elements for a buffer that is empty
    int alloc(size_t n) {
        void *q = nullptr;
        const hipError_t e = kzMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) return kz_fail(e == hipErrorOutOfMemory ? KZ_ERR_OOM : KZ_ERR_HIP, "device allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
        p_ = (T *)q; cap_ = n;
        return KZ_OK;
    }
    // made again for n elements: what it held is freed FIRST and nothing is kept (the caller has synchronised whatever still reads it)
    int regrow(size_t n) { free(); return alloc(n); }
    // blocking copies of n elements from / to the host, `at` elements into the buffer
    int upload(const T *host, size_t n, size_t at = 0) { HIP_TRY(hipMemcpy(p_ + at, host, n * sizeof(T), hipMemcpyHostToDevice)); return KZ_OK; }
    int download(T *host, size_t n, size_t at = 0) const { HIP_TRY(hipMemcpy(host, p_ + at, n * sizeof(T), hipMemcpyDeviceToHost)); return KZ_OK; }
};

// The same for pinned host memory (the staging of tile descriptors and of packed tile rects).
template <class T> class PinnedBuf {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { free(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~PinnedBuf() { free(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
    void free() { if (p_) (void)hipHostFree(p_); p_ = nullptr; cap_ = 0; }
    int alloc(size_t n) {
        void *q = nullptr;
        const hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return kz_fail(e == hipErrorOutOfMemory ? KZ_ERR_OOM : KZ_ERR_HIP, "pinned host allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
        p_ = (T *)q; cap_ = n;
        return KZ_OK;
    }
    int regrow(size_t n) { free(); return alloc(n); }
};

// An event, created on first use: ensure() is a null check from then on.
class Event {
    hipEvent_t ev_ = nullptr;
public:
    Event() = default;
    Event(Event &&o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); ev_ = o.ev_; o.ev_ = nullptr; } return *this; }
    ~Event() { reset(); }
    hipEvent_t get() const { return ev_; }
    operator hipEvent_t() const { return ev_; }
    void reset() { if (ev_) (void)hipEventDestroy(ev_); ev_ = nullptr; }
    int ensure(unsigned flags = hipEventDefault) {            // hipEventDefault: an event that takes times
        if (ev_) return KZ_OK;
        HIP_TRY(hipEventCreateWithFlags(&ev_, flags));
        return KZ_OK;
    }
};

// A stream, created on first use with the flags (or the flags and the priority) its site asks for.
class Stream {
    hipStream_t st_ = nullptr;
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : st_(o.st_) { o.st_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); st_ = o.st_; o.st_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return st_; }
    operator hipStream_t() const { return st_; }
    void reset() { if (st_) (void)hipStreamDestroy(st_); st_ = nullptr; }
    int ensure(unsigned flags) {
        if (st_) return KZ_OK;
        HIP_TRY(hipStreamCreateWithFlags(&st_, flags));
        return KZ_OK;
    }
    int ensure(unsigned flags, int priority) {
        if (st_) return KZ_OK;
        HIP_TRY(hipStreamCreateWithPriority(&st_, flags, priority));
        return KZ_OK;
    }
};
