// devmem.h — the owners of device and pinned host memory (host only).  DevBuf<T> holds hipMalloc memory, PinnedBuf<T>
// hipHostMalloc memory: a pointer and a capacity in items, freed by the destructor, moved but never copied.  reserve()
// is the one growth routine: how much to ask for (floors, geometric steps, rounding) is the caller's arithmetic on
// `need`.  Kernel-argument structs and launchers take the raw pointer (get()): they are views, never owners.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <utility>

struct r360_ctx;
int ctx_wait(r360_ctx* ctx);
void r360_set_error(const char* fmt, ...);

namespace devmem {
// waits until no enqueued work can still read a buffer about to be freed: the context's stream, else `sync`, else nothing
inline int quiesce(r360_ctx* ctx, hipStream_t sync) {
    if (ctx) return ctx_wait(ctx);
    return sync && hipStreamSynchronize(sync) != hipSuccess ? -1 : 0;
}
inline int fail(const char* what, size_t bytes, hipError_t e) {
    r360_set_error("%s:%d %s(%zu bytes) -> %s", __FILE__, __LINE__, what, bytes, hipGetErrorString(e));
    return -1;
}
}  // namespace devmem

template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for `need` items; contents are not kept.  0 at once when it fits.  Otherwise waits (the context's stream, or
    // `sync` when ctx is null) if the buffer is live, frees and allocates exactly `need` items: 0, or -1 with the
    // thread's error set and the buffer empty when the wait or the allocation failed.
    int reserve(r360_ctx* ctx, size_t need, hipStream_t sync = nullptr) {
        if (need <= cap_) return 0;
        if (p_ && devmem::quiesce(ctx, sync)) return -1;
        reset();
        const hipError_t e = hipMalloc((void**)&p_, sizeof(T) * need);
        if (e != hipSuccess) { p_ = nullptr; return devmem::fail("hipMalloc", sizeof(T) * need, e); }
        cap_ = need;
        return 0;
    }
    // the same, all cap() items zeroed on `st` when, and only when, the buffer was newly allocated
    int reserve_zeroed(r360_ctx* ctx, size_t need, hipStream_t st) {
        if (need <= cap_) return 0;
        if (reserve(ctx, need, st)) return -1;
        const hipError_t e = hipMemsetAsync(p_, 0, sizeof(T) * cap_, st);
        if (e != hipSuccess) { reset(); return devmem::fail("hipMemsetAsync", sizeof(T) * need, e); }
        return 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    int reserve(r360_ctx* ctx, size_t need, hipStream_t sync = nullptr) {   // as DevBuf::reserve
        if (need <= cap_) return 0;
        if (p_ && devmem::quiesce(ctx, sync)) return -1;
        reset();
        const hipError_t e = hipHostMalloc((void**)&p_, sizeof(T) * need, hipHostMallocDefault);
        if (e != hipSuccess) { p_ = nullptr; return devmem::fail("hipHostMalloc", sizeof(T) * need, e); }
        cap_ = need;
        return 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
