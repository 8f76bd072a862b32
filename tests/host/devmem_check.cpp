// devmem_check.cpp — DevBuf / PinnedBuf (rgbd360_amd/csrc/host/devmem.h) against a mock HIP runtime: malloc-backed
// allocations with a live set, a "fail the k-th allocation" switch and a log of the calls in order.  Built by
// tests/test_devmem_host.py with g++ and the address / undefined-behaviour sanitizers, no HIP runtime linked; exits
// non-zero, naming the broken rule, when an owner leaks, dangles, frees twice, allocates without need, frees a live
// buffer without waiting first, or zeroes at the wrong time.  It also builds the memory part of the sized-once handles
// (rgbd360_amd/csrc/host/handles.cpp: calibration, frame, plane buffers, sensor pyramid) and makes every allocator,
// event, copy and memset call of each creation fail in turn: the creation must fail clean and then succeed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "r360_internal.h"   // the kernel-argument structs
#include "host/devmem.h"

// ------------------------------------------------------------------ the mock runtime
static std::set<void*> g_live;
static std::vector<std::string> g_log;
static int g_allocs = 0, g_fail_at = 0, g_errors = 0, g_wait_rc = 0;
static size_t g_last_bytes = 0, g_memset_bytes = 0;
static hipStream_t g_memset_stream = nullptr;
// every call that can fail (allocator, event creation, copy, memset) counts here, and call number g_fail_call fails
static int g_calls = 0, g_fail_call = 0;
static std::set<hipEvent_t> g_events;
static std::vector<size_t> g_sizes;   // the allocations' bytes, in order
static bool fail_here() { return ++g_calls == g_fail_call; }

static hipError_t mock_alloc(const char* what, void** p, size_t n) {
    g_log.push_back(what);
    g_last_bytes = n;
    g_sizes.push_back(n);
    const bool fail_call = fail_here();
    if (++g_allocs == g_fail_at || fail_call) {
        *p = (void*)0x1;   // a failed call leaves no usable pointer behind
        return hipErrorOutOfMemory;
    }
    *p = malloc(n ? n : 1);
    g_live.insert(*p);
    return hipSuccess;
}
static hipError_t mock_free(const char* what, void* p) {
    g_log.push_back(what);
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) {
        fprintf(stderr, "FAIL: %s of a pointer that is not live (double free or dangling)\n", what);
        exit(1);
    }
    free(p);
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) { return mock_alloc("malloc", p, n); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned flags) {
    if (flags != hipHostMallocDefault) { fprintf(stderr, "FAIL: hipHostMalloc flags %u\n", flags); exit(1); }
    return mock_alloc("hostmalloc", p, n);
}
hipError_t hipFree(void* p) { return mock_free("free", p); }
hipError_t hipHostFree(void* p) { return mock_free("hostfree", p); }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t st) {
    g_log.push_back("memset");
    if (fail_here()) return hipErrorInvalidValue;
    if (!g_live.count(p) || v != 0) { fprintf(stderr, "FAIL: memset of a buffer that is not live, or not to zero\n"); exit(1); }
    g_memset_bytes = n;
    g_memset_stream = st;
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    g_log.push_back("memcpy");
    if (fail_here()) return hipErrorInvalidValue;
    if (kind != hipMemcpyHostToDevice || !g_live.count(dst)) {
        fprintf(stderr, "FAIL: memcpy that is not an upload to the start of a live buffer\n");
        exit(1);
    }
    if (n) memcpy(dst, src, n);   // the address sanitizer sees a copy past either end
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    g_log.push_back("event");
    if (fail_here()) return hipErrorOutOfMemory;   // *e is left as it was
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    g_log.push_back("eventdestroy");
    if (!g_events.erase(e)) { fprintf(stderr, "FAIL: hipEventDestroy of an event that is not live\n"); exit(1); }
    free(e);
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_log.push_back("streamsync"); return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "mock error"; }

int ctx_wait(r360_ctx*) { g_log.push_back("wait"); return g_wait_rc; }
void r360_set_error(const char*, ...) { ++g_errors; }

// ------------------------------------------------------------------ the checks
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static std::string log_str() {
    std::string s;
    for (const std::string& e : g_log) s += (s.empty() ? "" : " ") + e;
    return s;
}
static void fresh() {
    g_log.clear(); g_sizes.clear();
    g_allocs = 0; g_fail_at = 0; g_errors = 0; g_wait_rc = 0; g_calls = 0; g_fail_call = 0;
}

static_assert(sizeof(DevBuf<int>) == sizeof(int*) + sizeof(size_t), "an owner is a pointer and a capacity");
static_assert(sizeof(PinnedBuf<int>) == sizeof(int*) + sizeof(size_t), "an owner is a pointer and a capacity");
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "move only");
static_assert(!std::is_copy_constructible<PinnedBuf<int>>::value && !std::is_copy_assignable<PinnedBuf<int>>::value, "move only");
// kernel-argument structs are views: they travel to the kernels by value
static_assert(std::is_trivially_copyable<PgoDev>::value, "PgoDev");
static_assert(std::is_trivially_copyable<RigcalDev>::value, "RigcalDev");
static_assert(std::is_trivially_copyable<TopoArgs>::value, "TopoArgs");
static_assert(std::is_trivially_copyable<PlaneDev>::value, "PlaneDev");
static_assert(std::is_trivially_copyable<LevelBufs>::value, "LevelBufs");
static_assert(std::is_trivially_copyable<LevelTrig>::value, "LevelTrig");
static_assert(std::is_trivially_copyable<SrcLevel>::value, "SrcLevel");

template <class Buf>
static void basic(const char* alloc, const char* release) {
    r360_ctx ctx{};
    const std::string A = alloc, F = release;
    {
        fresh();
        Buf b;
        CHECK(!b && b.get() == nullptr && b.cap() == 0);
        CHECK(b.reserve(&ctx, 0) == 0 && g_log.empty());                 // nothing asked for, nothing done
        CHECK(b.reserve(&ctx, 100) == 0 && b && b.cap() == 100);
        CHECK(log_str() == A);                                            // an empty buffer is not waited for
        CHECK(g_last_bytes == 100 * sizeof(double));
        b.get()[99] = 1.0;                                                // the whole capacity is there
        CHECK(b.reserve(&ctx, 100) == 0 && b.reserve(&ctx, 7) == 0 && log_str() == A);   // no-ops: no allocator call
        CHECK(b.reserve(&ctx, 101) == 0 && b.cap() == 101);
        CHECK(log_str() == A + " wait " + F + " " + A);                   // live: wait, then free, then allocate
        b.reset();
        CHECK(!b && b.cap() == 0 && g_live.empty());
        b.reset();                                                        // twice is fine
        CHECK(b.reserve(&ctx, 5) == 0);
    }
    CHECK(g_live.empty());                                                // the destructor freed
    {   // no context: the given stream is synchronised instead, or nothing at all
        fresh();
        Buf b;
        hipStream_t st = (hipStream_t)0x40;
        CHECK(b.reserve(nullptr, 10, st) == 0 && log_str() == A);
        CHECK(b.reserve(nullptr, 20, st) == 0 && log_str() == A + " streamsync " + F + " " + A);
        g_log.clear();
        CHECK(b.reserve(nullptr, 30) == 0 && log_str() == F + " " + A);
    }
    CHECK(g_live.empty());
    {   // a failed allocation: -1, the error set, the buffer empty; the next call starts over
        fresh();
        Buf b;
        CHECK(b.reserve(&ctx, 10) == 0);
        g_fail_at = g_allocs + 1;
        CHECK(b.reserve(&ctx, 20) == -1 && g_errors == 1);
        CHECK(!b && b.get() == nullptr && b.cap() == 0 && g_live.empty());
        g_log.clear();
        CHECK(b.reserve(&ctx, 20) == 0 && b.cap() == 20 && log_str() == A);
    }
    CHECK(g_live.empty());
    {   // a failed wait frees nothing: the buffer stays as it was
        fresh();
        Buf b;
        CHECK(b.reserve(&ctx, 10) == 0);
        g_wait_rc = -1;
        CHECK(b.reserve(&ctx, 20) == -1 && b && b.cap() == 10 && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // a moved-from owner frees nothing; the target frees what it held before
        fresh();
        Buf a, c;
        CHECK(a.reserve(&ctx, 10) == 0 && c.reserve(&ctx, 20) == 0);
        double* pa = a.get();
        Buf m(std::move(a));
        CHECK(!a && a.cap() == 0 && m.get() == pa && m.cap() == 10 && g_live.size() == 2);
        c = std::move(m);
        CHECK(!m && m.cap() == 0 && c.get() == pa && c.cap() == 10 && g_live.size() == 1);
        c = std::move(c);                                                 // self-assignment keeps the buffer
        CHECK(c.get() == pa && g_live.size() == 1);
    }
    CHECK(g_live.empty());
}

static void zeroed() {
    r360_ctx ctx{};
    hipStream_t st = (hipStream_t)0x80;
    fresh();
    {
        DevBuf<int> b;
        CHECK(b.reserve_zeroed(&ctx, 64, st) == 0 && log_str() == "malloc memset");
        CHECK(g_memset_bytes == 64 * sizeof(int) && g_memset_stream == st);
        CHECK(b.reserve_zeroed(&ctx, 64, st) == 0 && b.reserve_zeroed(&ctx, 3, st) == 0 && log_str() == "malloc memset");
        CHECK(b.reserve_zeroed(&ctx, 65, st) == 0 && log_str() == "malloc memset wait free malloc memset");
        CHECK(g_memset_bytes == 65 * sizeof(int));
        g_log.clear();
        CHECK(b.reserve(&ctx, 66) == 0 && log_str() == "wait free malloc");   // plain growth never zeroes
        g_fail_at = g_allocs + 1;
        g_log.clear();
        CHECK(b.reserve_zeroed(&ctx, 100, st) == -1 && !b && b.cap() == 0 && log_str() == "wait free malloc");
    }
    CHECK(g_live.empty());
}

// what a context or a handle does: three buffers reserved in a row, the call abandoned at the first failure
struct Three {
    DevBuf<float> a;
    DevBuf<int> b;
    PinnedBuf<double> c;
    int reserve(r360_ctx* ctx, size_t n) {
        if (a.reserve(ctx, n) || b.reserve_zeroed(ctx, 2 * n, nullptr) || c.reserve(ctx, n + 1)) return -1;
        return 0;
    }
};

static void sequence() {
    r360_ctx ctx{};
    for (int grown = 0; grown < 2; ++grown)       // the failure hits empty buffers, or live ones being regrown
        for (int k = 1; k <= 3; ++k) {
            fresh();
            {
                Three t;
                if (grown) CHECK(t.reserve(&ctx, 8) == 0 && g_live.size() == 3);
                g_fail_at = g_allocs + k;
                CHECK(t.reserve(&ctx, 16) == -1 && g_errors == 1);
                // the member that failed is empty, the ones before it have the new size, the ones after it their old one
                // (the call stopped there: those it did not reach are empty when there was no earlier round)
                CHECK(!t.a == (k == 1) && !t.b == (k == 2 || (!grown && k < 2)) && !t.c == (k == 3 || (!grown && k < 3)));
                CHECK(t.a.cap() == (k == 1 ? 0u : 16u));
                CHECK(t.b.cap() == (k == 2 ? 0u : k > 2 ? 32u : grown ? 16u : 0u));
                CHECK(t.c.cap() == (k == 3 ? 0u : grown ? 9u : 0u));
                g_fail_at = 0;
                CHECK(t.reserve(&ctx, 16) == 0 && t.a.cap() == 16 && t.b.cap() == 32 && t.c.cap() == 17);   // and recovers
                CHECK(g_live.size() == 3);
            }
            CHECK(g_live.empty());
        }
}

// ------------------------------------------------------------------ the sized-once handles (host/handles.cpp)
// Runs `make` once to count the calls that can fail, N, then N times with call k failing: it must return non-zero with
// the error set and leave the live buffers and events as it found them; the same call then succeeds, and `drop`
// releases it cleanly (a free of anything not live ends the program in the mock).  Returns N.
template <class Make, class Drop>
static int fail_each(Make make, Drop drop) {
    const size_t live0 = g_live.size(), ev0 = g_events.size();
    fresh();
    CHECK(make() == 0);
    const int N = g_calls;
    CHECK(N > 0);
    drop();
    CHECK(g_live.size() == live0 && g_events.size() == ev0);
    for (int k = 1; k <= N; ++k) {
        fresh();
        g_fail_call = k;
        CHECK(make() != 0 && g_errors >= 1);
        CHECK(g_live.size() == live0 && g_events.size() == ev0);
        g_fail_call = 0;
        CHECK(make() == 0);
        drop();
        CHECK(g_live.size() == live0 && g_events.size() == ev0);
    }
    return N;
}

// a calibration (sensors of rows x cols, or sphere-only with rows = 0), a frame on it, the frame's plane buffers and
// its sensor pyramid; n_*: the fallible calls each creation is known to make at these sizes
static void handles(int rows, int cols, int sph_rows, int sph_cols, int n_calib, int n_frame) {
    r360_ctx ctx{};
    r360_calib* const no_calib = (r360_calib*)0x10;
    r360_frame* const no_frame = (r360_frame*)0x20;
    r360_calib* cal = nullptr;
    r360_frame* f = nullptr;
    const int nc = fail_each(
        [&] {
            r360_calib* c = no_calib;
            const int rc = calib_new(&ctx, rows, cols, sph_rows, sph_cols, &c);
            if (rc) CHECK(c == no_calib); else cal = c;   // *out untouched on failure
            return rc;
        },
        [&] { delete cal; cal = nullptr; });
    CHECK(nc == n_calib);
    CHECK(calib_new(&ctx, rows, cols, sph_rows, sph_cols, &cal) == 0);
    CHECK(cal->n_levels == 1 && cal->trig[0].sinphi && cal->trig[0].costh && !cal->trig[1].sinphi);
    CHECK(!cal->d_rt == !rows && !cal->d_rt_inv == !rows && !cal->d_st_costh == !rows);
    const int sr = cal->sph_rows, sc = cal->sph_cols;
    CHECK(sr == (rows ? 5 : sph_rows) && sc == (rows ? 32 : sph_cols));

    const int nf = fail_each(
        [&] {
            r360_frame* g = no_frame;
            const int rc = frame_new(&ctx, cal, &g);
            if (rc) CHECK(g == no_frame); else f = g;
            return rc;
        },
        [&] { delete f; f = nullptr; });
    CHECK(nf == n_frame);
    fresh();
    CHECK(frame_new(&ctx, cal, &f) == 0);
    {   // the allocations of a frame, in order: sensor images, sphere images, the one level, counters and the level table
        const size_t ns = (size_t)8 * rows * cols, nsph = (size_t)sr * sc;
        std::vector<size_t> want;
        if (ns) want = {ns * 3, ns * 2, ns * 4};
        for (size_t b : {nsph * 3, nsph * 2, nsph * sizeof(float2), nsph * sizeof(float4), nsph * sizeof(float4), nsph * 4,
                         sizeof(int) * R360_MAX_PYR, sizeof(int) * R360_MAX_PYR * 1, sizeof(SrcLevel) * R360_MAX_PYR})
            want.push_back(b);
        CHECK(g_sizes == want);
        CHECK(f->lv[0].p0 && f->lv[0].pk && !f->lv[1].p0 && f->d_npts && f->bgr_ev && !f->d_bgr == !rows);
    }
    if (rows) {
        const int np = fail_each(
            [&] {
                const int rc = f->pl.alloc(f->rows, f->cols);
                // a failure leaves no partial set behind for the next call to take for complete
                if (rc) CHECK(!f->pl.v.cloud && !f->pl.v.h_nmodels && !f->pl.done && !f->pl.ready && f->pl.mem.dev.empty());
                else CHECK(f->pl.v.cloud && f->pl.v.h_nmodels && f->pl.done && f->pl.ready && f->pl.alloc(f->rows, f->cols) == 0);
                return rc;
            },
            [&] { f->pl.release(); });
        CHECK(np == 41);   // 35 device buffers, 4 pinned ones, 2 events
        CHECK(f->pl.alloc(f->rows, f->cols) == 0);
        CHECK(f->pl.w == cols / 2 && f->pl.h == rows / 2 && f->pl.v.contour_cap == 2L * 8 * f->pl.w * f->pl.h);
        { const PlaneDev view = f->pl.v; (void)view; }   // a view: copied, and the copy frees nothing
        f->pl.release();
        // one lazily allocated sensor-pyramid level (4 x 8 is below the halving limit): each drop starts a new frame
        const int nsp = fail_each(
            [&] {
                const int rc = f->alloc_sensor_pyramid();
                if (rc) CHECK(f->n_slevels == 0 && !f->sp[0].p0 && !f->sp[0].tg && f->sp_mem.dev.empty());
                else CHECK(f->n_slevels == 1 && f->sp[0].p0 && f->sp[0].tg && !f->sp[1].p0 && f->alloc_sensor_pyramid() == 0);
                return rc;
            },
            [&] {
                delete f;
                f = nullptr;
                CHECK(frame_new(&ctx, cal, &f) == 0);
            });
        CHECK(nsp == 2);
        CHECK(f->alloc_sensor_pyramid() == 0 && f->pl.alloc(f->rows, f->cols) == 0);
        // the CLAMS tables are replaced release first: free, then malloc, then the blocking copy
        std::vector<float> mult(24, 1.f), counts(24, 2.f);
        CHECK(cal->upload_clams(mult, counts) == 0);
        fresh();
        CHECK(cal->upload_clams(mult, counts) == 0 && log_str() == "free malloc memcpy free malloc memcpy");
        fresh();
        g_fail_call = 3;   // the second table's allocation fails: no dangling view
        CHECK(cal->upload_clams(mult, counts) == -1 && cal->clams.d_mult && !cal->clams.d_counts);
    }
    delete f;      // frame with everything: plane buffers, sensor pyramid, event
    delete cal;
    CHECK(g_live.empty() && g_events.empty());
}

int main() {
    handles(4, 8, 0, 0, 20, 15);    // sensors of 4 x 8: a sphere of 5 x 32, one level
    handles(0, 0, 2, 8, 8, 12);     // sphere-only, 2 x 8
    basic<DevBuf<double>>("malloc", "free");
    basic<PinnedBuf<double>>("hostmalloc", "hostfree");
    zeroed();
    sequence();
    CHECK(g_live.empty());
    printf("devmem ok\n");
    return 0;
}
