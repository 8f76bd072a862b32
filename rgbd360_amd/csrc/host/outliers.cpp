// outliers.cpp — pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval (restated from PCL 1.7, unpinned) for host
// clouds and for the context's global map where it lies.  Kernels: kernels/outlier_kernels.hip; semantics, the
// divergences from PCL and the index: DESIGN.md §5b-2.  Every device buffer is a DevBuf member of the r360_ctx's
// OutlierState, grown on demand and freed with the context.
#include <cmath>
#include <cstring>

#include "../r360_internal.h"

namespace {

enum Mode { FILTER, HOOK };

int check_params(const r360_ctx* ctx, const r360_outlier_params* p) {
    CHECK_ARG(ctx, "null ctx");
    CHECK_ARG(p, "null params");
    CHECK_ARG(p->kind == R360_OUTLIER_STATISTICAL || p->kind == R360_OUTLIER_RADIUS, "outliers: unknown kind");
    CHECK_ARG(p->mean_k >= 1 && p->mean_k <= R360_OUTLIER_KMAX, "outliers: mean_k must be 1..64");
    CHECK_ARG(std::isfinite(p->stddev_mul), "outliers: stddev_mul must be finite");
    CHECK_ARG(std::isfinite(p->max_dist) && p->max_dist > 0.f, "outliers: max_dist must be positive and finite");
    CHECK_ARG(std::isfinite(p->radius) && p->radius > 0.f, "outliers: radius must be positive and finite");
    CHECK_ARG(p->min_neighbors >= 0, "outliers: min_neighbors must not be negative");
    return 0;
}

// room for `need` items, growing geometrically so that a growing map does not reallocate per call
template <class B>
int grow(r360_ctx* ctx, B& b, size_t need) {
    if (need <= b.cap()) return 0;
    return b.reserve(ctx, std::max<size_t>(std::max<size_t>(need, 1024), b.cap() + b.cap() / 2));
}

float ord2f(unsigned e) {
    const unsigned u = (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int read_hdr(r360_ctx* ctx) {
    OutlierState& S = ctx->outl;
    R360_HIP(hipMemcpyAsync(S.h_hdr.get(), S.d_hdr.get(), sizeof(OutlierHdr), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

// The cell edge: limit / ring, a 2^-20 wider so that the rounding of x / ec never puts two points within the limit more
// than `ring` cells apart, doubled until every axis spans fewer than 2^21 - 2 cells (a coarser grid reads more
// candidates and finds the same ones).
void make_grid(const float mn[3], const float mx[3], double limit, int ring, OutlierGrid* G) {
    double ec = limit / ring * (1.0 + 1.0 / 1048576.0);
    for (;;) {
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) {
            const double lo = std::floor((double)mn[k] / ec), hi = std::floor((double)mx[k] / ec);
            if (!(std::fabs(lo) < 1.0e15 && std::fabs(hi) < 1.0e15) || hi - lo + 3.0 >= 2097152.0) ok = false;
            else G->base[k] = (long long)lo - 1;
        }
        if (ok) break;
        ec *= 2.0;
    }
    G->ec = ec;
    G->ring = ring;
    G->pad = 0;
}

}  // namespace

int outlier_build_grid(r360_ctx* ctx, const uint4* pts, size_t n, const MapHdr& bounds, double limit, int ring,
                       OutlierGrid* G, size_t* table_cap) {
    OutlierState& S = ctx->outl;
    hipStream_t st = ctx->stream;
    const size_t nf = (size_t)bounds.count;
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) { mn[k] = ord2f(bounds.mn[k]); mx[k] = ord2f(bounds.mx[k]); }
    make_grid(mn, mx, limit, ring, G);
    size_t cap = 1024;
    while (cap < 2 * nf) cap <<= 1;   // a power of two (the probe mask), at most half full
    *table_cap = cap;
    const size_t nb_scan = (std::max(cap, n) + R360_OUTLIER_SCAN_BLOCK - 1) / R360_OUTLIER_SCAN_BLOCK;
    if (grow(ctx, S.pslot, n) || grow(ctx, S.keys, cap) || grow(ctx, S.cnt, cap) || grow(ctx, S.start, cap) ||
        grow(ctx, S.fill, cap) || grow(ctx, S.spts, nf) || grow(ctx, S.bsum, nb_scan))
        return -1;
    R360_HIP(hipMemsetAsync(S.keys.get(), 0, sizeof(unsigned long long) * cap, st));
    R360_HIP(hipMemsetAsync(S.cnt.get(), 0, sizeof(unsigned) * cap, st));
    R360_HIP(hipMemsetAsync(S.fill.get(), 0, sizeof(unsigned) * cap, st));
    if (launch_out_cells(st, pts, n, *G, S.keys.get(), cap, S.cnt.get(), S.pslot.get(), S.d_hdr.get())) return -1;
    if (launch_out_scan(st, S.cnt.get(), cap, S.bsum.get(), S.start.get(), nullptr)) return -1;
    return launch_out_scatter(st, pts, n, S.pslot.get(), S.start.get(), S.fill.get(), S.spts.get(), nf, S.d_hdr.get());
}

int outlier_upload_cloud(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n) {
    OutlierState& S = ctx->outl;
    if (grow(ctx, S.in, n) || grow(ctx, S.out, n) || grow(ctx, S.up_xyz, 3 * n) || grow(ctx, S.up_rgba, n)) return -1;
    R360_HIP(hipMemcpyAsync(S.up_xyz.get(), xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    if (rgba) R360_HIP(hipMemcpyAsync(S.up_rgba.get(), rgba, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    return launch_map_pack_host(ctx->stream, S.up_xyz.get(), rgba ? S.up_rgba.get() : nullptr, n, S.in.get());
}

namespace {

// The filter named by prm on pts[0 .. n).  FILTER: the kept points into out (room for n), their number in *m.  HOOK:
// S.score (statistical) or S.count (radius, the full counts) filled for every row, nothing compacted.  Synchronous.
int outlier_run(r360_ctx* ctx, const uint4* pts, size_t n, const r360_outlier_params& prm, Mode mode, uint4* out,
                size_t out_cap, size_t* m, r360_outlier_stats* stats) {
    OutlierState& S = ctx->outl;
    hipStream_t st = ctx->stream;
    const bool stat = prm.kind == R360_OUTLIER_STATISTICAL;
    *m = 0;
    r360_outlier_stats z;
    memset(&z, 0, sizeof z);
    z.n_in = n;
    z.n_removed = n;
    if (stats) *stats = z;
    if (n == 0) return 0;
    if (S.d_bounds.reserve(ctx, 1) || S.h_bounds.reserve(ctx, 1) || S.d_hdr.reserve(ctx, 1) || S.h_hdr.reserve(ctx, 1) ||
        S.partial.reserve(ctx, R360_OUTLIER_MAXB))
        return -1;
    if (grow(ctx, S.score, n) || grow(ctx, S.count, n) || grow(ctx, S.keep, n) || grow(ctx, S.pos, n) || grow(ctx, S.pslot, n))
        return -1;
    if (launch_map_bounds(st, pts, n, S.d_bounds.get())) return -1;
    R360_HIP(hipMemcpyAsync(S.h_bounds.get(), S.d_bounds.get(), sizeof(MapHdr), hipMemcpyDeviceToHost, st));
    R360_HIP(hipMemsetAsync(S.d_hdr.get(), 0, sizeof(OutlierHdr), st));
    if (launch_out_init(st, n, S.score.get(), S.count.get(), S.keep.get())) return -1;
    if (ctx_wait(ctx)) return -1;
    const size_t nf = (size_t)S.h_bounds.get()->count;
    z.n_finite = nf;
    if (nf > 0) {
        const double limit = stat ? (double)prm.max_dist : (double)prm.radius;
        OutlierGrid G;
        size_t cap = 0;
        // the k-NN walk prunes cells by their distance, so finer cells save candidates; the count reads them all
        if (outlier_build_grid(ctx, pts, n, *S.h_bounds.get(), limit, stat ? 2 : 1, &G, &cap)) return -1;
        const double lim2 = limit * limit;
        if (stat) {
            if (launch_outlier_knn(st, S.spts.get(), nf, G, S.keys.get(), cap, S.start.get(), S.cnt.get(), lim2, prm.mean_k,
                                   S.score.get()))
                return -1;
        } else {
            const int stop = mode == HOOK ? INT32_MAX : prm.min_neighbors;
            if (launch_outlier_count(st, S.spts.get(), nf, G, S.keys.get(), cap, S.start.get(), S.cnt.get(), lim2, stop,
                                     S.count.get()))
                return -1;
        }
    } else if (grow(ctx, S.bsum, (n + R360_OUTLIER_SCAN_BLOCK - 1) / R360_OUTLIER_SCAN_BLOCK)) {
        return -1;
    }
    if (stat && launch_out_stats(st, S.score.get(), n, (double)prm.stddev_mul, S.partial.get(), S.d_hdr.get())) return -1;
    if (mode == FILTER) {
        if (stat) {
            if (launch_out_flag_stat(st, S.score.get(), n, S.d_hdr.get(), S.keep.get())) return -1;
        } else if (launch_out_flag_radius(st, S.count.get(), n, prm.min_neighbors, S.keep.get())) {
            return -1;
        }
        if (launch_out_scan(st, S.keep.get(), n, S.bsum.get(), S.pos.get(), &S.d_hdr.get()->n_out)) return -1;
        if (launch_out_compact(st, pts, n, S.keep.get(), S.pos.get(), out, out_cap, S.d_hdr.get())) return -1;
    }
    if (read_hdr(ctx)) return -1;
    const OutlierHdr& H = *S.h_hdr.get();
    if (H.err || H.n_out > n) {
        r360_set_error("outliers: internal error (flags %u, %llu kept of %zu)", H.err, H.n_out, n);
        return -1;
    }
    *m = (size_t)H.n_out;
    z.n_short = (size_t)H.n_short;
    z.n_removed = n - *m;
    if (stat) { z.mean = H.mean; z.stddev = H.stddev; z.threshold = H.threshold; }
    if (stats) *stats = z;
    return 0;
}

}  // namespace

extern "C" void r360_outlier_default_params(r360_outlier_params* p) {
    if (!p) return;
    p->kind = R360_OUTLIER_STATISTICAL;
    p->mean_k = 20;
    p->stddev_mul = 1.0f;
    p->max_dist = 0.5f;
    p->radius = 0.15f;
    p->min_neighbors = 5;
}

extern "C" int r360_cloud_filter_outliers(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n,
                                          const r360_outlier_params* params, float* out_xyz, uint32_t* out_rgba, size_t cap,
                                          size_t* n_out, r360_outlier_stats* stats) {
    if (int rc = check_params(ctx, params)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    CHECK_ARG(n_out && (n == 0 || out_xyz), "null output");
    *n_out = 0;
    if (stats) { memset(stats, 0, sizeof *stats); }
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    OutlierState& S = ctx->outl;
    if (outlier_upload_cloud(ctx, xyz, rgba, n)) return -1;
    size_t m = 0;
    if (int rc = outlier_run(ctx, S.in.get(), n, *params, FILTER, S.out.get(), S.out.cap(), &m, stats)) return rc;
    *n_out = m;
    if (cap < m) { r360_set_error("outlier filter: output capacity %zu < %zu points", cap, m); return -4; }
    if (m == 0) return 0;
    if (launch_map_unpack(ctx->stream, S.out.get(), m, S.up_xyz.get(), S.up_rgba.get())) return -1;
    R360_HIP(hipMemcpyAsync(out_xyz, S.up_xyz.get(), sizeof(float) * 3 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (rgba && out_rgba)
        R360_HIP(hipMemcpyAsync(out_rgba, S.up_rgba.get(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_filter_outliers(r360_ctx* ctx, const r360_outlier_params* params, r360_outlier_stats* stats) {
    if (int rc = check_params(ctx, params)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    if (M.map_n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    const int other = 1 - M.cur;
    // the result's buffer: the map's other half, as large as the current one, as the voxel step uses it
    if (M.map[other].cap() < M.map_n && M.map[other].reserve(ctx, M.map[M.cur].cap())) return -1;
    size_t m = 0;
    if (int rc = outlier_run(ctx, M.map[M.cur].get(), M.map_n, *params, FILTER, M.map[other].get(), M.map[other].cap(), &m, stats))
        return rc;
    M.cur = other;
    M.map_n = m;
    ctx->map_changed();
    return 0;
}

extern "C" int r360_cloud_outlier_eval(r360_ctx* ctx, const float* xyz, size_t n, const r360_outlier_params* params,
                                       double* score, int* count) {
    if (int rc = check_params(ctx, params)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    OutlierState& S = ctx->outl;
    if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
    size_t m = 0;
    if (int rc = outlier_run(ctx, S.in.get(), n, *params, HOOK, nullptr, 0, &m, nullptr)) return rc;
    if (params->kind == R360_OUTLIER_STATISTICAL) {
        if (score) R360_HIP(hipMemcpyAsync(score, S.score.get(), sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    } else if (count) {
        R360_HIP(hipMemcpyAsync(count, S.count.get(), sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    }
    return ctx_wait(ctx);
}
