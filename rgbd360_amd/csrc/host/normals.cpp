// normals.cpp — pcl::NormalEstimation (restated from PCL 1.7, unpinned) for host clouds and for the context's global map
// where it lies.  Kernels: kernels/normal_kernels.hip on the sparse grid of host/outliers.cpp; semantics and the
// divergences from PCL: DESIGN.md §5b-3.  Every device buffer is a DevBuf member of the r360_ctx's NormalState (or of
// its OutlierState, for the grid), grown on demand and freed with the context.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../r360_internal.h"

namespace {

int check_params(const r360_ctx* ctx, const r360_normal_params* p, const float* viewpoints, int n_view) {
    CHECK_ARG(ctx, "null ctx");
    CHECK_ARG(p, "null params");
    CHECK_ARG(p->k >= 3 && p->k <= R360_NORMAL_KMAX, "normals: k must be 3..64");
    CHECK_ARG(std::isfinite(p->radius) && p->radius > 0.f, "normals: radius must be positive and finite");
    CHECK_ARG(n_view >= 1 && n_view <= R360_NORMAL_VIEWMAX, "normals: n_view must be 1..4096");
    CHECK_ARG(viewpoints, "normals: null viewpoints");
    return 0;
}

template <class B>
int grow(r360_ctx* ctx, B& b, size_t need) {
    if (need <= b.cap()) return 0;
    return b.reserve(ctx, std::max<size_t>(std::max<size_t>(need, 1024), b.cap() + b.cap() / 2));
}

// The normals of pts[0 .. n) into ctx->nrm.out, and the parity hook's arrays where ev names them.  Synchronous.
int normals_run(r360_ctx* ctx, const uint4* pts, size_t n, const r360_normal_params& prm, const float* viewpoints,
                int n_view, const NormalEval& ev, r360_normal_stats* stats) {
    OutlierState& S = ctx->outl;
    NormalState& N = ctx->nrm;
    hipStream_t st = ctx->stream;
    r360_normal_stats z;
    memset(&z, 0, sizeof z);
    z.n_in = n;
    if (stats) *stats = z;
    if (n == 0) return 0;
    if (S.d_bounds.reserve(ctx, 1) || S.h_bounds.reserve(ctx, 1) || S.d_hdr.reserve(ctx, 1) || S.h_hdr.reserve(ctx, 1) ||
        N.d_hdr.reserve(ctx, 1) || N.h_hdr.reserve(ctx, 1) || grow(ctx, N.view, 3 * (size_t)n_view) || grow(ctx, N.out, n))
        return -1;
    R360_HIP(hipMemcpyAsync(N.view.get(), viewpoints, sizeof(float) * 3 * n_view, hipMemcpyHostToDevice, st));
    if (launch_map_bounds(st, pts, n, S.d_bounds.get())) return -1;
    R360_HIP(hipMemcpyAsync(S.h_bounds.get(), S.d_bounds.get(), sizeof(MapHdr), hipMemcpyDeviceToHost, st));
    R360_HIP(hipMemsetAsync(S.d_hdr.get(), 0, sizeof(OutlierHdr), st));
    R360_HIP(hipMemsetAsync(N.d_hdr.get(), 0, sizeof(NormalHdr), st));
    if (launch_normals_init(st, n, prm.k, N.out.get(), ev)) return -1;
    if (ctx_wait(ctx)) return -1;
    const size_t nf = (size_t)S.h_bounds.get()->count;
    z.n_finite = nf;
    if (nf > 0) {
        const double limit = (double)prm.radius;
        OutlierGrid G;
        size_t cap = 0;
        if (outlier_build_grid(ctx, pts, n, *S.h_bounds.get(), limit, 2, &G, &cap)) return -1;   // walk<true>'s cells
        if (launch_normals(st, pts, S.spts.get(), nf, G, S.keys.get(), cap, S.start.get(), S.cnt.get(), limit * limit, prm.k,
                           N.view.get(), n_view, N.out.get(), N.d_hdr.get(), ev))
            return -1;
    }
    R360_HIP(hipMemcpyAsync(S.h_hdr.get(), S.d_hdr.get(), sizeof(OutlierHdr), hipMemcpyDeviceToHost, st));
    R360_HIP(hipMemcpyAsync(N.h_hdr.get(), N.d_hdr.get(), sizeof(NormalHdr), hipMemcpyDeviceToHost, st));
    if (ctx_wait(ctx)) return -1;
    if (S.h_hdr.get()->err) {
        r360_set_error("normals: internal error (flags %u)", S.h_hdr.get()->err);
        return -1;
    }
    z.n_short = (size_t)N.h_hdr.get()->n_short;
    z.sum_neighbors = N.h_hdr.get()->sum_neighbors;
    if (stats) *stats = z;
    return 0;
}

// {nx, ny, nz, curvature} rows on the device into the caller's two arrays (either may be NULL)
int download_normals(r360_ctx* ctx, const float4* src, size_t n, float* normals, float* curvature) {
    if (n == 0 || (!normals && !curvature)) return 0;
    std::vector<float4> h(n);
    R360_HIP(hipMemcpyAsync(h.data(), src, sizeof(float4) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx_wait(ctx)) return -1;
    for (size_t i = 0; i < n; ++i) {
        if (normals) { normals[3 * i] = h[i].x; normals[3 * i + 1] = h[i].y; normals[3 * i + 2] = h[i].z; }
        if (curvature) curvature[i] = h[i].w;
    }
    return 0;
}

}  // namespace

extern "C" void r360_normal_default_params(r360_normal_params* p) {
    if (!p) return;
    p->k = 20;
    p->radius = 0.25f;
}

extern "C" int r360_cloud_normals(r360_ctx* ctx, const float* xyz, size_t n, const r360_normal_params* params,
                                  const float* viewpoints, int n_view, float* normals, float* curvature,
                                  r360_normal_stats* stats) {
    if (int rc = check_params(ctx, params, viewpoints, n_view)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
    const NormalEval none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (int rc = normals_run(ctx, ctx->outl.in.get(), n, *params, viewpoints, n_view, none, stats)) return rc;
    return download_normals(ctx, ctx->nrm.out.get(), n, normals, curvature);
}

extern "C" int r360_ctx_map_estimate_normals(r360_ctx* ctx, const r360_normal_params* params, const float* viewpoints,
                                             int n_view, r360_normal_stats* stats) {
    if (int rc = check_params(ctx, params, viewpoints, n_view)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    NormalState& N = ctx->nrm;
    if (M.map_n == 0) {
        N.map_n = 0;
        N.map_valid = true;
        return 0;
    }
    if (bind_device(ctx->device)) return -1;
    const NormalEval none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // into the call's own buffer, which becomes the map's only once the call has succeeded
    if (int rc = normals_run(ctx, M.map[M.cur].get(), M.map_n, *params, viewpoints, n_view, none, stats)) return rc;
    std::swap(N.out, N.map);
    N.map_n = M.map_n;
    N.map_valid = true;
    return 0;
}

extern "C" int r360_ctx_map_download_normals(r360_ctx* ctx, float* normals, float* curvature, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    const NormalState& N = ctx->nrm;
    *n = ctx->vmap.map_n;
    if (!N.map_valid || N.map_n != ctx->vmap.map_n) {
        r360_set_error("map normals: the map has no valid normals (estimate them after the map's last change)");
        return -1;
    }
    if (N.map_n == 0 || (!normals && !curvature)) return 0;
    if (cap < N.map_n) { r360_set_error("map normals download: capacity %zu < %zu points", cap, N.map_n); return -4; }
    if (bind_device(ctx->device)) return -1;
    return download_normals(ctx, N.map.get(), N.map_n, normals, curvature);
}

extern "C" int r360_cloud_normals_eval(r360_ctx* ctx, const float* xyz, size_t n, const r360_normal_params* params,
                                       const float* viewpoints, int n_view, int* knn, int* count, double* normal,
                                       double* eig, double* curvature) {
    if (int rc = check_params(ctx, params, viewpoints, n_view)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    NormalState& N = ctx->nrm;
    const size_t k = (size_t)params->k;
    if (grow(ctx, N.knn, n * k) || grow(ctx, N.count, n) || grow(ctx, N.ev, 7 * n)) return -1;
    if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
    double* e = N.ev.get();
    // count always: it is what makes the launch the hook's form of the kernel
    const NormalEval ev = {knn ? N.knn.get() : nullptr, N.count.get(), normal ? e : nullptr, eig ? e + 3 * n : nullptr,
                           curvature ? e + 6 * n : nullptr};
    if (int rc = normals_run(ctx, ctx->outl.in.get(), n, *params, viewpoints, n_view, ev, nullptr)) return rc;
    hipStream_t st = ctx->stream;
    if (knn) R360_HIP(hipMemcpyAsync(knn, ev.knn, sizeof(int) * n * k, hipMemcpyDeviceToHost, st));
    if (count) R360_HIP(hipMemcpyAsync(count, ev.count, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    if (normal) R360_HIP(hipMemcpyAsync(normal, ev.normal, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
    if (eig) R360_HIP(hipMemcpyAsync(eig, ev.eig, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
    if (curvature) R360_HIP(hipMemcpyAsync(curvature, ev.curvature, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    return ctx_wait(ctx);
}
