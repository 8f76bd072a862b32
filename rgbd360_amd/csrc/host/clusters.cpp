// clusters.cpp — pcl::EuclideanClusterExtraction and the normal-aware pcl::extractEuclideanClusters (restated from PCL 1.7,
// unpinned) for host clouds and for the context's global map where it lies.  Kernels: kernels/cluster_kernels.hip on the
// sparse grid of host/outliers.cpp; semantics, the divergences from PCL and the cost of the ranking: DESIGN.md §5b-4.
// Every device buffer is a DevBuf member of the r360_ctx's ClusterState (or of its OutlierState, for the grid and the
// scans' workgroup sums), grown on demand and freed with the context.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../r360_internal.h"
#include "cluster_rank.h"

static_assert(sizeof(ClusterRec) == sizeof(ClusterRankRec), "the kept components are ranked where they land");

namespace {

// the parameters first, the context last: the checks that need no context are the same with and without one
int check_params(const r360_ctx* ctx, const r360_cluster_params* p, bool use_normals, size_t n) {
    CHECK_ARG(p, "null params");
    CHECK_ARG(std::isfinite(p->tolerance) && p->tolerance > 0.f, "clusters: tolerance must be positive and finite");
    CHECK_ARG(p->min_size >= 1, "clusters: min_size must be at least 1");
    CHECK_ARG(p->max_size >= p->min_size, "clusters: max_size must not be below min_size");
    CHECK_ARG(!use_normals || (p->eps_angle >= 0.f && p->eps_angle <= 3.14159265358979323846f),
              "clusters: eps_angle must lie in [0, pi]");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    CHECK_ARG(ctx, "null ctx");
    return 0;
}

template <class B>
int grow(r360_ctx* ctx, B& b, size_t need) {
    if (need <= b.cap()) return 0;
    return b.reserve(ctx, std::max<size_t>(std::max<size_t>(need, 1024), b.cap() + b.cap() / 2));
}

int read_hdrs(r360_ctx* ctx) {
    OutlierState& S = ctx->outl;
    ClusterState& C = ctx->clu;
    R360_HIP(hipMemcpyAsync(S.h_hdr.get(), S.d_hdr.get(), sizeof(OutlierHdr), hipMemcpyDeviceToHost, ctx->stream));
    R360_HIP(hipMemcpyAsync(C.h_hdr.get(), C.d_hdr.get(), sizeof(ClusterHdr), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx_wait(ctx)) return -1;
    if (S.h_hdr.get()->err || C.h_hdr.get()->err) {
        r360_set_error("clusters: internal error (grid flags %u, cluster flags %u)", S.h_hdr.get()->err, C.h_hdr.get()->err);
        return -1;
    }
    return 0;
}

// The clusters of pts[0 .. n): labels into ctx->clu.labels, and with `records` the n_info records into ctx->clu.info.
// d_nrm: NULL (plain form) or the normals on the device, nstride floats apart.  filt_out: the points with label >= 0
// compacted into it (room for filt_cap), in input order.  ev: the parity hook's arrays.  Synchronous.
int clusters_run(r360_ctx* ctx, const uint4* pts, size_t n, const r360_cluster_params& prm, const float* d_nrm, int nstride,
                 bool records, uint4* filt_out, size_t filt_cap, const ClusterEval& ev, r360_cluster_stats* stats) {
    OutlierState& S = ctx->outl;
    ClusterState& C = ctx->clu;
    hipStream_t st = ctx->stream;
    r360_cluster_stats z;
    memset(&z, 0, sizeof z);
    z.n_in = n;
    if (stats) *stats = z;
    C.n_info = 0;
    if (n == 0) return 0;
    if (S.d_bounds.reserve(ctx, 1) || S.h_bounds.reserve(ctx, 1) || S.d_hdr.reserve(ctx, 1) || S.h_hdr.reserve(ctx, 1) ||
        C.d_hdr.reserve(ctx, 1) || C.h_hdr.reserve(ctx, 1))
        return -1;
    if (grow(ctx, C.parent, n) || grow(ctx, C.root, n) || grow(ctx, C.csize, n) || grow(ctx, C.crank, n) ||
        grow(ctx, C.keep, n) || grow(ctx, C.kpos, n) || grow(ctx, C.mflag, n) || grow(ctx, C.mpos, n) || grow(ctx, C.labels, n))
        return -1;
    if (launch_map_bounds(st, pts, n, S.d_bounds.get())) return -1;
    R360_HIP(hipMemcpyAsync(S.h_bounds.get(), S.d_bounds.get(), sizeof(MapHdr), hipMemcpyDeviceToHost, st));
    R360_HIP(hipMemsetAsync(S.d_hdr.get(), 0, sizeof(OutlierHdr), st));
    R360_HIP(hipMemsetAsync(C.d_hdr.get(), 0, sizeof(ClusterHdr), st));
    if (launch_clu_init(st, n, C.parent.get(), C.csize.get(), C.root.get(), C.labels.get(), ev)) return -1;
    if (ctx_wait(ctx)) return -1;
    const size_t nf = (size_t)S.h_bounds.get()->count;
    z.n_finite = nf;
    if (nf == 0) {     // every row dropped: the labels are the -1 of the init pass
        if (stats) *stats = z;
        return 0;
    }
    const double limit = (double)prm.tolerance;
    OutlierGrid G;
    size_t cap = 0;
    // ring 1: the union tests every candidate within reach, as the radius count does, so coarser cells save lookups
    if (outlier_build_grid(ctx, pts, n, *S.h_bounds.get(), limit, 1, &G, &cap)) return -1;
    const double thr = d_nrm ? std::cos((double)prm.eps_angle) : 0.0;
    if (launch_clu_union(st, S.spts.get(), nf, G, S.keys.get(), cap, S.start.get(), S.cnt.get(), limit * limit, d_nrm, nstride,
                         thr, C.parent.get(), n, C.d_hdr.get()))
        return -1;
    if (launch_clu_flatten(st, n, S.pslot.get(), C.parent.get(), C.root.get(), C.csize.get(), C.d_hdr.get())) return -1;
    if (launch_clu_mark(st, n, C.root.get(), C.csize.get(), prm.min_size, prm.max_size, C.keep.get(), C.d_hdr.get(), ev))
        return -1;
    if (launch_out_scan(st, C.keep.get(), n, S.bsum.get(), C.kpos.get(), &C.d_hdr.get()->n_kept)) return -1;
    const size_t list_cap = nf / (size_t)prm.min_size + 1;
    if (grow(ctx, C.list, list_cap)) return -1;
    if (launch_clu_list(st, n, C.keep.get(), C.kpos.get(), C.csize.get(), C.list.get(), list_cap, C.d_hdr.get())) return -1;
    if (read_hdrs(ctx)) return -1;
    const size_t nk = (size_t)C.h_hdr.get()->n_kept;
    z.n_components = (size_t)C.h_hdr.get()->n_components;
    if (nk > list_cap) { r360_set_error("clusters: internal error (%zu components kept, room for %zu)", nk, list_cap); return -1; }
    // ---- the ranking: the kept components' (root, size) records cross to the host, three small tables come back
    std::vector<int> rank_root;
    std::vector<unsigned> off, cpre;
    if (nk) {
        if (grow(ctx, C.h_list, nk)) return -1;
        R360_HIP(hipMemcpyAsync(C.h_list.get(), C.list.get(), sizeof(ClusterRec) * nk, hipMemcpyDeviceToHost, st));
        if (ctx_wait(ctx)) return -1;
    }
    const size_t m = cluster_rank_tables(reinterpret_cast<const ClusterRankRec*>(C.h_list.get()), nk, R360_CLUSTER_CHUNK,
                                         rank_root, off, cpre);
    z.n_clusters = nk;
    z.n_clustered = m;
    if (m > nf) { r360_set_error("clusters: internal error (%zu members of %zu points)", m, nf); return -1; }
    if (nk) {
        if (grow(ctx, C.h_tab, 3 * nk + 2) || grow(ctx, C.rank_root, nk) || grow(ctx, C.off, nk + 1) || grow(ctx, C.cpre, nk + 1))
            return -1;
        unsigned* t = C.h_tab.get();
        memcpy(t, rank_root.data(), sizeof(int) * nk);
        memcpy(t + nk, off.data(), sizeof(unsigned) * (nk + 1));
        memcpy(t + 2 * nk + 1, cpre.data(), sizeof(unsigned) * (nk + 1));
        R360_HIP(hipMemcpyAsync(C.rank_root.get(), t, sizeof(int) * nk, hipMemcpyHostToDevice, st));
        R360_HIP(hipMemcpyAsync(C.off.get(), t + nk, sizeof(unsigned) * (nk + 1), hipMemcpyHostToDevice, st));
        R360_HIP(hipMemcpyAsync(C.cpre.get(), t + 2 * nk + 1, sizeof(unsigned) * (nk + 1), hipMemcpyHostToDevice, st));
    }
    if (launch_clu_label(st, n, nk, C.rank_root.get(), C.crank.get(), C.root.get(), C.keep.get(), C.labels.get(),
                         C.mflag.get()))
        return -1;
    if (launch_out_scan(st, C.mflag.get(), n, S.bsum.get(), C.mpos.get(), &C.d_hdr.get()->n_clustered)) return -1;
    if (filt_out && launch_out_compact(st, pts, n, C.mflag.get(), C.mpos.get(), filt_out, filt_cap, S.d_hdr.get())) return -1;
    if (records && nk) {
        // ---- the members in rank order: (label, index) pairs in input order, then one stable split per label bit
        for (int b = 0; b < 2; ++b)
            if (grow(ctx, C.key[b], m) || grow(ctx, C.val[b], m)) return -1;
        if (launch_clu_members(st, n, C.mflag.get(), C.mpos.get(), C.labels.get(), C.key[0].get(), C.val[0].get(), m,
                               C.d_hdr.get()))
            return -1;
        int cur = 0;
        for (int bit = 0; ((size_t)1 << bit) < nk; ++bit) {
            // keep / kpos are free again: the label pass has read them
            if (launch_clu_bitflag(st, m, C.key[cur].get(), bit, C.keep.get())) return -1;
            if (launch_out_scan(st, C.keep.get(), m, S.bsum.get(), C.kpos.get(), &C.d_hdr.get()->n_zero)) return -1;
            if (launch_clu_split(st, m, C.key[cur].get(), C.val[cur].get(), C.keep.get(), C.kpos.get(), C.d_hdr.get(),
                                 C.key[1 - cur].get(), C.val[1 - cur].get()))
                return -1;
            cur = 1 - cur;
        }
        const size_t n_chunks = cpre[nk];
        if (grow(ctx, C.partial, 6 * n_chunks) || grow(ctx, C.mean, 3 * nk) || grow(ctx, C.bounds, nk) || grow(ctx, C.info, nk))
            return -1;
        if (launch_clu_moments(st, pts, C.val[cur].get(), nk, n_chunks, C.rank_root.get(), C.off.get(), C.cpre.get(),
                               C.partial.get(), C.mean.get(), C.bounds.get(), C.info.get()))
            return -1;
    }
    if (read_hdrs(ctx)) return -1;
    if ((size_t)C.h_hdr.get()->n_clustered != m) {
        r360_set_error("clusters: internal error (%llu labelled points, %zu members)", C.h_hdr.get()->n_clustered, m);
        return -1;
    }
    if (records) C.n_info = nk;
    if (stats) *stats = z;
    return 0;
}

int cloud_clusters(r360_ctx* ctx, const float* xyz, const float* normals, size_t n, const r360_cluster_params* params,
                   int* labels, r360_cluster_info* info, size_t info_cap, size_t* n_clusters, r360_cluster_stats* stats,
                   bool hook, int* root, int* comp_size) {
    if (int rc = check_params(ctx, params, normals != nullptr, n)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_clusters) *n_clusters = 0;
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    ClusterState& C = ctx->clu;
    hipStream_t st = ctx->stream;
    if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
    if (normals) {
        if (grow(ctx, C.nrm_in, 3 * n)) return -1;
        R360_HIP(hipMemcpyAsync(C.nrm_in.get(), normals, sizeof(float) * 3 * n, hipMemcpyHostToDevice, st));
    }
    if (hook && grow(ctx, C.comp_size, n)) return -1;
    const ClusterEval ev = {hook ? C.comp_size.get() : nullptr};
    if (int rc = clusters_run(ctx, ctx->outl.in.get(), n, *params, normals ? C.nrm_in.get() : nullptr, 3, true, nullptr, 0, ev,
                              stats))
        return rc;
    const size_t nk = C.n_info;
    if (n_clusters) *n_clusters = nk;
    if (labels) R360_HIP(hipMemcpyAsync(labels, C.labels.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    if (root) R360_HIP(hipMemcpyAsync(root, C.root.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    if (comp_size) R360_HIP(hipMemcpyAsync(comp_size, C.comp_size.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    const bool fits = !info || info_cap >= nk;
    if (info && fits && nk)
        R360_HIP(hipMemcpyAsync(info, C.info.get(), sizeof(r360_cluster_info) * nk, hipMemcpyDeviceToHost, st));
    if (ctx_wait(ctx)) return -1;
    if (!fits) { r360_set_error("clusters: record capacity %zu < %zu clusters", info_cap, nk); return -4; }
    return 0;
}

}  // namespace

extern "C" void r360_cluster_default_params(r360_cluster_params* p) {
    if (!p) return;
    p->tolerance = 0.10f;                      // two leaves of the 5 cm voxel grid
    p->min_size = 100;
    p->max_size = 1 << 30;
    p->eps_angle = 0.17453292519943295f;       // 10 degrees
}

extern "C" int r360_cloud_clusters(r360_ctx* ctx, const float* xyz, const float* normals, size_t n,
                                   const r360_cluster_params* params, int* labels, r360_cluster_info* info, size_t info_cap,
                                   size_t* n_clusters, r360_cluster_stats* stats) {
    return cloud_clusters(ctx, xyz, normals, n, params, labels, info, info_cap, n_clusters, stats, false, nullptr, nullptr);
}

extern "C" int r360_cloud_clusters_eval(r360_ctx* ctx, const float* xyz, const float* normals, size_t n,
                                        const r360_cluster_params* params, int* labels, r360_cluster_info* info,
                                        size_t info_cap, size_t* n_clusters, r360_cluster_stats* stats, int* root,
                                        int* comp_size) {
    return cloud_clusters(ctx, xyz, normals, n, params, labels, info, info_cap, n_clusters, stats, true, root, comp_size);
}

extern "C" int r360_ctx_map_cluster(r360_ctx* ctx, const r360_cluster_params* params, int use_normals,
                                    r360_cluster_stats* stats) {
    if (int rc = check_params(ctx, params, use_normals != 0, 0)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    NormalState& N = ctx->nrm;
    ClusterState& C = ctx->clu;
    if (use_normals && !(N.map_valid && N.map_n == M.map_n)) {
        r360_set_error("map clusters: the map has no valid normals (estimate them after the map's last change)");
        return -1;
    }
    if (M.map_n == 0) {
        C.map_n = 0;
        C.map_n_info = 0;
        C.map_valid = true;
        return 0;
    }
    if (bind_device(ctx->device)) return -1;
    const ClusterEval none = {nullptr};
    // into the call's own buffers, which become the map's only once the call has succeeded
    if (int rc = clusters_run(ctx, M.map[M.cur].get(), M.map_n, *params,
                              use_normals ? reinterpret_cast<const float*>(N.map.get()) : nullptr, 4, true, nullptr, 0, none,
                              stats))
        return rc;
    std::swap(C.labels, C.map_labels);
    std::swap(C.info, C.map_info);
    C.map_n = M.map_n;
    C.map_n_info = C.n_info;
    C.map_valid = true;
    return 0;
}

extern "C" int r360_ctx_map_download_labels(r360_ctx* ctx, int* labels, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    const ClusterState& C = ctx->clu;
    *n = ctx->vmap.map_n;
    if (!C.map_valid || C.map_n != ctx->vmap.map_n) {
        r360_set_error("map labels: the map has no valid labels (cluster it after the map's last change)");
        return -1;
    }
    if (C.map_n == 0 || !labels) return 0;
    if (cap < C.map_n) { r360_set_error("map labels download: capacity %zu < %zu points", cap, C.map_n); return -4; }
    if (bind_device(ctx->device)) return -1;
    R360_HIP(hipMemcpyAsync(labels, C.map_labels.get(), sizeof(int) * C.map_n, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_cluster_info(r360_ctx* ctx, r360_cluster_info* info, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    const ClusterState& C = ctx->clu;
    *n = 0;
    if (!C.map_valid || C.map_n != ctx->vmap.map_n) {
        r360_set_error("map clusters: the map has no valid labels (cluster it after the map's last change)");
        return -1;
    }
    *n = C.map_n_info;
    if (C.map_n_info == 0 || !info) return 0;
    if (cap < C.map_n_info) { r360_set_error("map cluster records: capacity %zu < %zu clusters", cap, C.map_n_info); return -4; }
    if (bind_device(ctx->device)) return -1;
    R360_HIP(hipMemcpyAsync(info, C.map_info.get(), sizeof(r360_cluster_info) * C.map_n_info, hipMemcpyDeviceToHost,
                            ctx->stream));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_filter_clusters(r360_ctx* ctx, const r360_cluster_params* params, int use_normals,
                                            r360_cluster_stats* stats) {
    if (int rc = check_params(ctx, params, use_normals != 0, 0)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    NormalState& N = ctx->nrm;
    if (use_normals && !(N.map_valid && N.map_n == M.map_n)) {
        r360_set_error("map clusters: the map has no valid normals (estimate them after the map's last change)");
        return -1;
    }
    if (M.map_n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    const int other = 1 - M.cur;
    // the result's buffer: the map's other half, as large as the current one, as the outlier filter uses it
    if (M.map[other].cap() < M.map_n && M.map[other].reserve(ctx, M.map[M.cur].cap())) return -1;
    const ClusterEval none = {nullptr};
    r360_cluster_stats z;
    if (int rc = clusters_run(ctx, M.map[M.cur].get(), M.map_n, *params,
                              use_normals ? reinterpret_cast<const float*>(N.map.get()) : nullptr, 4, false,
                              M.map[other].get(), M.map[other].cap(), none, &z))
        return rc;
    if (stats) *stats = z;
    M.cur = other;
    M.map_n = z.n_clustered;
    ctx->map_changed();
    return 0;
}
