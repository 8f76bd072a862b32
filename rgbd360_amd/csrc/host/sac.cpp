// sac.cpp — RANSAC plane segmentation: pcl::SACSegmentation with SACMODEL_PLANE / _PERPENDICULAR_PLANE / _PARALLEL_PLANE and
// SAC_RANSAC, and the peel loop of PCL's cluster-extraction recipe (restated; PCL is not pinned), for host clouds and
// for the context's global map where it lies.  Kernels: kernels/sac_kernels.hip; the sampler: host/sac_sample.h;
// semantics and the divergences from PCL: DESIGN.md §5b-5.  Every device buffer is a DevBuf member of the r360_ctx's
// SacState (the scans' workgroup sums and the upload staging are its OutlierState's), grown on demand and freed with the
// context: a call sizes them once, nothing is allocated per round or per plane.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>

#include "../r360_internal.h"

namespace {

// the parameters first, the context last: the checks that need no context are the same with and without one
int check_params(const r360_ctx* ctx, const r360_sac_params* p, bool use_normals, size_t n) {
    CHECK_ARG(p, "null params");
    CHECK_ARG(std::isfinite(p->distance_threshold) && p->distance_threshold > 0.f,
              "sac: distance_threshold must be positive and finite");
    CHECK_ARG(p->max_iterations >= 1 && p->max_iterations <= 65536, "sac: max_iterations must lie in 1 .. 65536");
    CHECK_ARG(p->probability > 0.f && p->probability < 1.f, "sac: probability must lie in (0, 1)");
    CHECK_ARG(p->max_planes >= 1 && p->max_planes <= R360_SAC_MAX_PLANES, "sac: max_planes must lie in 1 .. 64");
    CHECK_ARG(p->min_inliers >= 3, "sac: min_inliers must be at least 3");
    CHECK_ARG(p->stop_fraction >= 0.f && p->stop_fraction < 1.f, "sac: stop_fraction must lie in [0, 1)");
    CHECK_ARG(p->constraint == R360_SAC_NONE || p->constraint == R360_SAC_PERPENDICULAR || p->constraint == R360_SAC_PARALLEL,
              "sac: unknown constraint");
    const float half_pi = 1.57079632679489661923f;
    if (p->constraint != R360_SAC_NONE) {
        CHECK_ARG(std::isfinite(p->axis[0]) && std::isfinite(p->axis[1]) && std::isfinite(p->axis[2]) &&
                      (p->axis[0] != 0.f || p->axis[1] != 0.f || p->axis[2] != 0.f),
                  "sac: a constrained call's axis must be finite and non-zero");
        CHECK_ARG(p->eps_angle >= 0.f && p->eps_angle <= half_pi, "sac: eps_angle must lie in [0, pi/2]");
    }
    CHECK_ARG(!use_normals || (p->normal_angle >= 0.f && p->normal_angle <= half_pi), "sac: normal_angle must lie in [0, pi/2]");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    CHECK_ARG(ctx, "null ctx");
    return 0;
}

template <class B>
int grow(r360_ctx* ctx, B& b, size_t need) {
    if (need <= b.cap()) return 0;
    return b.reserve(ctx, std::max<size_t>(std::max<size_t>(need, 1024), b.cap() + b.cap() / 2));
}

int read_hdr(r360_ctx* ctx) {
    SacState& S = ctx->sac;
    R360_HIP(hipMemcpyAsync(S.h_hdr.get(), S.d_hdr.get(), sizeof(SacHdr), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx_wait(ctx)) return -1;
    if (S.h_hdr.get()->err) { r360_set_error("sac: internal error (flags %u)", S.h_hdr.get()->err); return -1; }
    return 0;
}

SacSearch make_search(const r360_sac_params& prm, unsigned p, size_t m) {
    SacSearch Q;
    memset(&Q, 0, sizeof Q);
    Q.seed = prm.seed;
    Q.p = p;
    Q.m = (unsigned)m;
    Q.constraint = prm.constraint;
    if (prm.constraint != R360_SAC_NONE) {
        const double ax = (double)prm.axis[0], ay = (double)prm.axis[1], az = (double)prm.axis[2];
        const double len = std::sqrt((ax * ax + ay * ay) + az * az);
        Q.axis[0] = ax / len; Q.axis[1] = ay / len; Q.axis[2] = az / len;
        Q.cos_eps = std::cos((double)prm.eps_angle);
        Q.sin_eps = std::sin((double)prm.eps_angle);
    }
    return Q;
}

SacGate make_gate(const r360_sac_params& prm, const float* d_nrm, int nstride) {
    SacGate G;
    G.nrm = d_nrm;
    G.nstride = nstride;
    G.thr = (double)prm.distance_threshold;
    G.cos_n = d_nrm ? std::cos((double)prm.normal_angle) : 0.0;
    return G;
}

// the buffers every call needs, the finite rows of pts[0 .. n) listed into pool[0], labels = -1; *nf their count
int sac_begin(r360_ctx* ctx, const uint4* pts, size_t n, size_t* nf) {
    SacState& S = ctx->sac;
    hipStream_t st = ctx->stream;
    if (S.d_hdr.reserve(ctx, 1) || S.h_hdr.reserve(ctx, 1)) return -1;
    if (grow(ctx, S.pool[0], n) || grow(ctx, S.pool[1], n) || grow(ctx, S.inl, n) || grow(ctx, S.flag, n) ||
        grow(ctx, S.fpos, n) || grow(ctx, S.labels, n) || grow(ctx, S.coef, 4 * R360_SAC_ROUND) ||
        grow(ctx, S.count, R360_SAC_ROUND) || grow(ctx, S.partial, 6 * ((n + R360_SAC_CHUNK - 1) / R360_SAC_CHUNK)) ||
        grow(ctx, S.mean, 3) || grow(ctx, S.info, R360_SAC_MAX_PLANES) ||
        grow(ctx, ctx->outl.bsum, (n + R360_OUTLIER_SCAN_BLOCK - 1) / R360_OUTLIER_SCAN_BLOCK))
        return -1;
    R360_HIP(hipMemsetAsync(S.d_hdr.get(), 0, sizeof(SacHdr), st));
    if (launch_sac_finite(st, pts, n, S.flag.get(), S.labels.get())) return -1;
    if (launch_out_scan(st, S.flag.get(), n, ctx->outl.bsum.get(), S.fpos.get(), &S.d_hdr.get()->n_finite)) return -1;
    if (launch_sac_pool0(st, n, S.flag.get(), S.fpos.get(), S.pool[0].get())) return -1;
    if (read_hdr(ctx)) return -1;
    *nf = (size_t)S.h_hdr.get()->n_finite;
    if (*nf > n) { r360_set_error("sac: internal error (%zu finite rows of %zu)", *nf, n); return -1; }
    return 0;
}

// flags of the pool's inliers of the plane at d_coef, their prefix and their count (into the header, not yet read)
int sac_select(r360_ctx* ctx, const uint4* pts, const int* pool, size_t m, const SacGate& G, const double* d_coef) {
    SacState& S = ctx->sac;
    if (launch_sac_select(ctx->stream, pts, pool, m, G, d_coef, S.flag.get())) return -1;
    return launch_out_scan(ctx->stream, S.flag.get(), m, ctx->outl.bsum.get(), S.fpos.get(), &S.d_hdr.get()->n_sel);
}

// The planes of pts[0 .. n): labels into ctx->sac.labels, the records into ctx->sac.info (n_info of them).  d_nrm: NULL
// (plain form) or the normals on the device, nstride floats apart.  Synchronous.
int sac_run(r360_ctx* ctx, const uint4* pts, size_t n, const r360_sac_params& prm, const float* d_nrm, int nstride,
            r360_sac_stats* stats) {
    SacState& S = ctx->sac;
    hipStream_t st = ctx->stream;
    r360_sac_stats z;
    memset(&z, 0, sizeof z);
    z.n_in = n;
    if (stats) *stats = z;
    S.n_info = 0;
    if (n == 0) return 0;
    size_t nf = 0;
    if (sac_begin(ctx, pts, n, &nf)) return -1;
    z.n_finite = nf;
    const SacGate G = make_gate(prm, d_nrm, nstride);
    const double log_fail = std::log(1.0 - (double)prm.probability);
    SacHdr* dh = S.d_hdr.get();
    const SacHdr* hh = S.h_hdr.get();
    size_t m = nf;
    int cur = 0;
    for (int p = 0; p < prm.max_planes; ++p) {
        if (m < (size_t)std::max(3, prm.min_inliers)) break;
        if ((double)m <= (double)prm.stop_fraction * (double)nf) break;
        const int* pool = S.pool[cur].get();
        const SacSearch Q = make_search(prm, (unsigned)p, m);
        const SacHdr fresh = {-1, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, (unsigned long long)nf, 0ull, 0u, 0u};
        *S.h_hdr.get() = fresh;
        R360_HIP(hipMemcpyAsync(dh, S.h_hdr.get(), sizeof(SacHdr), hipMemcpyHostToDevice, st));
        // ---- the search: a round's hypotheses, their counts, the best so far; one small read-back per round
        int evaluated = 0;
        for (;;) {
            const int nh = std::min(R360_SAC_ROUND, prm.max_iterations - evaluated);
            if (launch_sac_hyp(st, pts, pool, Q, evaluated, nh, S.coef.get(), nullptr)) return -1;
            R360_HIP(hipMemsetAsync(S.count.get(), 0, sizeof(int) * R360_SAC_ROUND, st));
            if (launch_sac_count(st, pts, pool, m, G, S.coef.get(), nh, S.count.get())) return -1;
            if (launch_sac_best(st, S.count.get(), S.coef.get(), evaluated, nh, dh)) return -1;
            if (read_hdr(ctx)) return -1;
            evaluated += nh;
            const double w = (double)hh->best_count / (double)m;
            double q = 1.0 - (w * w) * w;
            q = std::min(std::max(q, DBL_EPSILON), 1.0 - DBL_EPSILON);
            const double k = log_fail / std::log(q);
            if (!(evaluated < prm.max_iterations && (double)evaluated < k)) break;
        }
        z.n_evaluated += (size_t)evaluated;
        const int raw = hh->best_count;
        // ---- the final inliers: of the best hypothesis, or of the plane refined on them
        if (sac_select(ctx, pts, pool, m, G, dh->best_coef)) return -1;
        const bool refine = prm.optimize != 0 && raw >= 3;
        if (refine) {
            if (launch_sac_split(st, pool, m, S.flag.get(), S.fpos.get(), S.inl.get(), (size_t)raw, dh)) return -1;
            if (launch_sac_moments(st, pts, S.inl.get(), (size_t)raw, S.partial.get(), S.mean.get(), dh, nullptr, true, raw,
                                   evaluated))
                return -1;
            if (sac_select(ctx, pts, pool, m, G, dh->ref_coef)) return -1;
        }
        if (read_hdr(ctx)) return -1;
        const size_t size = (size_t)hh->n_sel;
        if (size > m) { r360_set_error("sac: internal error (%zu inliers of %zu rows)", size, m); return -1; }
        if (size < (size_t)prm.min_inliers) break;
        if (launch_sac_split(st, pool, m, S.flag.get(), S.fpos.get(), S.inl.get(), size, dh)) return -1;
        if (launch_sac_moments(st, pts, S.inl.get(), size, S.partial.get(), S.mean.get(), dh, S.info.get() + p, refine, raw,
                               evaluated))
            return -1;
        if (launch_sac_peel(st, pool, m, S.flag.get(), S.fpos.get(), p, S.labels.get(), S.pool[1 - cur].get(), n, dh)) return -1;
        cur = 1 - cur;
        m -= size;
        z.n_planes += 1;
        z.n_in_planes += size;
    }
    if (read_hdr(ctx)) return -1;
    S.n_info = z.n_planes;
    if (stats) *stats = z;
    return 0;
}

int upload_normals(r360_ctx* ctx, const float* normals, size_t n) {
    SacState& S = ctx->sac;
    if (grow(ctx, S.nrm_in, 3 * n)) return -1;
    R360_HIP(hipMemcpyAsync(S.nrm_in.get(), normals, sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

bool map_normals_valid(const r360_ctx* ctx) { return ctx->nrm.map_valid && ctx->nrm.map_n == ctx->vmap.map_n; }

}  // namespace

extern "C" void r360_sac_default_params(r360_sac_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->distance_threshold = 0.05f;             // one leaf of the 5 cm voxel grid
    p->max_iterations = 1024;
    p->probability = 0.99f;
    p->optimize = 1;
    p->constraint = R360_SAC_NONE;
    p->axis[2] = 1.f;
    p->eps_angle = 0.17453292519943295f;       // 10 degrees
    p->normal_angle = 0.17453292519943295f;
    p->max_planes = 8;
    p->min_inliers = 100;
    p->stop_fraction = 0.f;
    p->seed = 0;
}

extern "C" int r360_cloud_sac_planes(r360_ctx* ctx, const float* xyz, const float* normals, size_t n,
                                     const r360_sac_params* params, int* labels, r360_sac_plane* planes, size_t planes_cap,
                                     size_t* n_planes, r360_sac_stats* stats) {
    if (int rc = check_params(ctx, params, normals != nullptr, n)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_planes) *n_planes = 0;
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    SacState& S = ctx->sac;
    hipStream_t st = ctx->stream;
    if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
    if (normals && upload_normals(ctx, normals, n)) return -1;
    if (int rc = sac_run(ctx, ctx->outl.in.get(), n, *params, normals ? S.nrm_in.get() : nullptr, 3, stats)) return rc;
    const size_t np = S.n_info;
    if (n_planes) *n_planes = np;
    if (labels) R360_HIP(hipMemcpyAsync(labels, S.labels.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    const bool fits = !planes || planes_cap >= np;
    if (planes && fits && np)
        R360_HIP(hipMemcpyAsync(planes, S.info.get(), sizeof(r360_sac_plane) * np, hipMemcpyDeviceToHost, st));
    if (ctx_wait(ctx)) return -1;
    if (!fits) { r360_set_error("sac: record capacity %zu < %zu planes", planes_cap, np); return -4; }
    return 0;
}

extern "C" int r360_cloud_sac_eval(r360_ctx* ctx, const float* xyz, const float* normals, size_t n,
                                   const r360_sac_params* params, const double* coef_in, size_t n_hyp, int* samples,
                                   double* coef, int* count) {
    if (int rc = check_params(ctx, params, normals != nullptr, n)) return rc;
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n_hyp <= 65536, "sac eval: more than 65536 hypotheses");
    if (n_hyp == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    SacState& S = ctx->sac;
    hipStream_t st = ctx->stream;
    size_t nf = 0;
    if (n) {
        if (outlier_upload_cloud(ctx, xyz, nullptr, n)) return -1;
        if (normals && upload_normals(ctx, normals, n)) return -1;
        if (sac_begin(ctx, ctx->outl.in.get(), n, &nf)) return -1;
    }
    const bool drawn = coef_in == nullptr;
    if (nf < 3 && drawn) {               // nothing to draw from: every hypothesis scores 0
        for (size_t i = 0; i < n_hyp; ++i) {
            if (samples) samples[3 * i] = samples[3 * i + 1] = samples[3 * i + 2] = -1;
            if (coef) coef[4 * i] = coef[4 * i + 1] = coef[4 * i + 2] = coef[4 * i + 3] = std::nan("");
            if (count) count[i] = 0;
        }
        return 0;
    }
    if (grow(ctx, S.coef, 4 * std::max<size_t>(n_hyp, R360_SAC_ROUND)) || grow(ctx, S.count, std::max<size_t>(n_hyp, R360_SAC_ROUND)) ||
        grow(ctx, S.samples, 3 * n_hyp))
        return -1;
    const uint4* pts = ctx->outl.in.get();
    const SacGate G = make_gate(*params, normals ? S.nrm_in.get() : nullptr, 3);
    R360_HIP(hipMemsetAsync(S.count.get(), 0, sizeof(int) * n_hyp, st));
    if (drawn) {
        const SacSearch Q = make_search(*params, 0u, nf);
        if (launch_sac_hyp(st, pts, S.pool[0].get(), Q, 0, (int)n_hyp, S.coef.get(), S.samples.get())) return -1;
    } else {
        R360_HIP(hipMemcpyAsync(S.coef.get(), coef_in, sizeof(double) * 4 * n_hyp, hipMemcpyHostToDevice, st));
    }
    for (size_t h0 = 0; h0 < n_hyp; h0 += R360_SAC_ROUND) {
        const int nh = (int)std::min<size_t>(R360_SAC_ROUND, n_hyp - h0);
        if (launch_sac_count(st, pts, S.pool[0].get(), nf, G, S.coef.get() + 4 * h0, nh, S.count.get() + h0)) return -1;
    }
    if (samples) {
        if (drawn) R360_HIP(hipMemcpyAsync(samples, S.samples.get(), sizeof(int) * 3 * n_hyp, hipMemcpyDeviceToHost, st));
        else for (size_t i = 0; i < 3 * n_hyp; ++i) samples[i] = -1;
    }
    if (coef) R360_HIP(hipMemcpyAsync(coef, S.coef.get(), sizeof(double) * 4 * n_hyp, hipMemcpyDeviceToHost, st));
    if (count) R360_HIP(hipMemcpyAsync(count, S.count.get(), sizeof(int) * n_hyp, hipMemcpyDeviceToHost, st));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_sac_planes(r360_ctx* ctx, const r360_sac_params* params, int use_normals, r360_sac_stats* stats) {
    if (int rc = check_params(ctx, params, use_normals != 0, 0)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    SacState& S = ctx->sac;
    if (use_normals && !map_normals_valid(ctx)) {
        r360_set_error("map planes: the map has no valid normals (estimate them after the map's last change)");
        return -1;
    }
    if (M.map_n == 0) {
        S.map_n = 0;
        S.map_n_info = 0;
        S.map_valid = true;
        return 0;
    }
    if (bind_device(ctx->device)) return -1;
    // into the call's own buffers, which become the map's only once the call has succeeded
    if (int rc = sac_run(ctx, M.map[M.cur].get(), M.map_n, *params,
                         use_normals ? reinterpret_cast<const float*>(ctx->nrm.map.get()) : nullptr, 4, stats))
        return rc;
    std::swap(S.labels, S.map_labels);
    std::swap(S.info, S.map_info);
    S.map_n = M.map_n;
    S.map_n_info = S.n_info;
    S.map_valid = true;
    return 0;
}

extern "C" int r360_ctx_map_download_plane_labels(r360_ctx* ctx, int* labels, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    const SacState& S = ctx->sac;
    *n = ctx->vmap.map_n;
    if (!S.map_valid || S.map_n != ctx->vmap.map_n) {
        r360_set_error("map plane labels: the map has no valid plane labels (segment it after the map's last change)");
        return -1;
    }
    if (S.map_n == 0 || !labels) return 0;
    if (cap < S.map_n) { r360_set_error("map plane labels download: capacity %zu < %zu points", cap, S.map_n); return -4; }
    if (bind_device(ctx->device)) return -1;
    R360_HIP(hipMemcpyAsync(labels, S.map_labels.get(), sizeof(int) * S.map_n, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_plane_info(r360_ctx* ctx, r360_sac_plane* planes, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    const SacState& S = ctx->sac;
    *n = 0;
    if (!S.map_valid || S.map_n != ctx->vmap.map_n) {
        r360_set_error("map planes: the map has no valid plane labels (segment it after the map's last change)");
        return -1;
    }
    *n = S.map_n_info;
    if (S.map_n_info == 0 || !planes) return 0;
    if (cap < S.map_n_info) { r360_set_error("map plane records: capacity %zu < %zu planes", cap, S.map_n_info); return -4; }
    if (bind_device(ctx->device)) return -1;
    R360_HIP(hipMemcpyAsync(planes, S.map_info.get(), sizeof(r360_sac_plane) * S.map_n_info, hipMemcpyDeviceToHost,
                            ctx->stream));
    return ctx_wait(ctx);
}

extern "C" int r360_ctx_map_filter_planes(r360_ctx* ctx, const r360_sac_params* params, int use_normals, int keep_planes,
                                          r360_sac_stats* stats) {
    if (int rc = check_params(ctx, params, use_normals != 0, 0)) return rc;
    CHECK_ARG(keep_planes == 0 || keep_planes == 1, "map planes: keep_planes must be 0 or 1");
    if (stats) memset(stats, 0, sizeof *stats);
    MapState& M = ctx->vmap;
    SacState& S = ctx->sac;
    OutlierState& O = ctx->outl;
    if (use_normals && !map_normals_valid(ctx)) {
        r360_set_error("map planes: the map has no valid normals (estimate them after the map's last change)");
        return -1;
    }
    if (M.map_n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    hipStream_t st = ctx->stream;
    const int other = 1 - M.cur;
    // the result's buffer: the map's other half, as large as the current one, as the outlier filter uses it
    if (M.map[other].cap() < M.map_n && M.map[other].reserve(ctx, M.map[M.cur].cap())) return -1;
    if (O.d_hdr.reserve(ctx, 1) || O.h_hdr.reserve(ctx, 1)) return -1;
    r360_sac_stats z;
    const size_t n = M.map_n;
    if (int rc = sac_run(ctx, M.map[M.cur].get(), n, *params,
                         use_normals ? reinterpret_cast<const float*>(ctx->nrm.map.get()) : nullptr, 4, &z))
        return rc;
    R360_HIP(hipMemsetAsync(O.d_hdr.get(), 0, sizeof(OutlierHdr), st));
    if (launch_sac_keepflag(st, S.labels.get(), n, keep_planes, S.flag.get())) return -1;
    if (launch_out_scan(st, S.flag.get(), n, O.bsum.get(), S.fpos.get(), &S.d_hdr.get()->n_sel)) return -1;
    if (launch_out_compact(st, M.map[M.cur].get(), n, S.flag.get(), S.fpos.get(), M.map[other].get(), M.map[other].cap(),
                           O.d_hdr.get()))
        return -1;
    R360_HIP(hipMemcpyAsync(O.h_hdr.get(), O.d_hdr.get(), sizeof(OutlierHdr), hipMemcpyDeviceToHost, st));
    if (read_hdr(ctx)) return -1;
    const size_t kept = (size_t)S.h_hdr.get()->n_sel;
    const size_t want = keep_planes ? z.n_in_planes : n - z.n_in_planes;
    if (O.h_hdr.get()->err || kept != want) {
        r360_set_error("map planes: internal error (%zu points kept, %zu expected, flags %u)", kept, want, O.h_hdr.get()->err);
        return -1;
    }
    if (stats) *stats = z;
    M.cur = other;
    M.map_n = kept;
    ctx->map_changed();
    return 0;
}
