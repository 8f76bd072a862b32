// gicp.cpp — Generalized-ICP on the context's GPU: r360_gicp_set_source / set_target / align and the parity hooks
// (include/rgbd360_hip.h).  Kernels: kernels/gicp_kernels.hip; the host-only logic (intake, the grid's sizing and
// build, the 6x6 solve, the inner loop's accept / stop rule): host/gicp_host.h; statement and design: DESIGN.md §5c.
// Every device buffer is a DevBuf / PinnedBuf member of the r360_ctx's GicpState (devmem.h), grown on demand with a
// 1024-item floor and freed with the context: there is no handle type and no static owner.  Everything runs on the context's stream.
#include <cmath>
#include <cstring>

#include "../r360_internal.h"

namespace {

size_t floored(size_t need) { return std::max<size_t>(need, 1024); }   // the growth rule of every buffer here

int check_params(const r360_gicp_params* p) {
    CHECK_ARG(p, "null params");
    CHECK_ARG(p->k_correspondences >= 4 && p->k_correspondences <= R360_GICP_KMAX, "k_correspondences outside 4 .. 32");
    CHECK_ARG(std::isfinite(p->gicp_epsilon) && p->gicp_epsilon > 0.f, "gicp_epsilon must be positive and finite");
    CHECK_ARG(p->max_corr_dist > 0.f, "max_corr_dist must be positive");   // +inf: no gate
    CHECK_ARG(p->max_iterations >= 1 && p->max_inner_iterations >= 0, "negative iteration limit");
    return 0;
}

int set_cloud(r360_ctx* ctx, GicpCloud& C, const float* xyz, size_t n, const r360_gicp_params* p, const char* name) {
    CHECK_ARG(ctx, "null ctx");
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    if (int rc = check_params(p)) return rc;
    std::vector<float> pts, sorted;
    std::vector<unsigned> cell_start;
    gicp_intake(xyz, n, pts);
    const size_t m = pts.size() / 4;
    C.n = 0;   // the cloud is unset until this call has succeeded
    if (m < (size_t)p->k_correspondences) {
        r360_set_error("gicp: the %s cloud has %zu finite points, fewer than k_correspondences = %d", name, m,
                       p->k_correspondences);
        return -3;
    }
    GicpGrid G;
    gicp_build_grid(pts, G, sorted, cell_start);
    if (bind_device(ctx->device)) return -1;
    const size_t cells = cell_start.size() - 1;
    if (C.pts.reserve(ctx, floored(m)) || C.spts.reserve(ctx, floored(m)) || C.cov6.reserve(ctx, floored(6 * m)) ||
        C.cell_start.reserve(ctx, floored(cells + 1)) || C.knn.reserve(ctx, floored(m * (size_t)p->k_correspondences)))
        return -1;
    hipStream_t st = ctx->stream;
    R360_HIP(hipMemcpyAsync(C.pts.get(), pts.data(), sizeof(float) * 4 * m, hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(C.spts.get(), sorted.data(), sizeof(float) * 4 * m, hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(C.cell_start.get(), cell_start.data(), sizeof(unsigned) * (cells + 1), hipMemcpyHostToDevice, st));
    C.grid = G;
    C.cells = cells;
    C.k = p->k_correspondences;
    C.n = m;
    if (launch_gicp_knn_cov(st, C, p->gicp_epsilon) || ctx_wait(ctx)) { C.n = 0; return -1; }   // the host vectors end here
    return 0;
}

int ensure_pass_bufs(r360_ctx* ctx) {
    GicpState& S = ctx->gicp;
    const size_t want = floored(S.src.n);   // each buffer decides from its own capacity
    if (S.corr.reserve(ctx, want) || S.M6.reserve(ctx, 6 * want) || S.d2.reserve(ctx, want)) return -1;
    if (S.partials.reserve(ctx, (size_t)R360_GICP_MAXB * R360_GICP_W) || S.d_sums.reserve(ctx, R360_GICP_W)) return -1;
    return S.h_sums.reserve(ctx, R360_GICP_W);
}

int check_ready(r360_ctx* ctx, const r360_gicp_params* p, const float* pose) {
    CHECK_ARG(ctx && pose, "null arg");
    if (int rc = check_params(p)) return rc;
    for (int k = 0; k < 16; ++k) CHECK_ARG(std::isfinite(pose[k]), "non-finite pose");
    CHECK_ARG(ctx->gicp.src.n && ctx->gicp.tgt.n, "gicp: set the source and the target cloud first");
    return 0;
}

// column-major 4x4 float -> row-major 3x4 double, and back
void pose_in(const float* m, double* X) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) X[r * 4 + c] = (double)m[c * 4 + r];
}
void pose_out_f(const double* X, float* m) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) m[c * 4 + r] = (float)X[r * 4 + c];
    m[3] = m[7] = m[11] = 0.f;
    m[15] = 1.f;
}

double gate2_of(const r360_gicp_params* p) { return (double)p->max_corr_dist * (double)p->max_corr_dist; }

int corr_pass(r360_ctx* ctx, const double* X, double gate2, int want_m) {
    GicpState& S = ctx->gicp;
    GicpPose P;
    memcpy(P.m, X, sizeof P.m);
    return launch_gicp_corr(ctx->stream, S.src, S.tgt, P, gate2, want_m, S.corr.get(), S.M6.get(), S.d2.get());
}

// one inner pass at Y: the 29 sums on the host
int inner_pass(r360_ctx* ctx, const double* Y, double* sums) {
    GicpState& S = ctx->gicp;
    GicpPose P;
    memcpy(P.m, Y, sizeof P.m);
    if (launch_gicp_pass(ctx->stream, S.src, S.tgt, P, S.corr.get(), S.M6.get(), S.partials.get(), S.d_sums.get())) return -1;
    R360_HIP(hipMemcpyAsync(S.h_sums.get(), S.d_sums.get(), sizeof(double) * R360_GICP_W, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx_wait(ctx)) return -1;
    memcpy(sums, S.h_sums.get(), sizeof(double) * R360_GICP_W);
    return 0;
}

}  // namespace

extern "C" void r360_gicp_default_params(r360_gicp_params* p) {
    if (!p) return;
    p->k_correspondences = 20;
    p->gicp_epsilon = 1e-3f;
    p->max_corr_dist = 0.4f;
    p->max_iterations = 10;
    p->max_inner_iterations = 20;
    p->rotation_epsilon = 2e-3;
    p->transformation_epsilon = 1e-9;
}

extern "C" int r360_gicp_set_source(r360_ctx* ctx, const float* xyz, size_t n, const r360_gicp_params* p) {
    CHECK_ARG(ctx, "null ctx");
    return set_cloud(ctx, ctx->gicp.src, xyz, n, p, "source");
}

extern "C" int r360_gicp_set_target(r360_ctx* ctx, const float* xyz, size_t n, const r360_gicp_params* p) {
    CHECK_ARG(ctx, "null ctx");
    return set_cloud(ctx, ctx->gicp.tgt, xyz, n, p, "target");
}

extern "C" int r360_gicp_align(r360_ctx* ctx, const float init[16], const r360_gicp_params* p, float pose_out[16],
                               r360_gicp_stats* stats) {
    if (int rc = check_ready(ctx, p, init)) return rc;
    CHECK_ARG(pose_out, "null pose_out");
    if (bind_device(ctx->device)) return -1;
    if (ensure_pass_bufs(ctx)) return -1;
    GicpState& S = ctx->gicp;
    r360_gicp_stats st;
    memset(&st, 0, sizeof st);
    double X[12];
    pose_in(init, X);
    const double gate2 = gate2_of(p);
    int status = 0;
    while (true) {
        if (corr_pass(ctx, X, gate2, 1)) return -1;
        double Y[12], sums[R360_GICP_W];
        memcpy(Y, X, sizeof Y);
        int steps = 0;
        const int rc = gicp_inner([&](const double* y, double* s) { return inner_pass(ctx, y, s); },
                                  [](const double* d, float* E) { r360_exp_se3(d, 0, E); }, p->max_inner_iterations, Y,
                                  sums, &steps);
        if (rc < 0) return rc;
        st.n_corr = (size_t)sums[28];
        st.cost = st.n_corr ? sums[0] / (double)st.n_corr : 0.0;
        if (rc == 1) { status = 1; break; }   // ill-posed: the pose stays at X
        st.inner_steps += steps;
        double dR = 0, dt = 0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) dR = std::max(dR, std::fabs(Y[r * 4 + c] - X[r * 4 + c]));
            dt = std::max(dt, std::fabs(Y[r * 4 + 3] - X[r * 4 + 3]));
        }
        memcpy(X, Y, sizeof X);
        ++st.iterations;
        if (st.iterations >= p->max_iterations) break;
        if (dR < p->rotation_epsilon && dt < p->transformation_epsilon) { st.converged = 1; break; }
    }
    pose_out_f(X, pose_out);
    // getFitnessScore: every source point's nearest target at the final pose, no range limit
    if (corr_pass(ctx, X, INFINITY, 0)) return -1;
    if (launch_gicp_sum(ctx->stream, S.d2.get(), S.src.n, S.partials.get(), S.d_sums.get())) return -1;
    R360_HIP(hipMemcpyAsync(S.h_sums.get(), S.d_sums.get(), sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx_wait(ctx)) return -1;
    st.fitness = S.h_sums.get()[0] / (double)S.src.n;
    if (stats) *stats = st;
    return status;
}

extern "C" int r360_gicp_get_cloud(r360_ctx* ctx, int which, float* xyz, float* cov6, int* knn, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n && (which == 0 || which == 1), "invalid arguments");
    GicpCloud& C = which ? ctx->gicp.tgt : ctx->gicp.src;
    *n = C.n;
    if (C.n == 0 || (!xyz && !cov6 && !knn)) return 0;
    if (cap < C.n) { r360_set_error("gicp: capacity %zu < %zu points", cap, C.n); return -4; }
    if (bind_device(ctx->device)) return -1;
    if (ctx_wait(ctx)) return -1;
    if (xyz) {
        std::vector<float> p4(4 * C.n);
        R360_HIP(hipMemcpy(p4.data(), C.pts.get(), sizeof(float) * 4 * C.n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < C.n; ++i) memcpy(xyz + 3 * i, &p4[4 * i], 12);
    }
    if (cov6) {   // held in double on the device: M_i inverts a sum whose smallest eigenvalue is 2e-3
        std::vector<double> c(6 * C.n);
        R360_HIP(hipMemcpy(c.data(), C.cov6.get(), sizeof(double) * 6 * C.n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 6 * C.n; ++i) cov6[i] = (float)c[i];
    }
    if (knn) R360_HIP(hipMemcpy(knn, C.knn.get(), sizeof(int) * C.n * (size_t)C.k, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int r360_gicp_eval(r360_ctx* ctx, const float pose[16], const r360_gicp_params* p, int* corr, double* cost,
                              double H[36], double g[6], size_t* n_corr) {
    if (int rc = check_ready(ctx, p, pose)) return rc;
    if (bind_device(ctx->device)) return -1;
    if (ensure_pass_bufs(ctx)) return -1;
    GicpState& S = ctx->gicp;
    double X[12], sums[R360_GICP_W];
    pose_in(pose, X);
    if (corr_pass(ctx, X, gate2_of(p), 1)) return -1;
    if (inner_pass(ctx, X, sums)) return -1;
    if (corr) R360_HIP(hipMemcpy(corr, S.corr.get(), sizeof(int) * S.src.n, hipMemcpyDeviceToHost));
    if (cost) *cost = sums[0];
    if (g) memcpy(g, sums + 1, sizeof(double) * 6);
    if (H) gicp_unpack_H(sums, H);
    if (n_corr) *n_corr = (size_t)sums[28];
    return 0;
}
