// pgo.cpp — pose-graph optimisation on the context's GPU: r360_graph_* (include/rgbd360_hip.h).  Kernels:
// kernels/pgo_kernels.hip; statement and design: tests/pgo_model.py, DESIGN.md §5d.  The graph lives on the host; an
// optimise call checks it, builds the block structure (the distinct block columns per free vertex, the by-vertex list
// of (edge, side) entries in edge order), uploads everything and runs Levenberg-Marquardt: the damping, accept /
// reject and stop decisions here, from one small read-back per trial, everything else on the device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "../r360_internal.h"

struct r360_graph {
    r360_ctx* ctx = nullptr;
    int device = 0;               // the context's, kept so that destroying the graph never reads the context
    std::vector<double> poses;    // [n][16] column-major, as given
    std::vector<char> fixed;
    std::vector<int> ij;          // [m][2]
    std::vector<double> Z;        // [m][16] column-major
    std::vector<double> Om;       // [m][36] symmetrised
    // device
    PgoDev D;
    size_t cap_n = 0, cap_m = 0, cap_nf = 0, cap_ent = 0, cap_nnzb = 0;
    double* pose[2] = {nullptr, nullptr};   // [n][12] row-major 3x4: the current and the trial poses
    double* delta = nullptr;                // [6 nf]
    double* vec = nullptr;                  // multi-launch PCG: x, r, z, q, p0, p1
    double* partials = nullptr;             // max(R360_PGO_MAXB, 3 * PCG workgroups)
    size_t cap_part = 0;
    PgoOut* d_out = nullptr;
    PgoOut* h_out = nullptr;                // pinned
    PgoCgState* d_cg = nullptr;
    PgoCgState* h_cg = nullptr;             // pinned
};

namespace {

constexpr int MAX_VERTICES = 1 << 20;

template <class T>
int grow(r360_ctx* ctx, T*& p, size_t have, size_t need) {
    if (need <= have && p) return 0;
    if (p) {
        if (ctx_wait(ctx)) return -1;
        R360_HIP(hipFree(p));
        p = nullptr;
    }
    R360_HIP(hipMalloc(&p, sizeof(T) * std::max<size_t>(need, 1)));
    return 0;
}

bool finite_n(const double* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// column-major 4x4 -> row-major 3x4
void pose12(const double* T, double* P) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) P[r * 4 + c] = T[c * 4 + r];
}

struct Structure {
    std::vector<int> fidx, vfree, vptr, ventry, vblk, rowptr, colidx, diag;
};

// the graph-level checks (a free vertex with no edge; a connected component with no fixed vertex: union-find over the
// edges) and the block structure
int build_structure(const r360_graph* g, Structure& S) {
    const int n = (int)g->fixed.size(), m = (int)(g->ij.size() / 2);
    std::vector<int> parent(n), deg(n, 0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int a) {
        while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
        return a;
    };
    for (int e = 0; e < m; ++e) {
        const int i = g->ij[2 * e], j = g->ij[2 * e + 1];
        ++deg[i]; ++deg[j];
        parent[find(i)] = find(j);
    }
    std::vector<char> anchored(n, 0);
    for (int v = 0; v < n; ++v)
        if (g->fixed[v]) anchored[find(v)] = 1;
    for (int v = 0; v < n; ++v) {
        if (!g->fixed[v] && deg[v] == 0) { r360_set_error("graph: the free vertex %d has no edge", v); return R360_EINVAL; }
        if (!anchored[find(v)]) { r360_set_error("graph: the connected component of vertex %d has no fixed vertex", v); return R360_EINVAL; }
    }
    S.fidx.assign(n, -1);
    S.vfree.clear();
    for (int v = 0; v < n; ++v)
        if (!g->fixed[v]) { S.fidx[v] = (int)S.vfree.size(); S.vfree.push_back(v); }
    const int nf = (int)S.vfree.size();
    // by-vertex entries in edge order (a counting sort keeps it)
    S.vptr.assign(nf + 1, 0);
    for (int e = 0; e < m; ++e)
        for (int s = 0; s < 2; ++s) {
            const int k = S.fidx[g->ij[2 * e + s]];
            if (k >= 0) ++S.vptr[k + 1];
        }
    for (int k = 0; k < nf; ++k) S.vptr[k + 1] += S.vptr[k];
    S.ventry.assign(S.vptr[nf], 0);
    S.vblk.assign(S.vptr[nf], -1);
    std::vector<int> at(S.vptr.begin(), S.vptr.end() - 1);
    for (int e = 0; e < m; ++e)
        for (int s = 0; s < 2; ++s) {
            const int k = S.fidx[g->ij[2 * e + s]];
            if (k >= 0) S.ventry[at[k]++] = e * 2 + s;
        }
    // distinct block columns per row, ascending, the diagonal among them
    S.rowptr.assign(nf + 1, 0);
    S.colidx.clear();
    S.diag.assign(nf, 0);
    std::vector<int> cols;
    for (int k = 0; k < nf; ++k) {
        cols.assign(1, k);
        for (int q = S.vptr[k]; q < S.vptr[k + 1]; ++q) {
            const int ent = S.ventry[q];
            const int o = S.fidx[g->ij[2 * (ent >> 1) + (1 - (ent & 1))]];
            if (o >= 0) cols.push_back(o);
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        const int base = (int)S.colidx.size();
        for (int q = S.vptr[k]; q < S.vptr[k + 1]; ++q) {
            const int ent = S.ventry[q];
            const int o = S.fidx[g->ij[2 * (ent >> 1) + (1 - (ent & 1))]];
            if (o >= 0) S.vblk[q] = base + (int)(std::lower_bound(cols.begin(), cols.end(), o) - cols.begin());
        }
        S.diag[k] = base + (int)(std::lower_bound(cols.begin(), cols.end(), k) - cols.begin());
        S.colidx.insert(S.colidx.end(), cols.begin(), cols.end());
        S.rowptr[k + 1] = (int)S.colidx.size();
    }
    return 0;
}

template <class T>
int upload(hipStream_t st, T* dst, const std::vector<T>& src) {
    if (src.empty()) return 0;
    R360_HIP(hipMemcpyAsync(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, st));
    return 0;
}

// checks, structure, buffers, upload; the current poses land in g->pose[0].  The host vectors of this call live
// until its ctx_wait.
int prepare(r360_graph* g) {
    const int n = (int)g->fixed.size(), m = (int)(g->ij.size() / 2);
    CHECK_ARG(n >= 1, "graph: no vertex");
    Structure S;
    if (int rc = build_structure(g, S)) return rc;
    r360_ctx* ctx = g->ctx;
    if (bind_device(ctx->device)) return -1;
    const int nf = (int)S.vfree.size(), nnzb = (int)S.colidx.size();
    const size_t ent = S.ventry.size();
    PgoDev& D = g->D;
    if ((size_t)n > g->cap_n || !g->pose[0]) {
        if (grow(ctx, g->pose[0], 0, 12 * (size_t)n) || grow(ctx, g->pose[1], 0, 12 * (size_t)n) || grow(ctx, D.fidx, 0, n)) return -1;
        g->cap_n = n;
    }
    if ((size_t)m > g->cap_m || !D.ij) {
        const size_t mm = std::max(m, 1);
        if (grow(ctx, D.ij, 0, mm) || grow(ctx, D.Z, 0, 12 * mm) || grow(ctx, D.Om, 0, 36 * mm) ||
            grow(ctx, D.Hs, 0, R360_PGO_SLOT_H * mm) || grow(ctx, D.bs, 0, R360_PGO_SLOT_B * mm) ||
            grow(ctx, D.lin, 0, R360_PGO_SLOT_LIN * mm) || grow(ctx, D.cost, 0, mm))
            return -1;
        g->cap_m = m;
    }
    if ((size_t)nf > g->cap_nf || !D.vfree) {
        const size_t f = std::max(nf, 1);
        if (grow(ctx, D.vfree, 0, f) || grow(ctx, D.vptr, 0, f + 1) || grow(ctx, D.rowptr, 0, f + 1) || grow(ctx, D.diag, 0, f) ||
            grow(ctx, D.b, 0, 6 * f) || grow(ctx, D.minv, 0, 36 * f) || grow(ctx, g->delta, 0, 6 * f) || grow(ctx, g->vec, 0, 36 * f))
            return -1;
        g->cap_nf = nf;
    }
    if (ent > g->cap_ent || !D.ventry) {
        if (grow(ctx, D.ventry, 0, ent) || grow(ctx, D.vblk, 0, ent)) return -1;
        g->cap_ent = ent;
    }
    if ((size_t)nnzb > g->cap_nnzb || !D.colidx) {
        if (grow(ctx, D.colidx, 0, (size_t)nnzb) || grow(ctx, D.vals, 0, 36 * (size_t)std::max(nnzb, 1))) return -1;
        g->cap_nnzb = nnzb;
    }
    const size_t npart = std::max<size_t>(R360_PGO_MAXB, 3 * (size_t)((6 * nf + R360_PGO_CGM_TPB - 1) / R360_PGO_CGM_TPB));
    if (npart > g->cap_part) {
        if (grow(ctx, g->partials, 0, npart)) return -1;
        g->cap_part = npart;
    }
    D.n = n; D.m = m; D.nf = nf; D.nnzb = nnzb;
    std::vector<double> P(12 * (size_t)n), Z(12 * (size_t)m);
    std::vector<int2> ij(m);
    for (int v = 0; v < n; ++v) pose12(&g->poses[16 * (size_t)v], &P[12 * (size_t)v]);
    for (int e = 0; e < m; ++e) {
        pose12(&g->Z[16 * (size_t)e], &Z[12 * (size_t)e]);
        ij[e] = make_int2(g->ij[2 * e], g->ij[2 * e + 1]);
    }
    hipStream_t st = ctx->stream;
    if (upload(st, g->pose[0], P) || upload(st, D.Z, Z) || upload(st, D.ij, ij) || upload(st, D.Om, g->Om) ||
        upload(st, D.fidx, S.fidx) || upload(st, D.vfree, S.vfree) || upload(st, D.vptr, S.vptr) ||
        upload(st, D.ventry, S.ventry) || upload(st, D.vblk, S.vblk) || upload(st, D.rowptr, S.rowptr) ||
        upload(st, D.colidx, S.colidx) || upload(st, D.diag, S.diag))
        return -1;
    return ctx_wait(ctx);   // the host vectors end here
}

int check_params(const r360_graph_params* p) {
    CHECK_ARG(p->max_iterations >= 1 && p->max_trials >= 1, "graph: max_iterations and max_trials must be at least 1");
    CHECK_ARG(std::isfinite(p->gain_epsilon) && p->gain_epsilon >= 0.0, "graph: gain_epsilon must be finite and not negative");
    CHECK_ARG(std::isfinite(p->cg_tolerance) && p->cg_tolerance >= 0.0, "graph: cg_tolerance must be finite and not negative");
    CHECK_ARG(p->cg_max_iterations >= 0, "graph: negative cg_max_iterations");
    CHECK_ARG(p->cg_form >= 0 && p->cg_form <= 2, "graph: cg_form is 0, 1 or 2");
    return 0;
}

bool fits_one_workgroup(int nf) { return sizeof(double) * 4 * 6 * (size_t)nf <= (size_t)R360_PGO_CG1_LDS; }

int pick_form(const r360_graph_params* p, int nf, int* form) {
    if (p->cg_form == 1 && !fits_one_workgroup(nf)) {
        r360_set_error("graph: cg_form 1 holds at most %d free vertices, the graph has %d", R360_PGO_CG1_LDS / (8 * 4 * 6), nf);
        return R360_EINVAL;
    }
    *form = p->cg_form ? p->cg_form : (fits_one_workgroup(nf) ? 1 : 2);
    return 0;
}

// one damped solve into g->delta (form 2: its x vector); the figures arrive with the next read-back of d_out
int solve(r360_graph* g, int form, double lambda, double tol, int maxit, double** delta) {
    r360_ctx* ctx = g->ctx;
    if (launch_pgo_precond(ctx->stream, g->D, lambda)) return -1;
    if (form == 1) {
        *delta = g->delta;
        return launch_pgo_cg1(ctx->stream, g->D, lambda, tol * tol, maxit, g->delta, g->d_out);
    }
    *delta = g->vec;
    return launch_pgo_cgm(ctx, g->D, lambda, tol * tol, maxit, g->vec, g->partials, g->d_cg, g->h_cg, g->d_out);
}

int read_out(r360_graph* g) {
    R360_HIP(hipMemcpyAsync(g->h_out, g->d_out, sizeof(PgoOut), hipMemcpyDeviceToHost, g->ctx->stream));
    return ctx_wait(g->ctx);
}

int linearise(r360_graph* g, const double* poses) {
    if (launch_pgo_linearise(g->ctx->stream, g->D, poses, false, g->partials, &g->d_out->F)) return -1;
    return launch_pgo_assemble(g->ctx->stream, g->D, g->d_out);
}

}  // namespace

extern "C" int r360_graph_create(r360_ctx* ctx, r360_graph** out) {
    CHECK_ARG(ctx && out, "null arg");
    if (bind_device(ctx->device)) return -1;
    r360_graph* g = new r360_graph;
    g->ctx = ctx;
    g->device = ctx->device;
    if (hipMalloc(&g->d_out, sizeof(PgoOut)) != hipSuccess || hipMalloc(&g->d_cg, sizeof(PgoCgState)) != hipSuccess ||
        hipHostMalloc(&g->h_out, sizeof(PgoOut), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&g->h_cg, sizeof(PgoCgState), hipHostMallocDefault) != hipSuccess ||
        hipMemsetAsync(g->d_out, 0, sizeof(PgoOut), ctx->stream) != hipSuccess) {
        r360_set_error("graph: cannot allocate the read-back buffers");
        r360_graph_destroy(g);
        return -1;
    }
    *out = g;
    return 0;
}

extern "C" void r360_graph_destroy(r360_graph* g) {
    if (!g) return;
    // hipFree waits for the device's work itself; the context is not touched, it may be gone already
    hipSetDevice(g->device);
    PgoDev& D = g->D;
    hipFree(D.ij); hipFree(D.Z); hipFree(D.Om); hipFree(D.vfree); hipFree(D.fidx); hipFree(D.vptr); hipFree(D.ventry);
    hipFree(D.vblk); hipFree(D.rowptr); hipFree(D.colidx); hipFree(D.diag); hipFree(D.Hs); hipFree(D.bs); hipFree(D.lin);
    hipFree(D.cost); hipFree(D.vals); hipFree(D.b); hipFree(D.minv);
    hipFree(g->pose[0]); hipFree(g->pose[1]); hipFree(g->delta); hipFree(g->vec); hipFree(g->partials);
    hipFree(g->d_out); hipFree(g->d_cg);
    hipHostFree(g->h_out); hipHostFree(g->h_cg);
    delete g;
}

extern "C" int r360_graph_add_vertex(r360_graph* g, const double pose[16], int* id) {
    CHECK_ARG(g && pose, "null arg");
    CHECK_ARG(finite_n(pose, 16), "graph: non-finite pose");
    CHECK_ARG((int)g->fixed.size() < MAX_VERTICES, "graph: too many vertices");
    g->poses.insert(g->poses.end(), pose, pose + 16);
    g->fixed.push_back(g->fixed.empty() ? 1 : 0);
    if (id) *id = (int)g->fixed.size() - 1;
    return 0;
}

extern "C" int r360_graph_set_fixed(r360_graph* g, int id, int fixed) {
    CHECK_ARG(g, "null arg");
    CHECK_ARG(id >= 0 && id < (int)g->fixed.size(), "graph: no such vertex");
    CHECK_ARG(id != 0 || fixed, "graph: vertex 0 is always fixed");
    g->fixed[id] = fixed ? 1 : 0;
    return 0;
}

extern "C" int r360_graph_set_pose(r360_graph* g, int id, const double pose[16]) {
    CHECK_ARG(g && pose, "null arg");
    CHECK_ARG(id >= 0 && id < (int)g->fixed.size(), "graph: no such vertex");
    CHECK_ARG(finite_n(pose, 16), "graph: non-finite pose");
    memcpy(&g->poses[16 * (size_t)id], pose, sizeof(double) * 16);
    return 0;
}

extern "C" int r360_graph_add_edge(r360_graph* g, int from, int to, const double rel[16], const double info[36]) {
    CHECK_ARG(g && rel && info, "null arg");
    const int n = (int)g->fixed.size();
    CHECK_ARG(from >= 0 && to >= 0 && from < n && to < n, "graph: the edge names a missing vertex");
    CHECK_ARG(from != to, "graph: an edge joins a vertex to itself");
    CHECK_ARG(finite_n(rel, 16), "graph: non-finite relative pose");
    CHECK_ARG(finite_n(info, 36), "graph: non-finite information matrix");
    g->ij.push_back(from);
    g->ij.push_back(to);
    g->Z.insert(g->Z.end(), rel, rel + 16);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) g->Om.push_back((info[r * 6 + c] + info[c * 6 + r]) / 2);
    return 0;
}

extern "C" int r360_graph_size(const r360_graph* g, int* n_vertices, int* n_edges) {
    CHECK_ARG(g, "null arg");
    if (n_vertices) *n_vertices = (int)g->fixed.size();
    if (n_edges) *n_edges = (int)(g->ij.size() / 2);
    return 0;
}

extern "C" int r360_graph_get_poses(const r360_graph* g, double* poses, int cap, int* n) {
    CHECK_ARG(g && n, "null arg");
    *n = (int)g->fixed.size();
    if (!poses) return 0;
    if (cap < *n) { r360_set_error("graph: capacity %d < %d vertices", cap, *n); return -4; }
    memcpy(poses, g->poses.data(), sizeof(double) * g->poses.size());
    return 0;
}

extern "C" void r360_graph_default_params(r360_graph_params* p) {
    if (!p) return;
    p->max_iterations = 10;
    p->max_trials = 10;
    p->gain_epsilon = 1e-6;
    p->cg_tolerance = 1e-12;
    p->cg_max_iterations = 0;
    p->cg_form = 0;
}

extern "C" int r360_graph_optimize(r360_graph* g, const r360_graph_params* params, r360_graph_stats* stats) {
    CHECK_ARG(g, "null arg");
    r360_graph_params p;
    r360_graph_default_params(&p);
    if (params) p = *params;
    if (int rc = check_params(&p)) return rc;
    r360_graph_stats st;
    memset(&st, 0, sizeof st);
    const int m = (int)(g->ij.size() / 2);
    int nfree = 0;
    for (char f : g->fixed) nfree += f ? 0 : 1;
    if (nfree == 0 || m == 0) {   // nothing to move (a free vertex without an edge is caught below)
        Structure S;
        if (int rc = build_structure(g, S)) return rc;
        if (stats) *stats = st;
        return 0;
    }
    int form = 0;
    if (int rc = pick_form(&p, nfree, &form)) return rc;
    if (int rc = prepare(g)) return rc;
    r360_ctx* ctx = g->ctx;
    const PgoDev& D = g->D;
    const int cg_max = p.cg_max_iterations > 0 ? p.cg_max_iterations : 12 * D.nf;
    int cur = 0;
    if (linearise(g, g->pose[cur]) || read_out(g)) return -1;
    double F = g->h_out->F;
    st.F_initial = st.F_final = F;
    double lambda = 1e-5 * g->h_out->maxdiag, nu = 2.0;
    st.lambda = lambda;
    if (F == 0.0 || g->h_out->maxb == 0.0) {
        if (stats) *stats = st;
        return 0;
    }
    st.cg_form = form;
    bool stop = false;
    for (int it = 0; it < p.max_iterations && !stop; ++it) {
        bool accepted = false;
        double F1 = F;
        for (int trial = 0; trial < p.max_trials; ++trial) {
            double* delta = nullptr;
            if (int rc = solve(g, form, lambda, p.cg_tolerance, cg_max, &delta)) return rc;
            if (launch_pgo_update(ctx->stream, D, g->pose[cur], delta, lambda, g->pose[1 - cur], g->d_out)) return -1;
            if (launch_pgo_linearise(ctx->stream, D, g->pose[1 - cur], true, g->partials, &g->d_out->F)) return -1;
            if (read_out(g)) return -1;
            ++st.trials;
            st.cg_iterations += g->h_out->cg_iters;
            st.cg_iterations_max = std::max(st.cg_iterations_max, g->h_out->cg_iters);
            if (!g->h_out->cg_done) {
                st.status = R360_GRAPH_CG_NOT_CONVERGED;
                stop = true;
                break;
            }
            F1 = g->h_out->F;
            const double rho = (F - F1) / g->h_out->pred;
            if (std::isfinite(F1) && rho > 0.0) {
                const double c = 2.0 * rho - 1.0;
                lambda *= std::max(1.0 / 3.0, 1.0 - c * c * c);
                nu = 2.0;
                accepted = true;
                break;
            }
            lambda *= nu;
            nu *= 2.0;
        }
        st.lambda = lambda;
        if (stop) break;
        if (!accepted) {
            st.status = R360_GRAPH_STALLED;
            break;
        }
        ++st.iterations;
        const double gain = F - F1, Fold = F;
        cur = 1 - cur;
        F = F1;
        st.F_final = F;
        if (gain <= p.gain_epsilon * Fold) {
            st.status = R360_GRAPH_CONVERGED;
            break;
        }
        if (it == p.max_iterations - 1) {
            st.status = R360_GRAPH_ITERATION_LIMIT;
            break;
        }
        if (linearise(g, g->pose[cur])) return -1;
    }
    if (st.iterations > 0) {   // the free vertices' new poses; the others keep their bytes
        std::vector<double> P(12 * (size_t)D.n);
        if (ctx_wait(ctx)) return -1;
        R360_HIP(hipMemcpy(P.data(), g->pose[cur], sizeof(double) * P.size(), hipMemcpyDeviceToHost));
        for (int v = 0; v < D.n; ++v) {
            if (g->fixed[v]) continue;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) g->poses[16 * (size_t)v + c * 4 + r] = P[12 * (size_t)v + r * 4 + c];
        }
    }
    if (stats) *stats = st;
    return 0;
}

extern "C" int r360_graph_eval(r360_graph* g, double* F, double* b, double* H, int cap, int* n_unknowns) {
    CHECK_ARG(g && n_unknowns, "null arg");
    CHECK_ARG(g->fixed.size() <= 1024, "graph: the parity hooks take at most 1024 vertices");
    int nfree = 0;
    for (char f : g->fixed) nfree += f ? 0 : 1;
    const int N = 6 * nfree;
    *n_unknowns = N;
    if (!F && !b && !H) return 0;
    if ((b || H) && cap < N) { r360_set_error("graph: capacity %d < %d unknowns", cap, N); return -4; }
    if (int rc = prepare(g)) return rc;
    const PgoDev& D = g->D;
    if (linearise(g, g->pose[0]) || read_out(g)) return -1;
    if (F) *F = g->h_out->F;
    if (b && N) R360_HIP(hipMemcpy(b, D.b, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (H && N) {
        std::vector<int> rowptr(D.nf + 1), colidx(D.nnzb);
        std::vector<double> vals(36 * (size_t)D.nnzb);
        R360_HIP(hipMemcpy(rowptr.data(), D.rowptr, sizeof(int) * rowptr.size(), hipMemcpyDeviceToHost));
        R360_HIP(hipMemcpy(colidx.data(), D.colidx, sizeof(int) * colidx.size(), hipMemcpyDeviceToHost));
        R360_HIP(hipMemcpy(vals.data(), D.vals, sizeof(double) * vals.size(), hipMemcpyDeviceToHost));
        std::fill(H, H + (size_t)N * N, 0.0);
        for (int k = 0; k < D.nf; ++k)
            for (int q = rowptr[k]; q < rowptr[k + 1]; ++q)
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c)
                        H[(size_t)(6 * k + r) * N + 6 * colidx[q] + c] = vals[36 * (size_t)q + r * 6 + c];
    }
    return 0;
}

extern "C" int r360_graph_solve(r360_graph* g, const r360_graph_params* params, double lambda, double* delta, int cap,
                                int* n_unknowns, int* iterations, double* rel_residual, int* form_out) {
    CHECK_ARG(g && n_unknowns, "null arg");
    CHECK_ARG(g->fixed.size() <= 1024, "graph: the parity hooks take at most 1024 vertices");
    CHECK_ARG(std::isfinite(lambda) && lambda >= 0.0, "graph: lambda must be finite and not negative");
    r360_graph_params p;
    r360_graph_default_params(&p);
    if (params) p = *params;
    if (int rc = check_params(&p)) return rc;
    int nfree = 0;
    for (char f : g->fixed) nfree += f ? 0 : 1;
    const int N = 6 * nfree;
    *n_unknowns = N;
    if (!delta) return 0;
    if (cap < N) { r360_set_error("graph: capacity %d < %d unknowns", cap, N); return -4; }
    CHECK_ARG(N > 0, "graph: no free vertex");
    int form = 0;
    if (int rc = pick_form(&p, nfree, &form)) return rc;
    if (int rc = prepare(g)) return rc;
    if (linearise(g, g->pose[0])) return -1;
    double* d = nullptr;
    const int cg_max = p.cg_max_iterations > 0 ? p.cg_max_iterations : 12 * nfree;
    if (int rc = solve(g, form, lambda, p.cg_tolerance, cg_max, &d)) return rc;
    if (read_out(g)) return -1;
    R360_HIP(hipMemcpy(delta, d, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (iterations) *iterations = g->h_out->cg_iters;
    if (rel_residual) *rel_residual = g->h_out->bb > 0.0 ? std::sqrt(g->h_out->rr / g->h_out->bb) : 0.0;
    if (form_out) *form_out = form;
    return g->h_out->cg_done ? 0 : 1;
}

extern "C" int r360_graph_save(const r360_graph* g, const char* path) {
    CHECK_ARG(g && path, "null arg");
    std::vector<int> fixed(g->fixed.begin(), g->fixed.end());
    return r360_g2o_write(path, (int)g->fixed.size(), g->poses.data(), fixed.data(), (int)(g->ij.size() / 2), g->ij.data(),
                          g->Z.data(), g->Om.data());
}

extern "C" int r360_graph_load(r360_graph* g, const char* path) {
    CHECK_ARG(g && path, "null arg");
    int nv = 0, ne = 0;
    if (int rc = r360_g2o_read(path, nullptr, nullptr, 0, &nv, nullptr, nullptr, nullptr, 0, &ne)) return rc;
    std::vector<double> poses(16 * (size_t)nv), Z(16 * (size_t)ne), Om(36 * (size_t)ne);
    std::vector<int> fixed(nv), ij(2 * (size_t)ne);
    if (int rc = r360_g2o_read(path, poses.data(), fixed.data(), nv, &nv, ij.data(), Z.data(), Om.data(), ne, &ne)) return rc;
    for (int e = 0; e < ne; ++e) CHECK_ARG(ij[2 * e] != ij[2 * e + 1], "graph: an edge of the file joins a vertex to itself");
    g->poses = poses;
    g->fixed.assign(nv, 0);
    for (int v = 0; v < nv; ++v) g->fixed[v] = (fixed[v] || v == 0) ? 1 : 0;
    g->ij = ij;
    g->Z = Z;
    g->Om = Om;
    return 0;
}
