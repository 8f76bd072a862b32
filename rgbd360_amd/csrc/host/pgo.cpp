// pgo.cpp — pose-graph optimisation on the context's GPU: r360_graph_* (include/rgbd360_hip.h).  Kernels:
// kernels/pgo_kernels.hip; statement and design: tests/pgo_model.py, DESIGN.md §5d.  The graph lives on the host; an
// optimise call checks it, builds the block structure (the distinct block columns per free vertex, the by-vertex list
// of (edge, side) entries in edge order), uploads everything and runs Levenberg-Marquardt: the damping, accept /
// reject and stop decisions here, from one small read-back per trial, everything else on the device.  Every edge has
// a robust kernel and an active flag; the device sees the active edges alone, renumbered in edge order, so an
// inactive edge leaves no trace in any sum.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "../r360_internal.h"
#include "devmem.h"

struct r360_graph {
    r360_ctx* ctx = nullptr;
    int device = 0;               // the context's, kept so that destroying the graph never reads the context
    std::vector<double> poses;    // [n][16] column-major, as given
    std::vector<char> fixed;
    std::vector<int> ij;          // [m][2]
    std::vector<double> Z;        // [m][16] column-major
    std::vector<double> Om;       // [m][36] symmetrised
    std::vector<int> kind;        // [m] R360_GRAPH_KERNEL_*
    std::vector<double> kdelta;   // [m] the kernel's width (never read where the kind is NONE)
    std::vector<char> active;     // [m]
    int def_kind = R360_GRAPH_KERNEL_NONE;   // what add_edge and load give an edge
    double def_delta = 1.0;
    // device: the handle owns the buffers (host/devmem.h); D is the view of them the kernels take, refilled by prepare
    struct {
        DevBuf<int2> ij;
        DevBuf<int> kind, vfree, fidx, vptr, ventry, vblk, rowptr, colidx, diag;
        DevBuf<double> Z, Om, kdelta, Hs, bs, lin, cost, chi2, wgt, vals, b, minv;
    } own;
    PgoDev D;
    DevBuf<double> pose[2];                 // [n][12] row-major 3x4: the current and the trial poses
    DevBuf<double> delta;                   // [6 nf]
    DevBuf<double> vec;                     // multi-launch PCG: x, r, z, q, p0, p1
    DevBuf<double> partials;                // max(R360_PGO_MAXB, 3 * PCG workgroups)
    DevBuf<PgoOut> d_out;
    PinnedBuf<PgoOut> h_out;
    DevBuf<PgoCgState> d_cg;
    PinnedBuf<PgoCgState> h_cg;
};

namespace {

constexpr int MAX_VERTICES = 1 << 20;

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

// the active edges, in edge order
std::vector<int> active_edges(const r360_graph* g) {
    std::vector<int> sel;
    for (int e = 0; e < (int)g->active.size(); ++e)
        if (g->active[e]) sel.push_back(e);
    return sel;
}

// the graph-level checks (a free vertex with no edge; a connected component with no fixed vertex: union-find over the
// edges) and the block structure, both over the edges sel alone, numbered by their place in sel
int build_structure(const r360_graph* g, const std::vector<int>& sel, Structure& S) {
    const int n = (int)g->fixed.size(), m = (int)sel.size();
    auto end_of = [&](int e, int s) { return g->ij[2 * (size_t)sel[e] + s]; };
    std::vector<int> parent(n), deg(n, 0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int a) {
        while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
        return a;
    };
    for (int e = 0; e < m; ++e) {
        const int i = end_of(e, 0), j = end_of(e, 1);
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
            const int k = S.fidx[end_of(e, s)];
            if (k >= 0) ++S.vptr[k + 1];
        }
    for (int k = 0; k < nf; ++k) S.vptr[k + 1] += S.vptr[k];
    S.ventry.assign(S.vptr[nf], 0);
    S.vblk.assign(S.vptr[nf], -1);
    std::vector<int> at(S.vptr.begin(), S.vptr.end() - 1);
    for (int e = 0; e < m; ++e)
        for (int s = 0; s < 2; ++s) {
            const int k = S.fidx[end_of(e, s)];
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
            const int o = S.fidx[end_of(ent >> 1, 1 - (ent & 1))];
            if (o >= 0) cols.push_back(o);
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        const int base = (int)S.colidx.size();
        for (int q = S.vptr[k]; q < S.vptr[k + 1]; ++q) {
            const int ent = S.ventry[q];
            const int o = S.fidx[end_of(ent >> 1, 1 - (ent & 1))];
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

// the host copies of one upload of poses and edges; they live until the ctx_wait after it
struct Staged {
    std::vector<double> P, Z, Om, kdelta;
    std::vector<int2> ij;
    std::vector<int> kind;
};

// The current poses into g->pose[0] and the edges sel, in that order, with their kernels into the per-edge arrays
// of g->D (D.n and D.m set): all that the cost-only linearisation reads.  No wait: the caller's is the one.
int stage_edges(r360_graph* g, const std::vector<int>& sel, Staged& H) {
    const int n = (int)g->fixed.size(), m = (int)sel.size();
    r360_ctx* ctx = g->ctx;
    auto& O = g->own;
    const size_t mm = std::max(m, 1);
    if (g->pose[0].reserve(ctx, 12 * (size_t)n) || O.ij.reserve(ctx, mm) || O.Z.reserve(ctx, 12 * mm) ||
        O.Om.reserve(ctx, 36 * mm) || O.kind.reserve(ctx, mm) || O.kdelta.reserve(ctx, mm) || O.cost.reserve(ctx, mm) ||
        O.chi2.reserve(ctx, mm) || O.wgt.reserve(ctx, mm) || g->partials.reserve(ctx, R360_PGO_MAXB))
        return -1;
    PgoDev& D = g->D;
    D.n = n; D.m = m;
    D.ij = O.ij.get(); D.Z = O.Z.get(); D.Om = O.Om.get(); D.kind = O.kind.get(); D.kdelta = O.kdelta.get();
    D.cost = O.cost.get(); D.chi2 = O.chi2.get(); D.wgt = O.wgt.get();
    H.P.resize(12 * (size_t)n);
    H.Z.resize(12 * (size_t)m);
    H.ij.resize(m);
    H.kind.resize(m);
    H.kdelta.resize(m);
    const bool all = m == (int)g->active.size();   // then sel is 0 .. m - 1 and Omega goes up from where it lies
    if (!all) H.Om.resize(36 * (size_t)m);
    for (int v = 0; v < n; ++v) pose12(&g->poses[16 * (size_t)v], &H.P[12 * (size_t)v]);
    for (int k = 0; k < m; ++k) {
        const size_t e = (size_t)sel[k];
        pose12(&g->Z[16 * e], &H.Z[12 * (size_t)k]);
        H.ij[k] = make_int2(g->ij[2 * e], g->ij[2 * e + 1]);
        H.kind[k] = g->kind[e];
        H.kdelta[k] = g->kdelta[e];
        if (!all) memcpy(&H.Om[36 * (size_t)k], &g->Om[36 * e], sizeof(double) * 36);
    }
    hipStream_t st = ctx->stream;
    if (upload(st, g->pose[0].get(), H.P) || upload(st, D.Z, H.Z) || upload(st, D.ij, H.ij) ||
        upload(st, D.Om, all ? g->Om : H.Om) || upload(st, D.kind, H.kind) || upload(st, D.kdelta, H.kdelta))
        return -1;
    return 0;
}

// checks, structure, buffers, upload, all over the active edges; the current poses land in g->pose[0].  The host
// vectors of this call live until its ctx_wait.
int prepare(r360_graph* g) {
    const int n = (int)g->fixed.size();
    CHECK_ARG(n >= 1, "graph: no vertex");
    const std::vector<int> sel = active_edges(g);
    const int m = (int)sel.size();
    Structure S;
    if (int rc = build_structure(g, sel, S)) return rc;
    r360_ctx* ctx = g->ctx;
    if (bind_device(ctx->device)) return -1;
    const int nf = (int)S.vfree.size(), nnzb = (int)S.colidx.size();
    const size_t ent = S.ventry.size();
    auto& O = g->own;
    const size_t mm = std::max(m, 1), f = std::max(nf, 1), e1 = std::max<size_t>(ent, 1), nz = std::max(nnzb, 1);
    const size_t npart = std::max<size_t>(R360_PGO_MAXB, 3 * (size_t)((6 * nf + R360_PGO_CGM_TPB - 1) / R360_PGO_CGM_TPB));
    if (g->pose[1].reserve(ctx, 12 * (size_t)n) || O.fidx.reserve(ctx, n) ||
        O.Hs.reserve(ctx, R360_PGO_SLOT_H * mm) || O.bs.reserve(ctx, R360_PGO_SLOT_B * mm) ||
        O.lin.reserve(ctx, R360_PGO_SLOT_LIN * mm) ||
        O.vfree.reserve(ctx, f) || O.vptr.reserve(ctx, f + 1) || O.rowptr.reserve(ctx, f + 1) || O.diag.reserve(ctx, f) ||
        O.b.reserve(ctx, 6 * f) || O.minv.reserve(ctx, 36 * f) || g->delta.reserve(ctx, 6 * f) || g->vec.reserve(ctx, 36 * f) ||
        O.ventry.reserve(ctx, e1) || O.vblk.reserve(ctx, e1) || O.colidx.reserve(ctx, nz) || O.vals.reserve(ctx, 36 * nz) ||
        g->partials.reserve(ctx, npart))
        return -1;
    Staged H;
    if (stage_edges(g, sel, H)) return -1;
    PgoDev& D = g->D;
    D.nf = nf; D.nnzb = nnzb;
    D.vfree = O.vfree.get(); D.fidx = O.fidx.get();
    D.vptr = O.vptr.get(); D.ventry = O.ventry.get(); D.vblk = O.vblk.get(); D.rowptr = O.rowptr.get();
    D.colidx = O.colidx.get(); D.diag = O.diag.get(); D.Hs = O.Hs.get(); D.bs = O.bs.get(); D.lin = O.lin.get();
    D.vals = O.vals.get(); D.b = O.b.get(); D.minv = O.minv.get();
    hipStream_t st = ctx->stream;
    if (upload(st, D.fidx, S.fidx) || upload(st, D.vfree, S.vfree) || upload(st, D.vptr, S.vptr) ||
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
        *delta = g->delta.get();
        return launch_pgo_cg1(ctx->stream, g->D, lambda, tol * tol, maxit, g->delta.get(), g->d_out.get());
    }
    *delta = g->vec.get();
    return launch_pgo_cgm(ctx, g->D, lambda, tol * tol, maxit, g->vec.get(), g->partials.get(), g->d_cg.get(), g->h_cg.get(),
                          g->d_out.get());
}

int read_out(r360_graph* g) {
    R360_HIP(hipMemcpyAsync(g->h_out.get(), g->d_out.get(), sizeof(PgoOut), hipMemcpyDeviceToHost, g->ctx->stream));
    return ctx_wait(g->ctx);
}

int linearise(r360_graph* g, const double* poses) {
    if (launch_pgo_linearise(g->ctx->stream, g->D, poses, false, g->partials.get(), &g->d_out.get()->F)) return -1;
    return launch_pgo_assemble(g->ctx->stream, g->D, g->d_out.get());
}

}  // namespace

extern "C" int r360_graph_create(r360_ctx* ctx, r360_graph** out) {
    CHECK_ARG(ctx && out, "null arg");
    if (bind_device(ctx->device)) return -1;
    std::unique_ptr<r360_graph> g(new r360_graph);
    g->ctx = ctx;
    g->device = ctx->device;
    if (g->d_out.reserve_zeroed(ctx, 1, ctx->stream) || g->d_cg.reserve(ctx, 1) || g->h_out.reserve(ctx, 1) ||
        g->h_cg.reserve(ctx, 1))
        return -1;
    *out = g.release();
    return 0;
}

extern "C" void r360_graph_destroy(r360_graph* g) {
    if (!g) return;
    // hipFree waits for the device's work itself; the context is not touched, it may be gone already
    hipSetDevice(g->device);
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
    g->kind.push_back(g->def_kind);
    g->kdelta.push_back(g->def_delta);
    g->active.push_back(1);
    return 0;
}

namespace {
int check_kernel(int kind, double delta) {
    CHECK_ARG(kind == R360_GRAPH_KERNEL_NONE || kind == R360_GRAPH_KERNEL_HUBER || kind == R360_GRAPH_KERNEL_CAUCHY,
              "graph: the robust kernel is R360_GRAPH_KERNEL_NONE, _HUBER or _CAUCHY");
    CHECK_ARG(std::isfinite(delta) && delta > 0.0, "graph: the robust kernel's delta must be finite and positive");
    return 0;
}
}  // namespace

extern "C" int r360_graph_set_default_kernel(r360_graph* g, int kind, double delta) {
    CHECK_ARG(g, "null arg");
    if (int rc = check_kernel(kind, delta)) return rc;
    g->def_kind = kind;
    g->def_delta = delta;
    return 0;
}

extern "C" int r360_graph_set_edge_kernel(r360_graph* g, int edge, int kind, double delta) {
    CHECK_ARG(g, "null arg");
    CHECK_ARG(edge >= 0 && edge < (int)g->active.size(), "graph: no such edge");
    if (int rc = check_kernel(kind, delta)) return rc;
    g->kind[edge] = kind;
    g->kdelta[edge] = delta;
    return 0;
}

extern "C" int r360_graph_get_edge_kernel(const r360_graph* g, int edge, int* kind, double* delta) {
    CHECK_ARG(g, "null arg");
    CHECK_ARG(edge >= 0 && edge < (int)g->active.size(), "graph: no such edge");
    if (kind) *kind = g->kind[edge];
    if (delta) *delta = g->kdelta[edge];
    return 0;
}

extern "C" int r360_graph_set_edge_active(r360_graph* g, int edge, int active) {
    CHECK_ARG(g, "null arg");
    CHECK_ARG(edge >= 0 && edge < (int)g->active.size(), "graph: no such edge");
    g->active[edge] = active ? 1 : 0;
    return 0;
}

extern "C" int r360_graph_get_edge_active(const r360_graph* g, int edge, int* active) {
    CHECK_ARG(g, "null arg");
    CHECK_ARG(edge >= 0 && edge < (int)g->active.size(), "graph: no such edge");
    if (active) *active = g->active[edge];
    return 0;
}

extern "C" int r360_graph_edge_stats(r360_graph* g, double* chi2, double* weight, int cap, int* n) {
    CHECK_ARG(g && n, "null arg");
    const int m = (int)g->active.size();
    *n = m;
    if ((!chi2 && !weight) || m == 0) return 0;
    if (cap < m) { r360_set_error("graph: capacity %d < %d edges", cap, m); return -4; }
    if (bind_device(g->ctx->device)) return -1;
    std::vector<int> sel(m);
    std::iota(sel.begin(), sel.end(), 0);   // every edge, the inactive ones too: they report their chi2
    Staged H;
    if (stage_edges(g, sel, H)) return -1;
    if (launch_pgo_linearise(g->ctx->stream, g->D, g->pose[0].get(), true, g->partials.get(), &g->d_out.get()->F)) return -1;
    if (ctx_wait(g->ctx)) return -1;
    if (chi2) R360_HIP(hipMemcpy(chi2, g->D.chi2, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (weight) {
        R360_HIP(hipMemcpy(weight, g->D.wgt, sizeof(double) * m, hipMemcpyDeviceToHost));
        for (int e = 0; e < m; ++e)
            if (!g->active[e]) weight[e] = 0.0;
    }
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
    const std::vector<int> sel = active_edges(g);
    int nfree = 0;
    for (char f : g->fixed) nfree += f ? 0 : 1;
    if (nfree == 0 || sel.empty()) {   // nothing to move (a free vertex without an edge is caught below)
        Structure S;
        if (int rc = build_structure(g, sel, S)) return rc;
        if (stats) *stats = st;
        return 0;
    }
    int form = 0;
    if (int rc = pick_form(&p, nfree, &form)) return rc;
    if (int rc = prepare(g)) return rc;
    r360_ctx* ctx = g->ctx;
    const PgoDev& D = g->D;
    const PgoOut& out = *g->h_out.get();   // pinned: what the last read_out brought back
    const int cg_max = p.cg_max_iterations > 0 ? p.cg_max_iterations : 12 * D.nf;
    int cur = 0;
    if (linearise(g, g->pose[cur].get()) || read_out(g)) return -1;
    double F = out.F;
    st.F_initial = st.F_final = F;
    double lambda = 1e-5 * out.maxdiag, nu = 2.0;
    st.lambda = lambda;
    if (F == 0.0 || out.maxb == 0.0) {
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
            if (launch_pgo_update(ctx->stream, D, g->pose[cur].get(), delta, lambda, g->pose[1 - cur].get(), g->d_out.get()))
                return -1;
            if (launch_pgo_linearise(ctx->stream, D, g->pose[1 - cur].get(), true, g->partials.get(), &g->d_out.get()->F))
                return -1;
            if (read_out(g)) return -1;
            ++st.trials;
            st.cg_iterations += out.cg_iters;
            st.cg_iterations_max = std::max(st.cg_iterations_max, out.cg_iters);
            if (!out.cg_done) {
                st.status = R360_GRAPH_CG_NOT_CONVERGED;
                stop = true;
                break;
            }
            F1 = out.F;
            const double rho = (F - F1) / out.pred;
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
        if (linearise(g, g->pose[cur].get())) return -1;
    }
    if (st.iterations > 0) {   // the free vertices' new poses; the others keep their bytes
        std::vector<double> P(12 * (size_t)D.n);
        if (ctx_wait(ctx)) return -1;
        R360_HIP(hipMemcpy(P.data(), g->pose[cur].get(), sizeof(double) * P.size(), hipMemcpyDeviceToHost));
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
    if (linearise(g, g->pose[0].get()) || read_out(g)) return -1;
    if (F) *F = g->h_out.get()->F;
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
    if (linearise(g, g->pose[0].get())) return -1;
    double* d = nullptr;
    const int cg_max = p.cg_max_iterations > 0 ? p.cg_max_iterations : 12 * nfree;
    if (int rc = solve(g, form, lambda, p.cg_tolerance, cg_max, &d)) return rc;
    if (read_out(g)) return -1;
    R360_HIP(hipMemcpy(delta, d, sizeof(double) * N, hipMemcpyDeviceToHost));
    const PgoOut& out = *g->h_out.get();
    if (iterations) *iterations = out.cg_iters;
    if (rel_residual) *rel_residual = out.bb > 0.0 ? std::sqrt(out.rr / out.bb) : 0.0;
    if (form_out) *form_out = form;
    return out.cg_done ? 0 : 1;
}

extern "C" int r360_graph_save(const r360_graph* g, const char* path) {
    CHECK_ARG(g && path, "null arg");
    std::vector<int> fixed(g->fixed.begin(), g->fixed.end());
    const std::vector<int> sel = active_edges(g);
    std::vector<int> ij;
    std::vector<double> Z, Om;
    for (int e : sel) {   // the active edges alone: the file is the graph that gets optimised
        ij.insert(ij.end(), &g->ij[2 * (size_t)e], &g->ij[2 * (size_t)e] + 2);
        Z.insert(Z.end(), &g->Z[16 * (size_t)e], &g->Z[16 * (size_t)e] + 16);
        Om.insert(Om.end(), &g->Om[36 * (size_t)e], &g->Om[36 * (size_t)e] + 36);
    }
    return r360_g2o_write(path, (int)g->fixed.size(), g->poses.data(), fixed.data(), (int)sel.size(), ij.data(), Z.data(),
                          Om.data());
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
    g->kind.assign(ne, g->def_kind);
    g->kdelta.assign(ne, g->def_delta);
    g->active.assign(ne, 1);
    return 0;
}
