// topo.cpp — topological submaps: r360_topo_*, r360_topomap_* and r360_relocalize (include/rgbd360_hip.h).  Kernel:
// kernels/topo_kernels.hip; statement and design: tests/topo_model.py, DESIGN.md §5f.
//
// A partition call checks its matrices, uploads them and launches one workgroup per pending cluster, level by level:
// after each launch the host reads back one integer, the number of clusters the level queued for the next one, and
// stops when it is zero.  Up to R360_TOPO_LDS_MAX_NODES = 96 nodes a cluster's Laplacian and rotation matrix live in
// LDS (2 x 96 x 96 doubles + 14400 B of small arrays = 161856 B of the 163840 a workgroup may declare); from 97 nodes
// on they live in the cluster's slice of the context's scratch (1 MiB per graph, L2 resident).  The labels (the first
// node of every final part) and one record per bisection come back at the end; the host numbers the parts by their
// first node and orders the cuts by their cluster's lowest node, larger clusters first.
//
// The map handle is host bookkeeping: areas, one SSO table, the current area; only its partition() reaches the GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>

#include "../r360_internal.h"

int topo_allow_lds();

namespace {

constexpr int MAXN = R360_TOPO_MAX_NODES;

// every buffer of the context's TopoState (DevBuf / PinnedBuf members, freed with the context) is sized to exactly
// what the call needs, and decides from its own capacity
int reserve(r360_ctx* ctx, int graphs, size_t floats) {
    TopoState& S = ctx->topo;
    if (!S.lds_attr) {
        if (topo_allow_lds()) return -1;
        S.lds_attr = true;
    }
    if (S.count.reserve(ctx, 1) || S.h_count.reserve(ctx, 1) || S.hook_d.reserve(ctx, 2 * MAXN) || S.hook_i.reserve(ctx, MAXN))
        return -1;
    const size_t g = graphs;
    if (S.a_off.reserve(ctx, g) || S.gn.reserve(ctx, g) || S.pending[0].reserve(ctx, g * MAXN) ||
        S.pending[1].reserve(ctx, g * MAXN) || S.idx[0].reserve(ctx, g * MAXN) || S.idx[1].reserve(ctx, g * MAXN) ||
        S.label.reserve(ctx, g * MAXN) || S.rec.reserve(ctx, g * 2 * MAXN) || S.scratch.reserve(ctx, g * 2 * MAXN * MAXN))
        return -1;
    return S.A.reserve(ctx, floats);
}

int check_params(const r360_topo_params* p) {
    CHECK_ARG(!std::isnan(p->threshold_ncut), "topo: threshold_ncut is not a number");
    CHECK_ARG(p->min_cluster >= 1, "topo: min_cluster must be at least 1");
    return 0;
}

int check_matrix(const float* A, int n) {
    CHECK_ARG(A, "topo: null matrix");
    CHECK_ARG(n >= 1, "topo: a graph needs at least one node");
    if (n > MAXN) {
        r360_set_error("topo: %d nodes, at most %d (R360_TOPO_MAX_NODES)", n, MAXN);
        return R360_EINVAL;
    }
    for (int i = 0; i < n; ++i) {
        if (A[(size_t)i * n + i] != 0.0f) { r360_set_error("topo: the diagonal entry %d is not zero", i); return R360_EINVAL; }
        for (int j = i + 1; j < n; ++j) {
            const float a = A[(size_t)i * n + j], b = A[(size_t)j * n + i];
            if (!std::isfinite(a) || !std::isfinite(b)) { r360_set_error("topo: the entry (%d, %d) is not finite", i, j); return R360_EINVAL; }
            if (a < 0.0f || b < 0.0f) { r360_set_error("topo: the entry (%d, %d) is negative", i, j); return R360_EINVAL; }
            if (a != b) { r360_set_error("topo: the entries (%d, %d) and (%d, %d) differ", i, j, j, i); return R360_EINVAL; }
        }
    }
    return 0;
}

struct Hook { int* side; double* eig; double* fiedler; };

// The checked graphs [0, count) of one chunk.  recs: every bisection's record, ordered by graph, then by the cluster's
// lowest node, then larger clusters first (clusters that share their lowest node are nested): an order that does not
// depend on which side of a bisection the eigenvector's sign made side 1.
int run_chunk(r360_ctx* ctx, int count, const float* const* A, const int* n, const r360_topo_params& p, int* const* part_of,
              int* n_parts, std::vector<TopoRecord>* recs, const Hook* hook, bool* not_converged) {
    if (bind_device(ctx->device)) return -1;
    std::vector<long long> a_off(count);
    size_t floats = 0;
    for (int g = 0; g < count; ++g) {
        a_off[g] = (long long)floats;
        floats += (size_t)n[g] * n[g];
    }
    if (reserve(ctx, count, floats)) return -1;
    TopoState& S = ctx->topo;
    hipStream_t st = ctx->stream;
    std::vector<float> packed(floats);
    std::vector<int> idx0((size_t)count * MAXN, 0);
    std::vector<TopoCluster> pend(count);
    for (int g = 0; g < count; ++g) {
        memcpy(&packed[a_off[g]], A[g], sizeof(float) * (size_t)n[g] * n[g]);
        for (int i = 0; i < n[g]; ++i) idx0[(size_t)g * MAXN + i] = i;
        pend[g] = TopoCluster{g, 0, n[g], 0};
    }
    R360_HIP(hipMemcpyAsync(S.A.get(), packed.data(), sizeof(float) * floats, hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(S.a_off.get(), a_off.data(), sizeof(long long) * count, hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(S.gn.get(), n, sizeof(int) * count, hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(S.idx[0].get(), idx0.data(), sizeof(int) * idx0.size(), hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(S.pending[0].get(), pend.data(), sizeof(TopoCluster) * count, hipMemcpyHostToDevice, st));
    TopoArgs a;
    a.A = S.A.get(); a.a_off = S.a_off.get(); a.gn = S.gn.get();
    a.next_count = S.count.get();
    a.label = S.label.get();
    a.scratch = S.scratch.get();
    a.threshold = p.threshold_ncut;
    a.min_cluster = p.min_cluster;
    a.recursive = p.recursive ? 1 : 0;
    int pending = count, done = 0;
    for (int level = 0; pending > 0; ++level) {
        if ((size_t)done + pending > (size_t)count * 2 * MAXN || pending > count * MAXN) {
            r360_set_error("topo: the recursion queued more clusters than a graph has nodes");
            return -1;
        }
        a.pending = S.pending[level & 1].get();
        a.next = S.pending[1 - (level & 1)].get();
        a.idx_in = S.idx[level & 1].get();
        a.idx_out = S.idx[1 - (level & 1)].get();
        a.rec = S.rec.get() + done;
        const bool hooked = hook && level == 0;
        a.eig_out = hooked ? S.hook_d.get() : nullptr;
        a.fiedler_out = hooked ? S.hook_d.get() + MAXN : nullptr;
        a.side_out = hooked ? S.hook_i.get() : nullptr;
        R360_HIP(hipMemsetAsync(S.count.get(), 0, sizeof(int), st));
        if (launch_topo_level(st, a, pending)) return -1;
        R360_HIP(hipMemcpyAsync(S.h_count.get(), S.count.get(), sizeof(int), hipMemcpyDeviceToHost, st));
        if (ctx_wait(ctx)) return -1;   // the level's read-back: the clusters it queued
        done += pending;
        pending = *S.h_count.get();
    }
    std::vector<int> label((size_t)count * MAXN);
    std::vector<TopoRecord> r(done);
    R360_HIP(hipMemcpy(label.data(), S.label.get(), sizeof(int) * label.size(), hipMemcpyDeviceToHost));
    R360_HIP(hipMemcpy(r.data(), S.rec.get(), sizeof(TopoRecord) * done, hipMemcpyDeviceToHost));
    if (hook) {
        if (hook->side) R360_HIP(hipMemcpy(hook->side, S.hook_i.get(), sizeof(int) * n[0], hipMemcpyDeviceToHost));
        if (hook->eig) R360_HIP(hipMemcpy(hook->eig, S.hook_d.get(), sizeof(double) * n[0], hipMemcpyDeviceToHost));
        if (hook->fiedler) R360_HIP(hipMemcpy(hook->fiedler, S.hook_d.get() + MAXN, sizeof(double) * n[0], hipMemcpyDeviceToHost));
    }
    std::sort(r.begin(), r.end(), [](const TopoRecord& x, const TopoRecord& y) {
        if (x.graph != y.graph) return x.graph < y.graph;
        if (x.first != y.first) return x.first < y.first;
        return x.n > y.n;
    });
    for (const TopoRecord& x : r)
        if (x.status) *not_converged = true;
    for (int g = 0; g < count; ++g) {
        // a part's label is its first node: the parts in the order of their labels
        const int* lab = &label[(size_t)g * MAXN];
        std::vector<int> firsts(lab, lab + n[g]);
        std::sort(firsts.begin(), firsts.end());
        firsts.erase(std::unique(firsts.begin(), firsts.end()), firsts.end());
        if (part_of && part_of[g])
            for (int i = 0; i < n[g]; ++i)
                part_of[g][i] = (int)(std::lower_bound(firsts.begin(), firsts.end(), lab[i]) - firsts.begin());
        if (n_parts) n_parts[g] = (int)firsts.size();
    }
    if (recs) *recs = std::move(r);
    return 0;
}

r360_topo_params params_or_default(const r360_topo_params* params) {
    r360_topo_params p;
    r360_topo_default_params(&p);
    if (params) p = *params;
    return p;
}

}  // namespace

extern "C" void r360_topo_default_params(r360_topo_params* p) {
    if (!p) return;
    p->threshold_ncut = 0.8;
    p->min_cluster = 3;
    p->recursive = 1;
}

extern "C" int r360_topo_bisect(r360_ctx* ctx, const float* A, int n, int* side, double* cut, double* eigenvalues,
                                double* fiedler, int* sweeps) {
    CHECK_ARG(ctx, "null arg");
    if (int rc = check_matrix(A, n)) return rc;
    r360_topo_params p;
    r360_topo_default_params(&p);
    p.recursive = 0;
    std::vector<TopoRecord> recs;
    Hook hook{side, eigenvalues, fiedler};
    bool nc = false;
    if (int rc = run_chunk(ctx, 1, &A, &n, p, nullptr, nullptr, &recs, &hook, &nc)) return rc;
    if (cut) *cut = recs[0].cut;
    if (sweeps) *sweeps = recs[0].sweeps;
    return nc ? R360_TOPO_NOT_CONVERGED : 0;
}

extern "C" int r360_topo_partition(r360_ctx* ctx, const float* A, int n, const r360_topo_params* params, int* part_of,
                                   int* n_parts, double* cuts, int* n_bisections) {
    CHECK_ARG(ctx && part_of && n_parts, "null arg");
    const r360_topo_params p = params_or_default(params);
    if (int rc = check_params(&p)) return rc;
    if (int rc = check_matrix(A, n)) return rc;
    std::vector<TopoRecord> recs;
    bool nc = false;
    if (int rc = run_chunk(ctx, 1, &A, &n, p, &part_of, n_parts, &recs, nullptr, &nc)) return rc;
    if (cuts)
        for (size_t k = 0; k < recs.size(); ++k) cuts[k] = recs[k].cut;
    if (n_bisections) *n_bisections = (int)recs.size();
    return nc ? R360_TOPO_NOT_CONVERGED : 0;
}

extern "C" int r360_topo_partition_batch(r360_ctx* ctx, int count, const float* const* A, const int* n,
                                         const r360_topo_params* params, int* const* part_of, int* n_parts) {
    CHECK_ARG(ctx && count >= 0, "null arg");
    if (count == 0) return 0;
    CHECK_ARG(A && n && part_of && n_parts, "null arg");
    const r360_topo_params p = params_or_default(params);
    if (int rc = check_params(&p)) return rc;
    for (int g = 0; g < count; ++g) {
        CHECK_ARG(part_of[g], "null arg");
        if (int rc = check_matrix(A[g], n[g])) return rc;
    }
    bool nc = false;
    for (int g0 = 0; g0 < count; g0 += R360_TOPO_CHUNK) {
        const int c = std::min(R360_TOPO_CHUNK, count - g0);
        if (int rc = run_chunk(ctx, c, A + g0, n + g0, p, part_of + g0, n_parts + g0, nullptr, nullptr, &nc)) return rc;
    }
    return nc ? R360_TOPO_NOT_CONVERGED : 0;
}

// ------------------------------------------------------------------ the map's bookkeeping
struct r360_topomap {
    r360_ctx* ctx = nullptr;
    std::vector<int> area_of;
    std::map<std::pair<int, int>, float> sso;   // (lower id, higher id)
    int n_areas = 1, current = 0;
};

namespace {

float sso_of(const r360_topomap* m, int a, int b) {
    auto it = m->sso.find({std::min(a, b), std::max(a, b)});
    return it == m->sso.end() ? 0.0f : it->second;
}

std::vector<int> neighbors_of(const r360_topomap* m, int area) {
    std::set<int> out{area};
    for (const auto& e : m->sso) {
        if (!(e.second > 0.0f)) continue;
        const int a = m->area_of[e.first.first], b = m->area_of[e.first.second];
        if (a == area) out.insert(b);
        if (b == area) out.insert(a);
    }
    return std::vector<int>(out.begin(), out.end());
}

void vicinity_of(const r360_topomap* m, std::vector<int>& areas, std::vector<int>& kfs) {
    areas = neighbors_of(m, m->current);
    kfs.clear();
    for (int area : areas)
        for (int k = 0; k < (int)m->area_of.size(); ++k)
            if (m->area_of[k] == area) kfs.push_back(k);
}

void vicinity_matrix(const r360_topomap* m, const std::vector<int>& kfs, float* A) {
    const size_t n = kfs.size();
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) A[i * n + j] = i == j ? 0.0f : sso_of(m, kfs[i], kfs[j]);
}

}  // namespace

extern "C" int r360_topomap_create(r360_ctx* ctx, r360_topomap** out) {
    CHECK_ARG(ctx && out, "null arg");
    r360_topomap* m = new r360_topomap;
    m->ctx = ctx;
    *out = m;
    return 0;
}

extern "C" void r360_topomap_destroy(r360_topomap* m) { delete m; }

extern "C" int r360_topomap_add_keyframe(r360_topomap* m, int* kf) {
    CHECK_ARG(m, "null arg");
    m->area_of.push_back(m->current);
    if (kf) *kf = (int)m->area_of.size() - 1;
    return 0;
}

extern "C" int r360_topomap_drop_last(r360_topomap* m) {
    CHECK_ARG(m, "null arg");
    CHECK_ARG(!m->area_of.empty(), "topomap: no keyframe to drop");
    const int k = (int)m->area_of.size() - 1;
    m->area_of.pop_back();
    for (auto it = m->sso.begin(); it != m->sso.end();)
        it = (it->first.second == k) ? m->sso.erase(it) : std::next(it);
    return 0;
}

extern "C" int r360_topomap_add_connection(r360_topomap* m, int kf1, int kf2, float sso) {
    CHECK_ARG(m, "null arg");
    const int n = (int)m->area_of.size();
    CHECK_ARG(kf1 >= 0 && kf2 >= 0 && kf1 < n && kf2 < n, "topomap: the connection names a missing keyframe");
    CHECK_ARG(kf1 != kf2, "topomap: a connection joins a keyframe to itself");
    CHECK_ARG(std::isfinite(sso) && sso >= 0.0f, "topomap: the SSO must be finite and not negative");
    m->sso[{std::min(kf1, kf2), std::max(kf1, kf2)}] = sso;
    return 0;
}

extern "C" int r360_topomap_vicinity(r360_topomap* m, int* kf_ids, float* sso, int cap, int* n) {
    CHECK_ARG(m && n, "null arg");
    std::vector<int> areas, kfs;
    vicinity_of(m, areas, kfs);
    *n = (int)kfs.size();
    if (!kf_ids && !sso) return 0;
    if (cap < *n) { r360_set_error("topomap: capacity %d < %d keyframes", cap, *n); return -4; }
    if (kf_ids) std::copy(kfs.begin(), kfs.end(), kf_ids);
    if (sso) vicinity_matrix(m, kfs, sso);
    return 0;
}

extern "C" int r360_topomap_partition(r360_topomap* m, const r360_topo_params* params, int* n_new_areas) {
    CHECK_ARG(m, "null arg");
    if (n_new_areas) *n_new_areas = 0;
    std::vector<int> areas, kfs;
    vicinity_of(m, areas, kfs);
    const int n = (int)kfs.size();
    if (n < 3) return 0;
    if (n > MAXN) {
        r360_set_error("topomap: the vicinity holds %d keyframes, at most %d (R360_TOPO_MAX_NODES)", n, MAXN);
        return R360_EINVAL;
    }
    std::vector<float> A((size_t)n * n);
    vicinity_matrix(m, kfs, A.data());
    std::vector<int> part(n);
    int n_parts = 0;
    const int rc = r360_topo_partition(m->ctx, A.data(), n, params, part.data(), &n_parts, nullptr, nullptr);
    if (rc < 0) return rc;
    const int k = n_parts - (int)areas.size();
    if (k <= 0) return rc;
    for (int a = 0; a < k; ++a) areas.push_back(m->n_areas + a);
    m->n_areas += k;
    for (int i = 0; i < n; ++i) m->area_of[kfs[i]] = areas[part[i]];
    m->current = m->area_of[*std::max_element(kfs.begin(), kfs.end())];
    if (n_new_areas) *n_new_areas = k;
    return rc;
}

extern "C" int r360_topomap_areas(const r360_topomap* m, int* area_of, int cap, int* n_kf, int* n_areas, int* current_area) {
    CHECK_ARG(m, "null arg");
    const int n = (int)m->area_of.size();
    if (n_kf) *n_kf = n;
    if (n_areas) *n_areas = m->n_areas;
    if (current_area) *current_area = m->current;
    if (!area_of) return 0;
    if (cap < n) { r360_set_error("topomap: capacity %d < %d keyframes", cap, n); return -4; }
    std::copy(m->area_of.begin(), m->area_of.end(), area_of);
    return 0;
}

extern "C" int r360_topomap_neighbors(const r360_topomap* m, int area, int* out, int cap, int* n) {
    CHECK_ARG(m && n, "null arg");
    CHECK_ARG(area >= 0 && area < m->n_areas, "topomap: no such area");
    const std::vector<int> nb = neighbors_of(m, area);
    *n = (int)nb.size();
    if (!out) return 0;
    if (cap < *n) { r360_set_error("topomap: capacity %d < %d areas", cap, *n); return -4; }
    std::copy(nb.begin(), nb.end(), out);
    return 0;
}

extern "C" int r360_topomap_selected(const r360_topomap* m, int area, int* kf) {
    CHECK_ARG(m && kf, "null arg");
    CHECK_ARG(area >= 0 && area < m->n_areas, "topomap: no such area");
    int best = -1;
    double best_sum = 0.0;
    const int n = (int)m->area_of.size();
    for (int a = 0; a < n; ++a) {
        if (m->area_of[a] != area) continue;
        double s = 0.0;
        for (int b = 0; b < n; ++b)
            if (b != a && m->area_of[b] == area) s += (double)sso_of(m, a, b);
        if (best < 0) best = a;   // an area with all-zero sums takes its lowest id
        if (s > best_sum) { best = a; best_sum = s; }
    }
    *kf = best;
    return 0;
}

// ------------------------------------------------------------------ relocalisation
extern "C" int r360_relocalize(r360_batch* b, r360_frame* const* kfs, int n_kf, r360_frame* frame, size_t max_match_planes,
                               int min_matches, float min_area, int* kf, double* pose, double* info) {
    CHECK_ARG(b && frame && kf && n_kf >= 0 && (kfs || n_kf == 0), "null arg");
    *kf = -1;
    const int lanes = std::max(1, r360_batch_lanes(b));
    std::vector<r360_pair_job> jobs(lanes);
    std::vector<r360_pair_result> res(lanes);
    for (int hi = n_kf - 1; hi >= 0; hi -= lanes) {
        const int c = std::min(lanes, hi + 1);
        for (int k = 0; k < c; ++k) {
            CHECK_ARG(kfs[hi - k], "null keyframe");
            memset(&jobs[k], 0, sizeof(r360_pair_job));
            jobs[k].ref = kfs[hi - k];
            jobs[k].trg = frame;
            jobs[k].dense = R360_JOB_PBMAP_ONLY;
        }
        if (int rc = r360_batch_register(b, jobs.data(), c, max_match_planes, R360_PLANAR_3DoF, min_matches, min_area, nullptr,
                                         res.data()))
            return rc;
        for (int k = 0; k < c; ++k) {
            const r360_pair_result& r = res[k];
            if (r.good && r.n_match >= min_matches && r.area_matched > min_area) {
                *kf = hi - k;
                if (pose)
                    for (int e = 0; e < 16; ++e) pose[e] = (double)r.pbmap_pose[e];
                if (info)
                    for (int e = 0; e < 36; ++e) info[e] = (double)r.pbmap_info[e];
                return 0;
            }
        }
    }
    return 0;
}
