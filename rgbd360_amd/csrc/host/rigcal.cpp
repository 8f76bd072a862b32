// rigcal.cpp — rig extrinsic calibration from control planes on the context's GPU: r360_rigcal_*
// (include/rgbd360_hip.h).  Kernels: kernels/rigcal_kernels.hip; statement and design: tests/rigcal_model.py,
// DESIGN.md §5e.  The correspondence rows live on the host; a solve uploads them once (pairs back to back, a
// workgroup never spanning two pairs) and runs the reference's loops: per-row terms and every sum on the device, the
// 21x21 solve, its conditioning, the Rodrigues update and the accept / stop decisions here, from one small read-back
// per linearisation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../r360_internal.h"
#include "devmem.h"

struct r360_rigcal {
    r360_ctx* ctx = nullptr;      // may be null: rows and files only
    int device = 0;
    std::vector<double> pair[R360_RIGCAL_PAIRS];   // [n][10]
    double init[8][16];           // column-major
    double est[8][16];
    double cov[8][9] = {};        // the collector's sums of n_i n_j^T per adjacent pair, (0, 7) under 7
    // device: the handle owns the buffers (host/devmem.h); D is the view of them the kernels take, refilled by upload
    bool dirty = true;
    RigcalDev D;
    DevBuf<double> d_rows;
    DevBuf<int> d_tab;            // pair_start [29], wg_start [29], wg_pair [nwg]
    DevBuf<double> d_rec;         // D.rec
    DevBuf<double> d_out;         // D.out
    DevBuf<double> d_rot;         // [2][8][9]
    PinnedBuf<double> h_out;      // [R360_RIGCAL_OUT]
    int pair_start[R360_RIGCAL_PAIRS + 1] = {0};
    // trimmer
    DevBuf<int> d_counts;         // counts [n], flags [n] of one chunk of n trials
    DevBuf<unsigned char> d_mask;
};

namespace {

constexpr double THRESHOLD_CONDITIONING = 8000.0;   // Miscellaneous.h:76
constexpr double EPSILON_TRANSF = 1e-5, CONVERGENCE_ERROR = 1e-6;
constexpr double SMALL_ANGLE = 1e-4;

int pair_index(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i - 1); }

bool missing_pair(const r360_rigcal* h) {
    for (int k = 0; k < 7; ++k)
        if (h->pair[pair_index(k, k + 1)].size() < 3 * 10) return true;
    return false;
}

// (a0 b0 + a1 b1) + a2 b2 throughout, as the model
void mul3(const double A[9], const double B[9], double C[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = (A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c]) + A[r * 3 + 2] * B[6 + c];
}
void mul3t(const double A[9], const double B[9], double C[9]) {   // A^T B
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
void skew(const double v[3], double K[9]) {
    K[0] = 0.0; K[1] = -v[2]; K[2] = v[1];
    K[3] = v[2]; K[4] = 0.0; K[5] = -v[0];
    K[6] = -v[1]; K[7] = v[0]; K[8] = 0.0;
}
void exp_so3(const double w[3], double R[9]) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = std::sqrt(th2);
    double a, b;
    if (th < SMALL_ANGLE) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double s = std::sin(0.5 * th);
        a = std::sin(th) / th;
        b = 2.0 * s * s / th2;
    }
    double K[9], K2[9];
    skew(w, K);
    mul3(K, K, K2);
    for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * K[k]) + b * K2[k];
}
bool inv3_apply(const double A[9], const double b[3], double x[3]) {
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double c10 = A[2] * A[7] - A[1] * A[8], c11 = A[0] * A[8] - A[2] * A[6], c12 = A[1] * A[6] - A[0] * A[7];
    const double c20 = A[1] * A[5] - A[2] * A[4], c21 = A[2] * A[3] - A[0] * A[5], c22 = A[0] * A[4] - A[1] * A[3];
    x[0] = ((c00 * b[0] + c10 * b[1]) + c20 * b[2]) / det;
    x[1] = ((c01 * b[0] + c11 * b[1]) + c21 * b[2]) / det;
    x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return true;
}

// rotation block of a column-major pose, row-major
void rot_of(const double T[16], double R[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = T[c * 4 + r];
}
void set_rot(double T[16], const double R[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[c * 4 + r] = R[r * 3 + c];
}

// H x = b by LU with partial pivoting, n = 21; false on a zero pivot
bool solve21(const double* H, const double* b, double* x) {
    constexpr int n = 21;
    double A[n][n + 1];
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < n; ++c) A[r][c] = H[r * n + c];
        A[r][n] = b[r];
    }
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int r = k + 1; r < n; ++r)
            if (std::fabs(A[r][k]) > std::fabs(A[piv][k])) piv = r;
        if (A[piv][k] == 0.0 || !std::isfinite(A[piv][k])) return false;
        if (piv != k)
            for (int c = k; c <= n; ++c) std::swap(A[k][c], A[piv][c]);
        for (int r = k + 1; r < n; ++r) {
            const double f = A[r][k] / A[k][k];
            for (int c = k; c <= n; ++c) A[r][c] -= f * A[k][c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = A[r][n];
        for (int c = r + 1; c < n; ++c) s -= A[r][c] * x[c];
        x[r] = s / A[r][r];
    }
    return true;
}

// sigma_max / sigma_min of the symmetric 21x21 matrix: cyclic Jacobi eigenvalues, largest over smallest magnitude
double conditioning21(const double* H) {
    constexpr int n = 21;
    double A[n][n];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) A[r][c] = 0.5 * (H[r * n + c] + H[c * n + r]);
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int r = 0; r < n; ++r) {
            diag += A[r][r] * A[r][r];
            for (int c = r + 1; c < n; ++c) off += A[r][c] * A[r][c];
        }
        if (!(off > 1e-40 * diag)) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
            }
    }
    double lo = INFINITY, hi = 0.0;
    for (int r = 0; r < n; ++r) {
        lo = std::min(lo, std::fabs(A[r][r]));
        hi = std::max(hi, std::fabs(A[r][r]));
    }
    return lo > 0.0 ? hi / lo : INFINITY;
}

// sigma_max / sigma_min of a general 3x3 matrix by one-sided Jacobi (the columns of C V end up orthogonal)
double conditioning3(const double* C) {
    double G[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) G[r][c] = C[r * 3 + c];
    for (int sweep = 0; sweep < 30; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; ++r) { alpha += G[r][p] * G[r][p]; beta += G[r][q] * G[r][q]; gamma += G[r][p] * G[r][q]; }
                if (gamma == 0.0) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double gp = G[r][p], gq = G[r][q];
                    G[r][p] = c * gp - s * gq;
                    G[r][q] = s * gp + c * gq;
                }
            }
    double lo = INFINITY, hi = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double s = std::sqrt((G[0][k] * G[0][k] + G[1][k] * G[1][k]) + G[2][k] * G[2][k]);
        lo = std::min(lo, s);
        hi = std::max(hi, s);
    }
    return lo > 0.0 ? hi / lo : INFINITY;
}

// Calibration.h:1176-1215: the turn (none about X) that brings the mean X axis of the eight rotations to (1, 0, 0)
void vertical_alignment(double est[8][16]) {
    const double X[3] = {1.0, 0.0, 0.0};
    double KX[9], Hr[9] = {0}, gr[3] = {0};
    skew(X, KX);
    for (int k = 0; k < 8; ++k) {
        const double Xp[3] = {est[k][0], est[k][1], est[k][2]};
        const double err[3] = {X[1] * Xp[2] - X[2] * Xp[1], X[2] * Xp[0] - X[0] * Xp[2], X[0] * Xp[1] - X[1] * Xp[0]};
        double KP[9], J[9], JtJ[9];
        skew(Xp, KP);
        mul3(KX, KP, J);
        for (double& v : J) v = -v;
        mul3t(J, J, JtJ);
        for (int q = 0; q < 9; ++q) Hr[q] += JtJ[q];
        for (int r = 0; r < 3; ++r) gr[r] += (J[r] * err[0] + J[3 + r] * err[1]) + J[6 + r] * err[2];
    }
    const double ng[3] = {-gr[0], -gr[1], -gr[2]};
    double m[3];
    if (!inv3_apply(Hr, ng, m)) return;   // exactly singular (the untouched specs): no turn
    const double w[3] = {0.0, m[1], m[2]};
    double rot[9];
    exp_so3(w, rot);
    for (int k = 0; k < 8; ++k) {
        double R[9], Rn[9];
        rot_of(est[k], R);
        mul3(rot, R, Rn);
        set_rot(est[k], Rn);
    }
}

size_t at_least_1(size_t need) { return std::max<size_t>(need, 1); }   // an empty set still has its buffers

int need_gpu(const r360_rigcal* h) {
    CHECK_ARG(h, "null arg");
    CHECK_ARG(h->ctx, "rigcal: the handle was created without a context");
    return 0;
}

// the rows, pairs back to back, and the workgroup tables
int upload(r360_rigcal* h) {
    if (bind_device(h->ctx->device)) return -1;
    if (!h->dirty) return 0;
    std::vector<double> rows;
    std::vector<int> tab(2 * (R360_RIGCAL_PAIRS + 1));
    int n = 0, nwg = 0;
    for (int p = 0; p < R360_RIGCAL_PAIRS; ++p) {
        tab[p] = n;
        tab[R360_RIGCAL_PAIRS + 1 + p] = nwg;
        const int np = (int)(h->pair[p].size() / 10);
        rows.insert(rows.end(), h->pair[p].begin(), h->pair[p].end());
        for (int w = 0; w < (np + R360_RIGCAL_TPB - 1) / R360_RIGCAL_TPB; ++w) tab.push_back(p);
        n += np;
        nwg += (np + R360_RIGCAL_TPB - 1) / R360_RIGCAL_TPB;
    }
    tab[R360_RIGCAL_PAIRS] = n;
    tab[2 * R360_RIGCAL_PAIRS + 1] = nwg;
    memcpy(h->pair_start, tab.data(), sizeof h->pair_start);
    r360_ctx* ctx = h->ctx;
    if (h->d_rows.reserve(ctx, at_least_1(rows.size())) || h->d_tab.reserve(ctx, at_least_1(tab.size())) ||
        h->d_rec.reserve(ctx, at_least_1((size_t)R360_RIGCAL_REC * nwg)))
        return -1;
    hipStream_t st = ctx->stream;
    if (!rows.empty()) R360_HIP(hipMemcpyAsync(h->d_rows.get(), rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, st));
    R360_HIP(hipMemcpyAsync(h->d_tab.get(), tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, st));
    if (ctx_wait(ctx)) return -1;   // the host vectors end here
    RigcalDev& D = h->D;
    D.n = n;
    D.nwg = nwg;
    D.rows = h->d_rows.get();
    D.pair_start = h->d_tab.get();
    D.wg_start = h->d_tab.get() + R360_RIGCAL_PAIRS + 1;
    D.wg_pair = h->d_tab.get() + 2 * (R360_RIGCAL_PAIRS + 1);
    D.rec = h->d_rec.get();
    h->dirty = false;
    return 0;
}

// one linearisation at rot[0] (or the cost at rot[1]) into h->h_out
int accumulate(r360_rigcal* h, const double rot[2][8][9], int mode, bool weighted, bool cost_only) {
    hipStream_t st = h->ctx->stream;
    R360_HIP(hipMemcpyAsync(h->d_rot.get(), rot, sizeof(double) * 144, hipMemcpyHostToDevice, st));
    if (launch_rigcal_accum(st, h->D, h->d_rot.get(), mode, weighted, cost_only)) return -1;
    double* const h_out = h->h_out.get();
    if (cost_only)
        R360_HIP(hipMemcpyAsync(h_out + R360_RIGCAL_OUT - 1, h->D.out + R360_RIGCAL_OUT - 1, sizeof(double), hipMemcpyDeviceToHost, st));
    else
        R360_HIP(hipMemcpyAsync(h_out, h->D.out, sizeof(double) * (R360_RIGCAL_OUT - 1), hipMemcpyDeviceToHost, st));
    return ctx_wait(h->ctx);
}

void rots_of(const double est[8][16], double rot[8][9]) {
    for (int k = 0; k < 8; ++k) rot_of(est[k], rot[k]);
}

int check_trim_params(const r360_rigcal_trim_params* p) {
    CHECK_ARG(std::isfinite(p->dist) && p->dist > 0.0, "rigcal: dist must be positive");
    CHECK_ARG(std::isfinite(p->degenerate) && p->degenerate >= 0.0, "rigcal: degenerate must be finite and not negative");
    CHECK_ARG(p->prob > 0.0 && p->prob < 1.0, "rigcal: prob must lie inside (0, 1)");
    CHECK_ARG(p->max_iterations >= 1 && p->max_iterations <= (1 << 24), "rigcal: max_iterations out of range");
    CHECK_ARG(p->max_redraws >= 1, "rigcal: max_redraws must be at least 1");
    CHECK_ARG(p->chunk >= 0 && p->chunk <= (1 << 20), "rigcal: chunk out of range");
    return 0;
}

int check_pair(int i, int j) {
    CHECK_ARG(i >= 0 && j > i && j < 8, "rigcal: a pair is (i, j) with 0 <= i < j < 8");
    return 0;
}

// Hartley-Zisserman's bound as MRPT's RANSAC::execute applies it (rigcal_model.adaptive_trials)
double adaptive_trials(int count, int n_rows, double prob) {
    const double eps = 2.220446049250313e-16;
    const double f = (double)count / (double)n_rows;
    double p_no = 1.0 - f * f * f;
    p_no = std::min(1.0 - eps, std::max(eps, p_no));
    return std::log(1.0 - prob) / std::log(p_no);
}

}  // namespace

extern "C" void r360_rigcal_specs(double rt8[8 * 16]) {
    if (!rt8) return;
    // Calibration.h:918-930, row-major here
    double T[8][4][4] = {};
    for (int r = 0; r < 4; ++r) T[0][r][r] = 1.0;
    T[0][2][3] = 0.055;
    const double PI = 3.14159265358979323846;
    const double c = std::cos(45 * PI / 180), s = std::sin(45 * PI / 180);
    double turn[4][4] = {{1, 0, 0, 0}, {0, c, -s, 0}, {0, s, c, 0}, {0, 0, 0, 1}};
    for (int k = 1; k < 8; ++k)
        for (int r = 0; r < 4; ++r)
            for (int cc = 0; cc < 4; ++cc) {
                double acc = 0.0;
                for (int q = 0; q < 4; ++q) acc += turn[r][q] * T[k - 1][q][cc];
                T[k][r][cc] = acc;
            }
    for (int k = 0; k < 8; ++k)
        for (int r = 0; r < 4; ++r)
            for (int cc = 0; cc < 4; ++cc) rt8[16 * k + cc * 4 + r] = T[k][r][cc];
}

extern "C" int r360_rigcal_create(r360_ctx* ctx, r360_rigcal** out) {
    CHECK_ARG(out, "null arg");
    std::unique_ptr<r360_rigcal> h(new r360_rigcal);
    h->ctx = ctx;
    r360_rigcal_specs(&h->init[0][0]);
    memcpy(h->est, h->init, sizeof h->est);
    if (ctx) {
        h->device = ctx->device;
        if (bind_device(ctx->device)) return -1;
        if (h->d_rot.reserve(ctx, 144) || h->d_out.reserve(ctx, R360_RIGCAL_OUT) || h->h_out.reserve(ctx, R360_RIGCAL_OUT))
            return -1;
        h->D.out = h->d_out.get();
    }
    *out = h.release();
    return 0;
}

extern "C" void r360_rigcal_destroy(r360_rigcal* h) {
    if (!h) return;
    // hipFree waits for the device's work itself; the context is not touched, it may be gone already
    if (h->ctx) hipSetDevice(h->device);
    delete h;
}

extern "C" int r360_rigcal_set_pair(r360_rigcal* h, int i, int j, const double* rows, int n, int cols) {
    CHECK_ARG(h, "null arg");
    if (int rc = check_pair(i, j)) return rc;
    CHECK_ARG(n >= 0 && n <= (1 << 24), "rigcal: row count out of range");
    CHECK_ARG(n == 0 || (rows && cols == 10), "rigcal: a correspondence matrix has 10 columns");
    for (size_t k = 0; k < (size_t)n * 10; ++k) CHECK_ARG(std::isfinite(rows[k]), "rigcal: non-finite correspondence");
    h->pair[pair_index(i, j)].assign(rows, rows + (size_t)n * 10);
    h->dirty = true;
    return 0;
}

extern "C" int r360_rigcal_get_pair(const r360_rigcal* h, int i, int j, double* rows, int cap, int* n) {
    CHECK_ARG(h && n, "null arg");
    if (int rc = check_pair(i, j)) return rc;
    const std::vector<double>& v = h->pair[pair_index(i, j)];
    *n = (int)(v.size() / 10);
    if (!rows) return 0;
    if (cap < *n) { r360_set_error("rigcal: capacity %d < %d rows", cap, *n); return -4; }
    if (!v.empty()) memcpy(rows, v.data(), sizeof(double) * v.size());
    return 0;
}

extern "C" int r360_rigcal_clear(r360_rigcal* h) {
    CHECK_ARG(h, "null arg");
    for (auto& v : h->pair) v.clear();
    memset(h->cov, 0, sizeof h->cov);
    h->dirty = true;
    return 0;
}

extern "C" int r360_rigcal_check(const r360_rigcal* h) {
    CHECK_ARG(h, "null arg");
    if (missing_pair(h)) {
        r360_set_error("rigcal: an adjacent pair (k, k+1) has fewer than 3 correspondences");
        return R360_EMISSING_PAIR;
    }
    return 0;
}

extern "C" int r360_rigcal_read_matrix(const char* path, double* rows, size_t cap, int* n_rows, int* n_cols) {
    CHECK_ARG(path && n_rows && n_cols, "null arg");
    FILE* f = fopen(path, "r");
    if (!f) { r360_set_error("rigcal: cannot open %s", path); return -1; }
    std::string text;
    char buf[1 << 14];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    int nr = 0, nc = -1;
    size_t at = 0, count = 0;
    bool overflow = false;
    while (at < text.size()) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(at, end - at);
        at = end + 1;
        const char* s = line.c_str();
        while (*s == ' ' || *s == '\t' || *s == '\r') ++s;
        if (!*s || *s == '%' || *s == '#') continue;   // MRPT's comment lines
        int c = 0;
        while (*s) {
            char* e = nullptr;
            const double v = strtod(s, &e);
            if (e == s) { r360_set_error("rigcal: bad number in %s, row %d", path, nr); return R360_EINVAL; }
            if (rows) {
                if (count < cap) rows[count] = v;
                else overflow = true;
            }
            ++count;
            ++c;
            s = e;
            while (*s == ' ' || *s == '\t' || *s == '\r' || *s == ',') ++s;
        }
        if (nc < 0) nc = c;
        if (c != nc) { r360_set_error("rigcal: ragged matrix in %s, row %d", path, nr); return R360_EINVAL; }
        ++nr;
    }
    *n_rows = nr;
    *n_cols = nc < 0 ? 0 : nc;
    if (overflow) { r360_set_error("rigcal: capacity %zu < %zu numbers", cap, count); return -4; }
    return 0;
}

extern "C" int r360_rigcal_write_matrix(const char* path, const double* rows, int n_rows, int n_cols) {
    CHECK_ARG(path && rows && n_rows >= 0 && n_cols >= 1, "bad arg");
    FILE* f = fopen(path, "w");
    if (!f) { r360_set_error("rigcal: cannot write %s", path); return -1; }
    for (int r = 0; r < n_rows; ++r)
        for (int c = 0; c < n_cols; ++c) fprintf(f, "%.16e%c", rows[(size_t)r * n_cols + c], c + 1 < n_cols ? ' ' : '\n');
    if (fclose(f)) { r360_set_error("rigcal: cannot write %s", path); return -1; }
    return 0;
}

extern "C" int r360_rigcal_load_dir(r360_rigcal* h, const char* dir) {
    CHECK_ARG(h && dir, "null arg");
    std::vector<double> loaded[R360_RIGCAL_PAIRS];
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 8; ++j) {
            char path[4096];
            snprintf(path, sizeof path, "%s/correspondences_%u_%u.txt", dir, (unsigned)i, (unsigned)j);
            FILE* f = fopen(path, "r");
            if (!f) continue;
            fclose(f);
            int nr = 0, nc = 0;
            if (int rc = r360_rigcal_read_matrix(path, nullptr, 0, &nr, &nc)) return rc;
            if (nr == 0) continue;
            if (nc != 10) { r360_set_error("rigcal: %s has %d columns, not 10", path, nc); return R360_EINVAL; }
            std::vector<double>& v = loaded[pair_index(i, j)];
            v.resize((size_t)nr * 10);
            if (int rc = r360_rigcal_read_matrix(path, v.data(), v.size(), &nr, &nc)) return rc;
            for (double x : v)
                if (!std::isfinite(x)) { r360_set_error("rigcal: non-finite number in %s", path); return R360_EINVAL; }
        }
    for (int p = 0; p < R360_RIGCAL_PAIRS; ++p) h->pair[p].swap(loaded[p]);
    h->dirty = true;
    return 0;
}

extern "C" int r360_rigcal_save_dir(const r360_rigcal* h, const char* dir) {
    CHECK_ARG(h && dir, "null arg");
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 8; ++j) {
            const std::vector<double>& v = h->pair[pair_index(i, j)];
            if (v.empty()) continue;
            char path[4096];
            snprintf(path, sizeof path, "%s/correspondences_%u_%u.txt", dir, (unsigned)i, (unsigned)j);
            if (int rc = r360_rigcal_write_matrix(path, v.data(), (int)(v.size() / 10), 10)) return rc;
        }
    return 0;
}

extern "C" int r360_rigcal_set_init(r360_rigcal* h, const double rt8[8 * 16]) {
    CHECK_ARG(h && rt8, "null arg");
    for (int k = 0; k < 128; ++k) CHECK_ARG(std::isfinite(rt8[k]), "rigcal: non-finite extrinsics");
    memcpy(h->init, rt8, sizeof h->init);
    memcpy(h->est, rt8, sizeof h->est);
    return 0;
}

extern "C" int r360_rigcal_get_estimate(const r360_rigcal* h, double rt8[8 * 16]) {
    CHECK_ARG(h && rt8, "null arg");
    memcpy(rt8, h->est, sizeof h->est);
    return 0;
}

extern "C" int r360_rigcal_save_extrinsics(const r360_rigcal* h, const char* dir) {
    CHECK_ARG(h && dir, "null arg");
    for (int k = 0; k < 8; ++k) {
        char path[4096];
        snprintf(path, sizeof path, "%s/Rt_0%d.txt", dir, k + 1);
        FILE* f = fopen(path, "w");
        if (!f) { r360_set_error("rigcal: cannot write %s", path); return -1; }
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) fprintf(f, "%.9g%c", (double)(float)h->est[k][c * 4 + r], c < 3 ? ' ' : '\n');
        if (fclose(f)) { r360_set_error("rigcal: cannot write %s", path); return -1; }
    }
    return 0;
}

extern "C" int r360_rigcal_rotation(r360_rigcal* h, int weighted, r360_rigcal_stats* stats) {
    if (int rc = need_gpu(h)) return rc;
    r360_rigcal_stats st;
    memset(&st, 0, sizeof st);
    memcpy(h->est, h->init, sizeof h->est);   // :1036-1037
    if (missing_pair(h)) {
        st.status = R360_RIGCAL_MISSING_PAIR;
        if (stats) *stats = st;
        return r360_rigcal_check(h);
    }
    if (int rc = upload(h)) return rc;
    st.rows = h->D.n;
    double rot[2][8][9];
    double increment = 1000.0, diff = 1000.0;
    int it = 0;
    bool bad = false;
    while (it < R360_RIGCAL_MAX_ITERATIONS && increment > EPSILON_TRANSF && diff > CONVERGENCE_ERROR) {
        rots_of(h->est, rot[0]);
        memcpy(rot[1], rot[0], sizeof rot[0]);
        if (accumulate(h, rot, 0, weighted != 0, false)) return -1;
        const double* H = h->h_out.get();
        const double* g = H + 441;
        const double* sc = H + 462;
        st.iterations = it + 1;
        st.error[it] = sc[0];
        st.angle[it] = sc[1];
        st.werr0[it] = st.werr1[it] = sc[3];
        st.conditioning[it] = conditioning21(H);
        if (st.conditioning[it] > THRESHOLD_CONDITIONING) { bad = true; break; }
        double upd[21];
        if (!solve21(H, g, upd)) { bad = true; break; }
        for (double& v : upd) v = -v;
        for (int k = 1; k < 8; ++k) {
            double E[9];
            exp_so3(upd + 3 * k - 3, E);
            mul3(E, rot[0][k], rot[1][k]);
        }
        const double e0 = sc[3];
        if (accumulate(h, rot, 0, weighted != 0, true)) return -1;
        const double e1 = h->h_out.get()[R360_RIGCAL_OUT - 1];
        st.werr1[it] = e1;
        if (e1 < e0) {
            for (int k = 1; k < 8; ++k) set_rot(h->est[k], rot[1][k]);
            st.accepted[it] = 1;
        }
        increment = 0.0;
        for (double v : upd) increment += v * v;
        st.update2[it] = increment;
        diff = e0 - e1;
        ++it;
    }
    if (bad) st.status = R360_RIGCAL_BAD_CONDITIONED;
    else if (it >= R360_RIGCAL_MAX_ITERATIONS && increment > EPSILON_TRANSF && diff > CONVERGENCE_ERROR) st.status = R360_RIGCAL_ITERATION_LIMIT;
    vertical_alignment(h->est);
    if (stats) *stats = st;
    return 0;
}

extern "C" int r360_rigcal_translation(r360_rigcal* h, int weighted, r360_rigcal_stats* stats) {
    if (int rc = need_gpu(h)) return rc;
    r360_rigcal_stats st;
    memset(&st, 0, sizeof st);
    if (missing_pair(h)) {
        st.status = R360_RIGCAL_MISSING_PAIR;
        if (stats) *stats = st;
        return r360_rigcal_check(h);
    }
    if (int rc = upload(h)) return rc;
    double rot[2][8][9];
    rots_of(h->est, rot[0]);
    memcpy(rot[1], rot[0], sizeof rot[0]);
    if (accumulate(h, rot, 1, weighted != 0, false)) return -1;
    const double* H = h->h_out.get();
    const double* g = H + 441;
    st.rows = h->D.n;
    st.iterations = 1;
    st.error[0] = H[462];
    st.conditioning[0] = conditioning21(H);
    double upd[21];
    if (!(st.conditioning[0] < THRESHOLD_CONDITIONING) || !solve21(H, g, upd)) {
        st.status = R360_RIGCAL_BAD_CONDITIONED;
        if (stats) *stats = st;
        return 0;
    }
    for (double& v : upd) v = -v;
    double center[3] = {0.0, 0.0, 0.0};
    for (int k = 1; k < 8; ++k)
        for (int r = 0; r < 3; ++r) center[r] = center[r] + upd[3 * k - 3 + r];
    for (int r = 0; r < 3; ++r) center[r] = center[r] / 8;
    for (int r = 0; r < 3; ++r) h->est[0][12 + r] = -center[r];
    for (int k = 1; k < 8; ++k)
        for (int r = 0; r < 3; ++r) h->est[k][12 + r] = upd[3 * k - 3 + r] - center[r];
    for (double v : upd) st.update2[0] += v * v;
    st.accepted[0] = 1;
    if (stats) *stats = st;
    return 0;
}

extern "C" int r360_rigcal_eval(r360_rigcal* h, int mode, int weighted, double* H, double* g, double* scalars) {
    if (int rc = need_gpu(h)) return rc;
    CHECK_ARG(mode == 0 || mode == 1, "rigcal: mode is 0 (rotation) or 1 (translation)");
    if (missing_pair(h)) return r360_rigcal_check(h);
    if (int rc = upload(h)) return rc;
    double rot[2][8][9];
    rots_of(h->est, rot[0]);
    memcpy(rot[1], rot[0], sizeof rot[0]);
    if (accumulate(h, rot, mode, weighted != 0, false)) return -1;
    if (H) memcpy(H, h->h_out.get(), sizeof(double) * 441);
    if (g) memcpy(g, h->h_out.get() + 441, sizeof(double) * 21);
    if (scalars) memcpy(scalars, h->h_out.get() + 462, sizeof(double) * 4);
    return 0;
}

extern "C" void r360_rigcal_default_collect_params(r360_rigcal_collect_params* p) {
    if (!p) return;
    p->min_inliers = 1000;
    p->pad = 0;
    p->max_elongation = 5.0;
    p->min_dot = 0.99;
    p->max_dist = 0.2;
}

extern "C" int r360_rigcal_add_frame(r360_rigcal* h, r360_frame* f, const r360_rigcal_collect_params* params, int* added) {
    if (int rc = need_gpu(h)) return rc;
    CHECK_ARG(f, "null frame");
    r360_rigcal_collect_params p;
    r360_rigcal_default_collect_params(&p);
    if (params) p = *params;
    // the sensors' planes (this also waits for the frame's plane stage and refuses a frame built without the flag)
    std::vector<r360_plane> planes[8];
    std::vector<int2> keys;
    std::vector<int> first[8];   // per plane: its first key; the last entry closes the list
    for (int s = 0; s < 8; ++s) {
        int n = 0;
        if (int rc = r360_frame_get_local_planes(f, s, nullptr, 0, &n)) return rc;
        planes[s].resize(n);
        if (n && r360_frame_get_local_planes(f, s, planes[s].data(), n, &n)) return -1;
        for (int i = 0; i < n; ++i) {
            int nl = 0;
            if (int rc = r360_frame_get_local_plane_labels(f, s, i, nullptr, 0, &nl)) return rc;
            std::vector<int> lab(nl);
            if (nl && r360_frame_get_local_plane_labels(f, s, i, lab.data(), nl, &nl)) return -1;
            first[s].push_back((int)keys.size());
            for (int l : lab) keys.push_back(make_int2(s, l));
        }
        first[s].push_back((int)keys.size());
    }
    CHECK_ARG(f->ctx->device == h->ctx->device, "rigcal: the frame lives on another device");
    // per plane: its pixels and the sum of (row + col) over them, from the final label image
    std::vector<longlong2> sums(keys.size());
    if (!keys.empty()) {
        r360_ctx* ctx = h->ctx;
        if (bind_device(ctx->device)) return -1;
        DevBuf<int2> d_keys;
        DevBuf<longlong2> d_sums;
        if (d_keys.reserve(ctx, keys.size()) || d_sums.reserve(ctx, keys.size())) return -1;
        int rc = hipMemcpyAsync(d_keys.get(), keys.data(), sizeof(int2) * keys.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess;
        if (!rc) rc = launch_rigcal_pixsum(ctx->stream, f->pl.v.labf, f->pl.w, f->pl.h, d_keys.get(), (int)keys.size(), d_sums.get());
        if (!rc) rc = hipMemcpyAsync(sums.data(), d_sums.get(), sizeof(longlong2) * keys.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess;
        if (!rc) rc = ctx_wait(ctx);
        if (rc) { r360_set_error("rigcal: the pixel sums failed"); return -1; }
    }
    struct Rig { double n[3], d, center; long long count; };
    std::vector<Rig> rig[8];
    for (int s = 0; s < 8; ++s) {
        const float* T = f->calib->rt[s];
        for (size_t i = 0; i < planes[s].size(); ++i) {
            const r360_plane& q = planes[s][i];
            Rig g;
            for (int r = 0; r < 3; ++r) g.n[r] = ((double)T[r] * q.normal[0] + (double)T[4 + r] * q.normal[1]) + (double)T[8 + r] * q.normal[2];
            g.d = (double)q.d - ((g.n[0] * T[12] + g.n[1] * T[13]) + g.n[2] * T[14]);
            long long cnt = 0, sum = 0;
            for (int k = first[s][i]; k < first[s][i + 1]; ++k) { cnt += sums[k].x; sum += sums[k].y; }
            g.count = cnt;
            g.center = cnt > 0 ? (double)sum / (double)cnt : 0.0;
            rig[s].push_back(g);
        }
    }
    if (added) std::fill(added, added + R360_RIGCAL_PAIRS, 0);
    for (int s1 = 0; s1 < 8; ++s1)
        for (int s2 = s1 + 1; s2 < 8; ++s2)
            for (size_t i = 0; i < rig[s1].size(); ++i)
                for (size_t j = 0; j < rig[s2].size(); ++j) {
                    const Rig& a = rig[s1][i];
                    const Rig& b = rig[s2][j];
                    const r360_plane& pa = planes[s1][i];
                    const r360_plane& pb = planes[s2][j];
                    if (!(a.count > p.min_inliers && b.count > p.min_inliers && pa.elongation < p.max_elongation &&
                          pb.elongation < p.max_elongation && (a.n[0] * b.n[0] + a.n[1] * b.n[1]) + a.n[2] * b.n[2] > p.min_dot &&
                          std::fabs(a.d - b.d) < p.max_dist))
                        continue;
                    const double row[10] = {pa.normal[0], pa.normal[1], pa.normal[2], pa.d, pb.normal[0], pb.normal[1], pb.normal[2], pb.d,
                                            (double)std::min(a.count, b.count), std::max(a.center, b.center)};
                    std::vector<double>& v = h->pair[pair_index(s1, s2)];
                    v.insert(v.end(), row, row + 10);
                    if (added) ++added[pair_index(s1, s2)];
                    const int k = s2 - s1 == 1 ? s1 : (s2 - s1 == 7 ? s2 : -1);
                    if (k >= 0)
                        for (int r = 0; r < 3; ++r)
                            for (int c = 0; c < 3; ++c) h->cov[k][r * 3 + c] += a.n[r] * b.n[c];
                }
    h->dirty = true;
    return 0;
}

extern "C" int r360_rigcal_conditioning(const r360_rigcal* h, float conditioning[8]) {
    CHECK_ARG(h && conditioning, "null arg");
    for (int k = 0; k < 8; ++k) {
        bool any = false;
        for (int q = 0; q < 9; ++q) any = any || h->cov[k][q] != 0.0;
        conditioning[k] = any ? (float)conditioning3(h->cov[k]) : 1.f;
    }
    return 0;
}

extern "C" void r360_rigcal_default_trim_params(r360_rigcal_trim_params* p) {
    if (!p) return;
    p->dist = 0.2;
    p->degenerate = 0.3;
    p->prob = 0.99;
    p->max_iterations = 5000;
    p->max_redraws = 100;
    p->chunk = 0;
    p->pad = 0;
}

extern "C" int r360_rigcal_ransac_eval(r360_rigcal* h, int i, int j, const r360_rigcal_trim_params* params, unsigned seed,
                                       int trial0, int n, int* counts, int* flags) {
    if (int rc = need_gpu(h)) return rc;
    if (int rc = check_pair(i, j)) return rc;
    CHECK_ARG(counts && flags, "null arg");
    CHECK_ARG(trial0 >= 0 && n >= 0 && n <= (1 << 20), "rigcal: trial range out of bounds");
    r360_rigcal_trim_params p;
    r360_rigcal_default_trim_params(&p);
    if (params) p = *params;
    if (int rc = check_trim_params(&p)) return rc;
    const int pi = pair_index(i, j);
    const int m = (int)(h->pair[pi].size() / 10);
    CHECK_ARG(m > 3, "rigcal: the trimmer needs more than 3 rows");
    if (n == 0) return 0;
    if (int rc = upload(h)) return rc;
    r360_ctx* ctx = h->ctx;
    if (h->d_counts.reserve(ctx, at_least_1(2 * (size_t)n))) return -1;
    const RigcalTrimParams kp = {p.dist, p.degenerate, p.max_redraws};
    int* const d_counts = h->d_counts.get();
    int* d_flags = d_counts + n;
    if (launch_rigcal_ransac(ctx->stream, h->d_rows.get() + (size_t)h->pair_start[pi] * 10, m, seed, trial0, n, kp, d_counts, d_flags)) return -1;
    if (ctx_wait(ctx)) return -1;
    R360_HIP(hipMemcpy(counts, d_counts, sizeof(int) * n, hipMemcpyDeviceToHost));
    R360_HIP(hipMemcpy(flags, d_flags, sizeof(int) * n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int r360_rigcal_trim(r360_rigcal* h, int i, int j, const r360_rigcal_trim_params* params, unsigned seed,
                                r360_rigcal_trim_stats* stats, unsigned char* mask, int cap) {
    if (int rc = need_gpu(h)) return rc;
    if (int rc = check_pair(i, j)) return rc;
    r360_rigcal_trim_params p;
    r360_rigcal_default_trim_params(&p);
    if (params) p = *params;
    if (int rc = check_trim_params(&p)) return rc;
    const int pi = pair_index(i, j);
    const int m = (int)(h->pair[pi].size() / 10);
    if (mask && cap < m) { r360_set_error("rigcal: capacity %d < %d rows", cap, m); return -4; }
    r360_rigcal_trim_stats st = {m, 0, -1, 0};
    if (mask) memset(mask, 1, m);
    if (m <= 3) {   // Calibration.h:234
        if (stats) *stats = st;
        return 0;
    }
    const int chunk = p.chunk > 0 ? p.chunk : 256;
    std::vector<int> counts(chunk), flags(chunk);
    int best = -1, trial = 0;
    double N = INFINITY;
    // the sequential loop of the model, replayed over the chunk's per-trial results in trial order
    while (trial < N && trial < p.max_iterations) {
        const int n = std::min(chunk, p.max_iterations - trial);
        if (int rc = r360_rigcal_ransac_eval(h, i, j, &p, seed, trial, n, counts.data(), flags.data())) return rc;
        const int t0 = trial;
        for (int k = 0; k < n && trial < N && trial < p.max_iterations; ++k) {
            if (!flags[k] && counts[k] > best) {
                best = counts[k];
                st.winner = t0 + k;
                N = adaptive_trials(best, m, p.prob);
            }
            ++trial;
        }
    }
    st.trials = trial;
    if (best < 0) {
        st.no_model = 1;
        if (stats) *stats = st;
        return 0;
    }
    st.inliers = best;
    r360_ctx* ctx = h->ctx;
    if (h->d_mask.reserve(ctx, at_least_1((size_t)m))) return -1;
    const RigcalTrimParams kp = {p.dist, p.degenerate, p.max_redraws};
    if (launch_rigcal_mask(ctx->stream, h->d_rows.get() + (size_t)h->pair_start[pi] * 10, m, seed, st.winner, kp, h->d_mask.get())) return -1;
    if (ctx_wait(ctx)) return -1;
    std::vector<unsigned char> hm(m);
    R360_HIP(hipMemcpy(hm.data(), h->d_mask.get(), m, hipMemcpyDeviceToHost));
    std::vector<double> kept;
    kept.reserve((size_t)best * 10);
    for (int r = 0; r < m; ++r)
        if (hm[r]) kept.insert(kept.end(), h->pair[pi].begin() + (size_t)r * 10, h->pair[pi].begin() + (size_t)(r + 1) * 10);
    h->pair[pi].swap(kept);
    h->dirty = true;
    if (mask) memcpy(mask, hm.data(), m);
    if (stats) *stats = st;
    return 0;
}
