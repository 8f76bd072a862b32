// pgo_kernels.hip — pose-graph optimisation (the reference's GraphOptimizer.h over g2o, restated and unpinned;
// statement: tests/pgo_model.py) on gfx950, fp64 throughout.
//
//   k_pgo_linearise   one lane per active edge: e, c = e^T Omega e, the edge's robust kernel (none, Huber, Cauchy:
//                     rho(c) and w = rho'(c)), the Jacobians' 3x3 blocks, w Omega e, the four products
//                     Ja^T (w Omega) Jc and the two vectors Ja^T (w Omega) e into the edge's slots; the cost-only
//                     form writes rho, c and w alone
//   k_pgo_sum / final the cost: workgroup records, then one wave sums them, both in a fixed order
//   k_pgo_assemble    one wave per free vertex gathers its slots in edge order into the block-CSR rows of H and b
//   k_pgo_norms       max diag(H) and max |b| (a maximum has no order)
//   k_pgo_precond     (H_kk + lambda I)^-1 by a 6x6 Cholesky in registers, one lane per column of the inverse
//   k_pgo_cg1         block-Jacobi PCG of (H + lambda I) d = -b in one workgroup, its four vectors in LDS; the loop
//                     is bounded by maxit, and nothing waits for another workgroup
//   k_pgo_cgm_*       the same arithmetic, one launch per SpMV and per fused update-and-dot step; every workgroup
//                     sums the previous launch's partial sums itself, in the same order
//   k_pgo_update      T [+] d per vertex into the trial buffer; k_pgo_pred: d . (lambda d - b)
//
// No atomics anywhere and every sum has an order fixed by the graph alone: two runs give the same bytes (the
// Makefile keeps -munsafe-fp-atomics off this file).  The 3x3 products repeat the model's order of additions,
// (a0 b0 + a1 b1) + a2 b2, uncontracted, so a chain built from its own relative poses has F == 0 exactly.
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int LIN_TPB = 64;
constexpr double SMALL_ANGLE = 1e-4;   // pgo_model.SMALL_ANGLE

struct M3 { double m[3][3]; };

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}
// A B and A^T B
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[r][c] = dot3(A.m[r][0], B.m[0][c], A.m[r][1], B.m[1][c], A.m[r][2], B.m[2][c]);
    return C;
}
__device__ __forceinline__ M3 mul_t(const M3& A, const M3& B) {
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[r][c] = dot3(A.m[0][r], B.m[0][c], A.m[1][r], B.m[1][c], A.m[2][r], B.m[2][c]);
    return C;
}
__device__ __forceinline__ M3 transpose(const M3& A) {
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[r][c] = A.m[c][r];
    return C;
}
__device__ __forceinline__ M3 skew(double x, double y, double z) {
    M3 K = {{{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}}};
    return K;
}
// (I + a K) + b K^2
__device__ __forceinline__ M3 poly(const M3& K, double a, double b) {
    const M3 K2 = mul(K, K);
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[r][c] = ((r == c ? 1.0 : 0.0) + a * K.m[r][c]) + b * K2.m[r][c];
    return C;
}
__device__ __forceinline__ M3 exp_so3(double x, double y, double z) {
    const double th2 = (x * x + y * y) + z * z;
    const double th = sqrt(th2);
    double a, b;
    if (th < SMALL_ANGLE) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double s = sin(0.5 * th);
        a = sin(th) / th;
        b = 2.0 * s * s / th2;
    }
    return poly(skew(x, y, z), a, b);
}
__device__ __forceinline__ void log_so3(const M3& R, double w[3]) {
    const double v0 = 0.5 * (R.m[2][1] - R.m[1][2]), v1 = 0.5 * (R.m[0][2] - R.m[2][0]), v2 = 0.5 * (R.m[1][0] - R.m[0][1]);
    const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double c = 0.5 * (((R.m[0][0] + R.m[1][1]) + R.m[2][2]) - 1.0);
    const double th = atan2(s, c);
    const double f = th < SMALL_ANGLE ? 1.0 + th * th / 6.0 : th / s;
    w[0] = f * v0; w[1] = f * v1; w[2] = f * v2;
}
__device__ __forceinline__ M3 jr_inv(const double w[3]) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    const double c = th < SMALL_ANGLE ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    return poly(skew(w[0], w[1], w[2]), 0.5, c);
}
__device__ __forceinline__ void load_pose(const double* P, M3& R, double t[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R.m[r][c] = P[r * 4 + c];
        t[r] = P[r * 4 + 3];
    }
}

// A 6x6 Jacobian [[A, B], [0, D]] in 3x3 blocks.
struct J6 { M3 A, B, D; };
// W = J^T Omega: rows 0..2 = A^T Om[0..2], rows 3..5 = B^T Om[0..2] + D^T Om[3..5]
__device__ __forceinline__ void jt_omega(const J6& J, const double (&Om)[6][6], double (&W)[6][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            W[r][c] = dot3(J.A.m[0][r], Om[0][c], J.A.m[1][r], Om[1][c], J.A.m[2][r], Om[2][c]);
            W[3 + r][c] = dot3(J.B.m[0][r], Om[0][c], J.B.m[1][r], Om[1][c], J.B.m[2][r], Om[2][c]) +
                          dot3(J.D.m[0][r], Om[3][c], J.D.m[1][r], Om[4][c], J.D.m[2][r], Om[5][c]);
        }
}
// out = W J (row-major 6x6): columns 0..2 = W[:, 0..2] A, columns 3..5 = W[:, 0..2] B + W[:, 3..5] D
__device__ __forceinline__ void w_times_j(const double (&W)[6][6], const J6& J, double* __restrict__ out) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out[r * 6 + c] = dot3(W[r][0], J.A.m[0][c], W[r][1], J.A.m[1][c], W[r][2], J.A.m[2][c]);
            out[r * 6 + 3 + c] = dot3(W[r][0], J.B.m[0][c], W[r][1], J.B.m[1][c], W[r][2], J.B.m[2][c]) +
                                 dot3(W[r][3], J.D.m[0][c], W[r][4], J.D.m[1][c], W[r][5], J.D.m[2][c]);
        }
}

template <bool COST_ONLY>
__global__ void __launch_bounds__(LIN_TPB) k_pgo_linearise(PgoDev D, const double* __restrict__ poses) {
    const int k = blockIdx.x * LIN_TPB + threadIdx.x;
    if (k >= D.m) return;
    const int2 ij = D.ij[k];
    M3 Ri, Rj, RZ;
    double ti[3], tj[3], tZ[3];
    load_pose(poses + (size_t)ij.x * 12, Ri, ti);
    load_pose(poses + (size_t)ij.y * 12, Rj, tj);
    load_pose(D.Z + (size_t)k * 12, RZ, tZ);
    const M3 RB = mul_t(Ri, Rj);
    const double d0 = tj[0] - ti[0], d1 = tj[1] - ti[1], d2 = tj[2] - ti[2];
    double tB[3], e[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) tB[a] = dot3(Ri.m[0][a], d0, Ri.m[1][a], d1, Ri.m[2][a], d2);
    const M3 RE = mul_t(RZ, RB);
    const double u0 = tB[0] - tZ[0], u1 = tB[1] - tZ[1], u2 = tB[2] - tZ[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = dot3(RZ.m[0][a], u0, RZ.m[1][a], u1, RZ.m[2][a], u2);
    log_so3(RE, e + 3);
    double Om[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Om[r][c] = D.Om[(size_t)k * 36 + r * 6 + c];
    double Oe[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += Om[r][c] * e[c];
        Oe[r] = s;
    }
    double f = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) f += e[r] * Oe[r];
    // the robust kernel (g2o's RobustKernelHuber / RobustKernelCauchy on c = f, delta on sqrt(c)): rho(c) is the
    // edge's cost, w = rho'(c) scales Omega e and Omega.  Without a kernel w = 1.0 and the products below are
    // bit for bit those of the unscaled Omega.
    double w = 1.0, rho = f;
    const int kind = D.kind[k];
    if (kind != R360_GRAPH_KERNEL_NONE) {
        const double dl = D.kdelta[k], d2 = dl * dl;
        if (kind == R360_GRAPH_KERNEL_CAUCHY) {
            const double q = f / d2;
            w = 1.0 / (1.0 + q);
            rho = d2 * log1p(q);
        } else if (f > d2) {
            const double s = sqrt(f);
            w = dl / s;
            rho = 2.0 * dl * s - d2;
        }
    }
    D.cost[k] = rho;
    D.chi2[k] = f;
    D.wgt[k] = w;
    if (COST_ONLY) return;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        Oe[r] *= w;
#pragma unroll
        for (int c = 0; c < 6; ++c) Om[r][c] *= w;
    }

    const M3 Jr = jr_inv(e + 3);
    const M3 RZt = transpose(RZ);
    J6 Ji, Jj;
    const M3 RZtK = mul(RZt, skew(tB[0], tB[1], tB[2]));
    const M3 JrRBt = mul(Jr, transpose(RB));
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Ji.A.m[r][c] = -RZt.m[r][c];
            Ji.B.m[r][c] = RZtK.m[r][c];
            Ji.D.m[r][c] = -JrRBt.m[r][c];
            Jj.A.m[r][c] = RE.m[r][c];
            Jj.B.m[r][c] = 0.0;
            Jj.D.m[r][c] = Jr.m[r][c];
        }
    double* lin = D.lin + (size_t)k * R360_PGO_SLOT_LIN;
#pragma unroll
    for (int r = 0; r < 6; ++r) { lin[r] = e[r]; lin[6 + r] = Oe[r]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lin[12 + r * 3 + c] = Jj.A.m[r][c];
            lin[21 + r * 3 + c] = Jj.D.m[r][c];
            lin[30 + r * 3 + c] = Ji.A.m[r][c];
            lin[39 + r * 3 + c] = Ji.B.m[r][c];
            lin[48 + r * 3 + c] = Ji.D.m[r][c];
        }
    double* Hs = D.Hs + (size_t)k * R360_PGO_SLOT_H;
    double* bs = D.bs + (size_t)k * R360_PGO_SLOT_B;
    double W[6][6];
    jt_omega(Ji, Om, W);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += W[r][c] * e[c];
        bs[r] = s;
    }
    w_times_j(W, Ji, Hs);
    w_times_j(W, Jj, Hs + 36);
    jt_omega(Jj, Om, W);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += W[r][c] * e[c];
        bs[6 + r] = s;
    }
    w_times_j(W, Ji, Hs + 72);
    w_times_j(W, Jj, Hs + 108);
}

// the sum of x over a workgroup of T threads, the same value in every thread: lanes by a shuffle tree, then the
// waves' sums in wave order.  scratch: T / 64 doubles of LDS, free again at return.
template <int T>
__device__ __forceinline__ double wg_sum(double x, double* scratch) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = scratch[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) s += scratch[w];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(TPB) k_pgo_sum(const double* __restrict__ v, int n, double* __restrict__ partials) {
    __shared__ double lds[TPB / 64];
    double acc = 0.0;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) acc += v[i];
    const double s = wg_sum<TPB>(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// one wave: lane l adds records l, l + 64, ... in that order, then the shuffle tree
__global__ void __launch_bounds__(64) k_pgo_final(const double* __restrict__ partials, int nb, double* __restrict__ out) {
    double x = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) x += partials[b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
    if (threadIdx.x == 0) *out = x;
}

// One wave per free vertex.  Lane l < 36 owns entry l of every block of the row, lanes 36 .. 41 the row's slice of b.
__global__ void __launch_bounds__(TPB) k_pgo_assemble(PgoDev D) {
    const int row = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= D.nf || lane >= 42) return;
    const int q0 = D.vptr[row], q1 = D.vptr[row + 1];
    if (lane >= 36) {
        double acc = 0.0;
        for (int q = q0; q < q1; ++q) {
            const int ent = D.ventry[q];
            acc += D.bs[(size_t)(ent >> 1) * R360_PGO_SLOT_B + (ent & 1) * 6 + (lane - 36)];
        }
        D.b[row * 6 + (lane - 36)] = acc;
        return;
    }
    const int dg = D.diag[row];
    for (int p = D.rowptr[row]; p < D.rowptr[row + 1]; ++p) {
        double acc = 0.0;
        for (int q = q0; q < q1; ++q) {
            const int ent = D.ventry[q];
            const int s = ent & 1;
            const double* Hs = D.Hs + (size_t)(ent >> 1) * R360_PGO_SLOT_H;
            if (p == dg) acc += Hs[(s * 2 + s) * 36 + lane];
            else if (D.vblk[q] == p) acc += Hs[(s * 2 + (1 - s)) * 36 + lane];
        }
        D.vals[(size_t)p * 36 + lane] = acc;
    }
}

__global__ void __launch_bounds__(TPB) k_pgo_norms(PgoDev D, PgoOut* __restrict__ out) {
    __shared__ double lds[2][TPB];
    double md = 0.0, mb = 0.0;
    for (int i = threadIdx.x; i < 6 * D.nf; i += TPB) {
        md = fmax(md, D.vals[(size_t)D.diag[i / 6] * 36 + (i % 6) * 7]);
        mb = fmax(mb, fabs(D.b[i]));
    }
    lds[0][threadIdx.x] = md;
    lds[1][threadIdx.x] = mb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < TPB; ++t) { md = fmax(md, lds[0][t]); mb = fmax(mb, lds[1][t]); }
        out->maxdiag = md;
        out->maxb = mb;
    }
}

// thread (row, l): column l of (H_rr + lambda I)^-1 through the Cholesky factor, all in registers
__global__ void __launch_bounds__(TPB) k_pgo_precond(PgoDev D, double lambda) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= 6 * D.nf) return;
    const int row = t / 6, l = t % 6;
    const double* A = D.vals + (size_t)D.diag[row] * 36;
    double L[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double s = A[r * 6 + c] + (r == c ? lambda : 0.0);
#pragma unroll
            for (int k = 0; k < c; ++k) s -= L[r][k] * L[c][k];
            L[r][c] = r == c ? sqrt(s) : s / L[c][c];
        }
    double y[6], x[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = r == l ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < r; ++k) s -= L[r][k] * y[k];
        y[r] = s / L[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = y[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= L[k][r] * x[k];
        x[r] = s / L[r][r];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) D.minv[(size_t)row * 36 + r * 6 + l] = x[r];
}

// row i of (H + lambda I) v and of M^-1 v: the order within a block row is the blocks' order, then the columns'
template <class V>
__device__ __forceinline__ double spmv_row(const PgoDev& D, int i, double lambda, V&& v) {
    const int row = i / 6, a = i % 6;
    double acc = 0.0;
    for (int p = D.rowptr[row]; p < D.rowptr[row + 1]; ++p) {
        const double* blk = D.vals + (size_t)p * 36 + a * 6;
        const int c0 = D.colidx[p] * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc += blk[c] * v(c0 + c);
    }
    return acc + lambda * v(i);
}
__device__ __forceinline__ double minv_row(const PgoDev& D, int i, const double* r) {
    const int row = i / 6, a = i % 6;
    const double* blk = D.minv + (size_t)row * 36 + a * 6;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) acc += blk[c] * r[row * 6 + c];
    return acc;
}

constexpr int CG1 = R360_PGO_CG1_TPB;
__global__ void __launch_bounds__(CG1) k_pgo_cg1(PgoDev D, double lambda, double tol2, int maxit,
                                                 double* __restrict__ delta, PgoOut* __restrict__ out) {
    extern __shared__ double sm[];
    __shared__ double scratch[CG1 / 64];
    const int N = 6 * D.nf;
    double* x = sm;
    double* r = sm + N;
    double* p = sm + 2 * (size_t)N;
    double* q = sm + 3 * (size_t)N;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < N; i += CG1) {
        const double rhs = -D.b[i];
        x[i] = 0.0;
        r[i] = rhs;
        acc += rhs * rhs;
    }
    const double bb = wg_sum<CG1>(acc, scratch);   // its barriers publish r
    acc = 0.0;
    for (int i = tid; i < N; i += CG1) {
        const double z = minv_row(D, i, r);
        p[i] = z;
        acc += r[i] * z;
    }
    double rz = wg_sum<CG1>(acc, scratch);         // ... and p
    double rr = bb;
    int it = 0;
    bool done = bb == 0.0;
    while (!done && it < maxit) {
        acc = 0.0;
        for (int i = tid; i < N; i += CG1) {
            const double ap = spmv_row(D, i, lambda, [&](int c) { return p[c]; });
            q[i] = ap;
            acc += p[i] * ap;
        }
        const double alpha = rz / wg_sum<CG1>(acc, scratch);
        acc = 0.0;
        for (int i = tid; i < N; i += CG1) {
            x[i] += alpha * p[i];
            const double ri = r[i] - alpha * q[i];
            r[i] = ri;
            acc += ri * ri;
        }
        rr = wg_sum<CG1>(acc, scratch);
        ++it;
        if (rr <= tol2 * bb) { done = true; break; }
        acc = 0.0;
        for (int i = tid; i < N; i += CG1) {
            const double z = minv_row(D, i, r);
            q[i] = z;
            acc += r[i] * z;
        }
        const double rzn = wg_sum<CG1>(acc, scratch);
        const double beta = rzn / rz;
        rz = rzn;
        for (int i = tid; i < N; i += CG1) p[i] = q[i] + beta * p[i];
        __syncthreads();
    }
    for (int i = tid; i < N; i += CG1) delta[i] = x[i];
    if (tid == 0) {
        out->cg_iters = it;
        out->cg_done = done ? 1 : 0;
        out->bb = bb;
        out->rr = rr;
    }
}

// ---- multi-launch PCG.  vec: x, r, z, q, p[0], p[1]; partials: [0] p.Ap, [1] r.r, [2] r.z per workgroup.
constexpr int CGM = R360_PGO_CGM_TPB;
__device__ __forceinline__ double part_sum(const double* part, int nb, double* scratch) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += CGM) a += part[b];
    return wg_sum<CGM>(a, scratch);
}

__global__ void __launch_bounds__(CGM) k_pgo_cgm_init(PgoDev D, double* __restrict__ vec, double* __restrict__ part,
                                                      PgoCgState* __restrict__ S) {
    __shared__ double scratch[CGM / 64];
    __shared__ double tile[CGM];
    const int N = 6 * D.nf, nb = gridDim.x;
    const int i = blockIdx.x * CGM + threadIdx.x;
    double* x = vec;
    double* r = vec + N;
    double* z = vec + 2 * (size_t)N;
    double rhs = 0.0;
    if (i < N) {
        rhs = -D.b[i];
        x[i] = 0.0;
        r[i] = rhs;
    }
    tile[threadIdx.x] = rhs;
    __syncthreads();
    double zi = 0.0;
    if (i < N) {
        const int row = i / 6, a = i % 6, t0 = threadIdx.x - a;
        const double* blk = D.minv + (size_t)row * 36 + a * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) zi += blk[c] * tile[t0 + c];
        z[i] = zi;
    }
    const double s_rr = wg_sum<CGM>(rhs * rhs, scratch);
    const double s_rz = wg_sum<CGM>(rhs * zi, scratch);
    if (threadIdx.x == 0) {
        part[nb + blockIdx.x] = s_rr;
        part[2 * nb + blockIdx.x] = s_rz;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { S->iters = 0; S->done = 0; S->rz[0] = S->rz[1] = 0.0; S->bb = 0.0; S->rr = 0.0; }
}

// What every workgroup works out at the start of step k from the previous launch's partial sums: r.r, the stop
// test, beta.  Returns false when the solve has ended.  Workgroup 0 records the scalars for later launches.
__device__ __forceinline__ bool cgm_step_begin(const PgoCgState* S, PgoCgState* Sw, const double* part, int nb, int k,
                                               double tol2, double* scratch, double* beta) {
    if (S->done) return false;
    const double rr = part_sum(part + nb, nb, scratch);
    const double rzn = part_sum(part + 2 * nb, nb, scratch);
    const double bb = k == 0 ? rr : S->bb;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) {
        Sw->rr = rr;
        Sw->iters = k;
        if (k == 0) Sw->bb = bb;
    }
    if (k == 0 ? bb == 0.0 : rr <= tol2 * bb) {
        if (first) Sw->done = 1;
        return false;
    }
    *beta = k == 0 ? 0.0 : rzn / S->rz[(k + 1) & 1];
    if (first) Sw->rz[k & 1] = rzn;
    return true;
}

__global__ void __launch_bounds__(CGM) k_pgo_cgm_spmv(PgoDev D, double lambda, double tol2, int k, double* __restrict__ vec,
                                                      double* __restrict__ part, PgoCgState* S) {
    __shared__ double scratch[CGM / 64];
    const int N = 6 * D.nf, nb = gridDim.x;
    double beta;
    if (!cgm_step_begin(S, S, part, nb, k, tol2, scratch, &beta)) return;
    const double* z = vec + 2 * (size_t)N;
    double* q = vec + 3 * (size_t)N;
    const double* pold = vec + (4 + ((k + 1) & 1)) * (size_t)N;
    double* pnew = vec + (4 + (k & 1)) * (size_t)N;
    const int i = blockIdx.x * CGM + threadIdx.x;
    double pap = 0.0;
    if (i < N) {
        double ap;
        if (k == 0) ap = spmv_row(D, i, lambda, [&](int c) { return z[c]; });
        else ap = spmv_row(D, i, lambda, [&](int c) { return z[c] + beta * pold[c]; });
        const double pi = k == 0 ? z[i] : z[i] + beta * pold[i];
        pnew[i] = pi;
        q[i] = ap;
        pap = pi * ap;
    }
    const double s = wg_sum<CGM>(pap, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(CGM) k_pgo_cgm_update(PgoDev D, int k, double* __restrict__ vec, double* __restrict__ part,
                                                        const PgoCgState* __restrict__ S) {
    __shared__ double scratch[CGM / 64];
    __shared__ double tile[CGM];
    if (S->done) return;
    const int N = 6 * D.nf, nb = gridDim.x;
    const double alpha = S->rz[k & 1] / part_sum(part, nb, scratch);
    double* x = vec;
    double* r = vec + N;
    double* z = vec + 2 * (size_t)N;
    const double* q = vec + 3 * (size_t)N;
    const double* p = vec + (4 + (k & 1)) * (size_t)N;
    const int i = blockIdx.x * CGM + threadIdx.x;
    double ri = 0.0;
    if (i < N) {
        x[i] += alpha * p[i];
        ri = r[i] - alpha * q[i];
        r[i] = ri;
    }
    tile[threadIdx.x] = ri;
    __syncthreads();
    double zi = 0.0;
    if (i < N) {
        const int row = i / 6, a = i % 6, t0 = threadIdx.x - a;
        const double* blk = D.minv + (size_t)row * 36 + a * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) zi += blk[c] * tile[t0 + c];
        z[i] = zi;
    }
    const double s_rr = wg_sum<CGM>(ri * ri, scratch);
    const double s_rz = wg_sum<CGM>(ri * zi, scratch);
    if (threadIdx.x == 0) {
        part[nb + blockIdx.x] = s_rr;
        part[2 * nb + blockIdx.x] = s_rz;
    }
}

// the stop test after the last step, alone (one workgroup), and the solve's figures for the host
__global__ void __launch_bounds__(CGM) k_pgo_cgm_check(int nb, double tol2, int k, const double* __restrict__ part,
                                                       PgoCgState* S, PgoOut* out) {
    __shared__ double scratch[CGM / 64];
    double beta;
    const bool was_done = S->done != 0;
    const bool go_on = cgm_step_begin(S, S, part, nb, k, tol2, scratch, &beta);
    __syncthreads();
    if (threadIdx.x == 0) {
        out->cg_iters = S->iters;
        out->cg_done = (was_done || !go_on) ? 1 : 0;
        out->bb = S->bb;
        out->rr = S->rr;
    }
}

__global__ void __launch_bounds__(TPB) k_pgo_update(PgoDev D, const double* __restrict__ poses, const double* __restrict__ delta,
                                                    double* __restrict__ trial) {
    const int v = blockIdx.x * TPB + threadIdx.x;
    if (v >= D.n) return;
    const double* P = poses + (size_t)v * 12;
    double* O = trial + (size_t)v * 12;
    const int k = D.fidx[v];
    if (k < 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) O[q] = P[q];
        return;
    }
    M3 R;
    double t[3];
    load_pose(P, R, t);
    const double* d = delta + (size_t)k * 6;
    const M3 Rn = mul(R, exp_so3(d[3], d[4], d[5]));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) O[r * 4 + c] = Rn.m[r][c];
        O[r * 4 + 3] = dot3(R.m[r][0], d[0], R.m[r][1], d[1], R.m[r][2], d[2]) + t[r];
    }
}

__global__ void __launch_bounds__(TPB) k_pgo_pred(PgoDev D, const double* __restrict__ delta, double lambda,
                                                  PgoOut* __restrict__ out) {
    __shared__ double lds[TPB / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < 6 * D.nf; i += TPB) acc += delta[i] * (lambda * delta[i] - D.b[i]);
    const double s = wg_sum<TPB>(acc, lds);
    if (threadIdx.x == 0) out->pred = s;
}

inline int blocks_of(int n, int tpb) { return (n + tpb - 1) / tpb; }

}  // namespace

int launch_pgo_linearise(hipStream_t st, const PgoDev& D, const double* poses, bool cost_only, double* partials, double* F) {
    if (D.m == 0) {
    } else if (cost_only) hipLaunchKernelGGL(k_pgo_linearise<true>, dim3(blocks_of(D.m, LIN_TPB)), dim3(LIN_TPB), 0, st, D, poses);
    else hipLaunchKernelGGL(k_pgo_linearise<false>, dim3(blocks_of(D.m, LIN_TPB)), dim3(LIN_TPB), 0, st, D, poses);
    R360_HIP(hipGetLastError());
    const int nb = std::max(1, std::min(blocks_of(D.m, TPB), R360_PGO_MAXB));
    hipLaunchKernelGGL(k_pgo_sum, dim3(nb), dim3(TPB), 0, st, D.cost, D.m, partials);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pgo_final, dim3(1), dim3(64), 0, st, partials, nb, F);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pgo_assemble(hipStream_t st, const PgoDev& D, PgoOut* out) {
    if (D.nf > 0) hipLaunchKernelGGL(k_pgo_assemble, dim3(blocks_of(D.nf, TPB / 64)), dim3(TPB), 0, st, D);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pgo_norms, dim3(1), dim3(TPB), 0, st, D, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pgo_precond(hipStream_t st, const PgoDev& D, double lambda) {
    hipLaunchKernelGGL(k_pgo_precond, dim3(blocks_of(6 * D.nf, TPB)), dim3(TPB), 0, st, D, lambda);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pgo_cg1(hipStream_t st, const PgoDev& D, double lambda, double tol2, int maxit, double* delta, PgoOut* out) {
    const size_t lds = sizeof(double) * 4 * 6 * (size_t)D.nf;
    if (lds > (size_t)R360_PGO_CG1_LDS) { r360_set_error("graph: too many unknowns for the single-workgroup solve"); return -2; }
    hipLaunchKernelGGL(k_pgo_cg1, dim3(1), dim3(CG1), lds, st, D, lambda, tol2, maxit, delta, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pgo_cgm(r360_ctx* ctx, const PgoDev& D, double lambda, double tol2, int maxit, double* vec, double* partials,
                   PgoCgState* d_state, PgoCgState* h_state, PgoOut* out) {
    hipStream_t st = ctx->stream;
    const int N = 6 * D.nf, nb = blocks_of(N, CGM);
    hipLaunchKernelGGL(k_pgo_cgm_init, dim3(nb), dim3(CGM), 0, st, D, vec, partials, d_state);
    R360_HIP(hipGetLastError());
    constexpr int BATCH = 64;   // steps enqueued between two looks at the stop flag
    int k = 0;
    while (true) {
        const int end = std::min(maxit, k + BATCH);
        for (; k < end; ++k) {
            hipLaunchKernelGGL(k_pgo_cgm_spmv, dim3(nb), dim3(CGM), 0, st, D, lambda, tol2, k, vec, partials, d_state);
            hipLaunchKernelGGL(k_pgo_cgm_update, dim3(nb), dim3(CGM), 0, st, D, k, vec, partials, d_state);
        }
        R360_HIP(hipGetLastError());
        if (k >= maxit) break;
        R360_HIP(hipMemcpyAsync(h_state, d_state, sizeof(PgoCgState), hipMemcpyDeviceToHost, st));
        if (ctx_wait(ctx)) return -1;
        if (h_state->done) break;
    }
    hipLaunchKernelGGL(k_pgo_cgm_check, dim3(1), dim3(CGM), 0, st, nb, tol2, k, partials, d_state, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pgo_update(hipStream_t st, const PgoDev& D, const double* poses, const double* delta, double lambda,
                      double* trial, PgoOut* out) {
    hipLaunchKernelGGL(k_pgo_update, dim3(blocks_of(D.n, TPB)), dim3(TPB), 0, st, D, poses, delta, trial);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pgo_pred, dim3(1), dim3(TPB), 0, st, D, delta, lambda, out);
    R360_HIP(hipGetLastError());
    return 0;
}
