// topo_kernels.hip — spectral bisection of the sensed-space-overlap graph (r360_topo_*, host/topo.cpp; statement:
// tests/topo_model.py).  One workgroup per pending cluster of one recursion level, for every graph of
// a batch: it gathers the cluster's submatrix through its index list, forms the Laplacian L, diagonalises it with a
// cyclic Jacobi method (round-robin pairing: n/2 disjoint rotations per step, a bye for odd n), sorts the
// eigenvalues (ties by index), thresholds the Fiedler vector at its mean, computes the normalised cut, decides whether
// the cluster splits and writes the children's index lists for the next level.  All fp64, every sum in a fixed
// order, no floating-point atomics, no contraction: the same input gives the same bits, lone or batched.
//
// L and the transposed rotation matrix VT (row k = eigenvector k) live in LDS up to R360_TOPO_LDS_MAX_NODES nodes
// and in the cluster's slice of the context's scratch above; the code is the same, inlined once per address space.
#include "../r360_internal.h"

namespace {

constexpr int TPB = R360_TOPO_TPB;
constexpr int MAXN = R360_TOPO_MAX_NODES;

// thread t's items e = t, t + TPB, ... of a (rows x width) loop as (e / width, e % width) without a division per item
struct Walk {
    int q, r, dq, dr, width;
    __device__ Walk(int t, int w) : q(t / w), r(t % w), dq(TPB / w), dr(TPB % w), width(w) {}
    __device__ void next() {
        q += dq;
        r += dr;
        if (r >= width) { r -= width; ++q; }
    }
};

// pair k of round r among m players (m even): player m - 1 stays, the others rotate
__device__ __forceinline__ void rr_pair(int m, int r, int k, int& p, int& q) {
    int a, b;
    if (k == 0) {
        a = m - 1;
        b = r;
    } else {
        a = (r + k) % (m - 1);
        b = (r - k + (m - 1)) % (m - 1);
    }
    p = min(a, b);
    q = max(a, b);
}

// Jacobi on L (n x n, symmetric, row-major) with VT = I on entry; on return diag(L) holds the eigenvalues and row k
// of VT the eigenvector of L[k][k].  s_pq [2][128], s_c / s_s [128], s_row [256], s_sc [0] = ||L||_F, [1] = off(L).
// Returns the sweeps done; *status = 1 when they ran out before off(L) <= 1e-14 ||L||_F.
__device__ __forceinline__ int jacobi(double* L, double* VT, int n, int* s_pq, double* s_c, double* s_s, double* s_row,
                                      double* s_sc, int* status) {
    const int t = threadIdx.x;
    const int m = n + (n & 1), half = m / 2;
    if (t < n) {
        double f = 0.0;
        for (int j = 0; j < n; ++j) f += L[t * n + j] * L[t * n + j];
        s_row[t] = f;
    }
    __syncthreads();
    if (t == 0) {
        double f = 0.0;
        for (int i = 0; i < n; ++i) f += s_row[i];
        s_sc[0] = sqrt(f);
    }
    int sweeps = 0;
    *status = 0;
    for (;;) {
        __syncthreads();
        if (t < n) {
            double f = 0.0;
            for (int j = 0; j < n; ++j)
                if (j != t) f += L[t * n + j] * L[t * n + j];
            s_row[t] = f;
        }
        __syncthreads();
        if (t == 0) {
            double f = 0.0;
            for (int i = 0; i < n; ++i) f += s_row[i];
            s_sc[1] = sqrt(f);
        }
        __syncthreads();
        if (s_sc[1] <= 1e-14 * s_sc[0]) break;
        if (sweeps == R360_TOPO_MAX_SWEEPS) {
            *status = 1;
            break;
        }
        for (int r = 0; r < m - 1; ++r) {
            if (t < half) {
                int p, q;
                rr_pair(m, r, t, p, q);
                double c = 1.0, s = 0.0;
                if (q >= n) {
                    p = -1;   // the bye of an odd n
                } else {
                    const double apq = L[p * n + q];
                    if (apq != 0.0) {
                        const double theta = (L[q * n + q] - L[p * n + p]) / (2.0 * apq);
                        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        s = tt * c;
                    }
                }
                s_pq[t] = p;
                s_pq[128 + t] = q;
                s_c[t] = c;
                s_s[t] = s;
            }
            __syncthreads();
            // L <- L J: columns p and q of every row
            for (Walk w(t, half); w.q < n; w.next()) {
                const int k = w.r, i = w.q, p = s_pq[k], q = s_pq[128 + k];
                if (p < 0) continue;
                const double c = s_c[k], s = s_s[k];
                const double x = L[i * n + p], y = L[i * n + q];
                L[i * n + p] = c * x - s * y;
                L[i * n + q] = s * x + c * y;
            }
            __syncthreads();
            // L <- J^T L and VT <- J^T VT: rows p and q; the rotated pair's own entry is zero by construction
            for (Walk w(t, n); w.q < half; w.next()) {
                const int k = w.q, j = w.r, p = s_pq[k], q = s_pq[128 + k];
                if (p < 0) continue;
                const double c = s_c[k], s = s_s[k];
                const double x = L[p * n + j], y = L[q * n + j];
                L[p * n + j] = (j == q) ? 0.0 : c * x - s * y;
                L[q * n + j] = (j == p) ? 0.0 : s * x + c * y;
                const double u = VT[p * n + j], v = VT[q * n + j];
                VT[p * n + j] = c * u - s * v;
                VT[q * n + j] = s * u + c * v;
            }
            __syncthreads();
        }
        ++sweeps;
    }
    return sweeps;
}

// gather, Laplacian, Jacobi, sort; leaves the eigenvalues ascending in s_ev and the Fiedler vector in s_v
__device__ __forceinline__ int eigen(double* L, double* VT, const float* Ag, int ng, int n, const int* s_idx, int* s_pq,
                                     double* s_c, double* s_s, double* s_row, double* s_sc, double* s_ev, double* s_v,
                                     int* status) {
    const int t = threadIdx.x;
    for (Walk w(t, n); w.q < n; w.next()) {
        const int i = w.q, j = w.r;
        L[i * n + j] = (i == j) ? 0.0 : 0.0 - (double)Ag[(size_t)s_idx[i] * ng + s_idx[j]];
        VT[i * n + j] = (i == j) ? 1.0 : 0.0;
    }
    if (t < n) {
        double d = 0.0;
        for (int j = 0; j < n; ++j) d += (double)Ag[(size_t)s_idx[t] * ng + s_idx[j]];
        s_row[t] = d;
    }
    __syncthreads();
    if (t < n) L[t * n + t] = s_row[t];
    __syncthreads();
    const int sweeps = jacobi(L, VT, n, s_pq, s_c, s_s, s_row, s_sc, status);
    if (t < n) s_row[t] = L[t * n + t];
    __syncthreads();
    const int kf = min(1, n - 1);
    if (t < n) {
        const double e = s_row[t];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (s_row[j] < e || (s_row[j] == e && j < t)) ? 1 : 0;
        s_ev[rank] = e;
        if (rank == kf) s_pq[0] = t;
    }
    __syncthreads();
    if (t < n) s_v[t] = VT[s_pq[0] * n + t];
    __syncthreads();
    return sweeps;
}

__global__ __launch_bounds__(R360_TOPO_TPB) void k_topo_level(TopoArgs a) {
    extern __shared__ double smem[];
    // the fixed part, R360_TOPO_FIXED_DOUBLES in all
    int* s_idx = reinterpret_cast<int*>(smem);          // [256] the cluster's nodes
    int* s_flag = s_idx + MAXN;                         // [256] 1: side 1
    int* s_pq = reinterpret_cast<int*>(smem + 256);     // [2][128] the step's pairs
    double* s_c = smem + 384;                           // [128]
    double* s_s = smem + 512;                           // [128]
    double* s_ev = smem + 640;                          // [256]
    double* s_v = smem + 896;                           // [256]
    double* s_r0 = smem + 1152;                         // [256]
    double* s_r1 = smem + 1408;                         // [256]
    double* s_sc = smem + 1664;                         // [8] scalars
    int* s_pos = reinterpret_cast<int*>(smem + 1672);   // [256]
    double* s_mat = smem + R360_TOPO_FIXED_DOUBLES;     // L and VT of the LDS path

    const int t = threadIdx.x;
    const TopoCluster cl = a.pending[blockIdx.x];
    const int n = cl.n, g = cl.graph, ng = a.gn[g];
    const float* Ag = a.A + a.a_off[g];
    if (t < n) s_idx[t] = a.idx_in[g * MAXN + cl.off + t];
    __syncthreads();

    int status = 0, sweeps;
    if (n <= R360_TOPO_LDS_MAX_NODES) {
        sweeps = eigen(s_mat, s_mat + n * n, Ag, ng, n, s_idx, s_pq, s_c, s_s, s_r0, s_sc, s_ev, s_v, &status);
    } else {
        double* scr = a.scratch + ((size_t)g * MAXN + cl.off) * 2 * MAXN;   // 2 n MAXN >= 2 n^2 doubles, disjoint
        sweeps = eigen(scr, scr + n * n, Ag, ng, n, s_idx, s_pq, s_c, s_s, s_r0, s_sc, s_ev, s_v, &status);
    }

    // the sides: v_i >= mean; an empty side falls back to {i <= n / 2}
    if (t == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += s_v[i];
        const double mean = sum / n;
        int n1 = 0;
        for (int i = 0; i < n; ++i) n1 += s_v[i] >= mean ? 1 : 0;
        s_sc[2] = mean;
        s_pq[1] = (n1 == 0 || n1 == n) ? 1 : 0;
    }
    __syncthreads();
    if (t < n) s_flag[t] = s_pq[1] ? (t <= n / 2 ? 1 : 0) : (s_v[t] >= s_sc[2] ? 1 : 0);
    __syncthreads();
    // positions inside the sides, and the cut's row sums: across (side 1 rows) and inside (j >= i, the same side)
    if (t < n) {
        const int f = s_flag[t];
        int pos = 0;
        for (int j = 0; j < t; ++j) pos += s_flag[j] == f ? 1 : 0;
        s_pos[t] = pos;
        double across = 0.0, inside = 0.0;
        for (int j = 0; j < n; ++j) {
            const double w = (double)Ag[(size_t)s_idx[t] * ng + s_idx[j]];
            if (s_flag[j] != f) across += w;
            else if (j >= t) inside += w;
        }
        s_r0[t] = across;
        s_r1[t] = inside;
    }
    __syncthreads();
    if (t == 0) {
        double c = 0.0, aa = 0.0, bb = 0.0;
        int n1 = 0, first1 = -1, first2 = -1;
        for (int i = 0; i < n; ++i) {
            if (s_flag[i]) {
                c += s_r0[i];
                aa += s_r1[i];
                if (first1 < 0) first1 = s_idx[i];
                ++n1;
            } else {
                bb += s_r1[i];
                if (first2 < 0) first2 = s_idx[i];
            }
        }
        const double cut = (c == 0.0) ? 0.0 : c / (aa + c) + c / (bb + c);
        const int split = (!(cut > a.threshold) && n1 >= a.min_cluster && n - n1 >= a.min_cluster) ? 1 : 0;
        TopoRecord rec;
        rec.cut = cut;
        rec.graph = g; rec.off = cl.off; rec.n = n; rec.level = cl.level;
        rec.n1 = n1; rec.split = split; rec.sweeps = sweeps; rec.status = status;
        rec.first = s_idx[0]; rec.pad = 0;
        a.rec[blockIdx.x] = rec;
        int slot = -1;
        if (split && a.recursive) {
            slot = atomicAdd(a.next_count, 2);   // an integer ticket: the order of the next level's list is free
            a.next[slot] = TopoCluster{g, cl.off, n1, cl.level + 1};
            a.next[slot + 1] = TopoCluster{g, cl.off + n1, n - n1, cl.level + 1};
        }
        s_pq[2] = split;
        s_pq[3] = n1;
        s_pq[4] = first1;
        s_pq[5] = first2;
    }
    __syncthreads();
    if (t < n) {
        const int split = s_pq[2], n1 = s_pq[3], f = s_flag[t];
        if (!split) {
            a.label[g * MAXN + s_idx[t]] = s_idx[0];
        } else if (a.recursive) {
            a.idx_out[g * MAXN + cl.off + (f ? 0 : n1) + s_pos[t]] = s_idx[t];
        } else {
            a.label[g * MAXN + s_idx[t]] = f ? s_pq[4] : s_pq[5];
        }
        if (a.eig_out && blockIdx.x == 0) {
            a.eig_out[t] = s_ev[t];
            a.fiedler_out[t] = s_v[t];
            a.side_out[t] = f ? 1 : 2;
        }
    }
}

}  // namespace

int launch_topo_level(hipStream_t st, const TopoArgs& a, int n_pending) {
    if (n_pending <= 0) return 0;
    hipLaunchKernelGGL(k_topo_level, dim3(n_pending), dim3(TPB), R360_TOPO_LDS_BYTES, st, a);
    R360_HIP(hipGetLastError());
    return 0;
}

int topo_allow_lds() {
    R360_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_topo_level), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)R360_TOPO_LDS_BYTES));
    return 0;
}
