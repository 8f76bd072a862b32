// gicp_kernels.hip — Generalized-ICP (pcl::GeneralizedIterativeClosestPoint restated, unpinned; statement:
// tests/gicp_model.py) on gfx950.
//
//   k_gicp_knn_cov   per point: the k nearest points of its own cloud through the uniform grid (rings of cells
//                    around the point's cell until no unseen cell can hold a closer point), kept in ascending
//                    (distance, index) order in an LDS column per lane; then the neighbourhood's covariance and its
//                    3x3 symmetric eigen-solve (cyclic Jacobi) in fp64 and C = I - (1 - eps) v0 v0^T, kept in fp64
//   k_gicp_corr      per source point: the nearest target of R s + t through the target's grid, the strict gate and
//                    M = (Ct_j + R Cs_i R^T)^-1 by an fp64 cofactor inverse
//   k_gicp_pass      f, g, H (upper triangle) and the correspondence count at a pose: per thread, wave (shuffles),
//                    workgroup (LDS), then k_gicp_final sums the workgroups' records in a fixed order
//   k_gicp_sum       the same two-stage sum of one array (the fitness score)
//
// Distances are fp64 of the float coordinates, ties go to the lower index.  No atomics anywhere: every sum has a
// fixed order, so two runs give the same bytes (the Makefile keeps -munsafe-fp-atomics off this file as well).
#include "../r360_internal.h"

namespace {

constexpr int KNN_TPB = 64;
constexpr int TPB = 256;
constexpr int W = R360_GICP_W;

struct Cell3 { int x, y, z; };
__device__ __forceinline__ Cell3 cell_of(const GicpGrid& G, float x, float y, float z) {
    Cell3 c;
    c.x = gicp_cell1(x, G.mn[0], G.inv, G.dim[0]);
    c.y = gicp_cell1(y, G.mn[1], G.inv, G.dim[1]);
    c.z = gicp_cell1(z, G.mn[2], G.inv, G.dim[2]);
    return c;
}

// Lower bound on the distance from a query in cell c (or beyond the grid's edge on c's side) to any point of a cell
// more than r cells away along some axis: r cell edges, less 1 % of an edge for the float rounding of the cell
// index (below 2^-13 of an edge: at most 1024 cells per axis, float coordinates).
__device__ __forceinline__ double ring_bound2(const GicpGrid& G, int r) {
    const double b = ((double)r - 0.01) * (double)G.h;
    return b > 0.0 ? b * b : 0.0;
}

// Calls visit(first, last) for the sorted-point ranges of the cells at Chebyshev distance exactly r from c.
template <class F>
__device__ __forceinline__ void ring_cells(const GicpGrid& G, const unsigned* __restrict__ cell_start, Cell3 c, int r,
                                           F&& visit) {
    const int z0 = max(c.z - r, 0), z1 = min(c.z + r, G.dim[2] - 1);
    const int y0 = max(c.y - r, 0), y1 = min(c.y + r, G.dim[1] - 1);
    const int x0 = max(c.x - r, 0), x1 = min(c.x + r, G.dim[0] - 1);
    for (int z = z0; z <= z1; ++z) {
        const bool zf = (z - c.z == r) || (c.z - z == r);
        for (int y = y0; y <= y1; ++y) {
            const size_t row = ((size_t)z * G.dim[1] + y) * G.dim[0];
            // on the shell's z and y faces a whole row of cells is one range, elsewhere the row's two end cells
            const bool full = zf || (y - c.y == r) || (c.y - y == r);
            for (int seg = 0; seg < (full ? 1 : 2); ++seg) {
                int a = x0, b = x1;
                if (!full) {
                    a = b = seg ? c.x + r : c.x - r;
                    if (a < 0 || a >= G.dim[0]) continue;
                }
                visit(cell_start[row + a], cell_start[row + b + 1]);   // the one call site: visit is inlined
            }
        }
    }
}

__device__ __forceinline__ double dist2(float ax, float ay, float az, double px, double py, double pz) {
    const double dx = (double)ax - px, dy = (double)ay - py, dz = (double)az - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

#include "jacobi3.inc"   // jacobi_rot: one rotation of the 3x3 eigen-solve, shared with normal_kernels.hip

// One lane per point, in cell order (neighbouring lanes walk neighbouring cells).  LDS: per lane a column of k
// squared distances (double) and k indices; no lane reads another's column, so there is no barrier.
__global__ void __launch_bounds__(KNN_TPB) k_gicp_knn_cov(const float4* __restrict__ pts, const float4* __restrict__ spts,
                                                          const unsigned* __restrict__ cell_start, GicpGrid G, unsigned n,
                                                          int k, double eps, int* __restrict__ knn,
                                                          double* __restrict__ cov6) {
    extern __shared__ double smem[];
    double* ld = smem;                                   // [k][64]
    int* li = reinterpret_cast<int*>(smem + (size_t)k * KNN_TPB);   // [k][64]
    const int lane = threadIdx.x;
    const unsigned t = blockIdx.x * KNN_TPB + lane;
    if (t >= n) return;
    const float4 me = spts[t];
    const int self = __float_as_int(me.w);
    const double px = me.x, py = me.y, pz = me.z;
    const Cell3 c = cell_of(G, me.x, me.y, me.z);
    const int rmax = max(G.dim[0], max(G.dim[1], G.dim[2])) - 1;
    int cnt = 0;
    for (int r = 0;; ++r) {
        ring_cells(G, cell_start, c, r, [&](unsigned first, unsigned last) __attribute__((always_inline)) {
            for (unsigned q = first; q < last; ++q) {
                const float4 o = spts[q];
                const int j = __float_as_int(o.w);
                const double d = dist2(o.x, o.y, o.z, px, py, pz);
                int pos;
                if (cnt == k) {
                    const double wd = ld[(k - 1) * KNN_TPB + lane];
                    if (!(d < wd || (d == wd && j < li[(k - 1) * KNN_TPB + lane]))) continue;
                    pos = k - 1;
                } else {
                    pos = cnt++;
                }
                while (pos > 0) {
                    const double pd = ld[(pos - 1) * KNN_TPB + lane];
                    const int pj = li[(pos - 1) * KNN_TPB + lane];
                    if (!(pd > d || (pd == d && pj > j))) break;
                    ld[pos * KNN_TPB + lane] = pd;
                    li[pos * KNN_TPB + lane] = pj;
                    --pos;
                }
                ld[pos * KNN_TPB + lane] = d;
                li[pos * KNN_TPB + lane] = j;
            }
        });
        if (r >= rmax) break;                            // the cube covers the grid
        if (cnt == k && ld[(k - 1) * KNN_TPB + lane] < ring_bound2(G, r)) break;
    }
    // n >= k, so the list is full here
    double mx = 0, my = 0, mz = 0;
    for (int s = 0; s < k; ++s) {
        const int j = li[s * KNN_TPB + lane];
        knn[(size_t)self * k + s] = j;
        const float4 o = pts[j];
        mx += (double)o.x; my += (double)o.y; mz += (double)o.z;
    }
    const double ik = 1.0 / (double)k;
    mx *= ik; my *= ik; mz *= ik;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int s = 0; s < k; ++s) {
        const float4 o = pts[li[s * KNN_TPB + lane]];
        const double dx = (double)o.x - mx, dy = (double)o.y - my, dz = (double)o.z - mz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
    }
    a00 *= ik; a01 *= ik; a02 *= ik; a11 *= ik; a12 *= ik; a22 *= ik;
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
    for (int sweep = 0; sweep < 10; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // v0: the eigenvector of the smallest eigenvalue (the first of equal ones)
    // picked with 0 / 1 weights: a chain of selects here became an indexed table in scratch memory
    const double w0 = (a00 <= a11 && a00 <= a22) ? 1.0 : 0.0;
    const double w1 = (w0 == 0.0 && a11 <= a22) ? 1.0 : 0.0;
    const double w2 = (1.0 - w0) - w1;
    double ex = (w0 * v00 + w1 * v01) + w2 * v02;
    double ey = (w0 * v10 + w1 * v11) + w2 * v12;
    double ez = (w0 * v20 + w1 * v21) + w2 * v22;
    const double nn = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
    ex *= nn; ey *= nn; ez *= nn;
    const double w = 1.0 - eps;
    double* o = cov6 + (size_t)self * 6;
    o[0] = 1.0 - w * ex * ex; o[1] = -w * ex * ey; o[2] = -w * ex * ez;
    o[3] = 1.0 - w * ey * ey; o[4] = -w * ey * ez; o[5] = 1.0 - w * ez * ez;
}

__global__ void __launch_bounds__(TPB) k_gicp_corr(const float4* __restrict__ spt, const double* __restrict__ scov, unsigned ns,
                                                   const float4* __restrict__ tsorted,
                                                   const unsigned* __restrict__ cell_start, const double* __restrict__ tcov,
                                                   GicpGrid G, GicpPose X, double gate2, int want_m,
                                                   int* __restrict__ corr, double* __restrict__ M6,
                                                   double* __restrict__ d2out) {
    const unsigned i = blockIdx.x * TPB + threadIdx.x;
    if (i >= ns) return;
    const float4 s = spt[i];
    const double* R = X.m;
    const double px = (R[0] * s.x + R[1] * s.y) + (R[2] * s.z + R[3]);
    const double py = (R[4] * s.x + R[5] * s.y) + (R[6] * s.z + R[7]);
    const double pz = (R[8] * s.x + R[9] * s.y) + (R[10] * s.z + R[11]);
    // the query's cell in double: the pose may put it where a float has no resolution left for the grid
    Cell3 c;
    c.x = (int)fmin(fmax(floor((px - (double)G.mn[0]) * (double)G.inv), 0.0), (double)(G.dim[0] - 1));
    c.y = (int)fmin(fmax(floor((py - (double)G.mn[1]) * (double)G.inv), 0.0), (double)(G.dim[1] - 1));
    c.z = (int)fmin(fmax(floor((pz - (double)G.mn[2]) * (double)G.inv), 0.0), (double)(G.dim[2] - 1));
    const int rmax = max(G.dim[0], max(G.dim[1], G.dim[2])) - 1;
    double best = INFINITY;
    int bj = -1;
    for (int r = 0;; ++r) {
        ring_cells(G, cell_start, c, r, [&](unsigned first, unsigned last) __attribute__((always_inline)) {
            for (unsigned q = first; q < last; ++q) {
                const float4 o = tsorted[q];
                const int j = __float_as_int(o.w);
                const double d = dist2(o.x, o.y, o.z, px, py, pz);
                if (d < best || (d == best && j < bj)) { best = d; bj = j; }
            }
        });
        if (r >= rmax) break;
        const double b2 = ring_bound2(G, r);
        if (best < b2 || b2 >= gate2) break;             // nothing unseen is closer, or nothing unseen passes the gate
    }
    const bool ok = bj >= 0 && best < gate2;
    corr[i] = ok ? bj : -1;
    d2out[i] = best;
    if (!want_m) return;
    double m[6] = {0, 0, 0, 0, 0, 0};
    if (ok) {
        const double* cs = scov + (size_t)i * 6;
        const double* ct = tcov + (size_t)bj * 6;
        const double c00 = cs[0], c01 = cs[1], c02 = cs[2], c11 = cs[3], c12 = cs[4], c22 = cs[5];
        // B = R Cs (3x3), S = Ct + B R^T (symmetric)
        double B[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double r0 = R[a * 4], r1 = R[a * 4 + 1], r2 = R[a * 4 + 2];
            B[a][0] = (r0 * c00 + r1 * c01) + r2 * c02;
            B[a][1] = (r0 * c01 + r1 * c11) + r2 * c12;
            B[a][2] = (r0 * c02 + r1 * c12) + r2 * c22;
        }
        double S[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b)
                S[a][b] = (B[a][0] * R[b * 4] + B[a][1] * R[b * 4 + 1]) + B[a][2] * R[b * 4 + 2];
        const double s00 = S[0][0] + ct[0], s01 = S[0][1] + ct[1], s02 = S[0][2] + ct[2];
        const double s11 = S[1][1] + ct[3], s12 = S[1][2] + ct[4], s22 = S[2][2] + ct[5];
        const double k00 = s11 * s22 - s12 * s12, k01 = s02 * s12 - s01 * s22, k02 = s01 * s12 - s02 * s11;
        const double k11 = s00 * s22 - s02 * s02, k12 = s01 * s02 - s00 * s12, k22 = s00 * s11 - s01 * s01;
        const double det = (s00 * k00 + s01 * k01) + s02 * k02;
        const double id = 1.0 / det;
        m[0] = k00 * id; m[1] = k01 * id; m[2] = k02 * id; m[3] = k11 * id; m[4] = k12 * id; m[5] = k22 * id;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) M6[(size_t)i * 6 + q] = m[q];
}

// wave, then workgroup sum of acc[NV] in a fixed order; thread v < NV of the workgroup writes record[v]
template <int NV>
__device__ __forceinline__ void block_sum(double (&acc)[NV], double* lds /* [TPB / 64][NV] */, double* record) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double x = acc[v];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
        if (lane == 0) lds[wave * NV + v] = x;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double x = lds[threadIdx.x];
#pragma unroll
        for (int w = 1; w < TPB / 64; ++w) x += lds[w * NV + threadIdx.x];
        record[threadIdx.x] = x;
    }
}

__global__ void __launch_bounds__(TPB) k_gicp_pass(const float4* __restrict__ spt, unsigned ns,
                                                   const float4* __restrict__ tpt, GicpPose Y,
                                                   const int* __restrict__ corr, const double* __restrict__ M6,
                                                   double* __restrict__ partials) {
    __shared__ double lds[(TPB / 64) * W];
    double acc[W];
#pragma unroll
    for (int v = 0; v < W; ++v) acc[v] = 0.0;
    const double* R = Y.m;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < ns; i += gridDim.x * TPB) {
        const int j = corr[i];
        if (j < 0) continue;
        const float4 s = spt[i];
        const float4 q = tpt[j];
        const double px = (R[0] * s.x + R[1] * s.y) + (R[2] * s.z + R[3]);
        const double py = (R[4] * s.x + R[5] * s.y) + (R[6] * s.z + R[7]);
        const double pz = (R[8] * s.x + R[9] * s.y) + (R[10] * s.z + R[11]);
        const double r[3] = {px - (double)q.x, py - (double)q.y, pz - (double)q.z};
        const double* mp = M6 + (size_t)i * 6;
        const double M[3][3] = {{mp[0], mp[1], mp[2]}, {mp[1], mp[3], mp[4]}, {mp[2], mp[4], mp[5]}};
        // J = [I | -[p]x]: its columns
        const double col[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, -pz, py}, {pz, 0, -px}, {-py, px, 0}};
        double Mr[3], Mc[6][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) Mr[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
#pragma unroll
        for (int b = 0; b < 6; ++b)
#pragma unroll
            for (int a = 0; a < 3; ++a) Mc[b][a] = (M[a][0] * col[b][0] + M[a][1] * col[b][1]) + M[a][2] * col[b][2];
        acc[0] += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[1 + a] += (col[a][0] * Mr[0] + col[a][1] * Mr[1]) + col[a][2] * Mr[2];
        int v = 7;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b, ++v)
                acc[v] += (col[a][0] * Mc[b][0] + col[a][1] * Mc[b][1]) + col[a][2] * Mc[b][2];
        acc[28] += 1.0;
    }
    block_sum<W>(acc, lds, partials + (size_t)blockIdx.x * W);
}

__global__ void __launch_bounds__(TPB) k_gicp_sum(const double* __restrict__ v, unsigned n, double* __restrict__ partials) {
    __shared__ double lds[TPB / 64];
    double acc[1] = {0.0};
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) acc[0] += v[i];
    block_sum<1>(acc, lds, partials + blockIdx.x);
}

// sums[v] = the nb workgroup records' entry v.  Wave w of the 16 takes the entries w, w + 16; its lane l adds
// records l, l + 64, ... in that order, then the 64 lanes' sums meet in one shuffle tree: the order depends on nb
// alone.  (One lane per entry walking all records in turn took 40 us for 256 records, four times the pass itself:
// every load waited for the add before it; one wave walking the 29 entries in turn still took 24 us.)
constexpr int FINAL_WAVES = 16;
__global__ void __launch_bounds__(64 * FINAL_WAVES) k_gicp_final(const double* __restrict__ partials, int nb, int nv,
                                                                double* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    for (int v = threadIdx.x >> 6; v < nv; v += FINAL_WAVES) {
        double x = 0.0;
        for (int b = lane; b < nb; b += 64) x += partials[(size_t)b * nv + v];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
        if (lane == 0) sums[v] = x;
    }
}

}  // namespace

int gicp_pass_blocks(size_t n) {
    const size_t b = (n + TPB - 1) / TPB;
    return (int)std::min<size_t>(std::max<size_t>(b, 1), R360_GICP_MAXB);
}

int launch_gicp_knn_cov(hipStream_t st, const GicpCloud& C, float eps) {
    if (C.n == 0) return 0;
    if (C.k < 1 || C.k > R360_GICP_KMAX || (size_t)C.k > C.n) { r360_set_error("gicp: k outside the kernel's range"); return -1; }
    const size_t lds = (size_t)C.k * KNN_TPB * (sizeof(double) + sizeof(int));
    const unsigned nb = (unsigned)((C.n + KNN_TPB - 1) / KNN_TPB);
    hipLaunchKernelGGL(k_gicp_knn_cov, dim3(nb), dim3(KNN_TPB), lds, st, C.pts.get(), C.spts.get(), C.cell_start.get(), C.grid,
                       (unsigned)C.n, C.k, (double)eps, C.knn.get(), C.cov6.get());
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_gicp_corr(hipStream_t st, const GicpCloud& S, const GicpCloud& T, const GicpPose& X, double gate2, int want_m,
                     int* corr, double* M6, double* d2) {
    if (S.n == 0) return 0;
    const unsigned nb = (unsigned)((S.n + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_gicp_corr, dim3(nb), dim3(TPB), 0, st, S.pts.get(), S.cov6.get(), (unsigned)S.n, T.spts.get(),
                       T.cell_start.get(), T.cov6.get(), T.grid, X, gate2, want_m, corr, M6, d2);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_gicp_pass(hipStream_t st, const GicpCloud& S, const GicpCloud& T, const GicpPose& Y, const int* corr,
                     const double* M6, double* partials, double* sums) {
    const int nb = gicp_pass_blocks(S.n);
    hipLaunchKernelGGL(k_gicp_pass, dim3(nb), dim3(TPB), 0, st, S.pts.get(), (unsigned)S.n, T.pts.get(), Y, corr, M6, partials);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gicp_final, dim3(1), dim3(64 * FINAL_WAVES), 0, st, partials, nb, W, sums);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_gicp_sum(hipStream_t st, const double* v, size_t n, double* partials, double* sums) {
    const int nb = gicp_pass_blocks(n);
    hipLaunchKernelGGL(k_gicp_sum, dim3(nb), dim3(TPB), 0, st, v, (unsigned)n, partials);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gicp_final, dim3(1), dim3(64 * FINAL_WAVES), 0, st, partials, nb, 1, sums);
    R360_HIP(hipGetLastError());
    return 0;
}
