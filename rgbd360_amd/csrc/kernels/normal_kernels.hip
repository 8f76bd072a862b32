// normal_kernels.hip — pcl::NormalEstimation (restated from PCL 1.7 features/normal_3d.h, unpinned) for host clouds and
// for the context's global map on gfx950.  Semantics and the divergences from PCL: DESIGN.md §5b-3; the numpy statement
// is tests/normal_model.py.
//
//   k_nrm_init     {NaN, NaN, NaN, NaN} for every row (what a dropped row keeps); the parity hook's arrays: -1 / NaN
//   k_normals      one lane per point in cell order, over the sparse grid of outlier_kernels.hip: the point and its
//                  k - 1 nearest other points within the radius as (squared distance, input index) pairs in an LDS
//                  column, then their mean, their covariance, its eigen-solve, the nearest viewpoint and the flip
//
// The order of the points inside a cell varies from run to run; nothing read back depends on it: the column holds the
// smallest pairs under a total order (squared distance, then input index), and the moments are summed in that order.
// No float atomics (the Makefile keeps -munsafe-fp-atomics off this file); the two counters are integers.
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int WALK_TPB = 64;       // one wave per workgroup: the LDS columns are k x 64 (double, int) pairs

#include "sparse_grid.inc"
#include "jacobi3.inc"

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ float nan_f() { return __uint_as_float(0x7fc00000u); }

__global__ void __launch_bounds__(TPB) k_nrm_init(size_t n, int k, float4* __restrict__ out, NormalEval E) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        out[i] = make_float4(nan_f(), nan_f(), nan_f(), nan_f());
        if (E.count) E.count[i] = -1;
        if (E.knn)
            for (int s = 0; s < k; ++s) E.knn[i * k + s] = -1;
        if (E.normal)
            for (int c = 0; c < 3; ++c) E.normal[3 * i + c] = nan_d();
        if (E.eig)
            for (int c = 0; c < 3; ++c) E.eig[3 * i + c] = nan_d();
        if (E.curvature) E.curvature[i] = nan_d();
    }
}

// (d2, j) before (e2, i) in the neighbourhood's order
__device__ __forceinline__ bool before(double d2, int j, double e2, int i) { return d2 < e2 || (d2 == e2 && j < i); }

template <bool EVAL>
__global__ void __launch_bounds__(WALK_TPB) k_normals(const uint4* __restrict__ pts, const float4* __restrict__ spts,
                                                      unsigned nf, OutlierGrid G,
                                                      const unsigned long long* __restrict__ keys, unsigned mask,
                                                      const unsigned* __restrict__ start, const unsigned* __restrict__ cnt,
                                                      double lim2, int k, const float* __restrict__ view, int n_view,
                                                      float4* __restrict__ out, NormalHdr* hdr, NormalEval E) {
    extern __shared__ double lds_nrm[];
    const int lane = threadIdx.x;
    double* cd = lds_nrm + lane;                                                  // [k][64] squared distances
    int* ci = reinterpret_cast<int*>(lds_nrm + (size_t)k * WALK_TPB) + lane;     // [k][64] input indices
    const unsigned t = blockIdx.x * WALK_TPB + lane;
    const bool active = t < nf;
    int m = 0;
    if (active) {
        const float4 me = spts[t];
        const int self = (int)__float_as_uint(me.w);
        const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
        // ---- the walk of outlier_kernels.hip's walk<true>, keeping indices; slot 0 is the point itself
        cd[0] = 0.0;
        ci[0] = self;
        m = 1;
        {
            const double qx = px / G.ec, qy = py / G.ec, qz = pz / G.ec;
            const double fx = floor(qx), fy = floor(qy), fz = floor(qz);
            const double ux = qx - fx, uy = qy - fy, uz = qz - fz;
            const long long cx = (long long)fx - G.base[0], cy = (long long)fy - G.base[1], cz = (long long)fz - G.base[2];
            const double ec2 = G.ec * G.ec;
            double kth = lim2;      // the last pair's distance once the column is full
            int kth_i = 0;
            const int R = G.ring;
            for (int pass = 0; pass < 2; ++pass) {
                const int lo = pass ? -R : 0, hi = pass ? R : 0;
                for (int dz = lo; dz <= hi; ++dz) {
                    const double gz = axis_gap(dz, uz);
                    for (int dy = lo; dy <= hi; ++dy) {
                        const double gy = axis_gap(dy, uy);
                        for (int dx = lo; dx <= hi; ++dx) {
                            if (pass && dx == 0 && dy == 0 && dz == 0) continue;
                            const double gx = axis_gap(dx, ux);
                            const double lb2 = (gx * gx + gy * gy + gz * gz) * ec2;
                            // nothing in that cell can be taken: beyond the radius, or (column full) beyond the last
                            // pair; at the last pair's distance a lower index still wins
                            if (lb2 > lim2 || (m == k && lb2 > kth)) continue;
                            const long long nx = cx + dx, ny = cy + dy, nz = cz + dz;
                            if (!(cell_in_range(nx) && cell_in_range(ny) && cell_in_range(nz))) continue;
                            const unsigned slot = find_cell(keys, mask, cell_key(nx, ny, nz));
                            if (slot == NOSLOT) continue;
                            const unsigned b = start[slot], e = b + cnt[slot];
                            for (unsigned j = b; j < e; ++j) {
                                if (j == t) continue;
                                const float4 q = spts[j];
                                const int qi = (int)__float_as_uint(q.w);
                                const double ddx = (double)q.x - px, ddy = (double)q.y - py, ddz = (double)q.z - pz;
                                const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;   // left to right, uncontracted
                                if (m < k ? d2 <= lim2 : before(d2, qi, kth, kth_i)) {
                                    int s = m < k ? m : k - 1;
                                    while (s > 1 && before(d2, qi, cd[(s - 1) * WALK_TPB], ci[(s - 1) * WALK_TPB])) {
                                        cd[s * WALK_TPB] = cd[(s - 1) * WALK_TPB];
                                        ci[s * WALK_TPB] = ci[(s - 1) * WALK_TPB];
                                        --s;
                                    }
                                    cd[s * WALK_TPB] = d2;
                                    ci[s * WALK_TPB] = qi;
                                    if (m < k) ++m;
                                    if (m == k) { kth = cd[(k - 1) * WALK_TPB]; kth_i = ci[(k - 1) * WALK_TPB]; }
                                }
                            }
                        }
                    }
                }
            }
        }
        if (EVAL) {
            if (E.count) E.count[self] = m;
            if (E.knn)
                for (int s = 0; s < m; ++s) E.knn[(size_t)self * k + s] = ci[s * WALK_TPB];
        }
        if (m >= 3) {
            // ---- mean and covariance, two passes in neighbourhood order
            double sx = 0, sy = 0, sz = 0;
            for (int s = 0; s < m; ++s) {
                const uint4 o = pts[ci[s * WALK_TPB]];
                sx += (double)__uint_as_float(o.x); sy += (double)__uint_as_float(o.y); sz += (double)__uint_as_float(o.z);
            }
            const double dm = (double)m;
            const double mx = sx / dm, my = sy / dm, mz = sz / dm;
            double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
            for (int s = 0; s < m; ++s) {
                const uint4 o = pts[ci[s * WALK_TPB]];
                const double dx = (double)__uint_as_float(o.x) - mx, dy = (double)__uint_as_float(o.y) - my,
                             dz = (double)__uint_as_float(o.z) - mz;
                a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
            }
            a00 /= dm; a01 /= dm; a02 /= dm; a11 /= dm; a12 /= dm; a22 /= dm;
            // ---- cyclic Jacobi, as k_gicp_knn_cov runs it
            double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
            for (int sweep = 0; sweep < 10; ++sweep) {
                if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
                jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
                jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
                jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            }
            // the eigenvector of the smallest eigenvalue (the first of equal ones), picked with 0 / 1 weights: a chain
            // of selects became an indexed table in scratch memory in k_gicp_knn_cov
            const double w0 = (a00 <= a11 && a00 <= a22) ? 1.0 : 0.0;
            const double w1 = (w0 == 0.0 && a11 <= a22) ? 1.0 : 0.0;
            const double w2 = (1.0 - w0) - w1;
            double ex = (w0 * v00 + w1 * v01) + w2 * v02;
            double ey = (w0 * v10 + w1 * v11) + w2 * v12;
            double ez = (w0 * v20 + w1 * v21) + w2 * v22;
            const double nn = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
            ex *= nn; ey *= nn; ez *= nn;
            const double l0 = fmin(a00, fmin(a11, a22)), l2 = fmax(a00, fmax(a11, a22));
            const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));   // the median
            const double tr = (l0 + l1) + l2;
            const double curv = tr == 0.0 ? 0.0 : fabs(l0) / tr;
            // ---- the nearest viewpoint (ties to the lower index), read uniformly by the whole wave
            double bx = 0, by = 0, bz = 0, best = 0;
            for (int v = 0; v < n_view; ++v) {
                const double vx = (double)view[3 * v] - px, vy = (double)view[3 * v + 1] - py, vz = (double)view[3 * v + 2] - pz;
                const double d2 = vx * vx + vy * vy + vz * vz;
                if (v == 0 || d2 < best) { best = d2; bx = vx; by = vy; bz = vz; }
            }
            if (bx * ex + by * ey + bz * ez < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
            out[self] = make_float4((float)ex, (float)ey, (float)ez, (float)curv);
            if (EVAL) {
                if (E.normal) { E.normal[3 * (size_t)self] = ex; E.normal[3 * (size_t)self + 1] = ey; E.normal[3 * (size_t)self + 2] = ez; }
                if (E.eig) { E.eig[3 * (size_t)self] = l0; E.eig[3 * (size_t)self + 1] = l1; E.eig[3 * (size_t)self + 2] = l2; }
                if (E.curvature) E.curvature[self] = curv;
            }
        }
    }
    // ---- the counters: integers, one atomic pair per wave
    unsigned sh = (active && m < 3) ? 1u : 0u, sm = (unsigned)m;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sh += (unsigned)__shfl_xor((int)sh, o);
        sm += (unsigned)__shfl_xor((int)sm, o);
    }
    if (lane == 0) {
        if (sh) atomicAdd(&hdr->n_short, (unsigned long long)sh);
        atomicAdd(&hdr->sum_neighbors, (unsigned long long)sm);
    }
}

inline int grid_for(size_t items, size_t per_block, int cap) {
    const size_t b = (items + per_block - 1) / per_block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

}  // namespace

int launch_normals_init(hipStream_t st, size_t n, int k, float4* out, const NormalEval& ev) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_nrm_init, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, k, out, ev);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_normals(hipStream_t st, const uint4* pts, const float4* spts, size_t nf, const OutlierGrid& G,
                   const unsigned long long* keys, size_t table_cap, const unsigned* start, const unsigned* cnt, double lim2,
                   int k, const float* view, int n_view, float4* out, NormalHdr* hdr, const NormalEval& ev) {
    if (nf == 0) return 0;
    const unsigned nb = (unsigned)((nf + WALK_TPB - 1) / WALK_TPB);
    // a (double, int) pair per entry: 12 B x 64 lanes x k, 15 KiB at k = 20 and 48 KiB at k = 64 (the default limit
    // of dynamic LDS is 64 KiB)
    const size_t lds = (sizeof(double) + sizeof(int)) * WALK_TPB * (size_t)k;
    const bool eval = ev.knn || ev.count || ev.normal || ev.eig || ev.curvature;
    if (eval)
        hipLaunchKernelGGL(k_normals<true>, dim3(nb), dim3(WALK_TPB), lds, st, pts, spts, (unsigned)nf, G, keys,
                           (unsigned)(table_cap - 1), start, cnt, lim2, k, view, n_view, out, hdr, ev);
    else
        hipLaunchKernelGGL(k_normals<false>, dim3(nb), dim3(WALK_TPB), lds, st, pts, spts, (unsigned)nf, G, keys,
                           (unsigned)(table_cap - 1), start, cnt, lim2, k, view, n_view, out, hdr, ev);
    R360_HIP(hipGetLastError());
    return 0;
}
