// outlier_kernels.hip — pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval (restated from PCL 1.7, unpinned) for
// host clouds and for the context's global map on gfx950.  Semantics, the two divergences from PCL and the design:
// DESIGN.md §5b-2; the numpy statement is tests/outlier_model.py.
//
//   k_out_init                           score = NaN, count = -1, keep = 0 for every row (what a dropped row keeps)
//   k_out_cells                          the point's cell key into an open-addressing table of occupied cells (atomicCAS),
//                                        one count per cell, the claimed slot per point
//   k_out_scan_*                         exclusive prefix sum of 32-bit values: the cells' first points, the kept rows' ranks
//   k_out_scatter                        the finite points into cell order {x, y, z, input index}
//   k_outlier_knn                        one lane per point in cell order: the k smallest squared distances to other points
//                                        within max_dist in an LDS column, then d_i or +inf
//   k_outlier_count                      the same walk, counting the other points within the radius
//   k_out_sum / k_out_final              mean, then the squared deviations, of the d_i: per thread, per wave by shuffles,
//                                        per workgroup in LDS, then one thread over the workgroup records
//   k_out_flag_* / k_out_compact         the keep flag per row; the kept rows at their ranks, bits unchanged
//
// The grid is sparse: a cell exists only where a point lies, so memory is proportional to the points and a query
// reads at most the (2 ring + 1)^3 cells around its own however far apart the points are.  The order of the points
// inside a cell varies from run to run (atomic ranks); nothing read back depends on it: the k smallest distances are
// a multiset, the count is a count.  No float atomics (the Makefile keeps -munsafe-fp-atomics off this file); every
// fp64 sum runs in a fixed order, so two runs give the same bytes.
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int WALK_TPB = 64;       // one wave per workgroup: the LDS columns are k x 64 doubles
#include "sparse_grid.inc"   // cell keys, find_cell, axis_gap: shared with normal_kernels.hip

__global__ void __launch_bounds__(TPB) k_out_init(size_t n, double* __restrict__ score, int* __restrict__ count,
                                                  unsigned* __restrict__ keep) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        score[i] = nan;
        count[i] = -1;
        keep[i] = 0u;
    }
}

__global__ void __launch_bounds__(TPB) k_out_cells(const uint4* __restrict__ pts, size_t n, OutlierGrid G,
                                                   unsigned long long* __restrict__ keys, unsigned mask,
                                                   unsigned* __restrict__ cnt, unsigned* __restrict__ pslot,
                                                   OutlierHdr* hdr) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const uint4 p = pts[i];
        unsigned slot = NOSLOT;
        if (finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z)) {
            const long long cx = (long long)floor((double)__uint_as_float(p.x) / G.ec) - G.base[0];
            const long long cy = (long long)floor((double)__uint_as_float(p.y) / G.ec) - G.base[1];
            const long long cz = (long long)floor((double)__uint_as_float(p.z) / G.ec) - G.base[2];
            if (cell_in_range(cx) && cell_in_range(cy) && cell_in_range(cz)) {
                const unsigned long long key = cell_key(cx, cy, cz);
                unsigned h = (unsigned)mix64(key) & mask;
                for (unsigned probe = 0; probe <= mask; ++probe) {   // the table is at most half full
                    const unsigned long long old = atomicCAS(&keys[h], 0ull, key);
                    if (old == 0ull || old == key) { slot = h; break; }
                    h = (h + 1) & mask;
                }
            }
            if (slot == NOSLOT) atomicOr(&hdr->err, 1u);
            else atomicAdd(&cnt[slot], 1u);
        }
        pslot[i] = slot;
    }
}

// exclusive scan of one value per thread over the workgroup; *total: the workgroup's sum
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* wsum, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();   // wsum may still be read from the previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    *total = tot;
    return off + inc - v;
}

__global__ void __launch_bounds__(TPB) k_out_scan_reduce(const unsigned* __restrict__ v, size_t n, unsigned* __restrict__ bsum) {
    __shared__ unsigned wsum[TPB / 64];
    const size_t base = (size_t)blockIdx.x * R360_OUTLIER_SCAN_BLOCK;
    unsigned s = 0;
    for (size_t j = threadIdx.x; j < R360_OUTLIER_SCAN_BLOCK; j += TPB)
        if (base + j < n) s += v[base + j];
    unsigned total;
    block_excl_scan(s, wsum, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TPB) k_out_scan_top(unsigned* bsum, size_t nb, unsigned long long* total_out) {
    __shared__ unsigned wsum[TPB / 64];
    unsigned carry = 0;
    for (size_t base = 0; base < nb; base += TPB) {
        const size_t i = base + threadIdx.x;
        const unsigned v = i < nb ? bsum[i] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(v, wsum, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

__global__ void __launch_bounds__(TPB) k_out_scan_apply(const unsigned* __restrict__ v, size_t n,
                                                        const unsigned* __restrict__ bsum, unsigned* __restrict__ out) {
    __shared__ unsigned wsum[TPB / 64];
    const size_t base = (size_t)blockIdx.x * R360_OUTLIER_SCAN_BLOCK;
    unsigned carry = bsum[blockIdx.x];
    for (size_t j = 0; j < R360_OUTLIER_SCAN_BLOCK; j += TPB) {
        const size_t w = base + j + threadIdx.x;
        const unsigned x = w < n ? v[w] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(x, wsum, &total);
        if (w < n) out[w] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(TPB) k_out_scatter(const uint4* __restrict__ pts, size_t n,
                                                     const unsigned* __restrict__ pslot, const unsigned* __restrict__ start,
                                                     unsigned* __restrict__ fill, float4* __restrict__ spts, size_t nf,
                                                     OutlierHdr* hdr) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const unsigned slot = pslot[i];
        if (slot == NOSLOT) continue;
        const uint4 p = pts[i];
        const size_t pos = (size_t)start[slot] + atomicAdd(&fill[slot], 1u);
        if (pos >= nf) { atomicOr(&hdr->err, 2u); continue; }
        spts[pos] = make_float4(__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), __uint_as_float((unsigned)i));
    }
}

// The walk of point t (in cell order) over the cells around its own, its own first.  KNN: the k smallest squared
// distances <= lim2 to other points, ascending in the lane's LDS column (col[j * 64]); returns how many were found.
// Otherwise: the number of other points with squared distance <= lim2, stopping once it reaches `stop`.
template <bool KNN>
__device__ __forceinline__ int walk(const float4* __restrict__ spts, unsigned t, const OutlierGrid& G,
                                    const unsigned long long* __restrict__ keys, unsigned mask,
                                    const unsigned* __restrict__ start, const unsigned* __restrict__ cnt, double lim2,
                                    int k, int stop, double* col, unsigned* idx_out) {
    const float4 me = spts[t];
    *idx_out = __float_as_uint(me.w);
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
    const double qx = px / G.ec, qy = py / G.ec, qz = pz / G.ec;
    const double fx = floor(qx), fy = floor(qy), fz = floor(qz);
    const double ux = qx - fx, uy = qy - fy, uz = qz - fz;
    const long long cx = (long long)fx - G.base[0], cy = (long long)fy - G.base[1], cz = (long long)fz - G.base[2];
    const double ec2 = G.ec * G.ec;
    int m = 0;              // KNN: filled entries of the column; else the count
    double kth = lim2;      // KNN: a candidate must be <= lim2 while the column fills, then < the k-th
    const int R = G.ring;
    for (int pass = 0; pass < 2; ++pass) {
        const int lo = pass ? -R : 0, hi = pass ? R : 0;
        for (int dz = lo; dz <= hi; ++dz) {
            const double gz = axis_gap(dz, uz);
            for (int dy = lo; dy <= hi; ++dy) {
                const double gy = axis_gap(dy, uy);
                for (int dx = lo; dx <= hi; ++dx) {
                    if (pass && dx == 0 && dy == 0 && dz == 0) continue;
                    if (!KNN && m >= stop) return m;
                    const double gx = axis_gap(dx, ux);
                    const double lb2 = (gx * gx + gy * gy + gz * gz) * ec2;
                    // nothing in that cell can be taken: beyond the limit, or (column full) not below the k-th
                    if (lb2 > lim2 || (KNN && m == k && lb2 >= kth)) continue;
                    const long long nx = cx + dx, ny = cy + dy, nz = cz + dz;
                    if (!(cell_in_range(nx) && cell_in_range(ny) && cell_in_range(nz))) continue;
                    const unsigned slot = find_cell(keys, mask, cell_key(nx, ny, nz));
                    if (slot == NOSLOT) continue;
                    const unsigned b = start[slot], e = b + cnt[slot];
                    for (unsigned j = b; j < e; ++j) {
                        if (j == t) continue;
                        const float4 q = spts[j];
                        const double ddx = (double)q.x - px, ddy = (double)q.y - py, ddz = (double)q.z - pz;
                        const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;   // left to right, uncontracted
                        if (KNN) {
                            if (m < k ? d2 <= lim2 : d2 < kth) {
                                int s = m < k ? m : k - 1;
                                while (s > 0 && col[(s - 1) * WALK_TPB] > d2) {
                                    col[s * WALK_TPB] = col[(s - 1) * WALK_TPB];
                                    --s;
                                }
                                col[s * WALK_TPB] = d2;
                                if (m < k) ++m;
                                if (m == k) kth = col[(k - 1) * WALK_TPB];
                            }
                        } else {
                            if (d2 <= lim2 && ++m >= stop) return m;
                        }
                    }
                }
            }
        }
    }
    return m;
}

__global__ void __launch_bounds__(WALK_TPB) k_outlier_knn(const float4* __restrict__ spts, unsigned nf, OutlierGrid G,
                                                          const unsigned long long* __restrict__ keys, unsigned mask,
                                                          const unsigned* __restrict__ start, const unsigned* __restrict__ cnt,
                                                          double lim2, int k, double* __restrict__ score) {
    extern __shared__ double lds_col[];   // [k][64]: lane l owns column l
    const unsigned t = blockIdx.x * WALK_TPB + threadIdx.x;
    if (t >= nf) return;
    double* col = lds_col + threadIdx.x;
    unsigned idx;
    const int m = walk<true>(spts, t, G, keys, mask, start, cnt, lim2, k, 0, col, &idx);
    double d = __longlong_as_double(0x7ff0000000000000ll);   // short: fewer than k others within max_dist
    if (m == k) {
        double s = 0.0;
        for (int j = 0; j < k; ++j) s += sqrt(col[j * WALK_TPB]);
        d = s / (double)k;
    }
    score[idx] = d;
}

__global__ void __launch_bounds__(WALK_TPB) k_outlier_count(const float4* __restrict__ spts, unsigned nf, OutlierGrid G,
                                                            const unsigned long long* __restrict__ keys, unsigned mask,
                                                            const unsigned* __restrict__ start, const unsigned* __restrict__ cnt,
                                                            double lim2, int stop, int* __restrict__ count) {
    const unsigned t = blockIdx.x * WALK_TPB + threadIdx.x;
    if (t >= nf) return;
    unsigned idx;
    const int m = walk<false>(spts, t, G, keys, mask, start, cnt, lim2, 0, stop, nullptr, &idx);
    count[idx] = m;
}

__device__ __forceinline__ bool is_finite_d(double d) {
    return ((unsigned long long)__double_as_longlong(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// PASS 0: the sum of the finite d_i, their number and the number of short points (+inf); PASS 1: the sum of
// (d_i - mean)^2.  Thread, wave (shuffles), workgroup (LDS), one record per workgroup: the order is fixed by n and the grid.
template <int PASS>
__global__ void __launch_bounds__(TPB) k_out_sum(const double* __restrict__ score, size_t n, const OutlierHdr* hdr,
                                                 OutlierPartial* __restrict__ partial) {
    const double mean = PASS ? hdr->mean : 0.0;
    double s = 0.0;
    unsigned long long m = 0, sh = 0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const double d = score[i];
        if (is_finite_d(d)) {
            const double e = d - mean;
            s += PASS ? e * e : d;
            ++m;
        } else if (d > 0.0) {   // +inf; NaN compares false
            ++sh;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o);
        m += (unsigned long long)__shfl_xor((long long)m, o);
        sh += (unsigned long long)__shfl_xor((long long)sh, o);
    }
    __shared__ double w_s[TPB / 64];
    __shared__ unsigned long long w_m[TPB / 64], w_sh[TPB / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { w_s[wave] = s; w_m[wave] = m; w_sh[wave] = sh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / 64; ++w) { s += w_s[w]; m += w_m[w]; sh += w_sh[w]; }
        OutlierPartial r;
        r.sum = s; r.m = m; r.n_short = sh; r.pad = 0;
        partial[blockIdx.x] = r;
    }
}

template <int PASS>
__global__ void __launch_bounds__(R360_OUTLIER_MAXB) k_out_final(const OutlierPartial* __restrict__ partial, int nb, double mul,
                                                                 OutlierHdr* hdr) {
    // the records arrive in LDS with one load per thread; thread 0 adds them in workgroup order
    __shared__ OutlierPartial rec[R360_OUTLIER_MAXB];
    if ((int)threadIdx.x < nb) rec[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    unsigned long long m = 0, sh = 0;
    for (int b = 0; b < nb; ++b) { s += rec[b].sum; m += rec[b].m; sh += rec[b].n_short; }
    if (PASS == 0) {
        hdr->n_stat = m;
        hdr->n_short = sh;
        hdr->sum = s;
        hdr->mean = m ? s / (double)m : 0.0;
    } else {
        hdr->ssq = s;
        const double sd = m < 2 ? 0.0 : sqrt(s / (double)(m - 1));
        hdr->stddev = sd;
        const double t = mul * sd;
        hdr->threshold = hdr->mean + t;
    }
}

__global__ void __launch_bounds__(TPB) k_out_flag_stat(const double* __restrict__ score, size_t n, const OutlierHdr* hdr,
                                                       unsigned* __restrict__ keep) {
    const double thr = hdr->threshold;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const double d = score[i];
        keep[i] = (is_finite_d(d) && d <= thr) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(TPB) k_out_flag_radius(const int* __restrict__ count, size_t n, int min_neighbors,
                                                         unsigned* __restrict__ keep) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const int c = count[i];
        keep[i] = (c >= 0 && c >= min_neighbors) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(TPB) k_out_compact(const uint4* __restrict__ pts, size_t n, const unsigned* __restrict__ keep,
                                                     const unsigned* __restrict__ pos, uint4* __restrict__ out, size_t out_cap,
                                                     OutlierHdr* hdr) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        if (!keep[i]) continue;
        const size_t p = pos[i];
        if (p >= out_cap) { atomicOr(&hdr->err, 4u); continue; }
        out[p] = pts[i];
    }
}

inline int grid_for(size_t items, size_t per_block, int cap) {
    const size_t b = (items + per_block - 1) / per_block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

}  // namespace

int launch_out_init(hipStream_t st, size_t n, double* score, int* count, unsigned* keep) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_out_init, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, score, count, keep);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_cells(hipStream_t st, const uint4* pts, size_t n, const OutlierGrid& G, unsigned long long* keys,
                     size_t table_cap, unsigned* cnt, unsigned* pslot, OutlierHdr* hdr) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_out_cells, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, pts, n, G, keys, (unsigned)(table_cap - 1),
                       cnt, pslot, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_scan(hipStream_t st, const unsigned* v, size_t n, unsigned* bsum, unsigned* out, unsigned long long* total) {
    if (n == 0) return 0;
    const size_t nb = (n + R360_OUTLIER_SCAN_BLOCK - 1) / R360_OUTLIER_SCAN_BLOCK;
    hipLaunchKernelGGL(k_out_scan_reduce, dim3((unsigned)nb), dim3(TPB), 0, st, v, n, bsum);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_out_scan_top, dim3(1), dim3(TPB), 0, st, bsum, nb, total);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_out_scan_apply, dim3((unsigned)nb), dim3(TPB), 0, st, v, n, bsum, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_scatter(hipStream_t st, const uint4* pts, size_t n, const unsigned* pslot, const unsigned* start,
                       unsigned* fill, float4* spts, size_t nf, OutlierHdr* hdr) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_out_scatter, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, pts, n, pslot, start, fill, spts, nf, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_outlier_knn(hipStream_t st, const float4* spts, size_t nf, const OutlierGrid& G, const unsigned long long* keys,
                       size_t table_cap, const unsigned* start, const unsigned* cnt, double lim2, int k, double* score) {
    if (nf == 0) return 0;
    const unsigned nb = (unsigned)((nf + WALK_TPB - 1) / WALK_TPB);
    const size_t lds = sizeof(double) * WALK_TPB * (size_t)k;   // k <= 64: at most 32 KiB
    hipLaunchKernelGGL(k_outlier_knn, dim3(nb), dim3(WALK_TPB), lds, st, spts, (unsigned)nf, G, keys,
                       (unsigned)(table_cap - 1), start, cnt, lim2, k, score);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_outlier_count(hipStream_t st, const float4* spts, size_t nf, const OutlierGrid& G, const unsigned long long* keys,
                         size_t table_cap, const unsigned* start, const unsigned* cnt, double lim2, int stop, int* count) {
    if (nf == 0) return 0;
    const unsigned nb = (unsigned)((nf + WALK_TPB - 1) / WALK_TPB);
    hipLaunchKernelGGL(k_outlier_count, dim3(nb), dim3(WALK_TPB), 0, st, spts, (unsigned)nf, G, keys,
                       (unsigned)(table_cap - 1), start, cnt, lim2, stop, count);
    R360_HIP(hipGetLastError());
    return 0;
}

int outlier_sum_blocks(size_t n) { return grid_for(n, 4 * TPB, R360_OUTLIER_MAXB); }

int launch_out_stats(hipStream_t st, const double* score, size_t n, double mul, OutlierPartial* partial, OutlierHdr* hdr) {
    const int nb = outlier_sum_blocks(n);
    hipLaunchKernelGGL(k_out_sum<0>, dim3(nb), dim3(TPB), 0, st, score, n, hdr, partial);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_out_final<0>, dim3(1), dim3(R360_OUTLIER_MAXB), 0, st, partial, nb, mul, hdr);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_out_sum<1>, dim3(nb), dim3(TPB), 0, st, score, n, hdr, partial);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_out_final<1>, dim3(1), dim3(R360_OUTLIER_MAXB), 0, st, partial, nb, mul, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_flag_stat(hipStream_t st, const double* score, size_t n, const OutlierHdr* hdr, unsigned* keep) {
    hipLaunchKernelGGL(k_out_flag_stat, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, score, n, hdr, keep);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_flag_radius(hipStream_t st, const int* count, size_t n, int min_neighbors, unsigned* keep) {
    hipLaunchKernelGGL(k_out_flag_radius, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, count, n, min_neighbors, keep);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_out_compact(hipStream_t st, const uint4* pts, size_t n, const unsigned* keep, const unsigned* pos, uint4* out,
                       size_t out_cap, OutlierHdr* hdr) {
    hipLaunchKernelGGL(k_out_compact, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, pts, n, keep, pos, out, out_cap, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}
