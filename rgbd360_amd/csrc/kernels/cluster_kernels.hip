// cluster_kernels.hip — pcl::EuclideanClusterExtraction and the normal-aware pcl::extractEuclideanClusters (restated from
// PCL 1.7 segmentation/extract_clusters.h, unpinned) for host clouds and for the context's global map on gfx950.
// Semantics and the divergences from PCL: DESIGN.md §5b-4; the numpy statement is tests/cluster_model.py.
//
//   k_clu_init       parent = the row itself, members = 0, root = label = -1 (what a dropped row keeps)
//   k_clu_union      one lane per point in cell order, over the sparse grid of outlier_kernels.hip: every candidate with
//                    a lower input index within the tolerance (and, conditional form, within the angle) is united with
//                    the point: both roots found, the larger hooked under the smaller by atomicCAS
//   k_clu_flatten    every finite row's root; members per root (integer adds, one per wave and root)
//   k_clu_mark       the roots within the size bounds flagged, the components counted
//   k_clu_list       the flagged roots compacted to (root, size) records: what crosses to the host for ranking
//   k_clu_rank / k_clu_label   a kept root's rank back from the host; every row's label and its member flag
//   k_clu_members / k_clu_bitflag / k_clu_split   the members as (label, input index) pairs in input order, then a stable
//                    split per label bit: after the passes every cluster's members are contiguous, in ascending index
//   k_clu_sum / k_clu_final   per cluster: bounds, centroid, then the centred moments, their eigen-solve and the record
//
// Hang safety: nothing here waits for another wave.  A parent only ever changes from the row itself to a smaller index
// or from an ancestor to a nearer-the-root ancestor, so a find walk visits strictly decreasing indices: at most n steps,
// counted, with an error bit beyond.  A union retries only when its CAS lost, which means another union hooked that
// root: at most n times in all, counted, with an error bit beyond.  On either bit the lane stops uniting.
// The final root of a component is its smallest index whatever the arrival order, the sizes are integer sums, and the
// moments are added in an order fixed by the member lists (ascending index) and the launch shape: two runs give the
// same bytes.  No float atomics (the Makefile keeps -munsafe-fp-atomics off this file).
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int WALK_TPB = 64;       // one wave per workgroup, as the other walks of the grid

#include "sparse_grid.inc"
#include "jacobi3.inc"

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool finite_f(float v) { return finite_bits(__float_as_uint(v)); }
__device__ __forceinline__ unsigned f2ord(unsigned u) { return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
__device__ __forceinline__ float ord2f(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(TPB) k_clu_init(size_t n, int* __restrict__ parent, int* __restrict__ csize,
                                                  int* __restrict__ root, int* __restrict__ labels, ClusterEval E) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        parent[i] = (int)i;
        csize[i] = 0;
        root[i] = -1;
        labels[i] = -1;
        if (E.comp_size) E.comp_size[i] = -1;
    }
}

// The root of x, with path halving (every other node of the walk re-pointed at its grandparent), or -1 with the error
// bit set when the walk took more than n steps.  The re-points are agent-scope atomic stores, like the CAS links.
__device__ int clu_find(int* parent, int x, int n, ClusterHdr* hdr) {
    int p = ld(parent + x);
    for (int step = 0; p != x; ++step) {
        if (step >= n) { atomicOr(&hdr->err, 1u); return -1; }
        const int gp = ld(parent + p);
        if (gp != p) st(parent + x, gp);
        x = gp;
        p = ld(parent + x);
    }
    return x;
}

// a and b into one component: the root of both afterwards, or -1 when a bound was overrun
__device__ int clu_unite(int* parent, int a, int b, int n, ClusterHdr* hdr) {
    for (int tries = 0; tries <= n; ++tries) {
        a = clu_find(parent, a, n, hdr);
        if (a < 0) return -1;
        b = clu_find(parent, b, n, hdr);
        if (b < 0) return -1;
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return b;
        a = old;     // another union hooked a meanwhile: go on from where it points
    }
    atomicOr(&hdr->err, 2u);
    return -1;
}

template <bool COND>
__global__ void __launch_bounds__(WALK_TPB) k_clu_union(const float4* __restrict__ spts, unsigned nf, OutlierGrid G,
                                                        const unsigned long long* __restrict__ keys, unsigned mask,
                                                        const unsigned* __restrict__ start, const unsigned* __restrict__ cnt,
                                                        double lim2, const float* __restrict__ nrm, int nstride, double thr,
                                                        int* parent, int n, ClusterHdr* hdr) {
    const unsigned t = blockIdx.x * WALK_TPB + threadIdx.x;
    if (t >= nf) return;
    const float4 me = spts[t];
    const int self = (int)__float_as_uint(me.w);
    double mnx = 0, mny = 0, mnz = 0;
    if (COND) {
        const float a = nrm[(size_t)self * nstride], b = nrm[(size_t)self * nstride + 1], c = nrm[(size_t)self * nstride + 2];
        if (!(finite_f(a) && finite_f(b) && finite_f(c))) return;   // no edges: a component of one
        mnx = (double)a; mny = (double)b; mnz = (double)c;
    }
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
    const double qx = px / G.ec, qy = py / G.ec, qz = pz / G.ec;
    const double fx = floor(qx), fy = floor(qy), fz = floor(qz);
    const double ux = qx - fx, uy = qy - fy, uz = qz - fz;
    const long long cx = (long long)fx - G.base[0], cy = (long long)fy - G.base[1], cz = (long long)fz - G.base[2];
    const double ec2 = G.ec * G.ec;
    const int R = G.ring;
    int mine = self;    // a node of the point's component near its root: where the next find starts
    for (int dz = -R; dz <= R; ++dz) {
        const double gz = axis_gap(dz, uz);
        for (int dy = -R; dy <= R; ++dy) {
            const double gy = axis_gap(dy, uy);
            for (int dx = -R; dx <= R; ++dx) {
                const double gx = axis_gap(dx, ux);
                if ((gx * gx + gy * gy + gz * gz) * ec2 > lim2) continue;   // nothing in that cell is within reach
                const long long nx = cx + dx, ny = cy + dy, nz = cz + dz;
                if (!(cell_in_range(nx) && cell_in_range(ny) && cell_in_range(nz))) continue;
                const unsigned slot = find_cell(keys, mask, cell_key(nx, ny, nz));
                if (slot == NOSLOT) continue;
                const unsigned b = start[slot], e = b + cnt[slot];
                for (unsigned j = b; j < e; ++j) {
                    const float4 q = spts[j];
                    const int qi = (int)__float_as_uint(q.w);
                    if (qi >= self) continue;    // every edge once, from its higher end
                    const double ddx = (double)q.x - px, ddy = (double)q.y - py, ddz = (double)q.z - pz;
                    const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;   // left to right, uncontracted
                    if (!(d2 <= lim2)) continue;
                    if (COND) {
                        const float a = nrm[(size_t)qi * nstride], bb = nrm[(size_t)qi * nstride + 1],
                                    c = nrm[(size_t)qi * nstride + 2];
                        if (!(finite_f(a) && finite_f(bb) && finite_f(c))) continue;
                        const double dot = mnx * (double)a + mny * (double)bb + mnz * (double)c;
                        if (!(dot >= thr)) continue;
                    }
                    mine = clu_unite(parent, mine, qi, n, hdr);
                    if (mine < 0) return;
                }
            }
        }
    }
}

// Every lane of the wave calls this (v: the lane has a value): one atomicAdd per distinct key among the wave's lanes.
__device__ __forceinline__ void wave_count_by_key(bool v, int key, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(v);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, lead);
        const unsigned long long same = __ballot(v && key == k) & todo;
        if (lane == lead) atomicAdd(&counts[k], __popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(TPB) k_clu_flatten(size_t n, const unsigned* __restrict__ pslot, int* parent,
                                                     int* __restrict__ root, int* __restrict__ csize, ClusterHdr* hdr) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t base = (size_t)blockIdx.x * TPB; base < n; base += stride) {   // uniform trips: the ballots need every lane
        const size_t i = base + threadIdx.x;
        bool v = i < n && pslot[i] != NOSLOT;
        int r = -1;
        if (v) {
            r = clu_find(parent, (int)i, (int)n, hdr);
            v = r >= 0;
            root[i] = r;
        }
        wave_count_by_key(v, r, csize);
    }
}

// one add of the wave's count of `flag` per wave
__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned mine) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += (unsigned)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(dst, (unsigned long long)mine);
}

__global__ void __launch_bounds__(TPB) k_clu_mark(size_t n, const int* __restrict__ root, const int* __restrict__ csize,
                                                  int min_size, int max_size, unsigned* __restrict__ keep, ClusterHdr* hdr,
                                                  ClusterEval E) {
    unsigned comps = 0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const int r = root[i];
        unsigned k = 0;
        if (r >= 0) {
            const int cs = csize[r];
            if (r == (int)i) {
                ++comps;
                k = (cs >= min_size && cs <= max_size) ? 1u : 0u;
            }
            if (E.comp_size) E.comp_size[i] = cs;
        }
        keep[i] = k;
    }
    wave_add(&hdr->n_components, comps);
}

__global__ void __launch_bounds__(TPB) k_clu_list(size_t n, const unsigned* __restrict__ keep, const unsigned* __restrict__ kpos,
                                                  const int* __restrict__ csize, ClusterRec* __restrict__ list, size_t list_cap,
                                                  ClusterHdr* hdr) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        if (!keep[i]) continue;
        const size_t p = kpos[i];
        if (p >= list_cap) { atomicOr(&hdr->err, 4u); continue; }
        ClusterRec r;
        r.root = (int)i;
        r.size = csize[i];
        list[p] = r;
    }
}

__global__ void __launch_bounds__(TPB) k_clu_rank(size_t nk, const int* __restrict__ rank_root, int* __restrict__ crank) {
    for (size_t r = (size_t)blockIdx.x * TPB + threadIdx.x; r < nk; r += (size_t)gridDim.x * TPB) crank[rank_root[r]] = (int)r;
}

__global__ void __launch_bounds__(TPB) k_clu_label(size_t n, const int* __restrict__ root, const unsigned* __restrict__ keep,
                                                   const int* __restrict__ crank, int* __restrict__ labels,
                                                   unsigned* __restrict__ mflag) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const int r = root[i];
        const int lab = (r >= 0 && keep[r]) ? crank[r] : -1;
        labels[i] = lab;
        mflag[i] = lab >= 0 ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(TPB) k_clu_members(size_t n, const unsigned* __restrict__ mflag, const unsigned* __restrict__ mpos,
                                                     const int* __restrict__ labels, int* __restrict__ key, int* __restrict__ val,
                                                     size_t m, ClusterHdr* hdr) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        if (!mflag[i]) continue;
        const size_t p = mpos[i];
        if (p >= m) { atomicOr(&hdr->err, 8u); continue; }
        key[p] = labels[i];
        val[p] = (int)i;
    }
}

__global__ void __launch_bounds__(TPB) k_clu_bitflag(size_t m, const int* __restrict__ key, int bit, unsigned* __restrict__ flag) {
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB)
        flag[j] = ((unsigned)key[j] >> bit & 1u) ^ 1u;
}

// the pairs whose bit is 0 first, then the others, each group in its present order (hdr->n_zero: how many have 0)
__global__ void __launch_bounds__(TPB) k_clu_split(size_t m, const int* __restrict__ key, const int* __restrict__ val,
                                                   const unsigned* __restrict__ flag, const unsigned* __restrict__ fpos,
                                                   const ClusterHdr* hdr, int* __restrict__ key_out, int* __restrict__ val_out) {
    const size_t zeros = (size_t)hdr->n_zero;
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB) {
        const size_t before = fpos[j];
        const size_t p = flag[j] ? before : zeros + (j - before);
        if (p >= m) continue;    // unreachable while the scan is right; never a store out of bounds
        key_out[p] = key[j];
        val_out[p] = val[j];
    }
}

// the cluster whose chunks hold chunk c: cpre[r] <= c < cpre[r + 1]
__device__ __forceinline__ unsigned cluster_of_chunk(const unsigned* __restrict__ cpre, unsigned nk, unsigned c) {
    unsigned lo = 0, hi = nk;     // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (cpre[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per chunk of R360_CLUSTER_CHUNK members of one cluster.  PASS 0: the coordinate sums and the bounds;
// PASS 1: the six centred products.  Thread (members t, t + 256, ...), wave (shuffles), workgroup (LDS, wave order):
// the order is fixed by the member list and the launch shape.
template <int PASS>
__global__ void __launch_bounds__(TPB) k_clu_sum(const uint4* __restrict__ pts, const int* __restrict__ val, unsigned nk,
                                                 const unsigned* __restrict__ off, const unsigned* __restrict__ cpre,
                                                 const double* __restrict__ mean, double* __restrict__ partial,
                                                 ClusterBounds* bounds) {
    const unsigned c = blockIdx.x;
    const unsigned r = cluster_of_chunk(cpre, nk, c);
    const unsigned b = off[r] + (c - cpre[r]) * R360_CLUSTER_CHUNK;
    const unsigned e = min(b + R360_CLUSTER_CHUNK, off[r + 1]);
    double s[6] = {0, 0, 0, 0, 0, 0};
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    double mx = 0, my = 0, mz = 0;
    if (PASS) { mx = mean[3 * r]; my = mean[3 * r + 1]; mz = mean[3 * r + 2]; }
    for (unsigned j = b + threadIdx.x; j < e; j += TPB) {
        const uint4 p = pts[val[j]];
        const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
        if (PASS == 0) {
            s[0] += x; s[1] += y; s[2] += z;
            const unsigned o[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], o[k]); hi[k] = max(hi[k], o[k]); }
        } else {
            const double dx = x - mx, dy = y - my, dz = z - mz;
            s[0] += dx * dx; s[1] += dx * dy; s[2] += dx * dz; s[3] += dy * dy; s[4] += dy * dz; s[5] += dz * dz;
        }
    }
    constexpr int NS = PASS ? 6 : 3;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += __shfl_xor(s[k], o);
        if (PASS == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], o));
                hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], o));
            }
        }
    }
    __shared__ double w_s[TPB / 64][6];
    __shared__ unsigned w_b[TPB / 64][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < NS; ++k) w_s[wave][k] = s[k];
        if (PASS == 0)
            for (int k = 0; k < 3; ++k) { w_b[wave][k] = lo[k]; w_b[wave][3 + k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / 64; ++w)
            for (int k = 0; k < NS; ++k) s[k] += w_s[w][k];
        for (int k = 0; k < NS; ++k) partial[6 * (size_t)c + k] = s[k];
        if (PASS == 0) {
            for (int w = 1; w < TPB / 64; ++w)
                for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], w_b[w][k]); hi[k] = max(hi[k], w_b[w][3 + k]); }
            for (int k = 0; k < 3; ++k) { atomicMin(&bounds[r].mn[k], lo[k]); atomicMax(&bounds[r].mx[k], hi[k]); }
        }
    }
}

__global__ void __launch_bounds__(TPB) k_clu_bounds_init(size_t nk, ClusterBounds* __restrict__ bounds) {
    for (size_t r = (size_t)blockIdx.x * TPB + threadIdx.x; r < nk; r += (size_t)gridDim.x * TPB) {
        ClusterBounds b;
        for (int k = 0; k < 3; ++k) { b.mn[k] = 0xffffffffu; b.mx[k] = 0u; }
        bounds[r] = b;
    }
}

// One thread per cluster: its chunks' sums added in chunk order.  PASS 0: the centroid; PASS 1: the covariance, its
// eigen-solve as k_normals runs it, and the record.
template <int PASS>
__global__ void __launch_bounds__(TPB) k_clu_final(unsigned nk, const int* __restrict__ rank_root, const unsigned* __restrict__ off,
                                                   const unsigned* __restrict__ cpre, const double* __restrict__ partial,
                                                   double* __restrict__ mean, const ClusterBounds* __restrict__ bounds,
                                                   r360_cluster_info* __restrict__ info) {
    const unsigned r = blockIdx.x * TPB + threadIdx.x;
    if (r >= nk) return;
    constexpr int NS = PASS ? 6 : 3;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (unsigned c = cpre[r]; c < cpre[r + 1]; ++c)
        for (int k = 0; k < NS; ++k) s[k] += partial[6 * (size_t)c + k];
    const int size = (int)(off[r + 1] - off[r]);
    const double dm = (double)size;
    if (PASS == 0) {
        for (int k = 0; k < 3; ++k) mean[3 * r + k] = s[k] / dm;
        return;
    }
    r360_cluster_info I;
    I.size = size;
    I.root = rank_root[r];
    for (int k = 0; k < 3; ++k) {
        I.min[k] = ord2f(bounds[r].mn[k]);
        I.max[k] = ord2f(bounds[r].mx[k]);
        I.centroid[k] = mean[3 * r + k];
        I.eig[k] = nan_d();
        I.normal[k] = nan_d();
    }
    I.curvature = nan_d();
    if (size >= 3) {
        double a00 = s[0] / dm, a01 = s[1] / dm, a02 = s[2] / dm, a11 = s[3] / dm, a12 = s[4] / dm, a22 = s[5] / dm;
        double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
        for (int sweep = 0; sweep < 10; ++sweep) {
            if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
            jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        const double w0 = (a00 <= a11 && a00 <= a22) ? 1.0 : 0.0;
        const double w1 = (w0 == 0.0 && a11 <= a22) ? 1.0 : 0.0;
        const double w2 = (1.0 - w0) - w1;
        double ex = (w0 * v00 + w1 * v01) + w2 * v02;
        double ey = (w0 * v10 + w1 * v11) + w2 * v12;
        double ez = (w0 * v20 + w1 * v21) + w2 * v22;
        const double nn = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
        ex *= nn; ey *= nn; ez *= nn;
        // no viewpoint: the largest-magnitude component positive, ties to the lower axis
        const double ax = fabs(ex), ay = fabs(ey), az = fabs(ez);
        const double lead = (ax >= ay && ax >= az) ? ex : (ay >= az ? ey : ez);
        if (lead < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
        const double l0 = fmin(a00, fmin(a11, a22)), l2 = fmax(a00, fmax(a11, a22));
        const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));   // the median
        const double tr = (l0 + l1) + l2;
        I.eig[0] = l0; I.eig[1] = l1; I.eig[2] = l2;
        I.normal[0] = ex; I.normal[1] = ey; I.normal[2] = ez;
        I.curvature = tr == 0.0 ? 0.0 : fabs(l0) / tr;
    }
    info[r] = I;
}

inline int grid_for(size_t items, size_t per_block, int cap) {
    const size_t b = (items + per_block - 1) / per_block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

}  // namespace

int launch_clu_init(hipStream_t st, size_t n, int* parent, int* csize, int* root, int* labels, const ClusterEval& ev) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clu_init, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, parent, csize, root, labels, ev);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_union(hipStream_t st, const float4* spts, size_t nf, const OutlierGrid& G, const unsigned long long* keys,
                     size_t table_cap, const unsigned* start, const unsigned* cnt, double lim2, const float* nrm,
                     int nstride, double thr, int* parent, size_t n, ClusterHdr* hdr) {
    if (nf == 0) return 0;
    const unsigned nb = (unsigned)((nf + WALK_TPB - 1) / WALK_TPB);
    if (nrm)
        hipLaunchKernelGGL(k_clu_union<true>, dim3(nb), dim3(WALK_TPB), 0, st, spts, (unsigned)nf, G, keys,
                           (unsigned)(table_cap - 1), start, cnt, lim2, nrm, nstride, thr, parent, (int)n, hdr);
    else
        hipLaunchKernelGGL(k_clu_union<false>, dim3(nb), dim3(WALK_TPB), 0, st, spts, (unsigned)nf, G, keys,
                           (unsigned)(table_cap - 1), start, cnt, lim2, nrm, nstride, thr, parent, (int)n, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_flatten(hipStream_t st, size_t n, const unsigned* pslot, int* parent, int* root, int* csize, ClusterHdr* hdr) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clu_flatten, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, pslot, parent, root, csize, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_mark(hipStream_t st, size_t n, const int* root, const int* csize, int min_size, int max_size, unsigned* keep,
                    ClusterHdr* hdr, const ClusterEval& ev) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clu_mark, dim3(grid_for(n, TPB, 1024)), dim3(TPB), 0, st, n, root, csize, min_size, max_size, keep,
                       hdr, ev);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_list(hipStream_t st, size_t n, const unsigned* keep, const unsigned* kpos, const int* csize, ClusterRec* list,
                    size_t list_cap, ClusterHdr* hdr) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clu_list, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, keep, kpos, csize, list, list_cap, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_label(hipStream_t st, size_t n, size_t nk, const int* rank_root, int* crank, const int* root,
                     const unsigned* keep, int* labels, unsigned* mflag) {
    if (n == 0) return 0;
    if (nk) {
        hipLaunchKernelGGL(k_clu_rank, dim3(grid_for(nk, TPB, 4096)), dim3(TPB), 0, st, nk, rank_root, crank);
        R360_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_clu_label, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, root, keep, crank, labels, mflag);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_members(hipStream_t st, size_t n, const unsigned* mflag, const unsigned* mpos, const int* labels, int* key,
                       int* val, size_t m, ClusterHdr* hdr) {
    if (n == 0 || m == 0) return 0;
    hipLaunchKernelGGL(k_clu_members, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, mflag, mpos, labels, key, val, m, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_bitflag(hipStream_t st, size_t m, const int* key, int bit, unsigned* flag) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_clu_bitflag, dim3(grid_for(m, TPB, 4096)), dim3(TPB), 0, st, m, key, bit, flag);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_split(hipStream_t st, size_t m, const int* key, const int* val, const unsigned* flag, const unsigned* fpos,
                     const ClusterHdr* hdr, int* key_out, int* val_out) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_clu_split, dim3(grid_for(m, TPB, 4096)), dim3(TPB), 0, st, m, key, val, flag, fpos, hdr, key_out, val_out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_clu_moments(hipStream_t st, const uint4* pts, const int* val, size_t nk, size_t n_chunks, const int* rank_root,
                       const unsigned* off, const unsigned* cpre, double* partial, double* mean, ClusterBounds* bounds,
                       r360_cluster_info* info) {
    if (nk == 0) return 0;
    const dim3 gk(grid_for(nk, TPB, 1 << 22)), gc((unsigned)n_chunks);
    hipLaunchKernelGGL(k_clu_bounds_init, dim3(grid_for(nk, TPB, 4096)), dim3(TPB), 0, st, nk, bounds);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_clu_sum<0>, gc, dim3(TPB), 0, st, pts, val, (unsigned)nk, off, cpre, mean, partial, bounds);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_clu_final<0>, gk, dim3(TPB), 0, st, (unsigned)nk, rank_root, off, cpre, partial, mean, bounds, info);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_clu_sum<1>, gc, dim3(TPB), 0, st, pts, val, (unsigned)nk, off, cpre, mean, partial, bounds);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_clu_final<1>, gk, dim3(TPB), 0, st, (unsigned)nk, rank_root, off, cpre, partial, mean, bounds, info);
    R360_HIP(hipGetLastError());
    return 0;
}
