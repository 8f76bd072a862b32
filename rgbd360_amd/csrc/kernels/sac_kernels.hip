// sac_kernels.hip — RANSAC plane segmentation (pcl::SACSegmentation with the three plane models and SAC_RANSAC, restated;
// PCL is not pinned) for host clouds and for the context's global map on gfx950.  Semantics and the divergences from
// PCL: DESIGN.md §5b-5; the numpy statement is tests/sac_model.py; the sampler and the plane of three points are
// host/sac_sample.h, shared with the host check.
//
//   k_sac_finite / k_sac_pool0   the finite rows flagged (labels = -1), then listed in ascending index: plane 0's pool
//   k_sac_hyp        one thread per hypothesis of the round: three pool positions, the plane, the axis constraint
//   k_sac_count      the hot path: the round's hypotheses in LDS, one pool row per lane in registers, per hypothesis a
//                    ballot and a popcount; per-wave counts meet in LDS, one integer atomicAdd per hypothesis and workgroup
//   k_sac_best       the round's highest count (lowest h) merged with the best so far
//   k_sac_select     inlier flags of one plane over the pool's positions (the count kernel's test, the same function)
//   k_sac_split / k_sac_peel     the inlier list; the labels and the next pool, both in ascending input index
//   k_sac_sum / k_sac_mean / k_sac_fit   chunked fixed-order fp64 moments of an inlier list, the eigen-solve of
//                    kernels/jacobi3.inc, and the refined plane or the plane's record
//
// Nothing waits for another wave.  Counts are integer sums, so arrival order cannot show; the moments are added in an
// order fixed by the list and the launch shape: two runs give the same bytes.  No float atomics (the Makefile keeps
// -munsafe-fp-atomics off this file).
#include "../r360_internal.h"
#include "../host/sac_sample.h"

namespace {

constexpr int TPB = R360_SAC_TPB;
constexpr int WAVES = TPB / 64;

#include "jacobi3.inc"

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool finite_u(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }

inline int grid_for(size_t items, size_t per_block, int cap) {
    const size_t b = (items + per_block - 1) / per_block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

__global__ void __launch_bounds__(TPB) k_sac_finite(const uint4* __restrict__ pts, size_t n, unsigned* __restrict__ flag,
                                                    int* __restrict__ labels) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const uint4 p = pts[i];
        flag[i] = (finite_u(p.x) && finite_u(p.y) && finite_u(p.z)) ? 1u : 0u;
        labels[i] = -1;
    }
}

__global__ void __launch_bounds__(TPB) k_sac_pool0(size_t n, const unsigned* __restrict__ flag, const unsigned* __restrict__ fpos,
                                                   int* __restrict__ pool) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB)
        if (flag[i]) pool[fpos[i]] = (int)i;     // fpos[i] <= i < n
}

__global__ void __launch_bounds__(R360_SAC_ROUND) k_sac_hyp(const uint4* __restrict__ pts, const int* __restrict__ pool,
                                                            SacSearch S, int h0, int nh, double* __restrict__ coef,
                                                            int* __restrict__ samples) {
    const int t = blockIdx.x * R360_SAC_ROUND + threadIdx.x;
    if (t >= nh) return;
    uint64_t pos[3];
    sac_sample3(S.seed, S.p, (uint32_t)(h0 + t), (uint64_t)S.m, pos);     // every position < m
    float q[3][3];
    for (int k = 0; k < 3; ++k) {
        const int i = pool[pos[k]];
        const uint4 p = pts[i];
        q[k][0] = __uint_as_float(p.x); q[k][1] = __uint_as_float(p.y); q[k][2] = __uint_as_float(p.z);
        if (samples) samples[3 * (size_t)t + k] = i;
    }
    double c[4];
    bool ok = sac_plane3(q[0], q[1], q[2], c);
    if (ok && S.constraint != R360_SAC_NONE) {
        const double dot = fabs((c[0] * S.axis[0] + c[1] * S.axis[1]) + c[2] * S.axis[2]);
        ok = S.constraint == R360_SAC_PERPENDICULAR ? dot >= S.cos_eps : dot <= S.sin_eps;
    }
    for (int k = 0; k < 4; ++k) coef[4 * (size_t)t + k] = ok ? c[k] : nan_d();
}

// one pool row as a lane holds it
struct SacRow { double x, y, z, nx, ny, nz; bool ok, nok; };

template <bool GATE>
__device__ __forceinline__ SacRow sac_load(const uint4* __restrict__ pts, const int* __restrict__ pool, size_t j, size_t m,
                                           const SacGate& G) {
    SacRow r = {0, 0, 0, 0, 0, 0, false, false};
    if (j < m) {
        const int i = pool[j];
        const uint4 p = pts[i];
        r.x = (double)__uint_as_float(p.x); r.y = (double)__uint_as_float(p.y); r.z = (double)__uint_as_float(p.z);
        r.ok = true;
        if (GATE) {
            const float* q = G.nrm + (size_t)i * G.nstride;
            const float a = q[0], b = q[1], c = q[2];
            r.nok = finite_u(__float_as_uint(a)) && finite_u(__float_as_uint(b)) && finite_u(__float_as_uint(c));
            r.nx = (double)a; r.ny = (double)b; r.nz = (double)c;
        }
    }
    return r;
}

// the inlier test: count and select share it.  NaN coefficients make every comparison false.
template <bool GATE>
__device__ __forceinline__ bool sac_inlier(const SacRow& r, double a, double b, double c, double d, double thr, double cos_n) {
    bool in = r.ok && fabs(((a * r.x + b * r.y) + c * r.z) + d) <= thr;
    if (GATE) in = in && r.nok && fabs((r.nx * a + r.ny * b) + r.nz * c) >= cos_n;
    return in;
}

template <bool GATE>
__global__ void __launch_bounds__(TPB) k_sac_count(const uint4* __restrict__ pts, const int* __restrict__ pool, size_t m,
                                                   SacGate G, const double* __restrict__ coef, int nh, int* __restrict__ count) {
    __shared__ double s_coef[R360_SAC_ROUND * 4];
    __shared__ int s_cnt[WAVES][R360_SAC_ROUND];
    for (int t = threadIdx.x; t < R360_SAC_ROUND * 4; t += TPB) s_coef[t] = t < nh * 4 ? coef[t] : nan_d();
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c0 = 0, c1 = 0;       // lane l keeps the wave's counts of hypotheses l and 64 + l
    // the bound is the workgroup's, so whole waves take every ballot
    for (size_t base = (size_t)blockIdx.x * TPB; base < m; base += (size_t)gridDim.x * TPB) {
        const SacRow r = sac_load<GATE>(pts, pool, base + threadIdx.x, m, G);
        // whole halves of the round, so the trip counts are fixed: a slot beyond nh holds NaN and counts nothing
#pragma unroll 8
        for (int h = 0; h < 64; ++h) {
            const bool in = sac_inlier<GATE>(r, s_coef[4 * h], s_coef[4 * h + 1], s_coef[4 * h + 2], s_coef[4 * h + 3], G.thr,
                                             G.cos_n);
            const int pc = __popcll(__ballot(in));
            c0 += lane == h ? pc : 0;
        }
        if (nh > 64)
#pragma unroll 8
        for (int h = 64; h < R360_SAC_ROUND; ++h) {
            const bool in = sac_inlier<GATE>(r, s_coef[4 * h], s_coef[4 * h + 1], s_coef[4 * h + 2], s_coef[4 * h + 3], G.thr,
                                             G.cos_n);
            const int pc = __popcll(__ballot(in));
            c1 += lane == h - 64 ? pc : 0;
        }
    }
    s_cnt[wave][lane] = c0;
    s_cnt[wave][64 + lane] = c1;
    __syncthreads();
    if ((int)threadIdx.x < nh) {
        int s = 0;
        for (int w = 0; w < WAVES; ++w) s += s_cnt[w][threadIdx.x];
        if (s) atomicAdd(&count[threadIdx.x], s);
    }
}

__global__ void __launch_bounds__(64) k_sac_best(const int* __restrict__ count, const double* __restrict__ coef, int h0, int nh,
                                                 SacHdr* hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int best = hdr->best_count, at = -1;
    for (int t = 0; t < nh; ++t)
        if (count[t] > best) { best = count[t]; at = t; }     // strictly: ties stay with the lowest h
    if (at >= 0) {
        hdr->best_count = best;
        hdr->best_h = h0 + at;
        for (int k = 0; k < 4; ++k) hdr->best_coef[k] = coef[4 * at + k];
    }
}

template <bool GATE>
__global__ void __launch_bounds__(TPB) k_sac_select(const uint4* __restrict__ pts, const int* __restrict__ pool, size_t m,
                                                    SacGate G, const double* __restrict__ coef, unsigned* __restrict__ flag) {
    const double a = coef[0], b = coef[1], c = coef[2], d = coef[3];
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB) {
        const SacRow r = sac_load<GATE>(pts, pool, j, m, G);
        flag[j] = sac_inlier<GATE>(r, a, b, c, d, G.thr, G.cos_n) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(TPB) k_sac_split(const int* __restrict__ pool, size_t m, const unsigned* __restrict__ flag,
                                                   const unsigned* __restrict__ fpos, int* __restrict__ inl, size_t inl_cap,
                                                   SacHdr* hdr) {
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB) {
        if (!flag[j]) continue;
        const size_t q = fpos[j];
        if (q >= inl_cap) { atomicOr(&hdr->err, 1u); continue; }
        inl[q] = pool[j];
    }
}

__global__ void __launch_bounds__(TPB) k_sac_peel(const int* __restrict__ pool, size_t m, const unsigned* __restrict__ flag,
                                                  const unsigned* __restrict__ fpos, int p, int* __restrict__ labels,
                                                  int* __restrict__ next, size_t n, SacHdr* hdr) {
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB) {
        const int i = pool[j];
        if ((size_t)(unsigned)i >= n) { atomicOr(&hdr->err, 1u); continue; }
        if (flag[j]) labels[i] = p;
        else next[j - fpos[j]] = i;      // fpos[j] <= j: the position is below m
    }
}

// One workgroup per chunk of R360_SAC_CHUNK list entries, as the cluster records' sums run: thread (entries t, t + 256,
// ...), wave (shuffles), workgroup (LDS, wave order).  PASS 0: the coordinate sums; PASS 1: the six centred products.
template <int PASS>
__global__ void __launch_bounds__(TPB) k_sac_sum(const uint4* __restrict__ pts, const int* __restrict__ inl, unsigned cnt,
                                                 const double* __restrict__ mean, double* __restrict__ partial) {
    const unsigned c = blockIdx.x;
    const unsigned b = c * R360_SAC_CHUNK;
    const unsigned e = min(b + R360_SAC_CHUNK, cnt);
    double s[6] = {0, 0, 0, 0, 0, 0};
    double mx = 0, my = 0, mz = 0;
    if (PASS) { mx = mean[0]; my = mean[1]; mz = mean[2]; }
    for (unsigned j = b + threadIdx.x; j < e; j += TPB) {
        const uint4 p = pts[inl[j]];
        const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
        if (PASS == 0) {
            s[0] += x; s[1] += y; s[2] += z;
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
    }
    __shared__ double w_s[WAVES][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NS; ++k) w_s[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w)
            for (int k = 0; k < NS; ++k) s[k] += w_s[w][k];
        for (int k = 0; k < NS; ++k) partial[6 * (size_t)c + k] = s[k];
    }
}

__global__ void __launch_bounds__(64) k_sac_mean(const double* __restrict__ partial, unsigned n_chunks, unsigned cnt,
                                                 double* __restrict__ mean) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[3] = {0, 0, 0};
    for (unsigned c = 0; c < n_chunks; ++c)
        for (int k = 0; k < 3; ++k) s[k] += partial[6 * (size_t)c + k];
    for (int k = 0; k < 3; ++k) mean[k] = s[k] / (double)cnt;
}

// One thread: the chunks' sums in chunk order, the covariance, its eigen-solve as k_clu_final runs it.  rec NULL: the
// refined plane into hdr->ref_coef.  Otherwise the record.
__global__ void __launch_bounds__(64) k_sac_fit(const double* __restrict__ partial, unsigned n_chunks, unsigned cnt,
                                                const double* __restrict__ mean, SacHdr* hdr, r360_sac_plane* rec, int refined,
                                                int raw_size, int evaluated) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (unsigned c = 0; c < n_chunks; ++c)
        for (int k = 0; k < 6; ++k) s[k] += partial[6 * (size_t)c + k];
    const double dm = (double)cnt;
    double ex = nan_d(), ey = nan_d(), ez = nan_d(), l0 = nan_d(), l1 = nan_d(), l2 = nan_d(), curv = nan_d();
    if (cnt >= 3) {
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
        ex = (w0 * v00 + w1 * v01) + w2 * v02;
        ey = (w0 * v10 + w1 * v11) + w2 * v12;
        ez = (w0 * v20 + w1 * v21) + w2 * v22;
        const double nn = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
        ex *= nn; ey *= nn; ez *= nn;
        l0 = fmin(a00, fmin(a11, a22)); l2 = fmax(a00, fmax(a11, a22));
        l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));   // the median
        const double tr = (l0 + l1) + l2;
        curv = tr == 0.0 ? 0.0 : fabs(l0) / tr;
    }
    if (!rec) {
        hdr->ref_coef[0] = ex; hdr->ref_coef[1] = ey; hdr->ref_coef[2] = ez;
        hdr->ref_coef[3] = -((ex * mean[0] + ey * mean[1]) + ez * mean[2]);
        return;
    }
    r360_sac_plane R;
    const double* src = refined ? hdr->ref_coef : hdr->best_coef;
    double c0 = src[0], c1 = src[1], c2 = src[2], c3 = src[3];
    // the largest-magnitude component of the normal positive, ties to the lower axis
    const double ax = fabs(c0), ay = fabs(c1), az = fabs(c2);
    const double lead = (ax >= ay && ax >= az) ? c0 : (ay >= az ? c1 : c2);
    if (lead < 0.0) { c0 = -c0; c1 = -c1; c2 = -c2; c3 = -c3; }
    R.coef[0] = c0; R.coef[1] = c1; R.coef[2] = c2; R.coef[3] = c3;
    for (int k = 0; k < 3; ++k) R.centroid[k] = mean[k];
    R.eig[0] = l0; R.eig[1] = l1; R.eig[2] = l2;
    R.curvature = curv;
    R.size = (int)cnt;
    R.raw_size = raw_size;
    R.best_hypothesis = hdr->best_h;
    R.evaluated = evaluated;
    *rec = R;
}

__global__ void __launch_bounds__(TPB) k_sac_keepflag(const int* __restrict__ labels, size_t n, int keep_planes,
                                                      unsigned* __restrict__ flag) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB)
        flag[i] = ((labels[i] >= 0) == (keep_planes != 0)) ? 1u : 0u;
}

}  // namespace

int launch_sac_finite(hipStream_t st, const uint4* pts, size_t n, unsigned* flag, int* labels) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sac_finite, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, pts, n, flag, labels);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_pool0(hipStream_t st, size_t n, const unsigned* flag, const unsigned* fpos, int* pool) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sac_pool0, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, n, flag, fpos, pool);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_hyp(hipStream_t st, const uint4* pts, const int* pool, const SacSearch& S, int h0, int nh, double* coef,
                   int* samples) {
    if (nh <= 0) return 0;
    if (S.m < 3) { r360_set_error("sac: internal error (a pool of %u rows sampled)", S.m); return -1; }
    hipLaunchKernelGGL(k_sac_hyp, dim3((nh + R360_SAC_ROUND - 1) / R360_SAC_ROUND), dim3(R360_SAC_ROUND), 0, st, pts, pool, S,
                       h0, nh, coef, samples);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_count(hipStream_t st, const uint4* pts, const int* pool, size_t m, const SacGate& G, const double* coef, int nh,
                     int* count) {
    if (nh <= 0 || m == 0) return 0;
    if (nh > R360_SAC_ROUND) { r360_set_error("sac: internal error (%d hypotheses in one round)", nh); return -1; }
    const dim3 g(grid_for(m, TPB, R360_SAC_MAXB));
    if (G.nrm)
        hipLaunchKernelGGL(k_sac_count<true>, g, dim3(TPB), 0, st, pts, pool, m, G, coef, nh, count);
    else
        hipLaunchKernelGGL(k_sac_count<false>, g, dim3(TPB), 0, st, pts, pool, m, G, coef, nh, count);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_best(hipStream_t st, const int* count, const double* coef, int h0, int nh, SacHdr* hdr) {
    if (nh <= 0) return 0;
    hipLaunchKernelGGL(k_sac_best, dim3(1), dim3(64), 0, st, count, coef, h0, nh, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_select(hipStream_t st, const uint4* pts, const int* pool, size_t m, const SacGate& G, const double* coef,
                      unsigned* flag) {
    if (m == 0) return 0;
    const dim3 g(grid_for(m, TPB, 4096));
    if (G.nrm)
        hipLaunchKernelGGL(k_sac_select<true>, g, dim3(TPB), 0, st, pts, pool, m, G, coef, flag);
    else
        hipLaunchKernelGGL(k_sac_select<false>, g, dim3(TPB), 0, st, pts, pool, m, G, coef, flag);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_split(hipStream_t st, const int* pool, size_t m, const unsigned* flag, const unsigned* fpos, int* inl,
                     size_t inl_cap, SacHdr* hdr) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_sac_split, dim3(grid_for(m, TPB, 4096)), dim3(TPB), 0, st, pool, m, flag, fpos, inl, inl_cap, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_peel(hipStream_t st, const int* pool, size_t m, const unsigned* flag, const unsigned* fpos, int p, int* labels,
                    int* next, size_t n, SacHdr* hdr) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_sac_peel, dim3(grid_for(m, TPB, 4096)), dim3(TPB), 0, st, pool, m, flag, fpos, p, labels, next, n, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_moments(hipStream_t st, const uint4* pts, const int* inl, size_t cnt, double* partial, double* mean,
                       SacHdr* hdr, r360_sac_plane* rec, bool refined, int raw_size, int evaluated) {
    if (cnt == 0) { r360_set_error("sac: internal error (moments of no points)"); return -1; }
    const unsigned nc = (unsigned)((cnt + R360_SAC_CHUNK - 1) / R360_SAC_CHUNK);
    hipLaunchKernelGGL(k_sac_sum<0>, dim3(nc), dim3(TPB), 0, st, pts, inl, (unsigned)cnt, mean, partial);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sac_mean, dim3(1), dim3(64), 0, st, partial, nc, (unsigned)cnt, mean);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sac_sum<1>, dim3(nc), dim3(TPB), 0, st, pts, inl, (unsigned)cnt, mean, partial);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sac_fit, dim3(1), dim3(64), 0, st, partial, nc, (unsigned)cnt, mean, hdr, rec, refined ? 1 : 0,
                       raw_size, evaluated);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_sac_keepflag(hipStream_t st, const int* labels, size_t n, int keep_planes, unsigned* flag) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sac_keepflag, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, labels, n, keep_planes, flag);
    R360_HIP(hipGetLastError());
    return 0;
}
