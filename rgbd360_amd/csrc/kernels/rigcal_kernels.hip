// rigcal_kernels.hip — rig extrinsic calibration from control planes (the reference's include/Calibration.h,
// restated: tests/rigcal_model.py) on gfx950, fp64 throughout.
//
//   k_rigcal_accum    one lane per correspondence row, 256 rows per workgroup, a workgroup inside one sensor pair: the
//                     row's 3x3 blocks ii, ij, jj, its two gradient 3-vectors and its scalars at the current
//                     rotations, summed over the workgroup into one record; the cost-only form writes the weighted
//                     error at the trial rotations alone
//   k_rigcal_pairsum  one workgroup: a wave per pair adds the pair's records in record order, then the blocks are
//                     scattered into the 21x21 matrix and the 21-vector as the reference's loops do (sensor 0's part
//                     skipped, the lower cross block the transpose of the upper) and the scalars added in pair order
//   k_rigcal_ransac   one wave per trial of the outlier trimmer: the draw (a lane-uniform integer hash, redrawn
//                     against the degenerate test), the pair fit (one-sided Jacobi SVD in registers, a 3x3 solve),
//                     lanes striding over the rows, the wave's inlier count
//   k_rigcal_mask     the inlier mask of one trial
//   k_rigcal_pixsum   the collector: per (sensor, label) the pixel count and the sum of (row + col) over a frame's
//                     final label image, one workgroup per key, integers
//
// No atomics anywhere and every sum has an order fixed by the data alone: two runs give the same bytes (the Makefile
// keeps -munsafe-fp-atomics off this file).  The 3-term products repeat the model's order of additions,
// (a0 b0 + a1 b1) + a2 b2, uncontracted, so a row's terms are the model's doubles.
#include "../r360_internal.h"

namespace {

constexpr int TPB = R360_RIGCAL_TPB;
constexpr int REC = R360_RIGCAL_REC;
constexpr int NV = 37;   // values per row: ii 0..8, ij 9..17, jj 18..26, g_i 27..29, g_j 30..32, scalars 33..36

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// pair index -> (s1, s2), s1 < s2, in the order (0,1) (0,2) .. (0,7) (1,2) .. (6,7)
__device__ __forceinline__ void pair_sensors(int p, int& s1, int& s2) {
    s1 = 0;
    int len = 7;
    while (p >= len) { p -= len; ++s1; --len; }
    s2 = s1 + 1 + p;
}

__device__ __forceinline__ void rotate(const double* __restrict__ R, double x, double y, double z, double n[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) n[r] = dot3(R[r * 3 + 0], x, R[r * 3 + 1], y, R[r * 3 + 2], z);
}

// A^T B for 3x3 arrays, the summed index in the fixed order
__device__ __forceinline__ void atb(const double (&A)[3][3], const double (&B)[3][3], double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[r * 3 + c] = dot3(A[0][r], B[0][c], A[1][r], B[1][c], A[2][r], B[2][c]);
}

template <int MODE, bool COST_ONLY>
__global__ void __launch_bounds__(TPB) k_rigcal_accum(RigcalDev D, const double* __restrict__ rot, int weighted) {
    __shared__ double lds[TPB / 64][REC];
    const int wg = blockIdx.x;
    const int pair = D.wg_pair[wg];
    const int row = D.pair_start[pair] + (wg - D.wg_start[pair]) * TPB + (int)threadIdx.x;
    const bool valid = row < D.pair_start[pair + 1];
    int s1, s2;
    pair_sensors(pair, s1, s2);
    const double* R1 = rot + (COST_ONLY ? 72 : 0) + 9 * s1;
    const double* R2 = rot + (COST_ONLY ? 72 : 0) + 9 * s2;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    if (valid) {
        const double* q = D.rows + (size_t)row * 10;
        double ni[3], nii[3];
        rotate(R1, q[0], q[1], q[2], ni);
        rotate(R2, q[4], q[5], q[6], nii);
        const double wrow = q[8] / (q[3] * q[9]);
        const double w = weighted ? wrow : 1.0;
        if (MODE == 0) {
            const double e[3] = {ni[0] - nii[0], ni[1] - nii[1], ni[2] - nii[2]};
            const double e2 = dot3(e[0], e[0], e[1], e[1], e[2], e[2]);
            v[36] = wrow * e2;
            if (!COST_ONLY) {
                const double m0 = -ni[0], m1 = -ni[1], m2 = -ni[2];
                const double Ji[3][3] = {{0.0, -m2, m1}, {m2, 0.0, -m0}, {-m1, m0, 0.0}};
                const double Jii[3][3] = {{0.0, -nii[2], nii[1]}, {nii[2], 0.0, -nii[0]}, {-nii[1], nii[0], 0.0}};
                atb(Ji, Ji, v);
                atb(Ji, Jii, v + 9);
                atb(Jii, Jii, v + 18);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    v[27 + r] = dot3(Ji[0][r], e[0], Ji[1][r], e[1], Ji[2][r], e[2]);
                    v[30 + r] = dot3(Jii[0][r], e[0], Jii[1][r], e[1], Jii[2][r], e[2]);
                }
#pragma unroll
                for (int k = 0; k < 33; ++k) v[k] = w * v[k];
                const double d = dot3(ni[0], nii[0], ni[1], nii[1], ni[2], nii[2]);
                v[33] = e2;
                v[34] = acos(fmin(1.0, fmax(-1.0, d)));
                v[35] = 1.0;
            }
        } else {
            const double e = q[3] - q[7];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[r * 3 + c] = w * (ni[r] * ni[c]);
                    v[9 + r * 3 + c] = w * (-ni[r] * nii[c]);
                    v[18 + r * 3 + c] = w * (nii[r] * nii[c]);
                }
                v[27 + r] = w * (-ni[r] * e);
                v[30 + r] = w * (nii[r] * e);
            }
            v[33] = e * e;
            v[35] = 1.0;
        }
    }
    // lanes by the shuffle tree, then the waves in wave order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = COST_ONLY ? 36 : 0; k < NV; ++k) {
        double x = v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
        if (lane == 0) lds[wave][k] = x;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < REC && (!COST_ONLY || k == 36)) {
        double s = 0.0;
        if (k < NV) {
            s = lds[0][k];
#pragma unroll
            for (int w = 1; w < TPB / 64; ++w) s += lds[w][k];
        }
        D.rec[(size_t)wg * REC + k] = s;
    }
}

__global__ void __launch_bounds__(1024) k_rigcal_pairsum(RigcalDev D, int cost_only) {
    __shared__ double psum[R360_RIGCAL_PAIRS][REC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < R360_RIGCAL_PAIRS; p += 16) {
        if (lane < REC && (!cost_only || lane == 36)) {
            double acc = 0.0;
            for (int wg = D.wg_start[p]; wg < D.wg_start[p + 1]; ++wg) acc += D.rec[(size_t)wg * REC + lane];
            psum[p][lane] = acc;
        }
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (cost_only) {
        if (e == 0) {
            double acc = 0.0;
            for (int p = 0; p < R360_RIGCAL_PAIRS; ++p) acc += psum[p][36];
            D.out[R360_RIGCAL_OUT - 1] = acc;
        }
        return;
    }
    if (e < 441) {
        const int r = e / 21, c = e % 21;
        const int br = r / 3, bc = c / 3, rr = r % 3, cc = c % 3;
        double acc = 0.0;
        int p = 0;
        for (int s1 = 0; s1 < 7; ++s1)
            for (int s2 = s1 + 1; s2 < 8; ++s2, ++p) {
                if (D.wg_start[p + 1] == D.wg_start[p]) continue;   // no rows: the reference's map has no such pair
                if (br == bc) {
                    if (s1 == br + 1) acc += psum[p][rr * 3 + cc];
                    if (s2 == br + 1) acc += psum[p][18 + rr * 3 + cc];
                } else if (br < bc) {
                    if (s1 == br + 1 && s2 == bc + 1) acc += psum[p][9 + rr * 3 + cc];
                } else {
                    if (s1 == bc + 1 && s2 == br + 1) acc += psum[p][9 + cc * 3 + rr];
                }
            }
        D.out[e] = acc;
    } else if (e < 462) {
        const int i = e - 441, k = i / 3 + 1, rr = i % 3;
        double acc = 0.0;
        int p = 0;
        for (int s1 = 0; s1 < 7; ++s1)
            for (int s2 = s1 + 1; s2 < 8; ++s2, ++p) {
                if (D.wg_start[p + 1] == D.wg_start[p]) continue;
                if (s1 == k) acc += psum[p][27 + rr];
                if (s2 == k) acc += psum[p][30 + rr];
            }
        D.out[e] = acc;
    } else if (e < 466) {
        double acc = 0.0;
        for (int p = 0; p < R360_RIGCAL_PAIRS; ++p)
            if (D.wg_start[p + 1] != D.wg_start[p]) acc += psum[p][33 + (e - 462)];
        D.out[e] = acc;
    }
}

// ------------------------------------------------------------------ the outlier trimmer
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// rigcal_model.draw3
__device__ __forceinline__ void draw3(unsigned seed, unsigned trial, unsigned redraw, unsigned n, int idx[3]) {
    const unsigned h = mix32(seed ^ mix32(trial * 0x9E3779B9u + mix32(redraw + 0x85EBCA6Bu)));
    unsigned i0 = mix32(h + 1u) % n;
    unsigned i1 = mix32(h + 2u) % (n - 1u);
    if (i1 >= i0) ++i1;
    unsigned i2 = mix32(h + 3u) % (n - 2u);
    const unsigned lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    idx[0] = (int)i0; idx[1] = (int)i1; idx[2] = (int)i2;
}

// A^-1 b by cofactors (rigcal_model.inv3_apply); false when the determinant is zero or not finite
__device__ __forceinline__ bool inv3_apply(const double (&A)[3][3], const double b[3], double x[3]) {
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1];
    const double c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    const double c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double det = (A[0][0] * c00 + A[0][1] * c01) + A[0][2] * c02;
    if (det == 0.0 || !isfinite(det)) return false;
    const double c10 = A[0][2] * A[2][1] - A[0][1] * A[2][2];
    const double c11 = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    const double c12 = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    const double c20 = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    const double c21 = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    const double c22 = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    x[0] = ((c00 * b[0] + c10 * b[1]) + c20 * b[2]) / det;
    x[1] = ((c01 * b[0] + c11 * b[1]) + c21 * b[2]) / det;
    x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return true;
}

// one Hestenes rotation of columns P, Q of G (and of V)
template <int P, int Q>
__device__ __forceinline__ void hestenes(double (&G)[3][3], double (&V)[3][3]) {
    const double alpha = dot3(G[0][P], G[0][P], G[1][P], G[1][P], G[2][P], G[2][P]);
    const double beta = dot3(G[0][Q], G[0][Q], G[1][Q], G[1][Q], G[2][Q], G[2][Q]);
    const double gamma = dot3(G[0][P], G[0][Q], G[1][P], G[1][Q], G[2][P], G[2][Q]);
    if (gamma == 0.0) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[r][P], gq = G[r][Q], vp = V[r][P], vq = V[r][Q];
        G[r][P] = c * gp - s * gq;
        G[r][Q] = s * gp + c * gq;
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

// The trial's model: the first non-degenerate draw of at most max_redraws, then the live getAlignment
// (rigcal_model.fit_pair).  Lane-uniform: every lane computes the same.  Returns 0 no draw, 1 a model, 2 a draw whose
// translation system is singular or whose C is rank-deficient (scores 0).
__device__ int fit_trial(const double* __restrict__ rows, int m, unsigned seed, int trial, const RigcalTrimParams& p,
                         double R[9], double t[3]) {
    int idx[3];
    bool found = false;
    for (int redraw = 0; redraw < p.max_redraws && !found; ++redraw) {
        draw3(seed, (unsigned)trial, (unsigned)redraw, (unsigned)m, idx);
        const double* a = rows + (size_t)idx[0] * 10;
        const double* b = rows + (size_t)idx[1] * 10;
        const double* c = rows + (size_t)idx[2] * 10;
        const double x0 = b[1] * c[2] - b[2] * c[1], x1 = b[2] * c[0] - b[0] * c[2], x2 = b[0] * c[1] - b[1] * c[0];
        found = !(fabs(dot3(a[0], x0, a[1], x1, a[2], x2)) < p.degenerate);
    }
    if (!found) return 0;
    double C[3][3] = {{1.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double A[3][3] = {{1.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* q = rows + (size_t)idx[k] * 10;
        const double e = q[3] - q[7];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                C[r][c] += q[4 + r] * q[c];
                A[r][c] += q[r] * q[c];
            }
            g[r] += q[r] * e;
        }
    }
    double x[3];
    if (!inv3_apply(A, g, x)) return 2;
    t[0] = -x[0]; t[1] = -x[1]; t[2] = -x[2];
    const double detC = (C[0][0] * (C[1][1] * C[2][2] - C[1][2] * C[2][1]) + C[0][1] * (C[1][2] * C[2][0] - C[1][0] * C[2][2])) +
                        C[0][2] * (C[1][0] * C[2][1] - C[1][1] * C[2][0]);
    // C V = U S by one-sided Jacobi: the columns of G end up orthogonal, s_k u_k
    double G[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = C[r][c];
    for (int sweep = 0; sweep < 12; ++sweep) {
        hestenes<0, 1>(G, V);
        hestenes<0, 2>(G, V);
        hestenes<1, 2>(G, V);
    }
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = sqrt(dot3(G[0][k], G[0][k], G[1][k], G[1][k], G[2][k], G[2][k]));
    const int kmin = (s[0] <= s[1] && s[0] <= s[2]) ? 0 : (s[1] <= s[2] ? 1 : 2);
    // a rank-deficient C (the drawn n_ii coplanar) defines no rotation: the trial scores 0 (rigcal_model.FIT_RCOND)
    if (!(s[kmin] > 1e-6 * fmax(s[0], fmax(s[1], s[2])))) return 2;
    // R = V diag(1, 1, det) U^T, the sign on the smallest singular value
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double d = (k == kmin && detC < 0.0) ? -1.0 : 1.0;
                acc += d * V[r][k] * (G[c][k] / s[k]);
            }
            R[r * 3 + c] = acc;
        }
    return 1;
}

__device__ __forceinline__ bool is_inlier(const double* __restrict__ q, const double R[9], const double t[3], double dist) {
    double rn[3];
    rotate(R, q[4], q[5], q[6], rn);
    const double d_err = fabs((q[7] - dot3(t[0], q[0], t[1], q[1], t[2], q[2])) - q[3]);
    const double c0 = q[1] * rn[2] - q[2] * rn[1], c1 = q[2] * rn[0] - q[0] * rn[2], c2 = q[0] * rn[1] - q[1] * rn[0];
    const double a_err = sqrt(dot3(c0, c0, c1, c1, c2, c2));
    return d_err < dist && a_err < dist / 2;
}

__global__ void __launch_bounds__(TPB) k_rigcal_ransac(const double* __restrict__ rows, int m, unsigned seed, int trial0, int n,
                                                       RigcalTrimParams p, int* __restrict__ counts, int* __restrict__ flags) {
    const int k = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= n) return;
    double R[9], t[3];
    const int has = fit_trial(rows, m, seed, trial0 + k, p, R, t);
    int cnt = 0;
    if (has == 1)
        for (int i = lane; i < m; i += 64) cnt += is_inlier(rows + (size_t)i * 10, R, t, p.dist) ? 1 : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_down(cnt, s, 64);
    if (lane == 0) {
        counts[k] = cnt;
        flags[k] = has == 0 ? 1 : 0;
    }
}

__global__ void __launch_bounds__(TPB) k_rigcal_mask(const double* __restrict__ rows, int m, unsigned seed, int trial,
                                                     RigcalTrimParams p, unsigned char* __restrict__ mask) {
    double R[9], t[3];
    const int has = fit_trial(rows, m, seed, trial, p, R, t);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < m; i += gridDim.x * TPB)
        mask[i] = (has == 1 && is_inlier(rows + (size_t)i * 10, R, t, p.dist)) ? 1 : 0;
}

// One workgroup per key {sensor, label}: the count and the sum of (row + col) of the organised-cloud indices that carry
// the label in the sensor's final label image.  Integers, so the tree's order does not matter.
__global__ void __launch_bounds__(TPB) k_rigcal_pixsum(const int* __restrict__ labf, int w, int h, const int2* __restrict__ keys,
                                                       longlong2* __restrict__ out) {
    __shared__ long long lds[TPB / 64][2];
    const int2 key = keys[blockIdx.x];
    const int* img = labf + (size_t)key.x * w * h;
    long long cnt = 0, sum = 0;
    for (int i = threadIdx.x; i < w * h; i += TPB)
        if (img[i] == key.y) { ++cnt; sum += i / w + i % w; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { cnt += __shfl_down(cnt, m, 64); sum += __shfl_down(sum, m, 64); }
    if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = cnt; lds[threadIdx.x >> 6][1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TPB / 64; ++k) { cnt += lds[k][0]; sum += lds[k][1]; }
        out[blockIdx.x] = make_longlong2(cnt, sum);
    }
}

}  // namespace

int launch_rigcal_pixsum(hipStream_t st, const int* labf, int w, int h, const int2* keys, int n_keys, longlong2* out) {
    if (n_keys <= 0) return 0;
    hipLaunchKernelGGL(k_rigcal_pixsum, dim3(n_keys), dim3(TPB), 0, st, labf, w, h, keys, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_rigcal_accum(hipStream_t st, const RigcalDev& D, const double* rot, int mode, bool weighted, bool cost_only) {
    if (D.nwg > 0) {
        const dim3 g(D.nwg), b(TPB);
        const int w = weighted ? 1 : 0;
        if (cost_only) hipLaunchKernelGGL((k_rigcal_accum<0, true>), g, b, 0, st, D, rot, w);
        else if (mode == 0) hipLaunchKernelGGL((k_rigcal_accum<0, false>), g, b, 0, st, D, rot, w);
        else hipLaunchKernelGGL((k_rigcal_accum<1, false>), g, b, 0, st, D, rot, w);
        R360_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rigcal_pairsum, dim3(1), dim3(1024), 0, st, D, cost_only ? 1 : 0);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_rigcal_ransac(hipStream_t st, const double* rows, int m, unsigned seed, int trial0, int n,
                         const RigcalTrimParams& p, int* counts, int* flags) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_rigcal_ransac, dim3((n + TPB / 64 - 1) / (TPB / 64)), dim3(TPB), 0, st, rows, m, seed, trial0, n, p,
                       counts, flags);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_rigcal_mask(hipStream_t st, const double* rows, int m, unsigned seed, int trial, const RigcalTrimParams& p,
                       unsigned char* mask) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_rigcal_mask, dim3(std::min((m + TPB - 1) / TPB, 64)), dim3(TPB), 0, st, rows, m, seed, trial, p, mask);
    R360_HIP(hipGetLastError());
    return 0;
}
