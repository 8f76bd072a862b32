// frame_kernels.hip — Frame360 construction on gfx950:
//   k_undistort : loadDepthEigen + CLAMS undistort           (Frame360.h:254-258, 293-310)
//   k_stitch_t  : stitchSphericalImage + cvtColor + depth m   (Frame360.h:1099-1148,
//                 RegisterPhotoICP.h:485-486, 316-317), tiled through LDS
//   k_pyramid   : pyrDown (gray) + buildPyramidRange (depth)  (RegisterPhotoICP.h:292-354)
//   k_gradient  : calcGradientXY for gray and depth + the alignFrames360 seam mask
//                 (RegisterPhotoICP.h:365-398, 4538-4549)
//   k_prep_l0, k_prep_tail : the sphere's pyramid and gradients, the two above tiled through LDS
// k_undistort, k_pyramid and k_gradient are HBM-streaming, one thread per output pixel.  Compiled with
// -ffp-contract=off so each float expression rounds exactly as the reference's scalar C++ does.
#include <type_traits>
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;

// ------------------------------------------------------------------ undistort
__global__ void k_undistort(const uint16_t* __restrict__ depth, float* __restrict__ depth_m, int rows, int cols,
                            const float* __restrict__ mult, const float* __restrict__ counts, int nx, int ny, int bin_w,
                            int bin_h, int nb, double bin_depth, int apply) {
    const long n = (long)R360_NUM_SENSORS * rows * cols;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float z = (float)depth[i] * 0.001f;                       // convertTo(CV_32FC1, 0.001)
        if (apply && z != 0) {                                    // discrete_depth_distortion_model.cpp:175-186
            const int s = (int)(i / ((long)rows * cols));
            const int pix = (int)(i - (long)s * rows * cols);
            const int v = pix / cols, u = pix - v * cols;
            const long fr = ((long)s * ny * nx + (long)(v / bin_h) * nx + (u / bin_w)) * nb;   // tables: [8][ny * nx][nb]
            int idx = (int)floor(z / bin_depth);
            idx = idx < nb - 1 ? idx : nb - 1;
            float start = (float)(bin_depth * idx);
            int idx1 = (z - start < bin_depth / 2) ? idx : idx + 1;  // interpolatedUndistort :48-68
            int idx0 = idx1 - 1;
            if (idx0 < 0 || idx1 >= nb || counts[fr + idx0] < 50 || counts[fr + idx1] < 50) {
                z *= mult[fr + idx];
            } else {
                double z0 = (idx0 + 1) * bin_depth - bin_depth * 0.5;
                double c1 = (z - z0) / bin_depth;
                double c0 = 1.0 - c1;
                double m = c0 * mult[fr + idx0] + c1 * mult[fr + idx1];
                z = (float)(z * m);
            }
        }
        depth_m[i] = z;
    }
}

// k_undistort with 4 consecutive pixels of one sensor row per thread (cols % 4 == 0): one 8-byte load and one 16-byte
// store per thread instead of a 2-byte load and a 4-byte store per pixel, the same per-pixel expressions
__device__ __forceinline__ float undistort_px(float z, int s, int v, int u, const float* __restrict__ mult,
                                              const float* __restrict__ counts, int nx, int ny, int bin_w, int bin_h,
                                              int nb, double bin_depth) {
    const long fr = ((long)s * ny * nx + (long)(v / bin_h) * nx + (u / bin_w)) * nb;   // tables: [8][ny * nx][nb]
    int idx = (int)floor(z / bin_depth);
    idx = idx < nb - 1 ? idx : nb - 1;
    float start = (float)(bin_depth * idx);
    int idx1 = (z - start < bin_depth / 2) ? idx : idx + 1;  // interpolatedUndistort :48-68
    int idx0 = idx1 - 1;
    if (idx0 < 0 || idx1 >= nb || counts[fr + idx0] < 50 || counts[fr + idx1] < 50) return z * mult[fr + idx];
    double z0 = (idx0 + 1) * bin_depth - bin_depth * 0.5;
    double c1 = (z - z0) / bin_depth;
    double c0 = 1.0 - c1;
    double m = c0 * mult[fr + idx0] + c1 * mult[fr + idx1];
    return (float)(z * m);
}

__global__ void k_undistort4(const uint16_t* __restrict__ depth, float* __restrict__ depth_m, int rows, int cols,
                             const float* __restrict__ mult, const float* __restrict__ counts, int nx, int ny, int bin_w,
                             int bin_h, int nb, double bin_depth, int apply) {
    const long nq = (long)R360_NUM_SENSORS * rows * cols / 4;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const uint2 d4 = reinterpret_cast<const uint2*>(depth)[q];
        const unsigned dv[4] = {d4.x & 0xffffu, d4.x >> 16, d4.y & 0xffffu, d4.y >> 16};
        float z[4];
        // the quad's sensor, row and first column (one row: cols % 4 == 0; 32-bit: a sensor image < 2^31 pixels)
        const int pq = rows * cols / 4;
        const int qi = (int)q;
        const int s = qi / pq;
        const int pix = (qi - s * pq) * 4;
        const int v = pix / cols, u0 = pix - v * cols;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            z[e] = (float)dv[e] * 0.001f;                          // convertTo(CV_32FC1, 0.001)
            if (apply && z[e] != 0)                                // discrete_depth_distortion_model.cpp:175-186
                z[e] = undistort_px(z[e], s, v, u0 + e, mult, counts, nx, ny, bin_w, bin_h, nb, bin_depth);
        }
        reinterpret_cast<float4*>(depth_m)[q] = make_float4(z[0], z[1], z[2], z[3]);
    }
}

// ------------------------------------------------------------------ stitch
// Sensor k owns sphere columns [(7-k)*rows, (8-k)*rows)  (:1119-1120).
// The sphere is walked in 64-row x 16-column tiles, one wave per sphere column: a sphere column maps onto one sensor
// row (the sensors are mounted on their side: sphere rows run along sensor columns), so a wave's 64 gathers of BGR
// bytes and ranges read a few consecutive cache lines of one sensor row, where row-major waves read 64 sensor rows (a
// line per byte).  The tile goes through LDS and is stored row-major, 4 consecutive pixels per thread: their BGR
// bytes, ranges and level-0 {gray, depth} as 3 + 2 + 8 dwords.  Per pixel the reference's float expressions (the
// sensor pose loaded once per column, which is one sensor), bit for bit.  The sphere's width is a multiple of the
// tile's (8 * rows with even sensor rows: r360_calib_create); launch_stitch refuses any other.
// LEAN: only the packed level-0 image is stored (4 of the 17 bytes per pixel), for frames whose other level-0
// outputs no kernel reads (frame_level0_lean; the full form runs again if one is asked for, then with pk = null: the
// packed image stays as it is, saliency flags included).
constexpr int STT_R = 64, STT_C = 16;
template <bool LEAN>
__global__ void __launch_bounds__(256) k_stitch_t(const uint8_t* __restrict__ bgr8, const uint16_t* __restrict__ depth8,
                                                  int rows, int cols, int H, int W, const float* __restrict__ sinphi,
                                                  const float* __restrict__ cosphi, const float* __restrict__ sinth,
                                                  const float* __restrict__ costh, const float* __restrict__ rt_inv,
                                                  float fx, float fy, float cx, float cy, uint8_t* __restrict__ sph_bgr,
                                                  uint16_t* __restrict__ sph_depth, float2* __restrict__ p0,
                                                  uint32_t* __restrict__ pk) {
    __shared__ uint32_t s_pk[STT_C][STT_R + 1];    // range mm | luma << 16
    __shared__ uint32_t s_bgr[LEAN ? 1 : STT_C][STT_R + 1];   // b | g << 8 | r << 16
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tiles_x = W / STT_C;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int row = ty * STT_R + lane;
    const bool in = row < H;
    const float v0 = in ? sinphi[row] : 0.f, cos_phi = in ? cosphi[row] : 0.f;
#pragma unroll
    for (int j = 0; j < STT_C / 4; ++j) {
        const int cl = w * (STT_C / 4) + j;
        const int col = __builtin_amdgcn_readfirstlane(tx * STT_C + cl);
        const int k = 7 - col / rows;
        const float* T = rt_inv + 16 * k;
        const float v1 = cos_phi * sinth[col];
        const float v2 = cos_phi * costh[col];
        float p0x = T[0] * v0 + T[4] * v1 + T[8] * v2;
        float p1 = T[1] * v0 + T[5] * v1 + T[9] * v2;
        float p2 = T[2] * v0 + T[6] * v1 + T[10] * v2;
        p0x = p0x + T[12]; p1 = p1 + T[13]; p2 = p2 + T[14];
        const float u = fx * p0x / p2 + cx;                          // :1133
        const float v = fy * p1 / p2 + cy;                           // :1134
        unsigned b = 0, g = 0, r = 0, dd = 0;
        if (in && u >= 0 && u < cols && v >= 0 && v < rows) {
            const int iu = (int)u, iv = (int)v;
            const long si = (long)k * rows * cols + (long)iv * cols + iu;
            b = bgr8[si * 3 + 0]; g = bgr8[si * 3 + 1]; r = bgr8[si * 3 + 2];
            const double du = (double)((u - cx) / fx), dv = (double)((v - cy) / fy);
            dd = (uint16_t)(depth8[si] * sqrt(1 + du * du + dv * dv));  // :1142 (range in mm)
        }
        const unsigned y = (b * 4899 + g * 9617 + r * 1868 + (1 << 13)) >> 14;
        s_pk[cl][lane] = dd | (y << 16);
        if (!LEAN) s_bgr[cl][lane] = b | (g << 8) | (r << 16);
    }
    __syncthreads();
    // row-major stores: thread t writes 4 consecutive pixels of tile row t / 4
    const int tr = threadIdx.x >> 2, c0 = (threadIdx.x & 3) * 4;
    const int grow = ty * STT_R + tr;
    if (grow >= H) return;
    const long i0 = (long)grow * W + tx * STT_C + c0;
    unsigned pk4[4], px[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) pk4[e] = s_pk[c0 + e][tr];
    if (pk) *reinterpret_cast<uint4*>(pk + i0) = make_uint4(pk4[0], pk4[1], pk4[2], pk4[3]);
    if (LEAN) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned q = s_bgr[c0 + e][tr];
        px[3 * e] = q & 255; px[3 * e + 1] = (q >> 8) & 255; px[3 * e + 2] = q >> 16;
    }
    uint3 wb;
    wb.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    wb.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    wb.z = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
    *reinterpret_cast<uint3*>(sph_bgr + 3 * i0) = wb;
    *reinterpret_cast<uint2*>(sph_depth + i0) = make_uint2((pk4[0] & 0xffffu) | (pk4[1] << 16),
                                                            (pk4[2] & 0xffffu) | (pk4[3] << 16));
    float2 o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)   // setSourceFrame / setTargetFrame level 0: gray /255, depth * 0.001
        o[e] = make_float2((float)(pk4[e] >> 16) * (float)(1. / 255), (float)(pk4[e] & 0xffffu) * 0.001f);
    *reinterpret_cast<float4*>(p0 + i0) = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
    *reinterpret_cast<float4*>(p0 + i0 + 2) = make_float4(o[2].x, o[2].y, o[3].x, o[3].y);
}

__device__ __forceinline__ int refl101(int p, int n) {
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - p - 2 : p;
}

// ------------------------------------------------------------------ pyramid (level l -> l+1)
// Level l's {gray, depth} through a loader: the float2 image, or level 0's packed image (4 B per pixel instead of
// 8: luma * (float)(1/255) and range * 0.001f are the stitch's own expressions, so the values are those of p0).
struct LvF2 {
    const float2* p;
    __device__ __forceinline__ float g(long i) const { return p[i].x; }
    __device__ __forceinline__ float d(long i) const { return p[i].y; }
    __device__ __forceinline__ float2 gd(long i) const { return p[i]; }
    // a pixel as it is kept in LDS, and its {gray, depth}
    typedef float2 cell;
    __device__ __forceinline__ cell raw(long i) const { return p[i]; }
    static __device__ __forceinline__ float2 val(cell v) { return v; }
};
// The luma is masked to its 8 bits: bits 24 / 25 of the word are the saliency flags (R360_PK_SAL_*), which k_prep_l0
// may be storing while the word is read.
struct LvPk {
    const uint32_t* p;
    typedef uint32_t cell;
    __device__ __forceinline__ cell raw(long i) const { return p[i]; }
    static __device__ __forceinline__ float2 val(cell v) {
        return make_float2((float)((v >> 16) & 0xffu) * (float)(1. / 255), (float)(v & 0xffffu) * 0.001f);
    }
    __device__ __forceinline__ float g(long i) const { return val(p[i]).x; }
    __device__ __forceinline__ float d(long i) const { return val(p[i]).y; }
    __device__ __forceinline__ float2 gd(long i) const { return val(p[i]); }
};

// nimg images of R x C stored back to back (the sphere: 1; the per-sensor pyramids: 8)
// (32-bit index arithmetic: nimg * R * C < 2^31, checked by the launchers)
template <class IN>
__global__ void k_pyramid(const IN in_all, int R, int C, float2* __restrict__ out_all, float min_d, float max_d,
                          int nimg) {
    const int dr = R / 2, dc = C / 2;
    const unsigned per = (unsigned)(dr * dc), n = per * (unsigned)nimg;
    for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const unsigned img = nimg > 1 ? j / per : 0u;
        const unsigned i = j - img * per;
        const long in0 = (long)img * R * C;
        float2* out = out_all + (long)img * per;
        const int y = (int)(i / (unsigned)dc), x = (int)(i - (unsigned)y * dc);
        // cv::pyrDown: horizontal [1 4 6 4 1] per source row, then the vertical SSE order.
        const int sx = 2 * x;
        const int xa = refl101(sx - 2, C), xb = refl101(sx - 1, C), xd = refl101(sx + 1, C), xe = refl101(sx + 2, C);
        float h[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int yy = refl101(2 * y - 2 + k, R);
            const long s = in0 + (long)yy * C;
            const float a = in_all.g(s + xa), b = in_all.g(s + xb), c = in_all.g(s + sx), d = in_all.g(s + xd),
                        e = in_all.g(s + xe);
            h[k] = c * 6 + (b + d) * 4 + a + e;
        }
        float t0 = h[0] + h[4];
        const float t1 = (h[1] + h[3]) + h[2];
        t0 = t0 + (h[2] + h[2]);
        t0 = t0 + t1 * 4.f;
        const float gray = t0 * (1.f / 256);
        // buildPyramidRange: mean of the 2x2 depths in (minDepth, maxDepth) (:330-348)
        float av = 0.f; unsigned nv = 0;
        const long s0 = in0 + (long)(2 * y) * C + sx;
        const long s1 = s0 + C;
        const float z0 = in_all.d(s0), z1 = in_all.d(s0 + 1), z2 = in_all.d(s1), z3 = in_all.d(s1 + 1);
        if (z0 > min_d && z0 < max_d) { av += z0; ++nv; }
        if (z1 > min_d && z1 < max_d) { av += z1; ++nv; }
        if (z2 > min_d && z2 < max_d) { av += z2; ++nv; }
        if (z3 > min_d && z3 < max_d) { av += z3; ++nv; }
        out[i] = make_float2(gray, nv > 0 ? av / nv : 0.f);
    }
}

// ------------------------------------------------------------------ gradients + seam mask
__device__ __forceinline__ float harm(float fl, float f, float fr) {
    if ((f > fr && f < fl) || (f < fr && f > fl)) return 2.f / (1 / (fr - f) + 1 / (f - fl));
    return 0.f;
}

// seam = 1: the sphere (alignFrames360's seam mask); 0: per-sensor images (alignFrames has none)
__global__ void k_gradient(const float2* __restrict__ p0, int R, int C, float4* __restrict__ tg, int nimg,
                           int mask_seams) {
    const long per = (long)R * C, n = per * nimg;
    const int ws = C / 8;   // >= 1: calib_build_tables stops the pyramid before a level narrower than 8
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long li = i % per;
        const int r = (int)(li / C), c = (int)(li - (long)r * C);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        // seam columns s*ws-1 and s*ws, s = 1..7, are zeroed by alignFrames360 (:4538-4549)
        const int m = ws > 0 ? c % ws : 1;
        const bool seam = mask_seams && ws > 0 && (c >= ws - 1) && (c < 7 * ws + 1) && (m == 0 || m == ws - 1);
        if (!seam && r >= 1 && r < R - 1 && c >= 1 && c < C - 1) {
            const float2 f = p0[i], fl = p0[i - 1], fr = p0[i + 1], fu = p0[i - C], fd = p0[i + C];
            o.x = harm(fl.x, f.x, fr.x);
            o.y = harm(fu.x, f.x, fd.x);
            o.z = harm(fl.y, f.y, fr.y);
            o.w = harm(fu.y, f.y, fd.y);
        }
        tg[i] = o;
    }
}

// ------------------------------------------------------------------ the sphere's pyramid and gradients, tiled
// The sphere's levels and their gradients in two launches (three for a 6-level pyramid) instead of one per level
// plus one for the gradients: a workgroup stages its tile with the halo the coarser levels need in LDS and builds
// from there every output that depends on it.  Per pixel the expressions of k_pyramid and k_gradient (seam mask on),
// on the same inputs: the horizontal 5-tap sum is computed once per (source row, output column) instead of once per
// output pixel, which is the same float expression.
__device__ __forceinline__ bool grad_live(int r, int c, int R, int C) {
    const int ws = C / 8;   // >= 1: calib_build_tables stops the pyramid before a level narrower than 8
    const int m = ws > 0 ? c % ws : 1;   // seam columns as k_gradient (alignFrames360 :4538-4549)
    const bool seam = ws > 0 && (c >= ws - 1) && (c < 7 * ws + 1) && (m == 0 || m == ws - 1);
    return !seam && r >= 1 && r < R - 1 && c >= 1 && c < C - 1;
}

__device__ __forceinline__ float4 grad_of(float2 f, float2 fl, float2 fr, float2 fu, float2 fd) {
    return make_float4(harm(fl.x, f.x, fr.x), harm(fu.x, f.x, fd.x), harm(fl.y, f.y, fr.y), harm(fu.y, f.y, fd.y));
}

// k_pyramid's vertical combination of the five row sums, and its 2x2 depth mean
__device__ __forceinline__ float pyr_gray(float h0, float h1, float h2, float h3, float h4) {
    float t0 = h0 + h4;
    const float t1 = (h1 + h3) + h2;
    t0 = t0 + (h2 + h2);
    t0 = t0 + t1 * 4.f;
    return t0 * (1.f / 256);
}
__device__ __forceinline__ float pyr_depth(float z0, float z1, float z2, float z3, float min_d, float max_d) {
    float av = 0.f; unsigned nv = 0;
    if (z0 > min_d && z0 < max_d) { av += z0; ++nv; }
    if (z1 > min_d && z1 < max_d) { av += z1; ++nv; }
    if (z2 > min_d && z2 < max_d) { av += z2; ++nv; }
    if (z3 > min_d && z3 < max_d) { av += z3; ++nv; }
    return nv > 0 ? av / nv : 0.f;
}

__device__ __forceinline__ int clampi(int p, int n) { return p < 0 ? 0 : (p >= n ? n - 1 : p); }

// Launch 1: one workgroup per L0_TR x L0_TC tile of level 0 writes the tile's level-0 gradients, its level-1 pixels
// and their gradients.  LDS cell (r, c) of s0 holds the level-0 pixel at refl101 of (y0 - 4 + r, x0 - 4 + c), the
// border rule of k_pyramid on global coordinates (a level-1 pixel's taps reach 2 rows / columns past the image at
// most; cells further out are clamped into the image and never used).  The halo of 4 supplies the ring of level-1
// pixels around the tile's own (their taps: 2 (y - 1) - 2 = 2 y - 4), recomputed here for the level-1 gradients.
// LDS: 24 x 136 x 4 (the packed image; x 8 from a float2 image) + 23 x 66 x 4 + 10 x 66 x 8 = 24.4 KB static: six
// workgroups per CU, so the 1200 of a VGA sphere are resident at once (at 8 B per cell it took two rounds).
constexpr int L0_TR = 16, L0_TC = 128, L0_HALO = 4;
constexpr int L0_SR = L0_TR + 2 * L0_HALO, L0_SC = L0_TC + 2 * L0_HALO;   // staged level-0 cells
constexpr int L0_1R = L0_TR / 2 + 2, L0_1C = L0_TC / 2 + 2;               // level-1 pixels: the tile's and a ring of 1
constexpr int L0_HR = 2 * L0_1R + 3;                                      // source rows under them

// Saliency flags (the packed image only; pkw = in.p, or null for none): with each level-0 gradient the workgroup
// stores the pixel's word again with bits 24 / 25 set from the gradient just computed, sal_p = !(|gx| < ti && |gy| <
// ti), sal_d = !(|dgx| < td && |dgy| < td): contribute_lean's tests.  The level-0 pass (PF 6) reads them from the
// target word it gathers anyway and runs the gradient gather and the terms only for flagged pixels.  The store races
// with the halo loads of the neighbouring workgroups, which read the same words; that is safe because a word is an
// aligned 32-bit store (a reader sees the old or the new word, never a mix), its low 24 bits do not change (they are
// rewritten with the value just read) and every reader masks the flags off (LvPk::val, PF 6's gray_of).  Every pixel
// of the image is stored, salient or not, so bits of an earlier build never survive.
template <class IN>
__global__ void __launch_bounds__(256) k_prep_l0(const IN in, int R, int C, float4* __restrict__ tg0,
                                                 float2* __restrict__ p1, float4* __restrict__ tg1, float min_d,
                                                 float max_d, uint32_t* pkw, float ti, float td) {
    __shared__ typename IN::cell s0[L0_SR][L0_SC];   // as loaded (the packed image: 4 B), IN::val() on every read
    __shared__ float sh[L0_HR][L0_1C];
    __shared__ float2 s1[L0_1R][L0_1C];
    const int tiles_x = (C + L0_TC - 1) / L0_TC;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * L0_TR, x0 = tx * L0_TC;
    // unconditional loads (every cell maps into the image), four in flight per thread
#pragma unroll 4
    for (int k = threadIdx.x; k < L0_SR * L0_SC; k += 256) {
        const int r = k / L0_SC, c = k - r * L0_SC;
        const int gy = clampi(refl101(y0 - L0_HALO + r, R), R), gx = clampi(refl101(x0 - L0_HALO + c, C), C);
        s0[r][c] = in.raw((long)gy * C + gx);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < L0_TR * L0_TC; k += 256) {
        const int r = k / L0_TC, c = k - r * L0_TC;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= R || gx >= C) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grad_live(gy, gx, R, C)) {
            const int lr = r + L0_HALO, lc = c + L0_HALO;
            o = grad_of(IN::val(s0[lr][lc]), IN::val(s0[lr][lc - 1]), IN::val(s0[lr][lc + 1]), IN::val(s0[lr - 1][lc]),
                        IN::val(s0[lr + 1][lc]));
        }
        tg0[(long)gy * C + gx] = o;
        if constexpr (std::is_same<typename IN::cell, uint32_t>::value) {
            if (pkw) {
                const bool sal_p = !(fabsf(o.x) < ti && fabsf(o.y) < ti);
                const bool sal_d = !(fabsf(o.z) < td && fabsf(o.w) < td);
                pkw[(long)gy * C + gx] = (s0[r + L0_HALO][c + L0_HALO] & R360_PK_VALUE) | (sal_p ? R360_PK_SAL_P : 0u) |
                                         (sal_d ? R360_PK_SAL_D : 0u);
            }
        }
    }
    if (!p1) return;   // a one-level pyramid
    // level-1 pixel (Y0 - 1 + i, X0 - 1 + j): its source rows are the cells 2 i .. 2 i + 4, its source columns the
    // cells 2 j .. 2 j + 4
    const int dr = R / 2, dc = C / 2, Y0 = y0 / 2, X0 = x0 / 2;
    for (int k = threadIdx.x; k < L0_HR * L0_1C; k += 256) {
        const int s = k / L0_1C, j = k - s * L0_1C;
        const typename IN::cell* row = s0[s] + 2 * j;
        const float a = IN::val(row[0]).x, b = IN::val(row[1]).x, c = IN::val(row[2]).x, d = IN::val(row[3]).x,
                    e = IN::val(row[4]).x;
        sh[s][j] = c * 6 + (b + d) * 4 + a + e;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < L0_1R * L0_1C; k += 256) {
        const int i = k / L0_1C, j = k - i * L0_1C;
        const int ly = Y0 - 1 + i, lx = X0 - 1 + j;
        if (ly < 0 || ly >= dr || lx < 0 || lx >= dc) continue;
        const float gray = pyr_gray(sh[2 * i][j], sh[2 * i + 1][j], sh[2 * i + 2][j], sh[2 * i + 3][j], sh[2 * i + 4][j]);
        const typename IN::cell* r0 = s0[2 * i + 2] + 2 * j + 2;   // level-0 pixel (2 ly, 2 lx)
        const typename IN::cell* r1 = s0[2 * i + 3] + 2 * j + 2;
        const float2 v = make_float2(gray, pyr_depth(IN::val(r0[0]).y, IN::val(r0[1]).y, IN::val(r1[0]).y,
                                                     IN::val(r1[1]).y, min_d, max_d));
        s1[i][j] = v;
        if (i >= 1 && i <= L0_TR / 2 && j >= 1 && j <= L0_TC / 2) p1[(long)ly * dc + lx] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (L0_TR / 2) * (L0_TC / 2); k += 256) {
        const int i = k / (L0_TC / 2), j = k - i * (L0_TC / 2);
        const int ly = Y0 + i, lx = X0 + j;
        if (ly >= dr || lx >= dc) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grad_live(ly, lx, dr, dc))   // an interior pixel: its four neighbours are level-1 pixels, all in s1
            o = grad_of(s1[i + 1][j + 1], s1[i + 1][j], s1[i + 1][j + 2], s1[i][j + 1], s1[i + 2][j + 1]);
        tg1[(long)ly * dc + lx] = o;
    }
}

// Launch 2, the tail: up to three levels a, b, c below a base level (level 1, or the last level of the previous tail
// launch) and their gradients.  One workgroup per TL_R x TL_C tile of level a = TL_R/2 x TL_C/2 of b = TL_R/4 x
// TL_C/4 of c.  It keeps in LDS, per level, the region the next level and the gradients need, pixel (oy + i, ox + j)
// in cell (i, j) with pixels outside the image left unset and never read:
//   c: its tile and a ring of 1 (the gradients' neighbours)   6 x 10
//   b: the pixels under c's region, 2 before and 2 after       15 x 23
//   a: the pixels under b's region                             33 x 49, from 69 x 101 base pixels read from global
// Taps go through refl101 on the source level's own coordinates as in k_pyramid; a reflected coordinate lies inside
// the region, which reaches 2 past the image at most where it needs a tap from there.
// LDS: 69 x 49 x 4 (row sums, reused by each level) + (33 x 49 + 15 x 23 + 6 x 10) x 8 = 29.2 KB static.
constexpr int TL_R = 16, TL_C = 32;
constexpr int TL_T = 512;   // threads: 3381 row sums from global per workgroup, 7 per thread
constexpr int TL_CR = TL_R / 4 + 2, TL_CC = TL_C / 4 + 2;
constexpr int TL_BR = 2 * TL_CR + 3, TL_BC = 2 * TL_CC + 3;
constexpr int TL_AR = 2 * TL_BR + 3, TL_AC = 2 * TL_BC + 3;

struct TailLevels {
    float2* p0[3];
    float4* tg[3];
    int nb;   // levels to build, 1..3
};

struct SrcGlobal {
    const float2* p; int C;
    __device__ __forceinline__ float2 at(int y, int x) const { return p[(long)y * C + x]; }
};
template <int NC>
struct SrcLds {
    const float2 (*s)[NC]; int oy, ox;
    __device__ __forceinline__ float2 at(int y, int x) const { return s[y - oy][x - ox]; }
};

// the DR x DC region of a level at (doy, dox) from its source level (Rs x Cs) into dst, with the pixels of the
// workgroup's own tr x tc tile at (ty0, tx0) stored to gout; h: (2 DR + 3) x DC row sums
// CLAMP (the step that reads global memory): pixels outside the image are read at the nearest pixel inside it and
// their results dropped or left unread, so that the loads stand outside every branch and several iterations' loads
// are in flight at once; the workgroup's time is the latency of these loads, not their bytes
template <int DR, int DC, bool CLAMP, class SRC>
__device__ __forceinline__ void tail_step(const SRC src, int Rs, int Cs, int doy, int dox, float* __restrict__ h,
                                          float2 (*dst)[DC], float2* __restrict__ gout, int ty0, int tx0, int tr, int tc,
                                          float min_d, float max_d) {
    const int Rd = Rs / 2, Cd = Cs / 2, sy0 = 2 * doy - 2;
#pragma unroll 2
    for (int k = threadIdx.x; k < (2 * DR + 3) * DC; k += TL_T) {
        const int s = k / DC, j = k - s * DC;
        int sy = sy0 + s, xd = dox + j;
        if (CLAMP) { sy = clampi(sy, Rs); xd = clampi(xd, Cd); }
        else if (sy < 0 || sy >= Rs || xd < 0 || xd >= Cd) continue;
        const int sx = 2 * xd;
        const float a = src.at(sy, refl101(sx - 2, Cs)).x, b = src.at(sy, refl101(sx - 1, Cs)).x, c = src.at(sy, sx).x,
                    d = src.at(sy, refl101(sx + 1, Cs)).x, e = src.at(sy, refl101(sx + 2, Cs)).x;
        h[k] = c * 6 + (b + d) * 4 + a + e;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = threadIdx.x; k < DR * DC; k += TL_T) {
        const int i = k / DC, j = k - i * DC;
        const int yd = doy + i, xd = dox + j;
        const bool in = yd >= 0 && yd < Rd && xd >= 0 && xd < Cd;
        if (!CLAMP && !in) continue;
        const int yq = CLAMP ? clampi(yd, Rd) : yd, xq = CLAMP ? clampi(xd, Cd) : xd;
        const float2 z0 = src.at(2 * yq, 2 * xq), z1 = src.at(2 * yq, 2 * xq + 1), z2 = src.at(2 * yq + 1, 2 * xq),
                     z3 = src.at(2 * yq + 1, 2 * xq + 1);
        if (CLAMP && !in) continue;
        float hh[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) hh[t] = h[(refl101(2 * yd - 2 + t, Rs) - sy0) * DC + j];
        const float2 v = make_float2(pyr_gray(hh[0], hh[1], hh[2], hh[3], hh[4]),
                                     pyr_depth(z0.y, z1.y, z2.y, z3.y, min_d, max_d));
        dst[i][j] = v;
        if (yd >= ty0 && yd < ty0 + tr && xd >= tx0 && xd < tx0 + tc) gout[(long)yd * Cd + xd] = v;
    }
    __syncthreads();
}

// the gradients of the workgroup's TR x TC tile at (ty0, tx0) of an R x C level held in s (pixel (oy + i, ox + j))
template <int TR, int TC, int NC>
__device__ __forceinline__ void tail_grad(const float2 (*s)[NC], int oy, int ox, int R, int C, int ty0, int tx0,
                                          float4* __restrict__ tg) {
    for (int k = threadIdx.x; k < TR * TC; k += TL_T) {
        const int i = k / TC, j = k - i * TC;
        const int y = ty0 + i, x = tx0 + j;
        if (y >= R || x >= C) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grad_live(y, x, R, C)) {
            const int ly = y - oy, lx = x - ox;
            o = grad_of(s[ly][lx], s[ly][lx - 1], s[ly][lx + 1], s[ly - 1][lx], s[ly + 1][lx]);
        }
        tg[(long)y * C + x] = o;
    }
}

__global__ void __launch_bounds__(TL_T) k_prep_tail(const float2* __restrict__ base, int R0, int C0, TailLevels T,
                                                   float min_d, float max_d) {
    __shared__ float sh[(2 * TL_AR + 3) * TL_AC];
    __shared__ float2 sa[TL_AR][TL_AC];
    __shared__ float2 sb[TL_BR][TL_BC];
    __shared__ float2 sc[TL_CR][TL_CC];
    const int Ra = R0 / 2, Ca = C0 / 2;
    const int tiles_x = (Ca + TL_C - 1) / TL_C;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int Yc = ty * (TL_R / 4), Xc = tx * (TL_C / 4);
    const int cy = Yc - 1, cx = Xc - 1;             // the regions' first pixels
    const int by = 2 * cy - 2, bx = 2 * cx - 2;
    const int ay = 2 * by - 2, ax = 2 * bx - 2;
    tail_step<TL_AR, TL_AC, true>(SrcGlobal{base, C0}, R0, C0, ay, ax, sh, sa, T.p0[0], 4 * Yc, 4 * Xc, TL_R, TL_C, min_d,
                            max_d);
    tail_grad<TL_R, TL_C>(sa, ay, ax, Ra, Ca, 4 * Yc, 4 * Xc, T.tg[0]);
    if (T.nb < 2) return;
    const int Rb = Ra / 2, Cb = Ca / 2;
    tail_step<TL_BR, TL_BC, false>(SrcLds<TL_AC>{sa, ay, ax}, Ra, Ca, by, bx, sh, sb, T.p0[1], 2 * Yc, 2 * Xc, TL_R / 2,
                            TL_C / 2, min_d, max_d);
    tail_grad<TL_R / 2, TL_C / 2>(sb, by, bx, Rb, Cb, 2 * Yc, 2 * Xc, T.tg[1]);
    if (T.nb < 3) return;
    tail_step<TL_CR, TL_CC, false>(SrcLds<TL_BC>{sb, by, bx}, Rb, Cb, cy, cx, sh, sc, T.p0[2], Yc, Xc, TL_R / 4, TL_C / 4,
                            min_d, max_d);
    tail_grad<TL_R / 4, TL_C / 4>(sc, cy, cx, Rb / 2, Cb / 2, Yc, Xc, T.tg[2]);
}

// setSourceFrame / setTargetFrame level 0 of each sensor's raw images (:480-516): CV_RGB2GRAY on the
// BGR-stored data /255, and the u16 depth * 0.001 (buildPyramidRange :316-317)
// pk (optional): the packed level-0 image of the sphere (LevelBufs::pk)
__global__ void k_sensor_level0(const uint8_t* __restrict__ bgr8, const uint16_t* __restrict__ depth8, long n,
                                float2* __restrict__ p0, uint32_t* __restrict__ pk) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int b = bgr8[3 * i], g = bgr8[3 * i + 1], r = bgr8[3 * i + 2];
        const int y = (b * 4899 + g * 9617 + r * 1868 + (1 << 13)) >> 14;
        p0[i] = make_float2((float)y * (float)(1. / 255), (float)depth8[i] * 0.001f);
        if (pk) pk[i] = depth8[i] | ((unsigned)y << 16);
    }
}

inline int grid_for(long n) {
    long b = (n + TPB - 1) / TPB;
    return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

}  // namespace

// ------------------------------------------------------------------ launchers
int launch_undistort(r360_frame* f) {
    const r360_calib* c = f->calib;
    const long n = (long)R360_NUM_SENSORS * f->rows * f->cols;
    const bool apply = c->has_intrinsics && c->clams.width == f->cols && c->clams.height == f->rows;
    if (f->cols % 4 == 0) {
        hipLaunchKernelGGL(k_undistort4, dim3(grid_for(n / 4)), dim3(TPB), 0, f->ctx->stream, f->d_depth, f->d_depth_m,
                           f->rows, f->cols, c->clams.d_mult, c->clams.d_counts, c->clams.nx, c->clams.ny, c->clams.bin_w,
                           c->clams.bin_h, c->clams.num_bins, c->clams.bin_depth, apply ? 1 : 0);
        R360_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_undistort, dim3(grid_for(n)), dim3(TPB), 0, f->ctx->stream, f->d_depth, f->d_depth_m, f->rows,
                       f->cols, c->clams.d_mult, c->clams.d_counts, c->clams.nx, c->clams.ny, c->clams.bin_w,
                       c->clams.bin_h, c->clams.num_bins, c->clams.bin_depth, apply ? 1 : 0);
    R360_HIP(hipGetLastError());
    return 0;
}

// A frame that only enters batched alignments (compact_all unset: the sequence runner's queued ring, or
// r360_frame_set_compaction(f, 0)) is lean when its level 0 is streamed as the packed image (the condition under which
// launch_pyramid skips level 0's compaction) and its stitch is the tiled one: the batched level-0 pass (PF 6), level
// 1 and the level-0 gradients read pk only, so its build leaves d_sph_bgr, d_sph_depth and lv[0].p0 unwritten
// (13 of the stitch's 17 bytes per pixel) until a reader asks for them (frame_level0_materialise).
bool frame_level0_lean(const r360_frame* f) {
    return !f->compact_all && f->rows > 0 && f->lv[0].pk && f->lv[0].cols % 64 == 0;
}

int launch_stitch(r360_frame* f, bool lean, bool keep_pk) {
    const r360_calib* c = f->calib;
    // the tiled kernel is the only one: 8 * rows with even sensor rows (r360_calib_create) is a multiple of its tile
    if (f->sph_cols % STT_C != 0) {
        r360_set_error("stitch: a sphere of %d columns is no multiple of the %d-column tile", f->sph_cols, STT_C);
        return -1;
    }
    if (hipEvent_t e = f->bgr_wait()) R360_HIP(hipStreamWaitEvent(f->ctx->stream, e, 0));   // a split upload's BGR copy
    const int slot = timing_begin(f->ctx, "k_stitch");
    // a stitch that writes the packed image writes whole words: the frame has no saliency flags until launch_pyramid
    uint32_t* pk = keep_pk ? nullptr : f->lv[0].pk;
    if (pk) f->sal_int = f->sal_depth = __builtin_nanf("");
    const dim3 grid((f->sph_cols / STT_C) * ((f->sph_rows + STT_R - 1) / STT_R));
    if (lean)
        hipLaunchKernelGGL(k_stitch_t<true>, grid, dim3(256), 0, f->ctx->stream, f->d_bgr, f->d_depth, f->rows,
                           f->cols, f->sph_rows, f->sph_cols, c->d_st_sinphi, c->d_st_cosphi, c->d_st_sinth,
                           c->d_st_costh, c->d_rt_inv, c->K[0], c->K[4], c->K[6], c->K[7], f->d_sph_bgr,
                           f->d_sph_depth, f->lv[0].p0, pk);
    else
        hipLaunchKernelGGL(k_stitch_t<false>, grid, dim3(256), 0, f->ctx->stream, f->d_bgr, f->d_depth, f->rows,
                           f->cols, f->sph_rows, f->sph_cols, c->d_st_sinphi, c->d_st_cosphi, c->d_st_sinth,
                           c->d_st_costh, c->d_rt_inv, c->K[0], c->K[4], c->K[6], c->K[7], f->d_sph_bgr,
                           f->d_sph_depth, f->lv[0].p0, pk);
    timing_end(f->ctx, slot);
    R360_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ ICP source points
// The source side of errorPhotoICP_sphere / calcHessGrad_sphere reads, per pixel with
// minDepth < depth < maxDepth, the LUT_xyz_sphere point (RegisterPhotoICP.h:4553-4587, the same float
// expressions) and the gray value; both are fixed for a source frame.  They are compacted here once per
// frame, in raster order (a deterministic two-kernel scan), so the pass streams only valid pixels.
// A block covers R360_SRC_BLOCK consecutive pixels, SRC_PPT consecutive ones per thread (256-thread workgroups: a
// 1024-thread one had to find 16 free wave slots on one CU, which under load delayed the frame's build).
constexpr int SRC_PPT = 16, SRC_TPB = R360_SRC_BLOCK / SRC_PPT;

// flattened (level, block) grid: level l owns blocks [blk0[l], blk0[l + 1]) (the coarse levels need a quarter, a
// sixteenth ... of level 0's blocks; a 2D grid sized for level 0 dispatched thousands of empty workgroups)
struct SrcGrid { int blk0[R360_MAX_PYR + 1]; int nl; };
__device__ __forceinline__ void src_block(const SrcGrid& G, int& level, int& b) {
    const int bid = blockIdx.x;
    level = 0;
    while (level + 1 < G.nl && bid >= G.blk0[level + 1]) ++level;
    b = bid - G.blk0[level];
}

__device__ __forceinline__ bool src_valid(float d, float min_d, float max_d) { return min_d < d && d < max_d; }

__global__ void __launch_bounds__(SRC_TPB) k_src_count(const SrcLevel* __restrict__ L, SrcGrid G, float min_d, float max_d,
                                                      int* __restrict__ cnt, int stride) {
    int lvl, bx;
    src_block(G, lvl, bx);
    const SrcLevel S = L[lvl];
    const long n = (long)S.rows * S.cols;
    const long b0 = (long)bx * R360_SRC_BLOCK;
    if (b0 >= n) return;
    int c = 0;
#pragma unroll
    for (int k = 0; k < SRC_PPT; ++k) {
        const long i = b0 + k * SRC_TPB + threadIdx.x;
        c += (i < n && src_valid(S.p0[i].y, min_d, max_d)) ? 1 : 0;
    }
    __shared__ int sh[SRC_TPB / 64];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < SRC_TPB / 64; ++w) t += sh[w];
        cnt[lvl * stride + bx] = t;
    }
}

__global__ void __launch_bounds__(SRC_TPB) k_src_compact(const SrcLevel* __restrict__ L, SrcGrid G, float min_d,
                                                        float max_d, const int* __restrict__ cnt, int stride,
                                                        int* __restrict__ npts) {
    int lvl, bx;
    src_block(G, lvl, bx);
    const SrcLevel S = L[lvl];
    const long n = (long)S.rows * S.cols;
    const long b0 = (long)bx * R360_SRC_BLOCK;
    if (b0 >= n) return;
    __shared__ int sh[SRC_TPB / 64 + 1];
    // this block's output offset: the counts of the blocks before it
    int base = 0;
    for (int b = threadIdx.x; b < bx; b += SRC_TPB) base += cnt[lvl * stride + b];
    for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = base;
    __syncthreads();
    base = 0;
    for (int w = 0; w < SRC_TPB / 64; ++w) base += sh[w];
    __syncthreads();
    // raster order: the block's pixels as SRC_PPT rows of SRC_TPB, pixel b0 + k SRC_TPB + t (coalesced loads); a
    // pixel's slot = the valid pixels of the rows before k, then of the waves before this one in row k, then of the
    // lanes before it (ballot masks: one LDS round for the whole block)
    __shared__ int s_cnt[SRC_PPT][SRC_TPB / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    float2 a[SRC_PPT];
    unsigned long long m[SRC_PPT];
#pragma unroll
    for (int k = 0; k < SRC_PPT; ++k) {
        const long i = b0 + (long)k * SRC_TPB + threadIdx.x;
        a[k] = i < n ? S.p0[i] : make_float2(0.f, 0.f);
        m[k] = __ballot(i < n && src_valid(a[k].y, min_d, max_d));
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < SRC_PPT; ++k) s_cnt[k][wid] = __popcll(m[k]);
    __syncthreads();
    int pos = base;
#pragma unroll
    for (int k = 0; k < SRC_PPT; ++k) {
        int before = pos, row = 0;
#pragma unroll
        for (int w = 0; w < SRC_TPB / 64; ++w) {
            const int cw = s_cnt[k][w];
            before += w < wid ? cw : 0;
            row += cw;
        }
        if ((m[k] >> lane) & 1ull) {
            const long i = b0 + (long)k * SRC_TPB + threadIdx.x;
            const int r = (int)(i / S.cols), cc = (int)(i - (long)r * S.cols);
            const float d = a[k].y;
            // LUT_xyz_sphere (:4580-4582): x = d sin(phi), y = -d cos(phi) sin(theta), z = -d cos(phi) cos(theta)
            S.pts[before + __popcll(m[k] & lt)] =
                make_float4(d * S.sinphi[r], -d * S.cosphi[r] * S.sinth[cc], -d * S.cosphi[r] * S.costh[cc], a[k].x);
        }
        pos += row;
    }
    if (bx == (int)((n - 1) / R360_SRC_BLOCK) && threadIdx.x == SRC_TPB - 1) npts[lvl] = pos;
}

int launch_sphere_level0(r360_frame* f) {
    const long n = (long)f->sph_rows * f->sph_cols;
    // cvtColor(CV_RGB2GRAY) / 255 and convertTo(CV_32F, 0.001): the stitch kernel's level-0 expressions
    hipLaunchKernelGGL(k_sensor_level0, dim3(grid_for(n)), dim3(TPB), 0, f->ctx->stream, f->d_sph_bgr, f->d_sph_depth,
                       n, f->lv[0].p0, f->lv[0].pk);
    f->sal_int = f->sal_depth = __builtin_nanf("");   // whole words: no saliency flags until launch_pyramid
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_pyramid(r360_frame* f) {
    // RegisterPhotoICP constructor defaults minDepth 0.3 / maxDepth 6.0 (:202-203)
    const float min_d = 0.3f, max_d = 6.0f;
    if ((long)f->lv[0].rows * f->lv[0].cols > 0x7fffffffL - 4096) {   // 32-bit pixel indices
        r360_set_error("sphere of %d x %d pixels is too large", f->lv[0].rows, f->lv[0].cols);
        return -1;
    }
    // launch 1: level 0's gradients, level 1 and its gradients, from level 0's packed image (half the bytes of its
    // float2 image, the same values) where the frame has one
    {
        const LevelBufs& L0 = f->lv[0];
        const bool more = f->n_levels > 1;
        float2* p1 = more ? f->lv[1].p0 : nullptr;
        float4* tg1 = more ? f->lv[1].tg : nullptr;
        const dim3 grid(((L0.rows + L0_TR - 1) / L0_TR) * ((L0.cols + L0_TC - 1) / L0_TC));
        if (L0.pk) {
            // the packed image's saliency flags, for the default thresholds of an alignment (r360_icp_default_params);
            // an alignment with lower ones passes every visible pixel to its heavy stage instead (icp_pk_nosal)
            r360_icp_params dp;
            r360_icp_default_params(&dp);
            hipLaunchKernelGGL(k_prep_l0<LvPk>, grid, dim3(256), 0, f->ctx->stream, LvPk{L0.pk}, L0.rows, L0.cols, L0.tg,
                               p1, tg1, min_d, max_d, L0.pk, dp.thres_sal_int, dp.thres_sal_depth);
            f->sal_int = dp.thres_sal_int;
            f->sal_depth = dp.thres_sal_depth;
        } else {
            hipLaunchKernelGGL(k_prep_l0<LvF2>, grid, dim3(256), 0, f->ctx->stream, LvF2{L0.p0}, L0.rows, L0.cols, L0.tg,
                               p1, tg1, min_d, max_d, (uint32_t*)nullptr, 0.f, 0.f);
        }
    }
    // launch 2: the levels below level 1 and their gradients, three per launch
    for (int l = 1; l + 1 < f->n_levels; l += 3) {
        TailLevels T{};
        T.nb = f->n_levels - 1 - l < 3 ? f->n_levels - 1 - l : 3;
        for (int k = 0; k < T.nb; ++k) { T.p0[k] = f->lv[l + 1 + k].p0; T.tg[k] = f->lv[l + 1 + k].tg; }
        const LevelBufs& A = f->lv[l + 1];
        hipLaunchKernelGGL(k_prep_tail, dim3(((A.rows + TL_R - 1) / TL_R) * ((A.cols + TL_C - 1) / TL_C)), dim3(TL_T), 0,
                           f->ctx->stream, f->lv[l].p0, f->lv[l].rows, f->lv[l].cols, T, min_d, max_d);
    }
    // the compacted points feed a lone alignment's passes (PF 5); batched passes stream the images (PF 6 at level 0
    // where its rows split into whole waves, PF 8 on levels of >= 64 columns), so frames that only enter batches
    // (f->compact_all unset: the sequence runner's queued ring) skip the levels a batched pass streams (built on
    // request: r360_frame_get_points)
    unsigned need = 0;
    for (int l = 0; l < f->n_levels; ++l) {
        const bool streamed = l == 0 && f->lv[0].pk ? f->lv[0].cols % 64 == 0 : f->lv[l].cols >= 64;
        if (f->compact_all || !streamed) need |= 1u << l;
    }
    f->compacted = need;
    return launch_src_compaction(f, need);
}

// The compaction of the levels in `levels` (bit l: level l), one count + one compact launch over a flattened
// (level, block) grid
int launch_src_compaction(r360_frame* f, unsigned levels) {
    const float min_d = 0.3f, max_d = 6.0f;
    int l1 = 0;
    for (int l = 0; l < f->n_levels; ++l)
        if ((levels >> l) & 1u) l1 = l + 1;
    if (l1 == 0) return 0;
    if ((levels & 1u) && frame_level0_materialise(f)) return -1;   // level 0's points come from lv[0].p0
    SrcGrid G{};
    G.nl = l1;
    for (int l = 0; l < l1; ++l)
        G.blk0[l + 1] = G.blk0[l] + (((levels >> l) & 1u) ? (int)(((long)f->lv[l].rows * f->lv[l].cols + R360_SRC_BLOCK - 1) /
                                                                      R360_SRC_BLOCK) : 0);
    const dim3 g(G.blk0[l1]);
    hipLaunchKernelGGL(k_src_count, g, dim3(SRC_TPB), 0, f->ctx->stream, f->d_src_levels, G, min_d, max_d, f->d_src_cnt,
                       f->src_blocks);
    hipLaunchKernelGGL(k_src_compact, g, dim3(SRC_TPB), 0, f->ctx->stream, f->d_src_levels, G, min_d, max_d,
                       f->d_src_cnt, f->src_blocks, f->d_npts);
    R360_HIP(hipGetLastError());
    return 0;
}

// The 8 sensors' pinhole pyramids (RegisterPhotoICP::setSourceFrame / setTargetFrame on
// frameRGBD_[k].getRGBImage() / getDepthImage(), MethodsRegisterRGBD360.cpp:337-338), all sensors per
// launch.  Levels are allocated on first use.
int launch_sensor_pyramid(r360_frame* f) {
    const float min_d = 0.3f, max_d = 6.0f;
    if (f->alloc_sensor_pyramid()) return -1;
    hipStream_t st = f->ctx->stream;
    const long n0 = 8L * f->rows * f->cols;
    if (n0 > 0x7fffffffL) {   // k_pyramid's 32-bit pixel indices
        r360_set_error("sensor images of %d x %d pixels are too large", f->rows, f->cols);
        return -1;
    }
    if (hipEvent_t e = f->bgr_wait()) R360_HIP(hipStreamWaitEvent(st, e, 0));   // a split upload's BGR copy
    hipLaunchKernelGGL(k_sensor_level0, dim3(grid_for(n0)), dim3(TPB), 0, st, f->d_bgr, f->d_depth, n0, f->sp[0].p0,
                       (uint32_t*)nullptr);
    for (int l = 1; l < f->n_slevels; ++l) {
        const long n = 8L * f->sp[l].rows * f->sp[l].cols;
        hipLaunchKernelGGL(k_pyramid<LvF2>, dim3(grid_for(n)), dim3(TPB), 0, st, LvF2{f->sp[l - 1].p0}, f->sp[l - 1].rows,
                           f->sp[l - 1].cols, f->sp[l].p0, min_d, max_d, 8);
    }
    for (int l = 0; l < f->n_slevels; ++l) {
        const long n = 8L * f->sp[l].rows * f->sp[l].cols;
        hipLaunchKernelGGL(k_gradient, dim3(grid_for(n)), dim3(TPB), 0, st, f->sp[l].p0, f->sp[l].rows, f->sp[l].cols,
                           f->sp[l].tg, 8, 0);
    }
    R360_HIP(hipGetLastError());
    return 0;
}
