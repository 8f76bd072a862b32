// gicp_host.h — the host-only parts of Generalized-ICP (host/gicp.cpp): cloud intake, the grid's sizing and build,
// the 6x6 solve and the inner Gauss-Newton loop's accept / stop logic.  Plain C++ with no HIP in it, so a stand-alone
// program can run it under the host sanitizers (tools/gicp_host_check.cpp).  Statement: DESIGN.md §5c.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// Uniform grid over a cloud's bounding box: cell of x along axis a = clamp(floorf((x - mn[a]) * inv), 0, dim[a] - 1),
// linear index (z * dim[1] + y) * dim[0] + x.  The same float expression runs on the host (the build) and the device.
struct GicpGrid { float mn[3]; float inv; float h; int dim[3]; };

constexpr size_t R360_GICP_DIRECT = 512;   // clouds up to this size: one cell, every query scans all points
constexpr int R360_GICP_MAXDIM = 1024;     // cells per axis at most

#if defined(__HIPCC__)
#define R360_GICP_HD __host__ __device__
#else
#define R360_GICP_HD
#endif
R360_GICP_HD inline int gicp_cell1(float x, float mn, float inv, int dim) {
    const float v = floorf((x - mn) * inv);
    return (int)fminf(fmaxf(v, 0.0f), (float)(dim - 1));   // a NaN clamps to 0
}

// rows with a non-finite coordinate dropped, order kept: xyzw {x, y, z, 0} per kept point
inline void gicp_intake(const float* xyz, size_t n, std::vector<float>& out) {
    out.clear();
    out.reserve(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
        out.push_back(x); out.push_back(y); out.push_back(z); out.push_back(0.0f);
    }
}

inline size_t gicp_grid_cells(const float ext[3], double h, int dim[3]) {
    size_t c = 1;
    for (int a = 0; a < 3; ++a) {
        const double d = std::floor((double)ext[a] / h) + 1.0;
        dim[a] = (int)std::min<double>(d, R360_GICP_MAXDIM);
        c *= (size_t)dim[a];
    }
    return c;
}

// The cell edge: the smallest h (by bisection) whose grid has at most n cells and at most R360_GICP_MAXDIM cells per
// axis, so a surface cloud keeps a few points per occupied cell.  A tiny cloud or one with no extent gets one cell.
inline void gicp_choose_grid(const float mn[3], const float mx[3], size_t n, GicpGrid& G) {
    float ext[3], emax = 0.f;
    for (int a = 0; a < 3; ++a) { G.mn[a] = mn[a]; ext[a] = mx[a] - mn[a]; emax = std::max(emax, ext[a]); }
    G.dim[0] = G.dim[1] = G.dim[2] = 1;
    if (n <= R360_GICP_DIRECT || !(emax > 0.f) || !std::isfinite(emax)) {
        G.h = std::isfinite(emax) && emax > 0.f ? 2.0f * emax : 1.0f;
        G.inv = 1.0f / G.h;
        if (!std::isfinite(G.inv) || !(G.inv > 0.f)) { G.h = 1.0f; G.inv = 1.0f; }
        return;
    }
    double lo = (double)emax / (R360_GICP_MAXDIM - 1), hi = 2.0 * (double)emax;   // hi: one cell
    int dim[3];
    for (int it = 0; it < 40; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (gicp_grid_cells(ext, mid, dim) <= n) hi = mid; else lo = mid;
    }
    G.h = (float)hi;
    G.inv = 1.0f / G.h;
    if (!std::isfinite(G.inv) || !(G.inv > 0.f) || !(G.h > 0.f)) {   // an extent near the float range's ends
        G.h = 1.0f; G.inv = 1.0f;
        return;
    }
    // the extents in cells as the device will compute them
    for (int a = 0; a < 3; ++a) {
        const float v = floorf(ext[a] * G.inv);
        G.dim[a] = (int)std::min(std::max(v, 0.0f), (float)(R360_GICP_MAXDIM - 1)) + 1;
    }
}

inline size_t gicp_cell_of(const GicpGrid& G, const float* p) {
    const int cx = gicp_cell1(p[0], G.mn[0], G.inv, G.dim[0]);
    const int cy = gicp_cell1(p[1], G.mn[1], G.inv, G.dim[1]);
    const int cz = gicp_cell1(p[2], G.mn[2], G.inv, G.dim[2]);
    return ((size_t)cz * G.dim[1] + cy) * G.dim[0] + cx;
}

// Counting sort of the kept points by cell (stable: ascending index inside a cell).  sorted: {x, y, z, index bits}
// per point; cell_start: cells + 1 offsets.
inline void gicp_build_grid(const std::vector<float>& pts, GicpGrid& G, std::vector<float>& sorted,
                            std::vector<unsigned>& cell_start) {
    const size_t n = pts.size() / 4;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float v = pts[4 * i + a];
            if (i == 0 || v < mn[a]) mn[a] = v;
            if (i == 0 || v > mx[a]) mx[a] = v;
        }
    gicp_choose_grid(mn, mx, n, G);
    const size_t cells = (size_t)G.dim[0] * G.dim[1] * G.dim[2];
    cell_start.assign(cells + 1, 0u);
    std::vector<unsigned> cell(n);
    for (size_t i = 0; i < n; ++i) {
        cell[i] = (unsigned)gicp_cell_of(G, &pts[4 * i]);
        ++cell_start[cell[i] + 1];
    }
    for (size_t c = 0; c < cells; ++c) cell_start[c + 1] += cell_start[c];
    std::vector<unsigned> at(cell_start.begin(), cell_start.end() - 1);
    sorted.resize(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const size_t o = at[cell[i]]++;
        const uint32_t idx = (uint32_t)i;
        memcpy(&sorted[4 * o], &pts[4 * i], 12);
        memcpy(&sorted[4 * o + 3], &idx, 4);
    }
}

// x = -H^-1 g by Gaussian elimination with partial pivoting in double, the earliest row on equal pivots: the
// arithmetic of the device solve (kernels/icp_la.inc, r360_solve6).  H row-major.  false: singular or non-finite.
inline bool gicp_solve6(const double* H, const double* g, double* x) {
    double a[6][7];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) a[i][j] = H[i * 6 + j];
        a[i][6] = -g[i];
    }
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double best = std::fabs(a[k][k]);
        for (int i = k + 1; i < 6; ++i)
            if (std::fabs(a[i][k]) > best) { best = std::fabs(a[i][k]); p = i; }
        if (!(best > 0.0) || !std::isfinite(best)) return false;
        if (p != k)
            for (int j = 0; j < 7; ++j) std::swap(a[k][j], a[p][j]);
        for (int i = k + 1; i < 6; ++i) {
            const double f = a[i][k] / a[k][k];
            for (int j = k; j < 7; ++j) a[i][j] -= f * a[k][j];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double s = a[i][6];
        for (int j = i + 1; j < 6; ++j) s -= a[i][j] * x[j];
        x[i] = s / a[i][i];
        if (!std::isfinite(x[i])) return false;
    }
    return true;
}

// sums of one inner pass: [0] f, [1..6] g, [7..27] H's upper triangle row-major, [28] the correspondence count
inline void gicp_unpack_H(const double* sums, double* H) {
    int q = 7;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++q) H[a * 6 + b] = H[b * 6 + a] = sums[q];
}

// Y (row-major 3x4, double) <- E (column-major 4x4 float, r360_exp_se3's output) * Y
inline void gicp_left_mul(const float* E, double* Y) {
    double o[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double)E[k * 4 + r] * Y[k * 4 + c];
            if (c == 3) s += (double)E[12 + r];
            o[r * 4 + c] = s;
        }
    memcpy(Y, o, sizeof o);
}

// The inner Gauss-Newton solve from Y (in / out).  pass(Y, sums) evaluates f, g, H and the count at Y and returns
// non-zero on error; expmap(delta, E) is r360_exp_se3 with pseudo = 0.  sums: the pass at the returned Y.
// Returns 0, 1 when ill-posed (no correspondence, or a singular system in the first step; Y untouched), < 0 on error.
template <class Pass, class Exp>
int gicp_inner(Pass&& pass, Exp&& expmap, int max_inner, double* Y, double* sums, int* steps) {
    *steps = 0;
    if (int rc = pass(Y, sums)) return rc < 0 ? rc : -1;
    if (!(sums[28] > 0.0)) return 1;
    while (*steps < max_inner) {
        double H[36], d[6];
        gicp_unpack_H(sums, H);
        if (!gicp_solve6(H, sums + 1, d)) {
            if (*steps == 0) return 1;
            break;
        }
        double dmax = 0;
        for (int k = 0; k < 6; ++k) dmax = std::max(dmax, std::fabs(d[k]));
        if (dmax < 1e-10) break;
        float E[16];
        expmap(d, E);
        double Yc[12], sc[29];
        memcpy(Yc, Y, sizeof Yc);
        gicp_left_mul(E, Yc);
        if (int rc = pass(Yc, sc)) return rc < 0 ? rc : -1;
        if (!(sc[0] < sums[0])) break;   // accept only a strict decrease
        memcpy(Y, Yc, sizeof Yc);
        memcpy(sums, sc, sizeof sc);
        ++*steps;
    }
    return 0;
}
