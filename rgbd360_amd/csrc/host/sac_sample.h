// sac_sample.h — the RANSAC plane search's counter-based sampler and its plane of three points, written once for the
// hypothesis kernel (kernels/sac_kernels.hip) and for the host check (tests/host/sac_host_check.cpp).  Plain C++ when
// not compiled by hipcc.  The statement: tests/sac_model.py, DESIGN.md §5b-5.  Every fp64 expression is written in the
// statement's order and must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define SAC_HD __host__ __device__ inline
#else
#define SAC_HD inline
#endif

SAC_HD uint64_t sac_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the high word of the 128-bit product
SAC_HD uint64_t sac_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// the key of hypothesis h of plane p; draw j of it over a pool of m
SAC_HD uint64_t sac_key(uint64_t seed, uint32_t p, uint32_t h) { return sac_mix(sac_mix(sac_mix(seed) ^ (uint64_t)p) ^ (uint64_t)h); }
SAC_HD uint64_t sac_draw(uint64_t key, uint32_t j, uint64_t m) { return sac_mulhi(sac_mix(key ^ (uint64_t)j), m); }

// three distinct pool positions in [0, m), m >= 3, without rejection; the sample order is (a, b, c)
SAC_HD void sac_sample3(uint64_t seed, uint32_t p, uint32_t h, uint64_t m, uint64_t pos[3]) {
    const uint64_t key = sac_key(seed, p, h);
    const uint64_t a = sac_draw(key, 0, m);
    uint64_t b = sac_draw(key, 1, m - 1);
    uint64_t c = sac_draw(key, 2, m - 2);
    if (b >= a) ++b;
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    pos[0] = a; pos[1] = b; pos[2] = c;
}

// The plane through p0, p1, p2 (float coordinates taken to double): coef = {n, d} with |n| = 1.  Returns false, and
// leaves coef alone, for a degenerate triple: s is not a finite number > 0.
SAC_HD bool sac_plane3(const float p0[3], const float p1[3], const float p2[3], double coef[4]) {
    const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
    const double ux = (double)p1[0] - x0, uy = (double)p1[1] - y0, uz = (double)p1[2] - z0;
    const double vx = (double)p2[0] - x0, vy = (double)p2[1] - y0, vz = (double)p2[2] - z0;
    double nx = uy * vz - uz * vy;
    double ny = uz * vx - ux * vz;
    double nz = ux * vy - uy * vx;
    const double s = (nx * nx + ny * ny) + nz * nz;
    if (!(s > 0.0) || !(s <= 1.7976931348623157e308)) return false;
    const double r = sqrt(s);
    nx /= r; ny /= r; nz /= r;
    coef[0] = nx; coef[1] = ny; coef[2] = nz;
    coef[3] = -((nx * x0 + ny * y0) + nz * z0);
    return true;
}
