// Stand-alone check of Generalized-ICP's host-only logic (rgbd360_amd/csrc/host/gicp_host.h): intake, the grid's
// sizing and counting sort (with the invariant the kernels' ring bound rests on, on thin, capped and mostly empty
// grids), the 6x6 solve and the inner loop's accept / stop rule fed with a canned quadratic.  With file arguments
// (float32 x y z rows) it checks and prints each file's grid instead.
// Meant for the host sanitizers, no GPU and no HIP:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gicp_host_check.cpp -o gicp_host_check
#include "../rgbd360_amd/csrc/host/gicp_host.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void check_grid(const std::vector<float>& xyz) {
    std::vector<float> pts, sorted;
    std::vector<unsigned> start;
    gicp_intake(xyz.data(), xyz.size() / 3, pts);
    const size_t n = pts.size() / 4;
    if (n == 0) return;
    GicpGrid G;
    gicp_build_grid(pts, G, sorted, start);
    const size_t cells = (size_t)G.dim[0] * G.dim[1] * G.dim[2];
    EXPECT(start.size() == cells + 1 && start[0] == 0 && start[cells] == n);
    EXPECT(G.dim[0] >= 1 && G.dim[0] <= R360_GICP_MAXDIM && G.dim[1] >= 1 && G.dim[2] >= 1);
    EXPECT(cells <= 8 * n + 8);
    std::vector<char> seen(n, 0);
    for (size_t c = 0; c < cells; ++c) {
        EXPECT(start[c] <= start[c + 1]);
        for (unsigned q = start[c]; q < start[c + 1]; ++q) {
            uint32_t idx;
            memcpy(&idx, &sorted[4 * q + 3], 4);
            EXPECT(idx < n && !seen[idx]);
            seen[idx] = 1;
            EXPECT(gicp_cell_of(G, &sorted[4 * q]) == c);
            EXPECT(memcmp(&sorted[4 * q], &pts[4 * idx], 12) == 0);
            if (q > start[c]) { uint32_t prev; memcpy(&prev, &sorted[4 * q - 1], 4); EXPECT(prev < idx); }
        }
    }
}

// What ring_bound2 (kernels/gicp_kernels.hip) assumes of a built grid: the offsets are monotone and end at n, every
// dim is in 1 .. R360_GICP_MAXDIM, and every point lies within 1 % of a cell edge of the box of the cell it was sorted
// into, on every axis, the clamped last cell included.  Returns the grid.
static GicpGrid check_ring_invariant(const std::vector<float>& xyz) {
    std::vector<float> pts, sorted;
    std::vector<unsigned> start;
    gicp_intake(xyz.data(), xyz.size() / 3, pts);
    const size_t n = pts.size() / 4;
    GicpGrid G;
    gicp_build_grid(pts, G, sorted, start);
    const size_t cells = (size_t)G.dim[0] * G.dim[1] * G.dim[2];
    EXPECT(start.size() == cells + 1 && start[0] == 0 && start[cells] == n);
    for (int a = 0; a < 3; ++a) EXPECT(G.dim[a] >= 1 && G.dim[a] <= R360_GICP_MAXDIM);
    const double h = (double)G.h, slack = 0.01 * h;
    for (size_t c = 0; c < cells; ++c) {
        EXPECT(start[c] <= start[c + 1]);
        const size_t cc[3] = {c % (size_t)G.dim[0], (c / (size_t)G.dim[0]) % (size_t)G.dim[1],
                              c / ((size_t)G.dim[0] * (size_t)G.dim[1])};
        for (unsigned q = start[c]; q < start[c + 1]; ++q)
            for (int a = 0; a < 3; ++a) {
                const double x = (double)sorted[4 * q + a], lo = (double)G.mn[a] + (double)cc[a] * h;
                EXPECT(x >= lo - slack && x <= lo + h + slack);
            }
    }
    return G;
}

// the crafted clouds of tests/_gicp_cases.py, by recipe (the generator differs, the shapes do not)
static void check_crafted_grids() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u01(0.f, 1.f);
    std::normal_distribution<float> gauss(0.f, 1.f);
    for (int rep = 0; rep < 8; ++rep) {   // the capped axis falls to 1023 or 1024 cells with the rounding: several draws
        std::vector<float> sheet(3 * 900), rod(3 * 2000), ribbon(3 * 7000), two(3 * 2000);
        for (size_t i = 0; i < 900; ++i) { sheet[3 * i] = 3.f * u01(rng); sheet[3 * i + 1] = 2.f * u01(rng); sheet[3 * i + 2] = 0.5f; }
        for (size_t i = 0; i < 2000; ++i) {
            rod[3 * i] = 10.f * u01(rng); rod[3 * i + 1] = 0.004f * u01(rng); rod[3 * i + 2] = 0.0002f * gauss(rng);
            const float off = i % 2 ? 1000.f : 0.f;   // interleaved: index order is not spatial order
            two[3 * i] = off + 6.f * u01(rng) - 3.f; two[3 * i + 1] = 4.f * u01(rng) - 2.f; two[3 * i + 2] = 3.f * u01(rng) - 1.5f;
        }
        for (size_t i = 0; i < 7000; ++i) {
            ribbon[3 * i] = 10.f * u01(rng); ribbon[3 * i + 1] = 0.05f * u01(rng); ribbon[3 * i + 2] = 0.0005f * gauss(rng);
        }
        GicpGrid G = check_ring_invariant(sheet);
        EXPECT(G.dim[0] >= 36 && G.dim[0] <= 38 && G.dim[1] >= 24 && G.dim[1] <= 26 && G.dim[2] == 1);
        G = check_ring_invariant(rod);
        EXPECT((G.dim[0] == 1023 || G.dim[0] == 1024) && G.dim[1] == 1 && G.dim[2] == 1);
        G = check_ring_invariant(ribbon);
        EXPECT((G.dim[0] == 1023 || G.dim[0] == 1024) && G.dim[1] >= 5 && G.dim[1] <= 6 && G.dim[2] == 1);
        G = check_ring_invariant(two);
        EXPECT(G.dim[0] >= 499 && G.dim[0] <= 503 && G.dim[1] == 2 && G.dim[2] == 2);
        check_grid(sheet); check_grid(rod); check_grid(ribbon); check_grid(two);
    }
}

// gicp_host_check FILE...: each file holds float32 x y z rows; prints "grid dx dy dz h" for it after the same checks
static int grids_of_files(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) {
        std::FILE* f = std::fopen(argv[k], "rb");
        EXPECT(f);
        std::vector<float> xyz;
        float buf[3];
        while (std::fread(buf, sizeof(float), 3, f) == 3) xyz.insert(xyz.end(), buf, buf + 3);
        std::fclose(f);
        EXPECT(!xyz.empty());
        const GicpGrid G = check_ring_invariant(xyz);
        check_grid(xyz);
        std::printf("grid %d %d %d %.9g\n", G.dim[0], G.dim[1], G.dim[2], (double)G.h);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return grids_of_files(argc, argv);
    check_crafted_grids();
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // intake
    {
        const float xyz[] = {1, 2, 3, nan, 0, 0, 4, 5, 6, 0, inf, 0, 7, 8, 9, 0, 0, -inf};
        std::vector<float> out;
        gicp_intake(xyz, 6, out);
        EXPECT(out.size() == 12 && out[0] == 1 && out[4] == 4 && out[8] == 7 && out[3] == 0);
        gicp_intake(nullptr, 0, out);
        EXPECT(out.empty());
    }
    // grids: a room, a plane, a line, one repeated point, a tiny cloud, huge and tiny extents, a crowded cell
    for (size_t n : {1u, 20u, 512u, 513u, 5000u, 60000u}) {
        std::vector<float> a(3 * n), b(3 * n), c(3 * n), d(3 * n, 2.5f), e(3 * n), f(3 * n), g(3 * n);
        for (size_t i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) a[3 * i + k] = 3.f * u(rng);
            b[3 * i] = u(rng); b[3 * i + 1] = u(rng); b[3 * i + 2] = 0.5f;
            c[3 * i] = u(rng); c[3 * i + 1] = 1.f; c[3 * i + 2] = -1.f;
            for (int k = 0; k < 3; ++k) e[3 * i + k] = 1e30f * u(rng);
            for (int k = 0; k < 3; ++k) f[3 * i + k] = 1000.f + 1e-4f * u(rng);
            for (int k = 0; k < 3; ++k) g[3 * i + k] = (i % 4 ? 0.01f : 5.f) * u(rng);
        }
        if (n > 2) a[3] = nan;
        for (const auto* v : {&a, &b, &c, &d, &e, &f, &g}) check_grid(*v);
    }
    // the solve
    {
        double H[36] = {0}, g[6], x[6];
        for (int i = 0; i < 6; ++i) { H[i * 6 + i] = i + 1.0; g[i] = -(i + 1.0) * (i - 2.5); }
        H[1] = H[6] = 0.25;
        EXPECT(gicp_solve6(H, g, x));
        for (int i = 0; i < 6; ++i) {
            double r = g[i];
            for (int j = 0; j < 6; ++j) r += H[i * 6 + j] * x[j];
            EXPECT(std::fabs(r) < 1e-12);
        }
        double Z[36] = {0};
        EXPECT(!gicp_solve6(Z, g, x));
        H[0] = nan;
        EXPECT(!gicp_solve6(H, g, x));
    }
    // the inner loop on f(t) = |t - t*|^2 (translation only): H = 2 I, g = 2 (t - t*); one step lands, the next
    // |delta| is below 1e-10 or the step is rejected
    {
        const double target[3] = {0.3, -0.2, 0.1};
        int passes = 0;
        auto pass = [&](const double* Y, double* s) {
            ++passes;
            for (int k = 0; k < 29; ++k) s[k] = 0;
            for (int k = 0; k < 3; ++k) { const double r = Y[k * 4 + 3] - target[k]; s[0] += r * r; s[1 + k] = 2 * r; }
            const int diag[6] = {7, 13, 18, 22, 25, 27};
            for (int k = 0; k < 6; ++k) s[diag[k]] = 2.0;
            s[28] = 10;
            return 0;
        };
        auto expmap = [](const double* d, float* E) {   // translation only
            for (int k = 0; k < 16; ++k) E[k] = (k % 5 == 0) ? 1.f : 0.f;
            for (int k = 0; k < 3; ++k) E[12 + k] = (float)d[k];
        };
        double Y[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, sums[29];
        int steps = -1;
        EXPECT(gicp_inner(pass, expmap, 20, Y, sums, &steps) == 0);
        EXPECT(steps >= 1 && steps <= 3 && passes <= steps + 2);
        for (int k = 0; k < 3; ++k) EXPECT(std::fabs(Y[k * 4 + 3] - target[k]) < 1e-7);
        // the step limit
        double Y2[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        EXPECT(gicp_inner(pass, expmap, 0, Y2, sums, &steps) == 0 && steps == 0 && Y2[3] == 0.0);
        // no correspondence, a singular first system, a failing pass
        auto none = [&](const double*, double* s) { for (int k = 0; k < 29; ++k) s[k] = 0; return 0; };
        EXPECT(gicp_inner(none, expmap, 20, Y2, sums, &steps) == 1 && steps == 0);
        auto singular = [&](const double*, double* s) { for (int k = 0; k < 29; ++k) s[k] = 0; s[28] = 5; s[0] = 1; return 0; };
        EXPECT(gicp_inner(singular, expmap, 20, Y2, sums, &steps) == 1 && steps == 0);
        auto failing = [&](const double*, double*) { return -1; };
        EXPECT(gicp_inner(failing, expmap, 20, Y2, sums, &steps) < 0);
    }
    std::puts("gicp host check ok");
    return 0;
}
