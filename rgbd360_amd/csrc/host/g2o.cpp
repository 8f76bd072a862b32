// g2o.cpp — the g2o text files the reference's GraphOptimizer::saveGraph writes (g2o's optimizer.save):
//   VERTEX_SE3:QUAT id x y z qx qy qz qw        FIX id        EDGE_SE3:QUAT i j x y z qx qy qz qw  o00 o01 .. o55
// (the 21 upper-triangular entries of the information matrix, row-major).  Host only, no context, like the PCD codec.
// Numbers are printed with %.17g, so translations and information matrices come back bit for bit.
//
// A rotation goes through a quaternion (Shepperd's method, qw >= 0).  So that a file that is read and written again
// comes out byte for byte, the writer snaps the quaternion's direction to a lattice before printing: the components'
// ratios to the largest one are rounded to multiples of 2^-48, then the quadruple is normalised.  The reader's matrix
// gives those ratios back within about 5e-16 (both directions are worked in long double, leaving the matrix's own
// rounding), far inside half a lattice step (1.8e-15), so the second writer finds the same lattice point.  The snap
// moves a rotation entry by less than 1e-14.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../r360_internal.h"

namespace {

// column-major 4x4 pose -> unit quaternion (x, y, z, w) on the lattice
void quat_of(const double* T, double q[4]) {
    long double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = T[c * 4 + r];
    const long double tr = R[0][0] + R[1][1] + R[2][2];
    long double u[4];
    int k = 3;
    long double best = tr;
    for (int a = 0; a < 3; ++a)
        if (R[a][a] > best) { best = R[a][a]; k = a; }
    if (k == 3) {
        u[3] = 0.5L * sqrtl(1.0L + tr);
        const long double s = 0.25L / u[3];
        u[0] = (R[2][1] - R[1][2]) * s;
        u[1] = (R[0][2] - R[2][0]) * s;
        u[2] = (R[1][0] - R[0][1]) * s;
    } else {
        const int i = k, j = (k + 1) % 3, l = (k + 2) % 3;
        u[i] = 0.5L * sqrtl(((1.0L + R[i][i]) - R[j][j]) - R[l][l]);
        const long double s = 0.25L / u[i];
        u[3] = (R[l][j] - R[j][l]) * s;
        u[j] = (R[j][i] + R[i][j]) * s;
        u[l] = (R[l][i] + R[i][l]) * s;
    }
    int m = 0;
    for (int a = 1; a < 4; ++a)
        if (fabsl(u[a]) > fabsl(u[m])) m = a;
    const long double step = 281474976710656.0L;   // 2^48
    long double c[4], n2 = 0.0L;
    for (int a = 0; a < 4; ++a) {
        c[a] = a == m ? 1.0L : rintl(u[a] / u[m] * step) / step;
        n2 += c[a] * c[a];
    }
    const long double inv = (c[3] < 0.0L ? -1.0L : 1.0L) / sqrtl(n2);
    for (int a = 0; a < 4; ++a) q[a] = (double)(c[a] * inv);
}

// translation and quaternion -> column-major 4x4
void pose_of(const double t[3], const double q[4], double* T) {
    const long double x = q[0], y = q[1], z = q[2], w = q[3];
    const long double s = 2.0L / (x * x + y * y + z * z + w * w);
    const long double R[3][3] = {{1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)},
                                 {s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)},
                                 {s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)}};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) T[c * 4 + r] = r < 3 ? (c < 3 ? (double)R[r][c] : t[r]) : (c == 3 ? 1.0 : 0.0);
}

// the next n numbers of a line; false if one is missing or malformed
bool numbers(char*& p, int n, double* out) {
    for (int k = 0; k < n; ++k) {
        char* end = nullptr;
        errno = 0;
        out[k] = strtod(p, &end);
        if (end == p || errno == ERANGE) return false;
        p = end;
    }
    return true;
}

bool is_integer(double v) { return v >= 0.0 && v < 2147483647.0 && v == std::floor(v); }

}  // namespace

extern "C" int r360_g2o_write(const char* path, int n_vertices, const double* poses, const int* fixed, int n_edges,
                              const int* ij, const double* rel, const double* info) {
    CHECK_ARG(path && n_vertices >= 0 && n_edges >= 0, "invalid arguments");
    CHECK_ARG(n_vertices == 0 || poses, "null poses");
    CHECK_ARG(n_edges == 0 || (ij && rel && info), "null edges");
    std::string out;
    char buf[1024];
    auto se3 = [&](const double* T) {
        double q[4];
        quat_of(T, q);
        snprintf(buf, sizeof buf, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g", T[12], T[13], T[14], q[0], q[1], q[2], q[3]);
        out += buf;
    };
    for (int v = 0; v < n_vertices; ++v) {
        for (int k = 0; k < 16; ++k) CHECK_ARG(std::isfinite(poses[(size_t)v * 16 + k]), "g2o: non-finite pose");
        snprintf(buf, sizeof buf, "VERTEX_SE3:QUAT %d", v);
        out += buf;
        se3(poses + (size_t)v * 16);
        out += "\n";
        if (fixed && fixed[v]) {
            snprintf(buf, sizeof buf, "FIX %d\n", v);
            out += buf;
        }
    }
    for (int e = 0; e < n_edges; ++e) {
        const int i = ij[2 * e], j = ij[2 * e + 1];
        CHECK_ARG(i >= 0 && j >= 0 && i < n_vertices && j < n_vertices, "g2o: an edge names a missing vertex");
        snprintf(buf, sizeof buf, "EDGE_SE3:QUAT %d %d", i, j);
        out += buf;
        se3(rel + (size_t)e * 16);
        const double* O = info + (size_t)e * 36;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) {
                snprintf(buf, sizeof buf, " %.17g", O[c * 6 + r]);   // column-major (r, c)
                out += buf;
            }
        out += "\n";
    }
    FILE* f = fopen(path, "wb");
    if (!f) { r360_set_error("g2o: cannot open %s for writing", path); return -1; }
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) { r360_set_error("g2o: short write to %s", path); return -1; }
    return 0;
}

extern "C" int r360_g2o_read(const char* path, double* poses, int* fixed, int cap_vertices, int* n_vertices, int* ij,
                             double* rel, double* info, int cap_edges, int* n_edges) {
    CHECK_ARG(path && n_vertices && n_edges, "invalid arguments");
    FILE* f = fopen(path, "rb");
    if (!f) { r360_set_error("g2o: cannot open %s", path); return -1; }
    std::string text;
    char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) text.append(chunk, got);
    fclose(f);
    // two passes over the lines: count and check, then store
    int nv = 0, ne = 0, max_ref = -1;
    std::vector<int> ids;
    const bool store = poses || fixed || ij || rel || info;
    for (int pass = 0; pass < (store ? 2 : 1); ++pass) {
        if (pass == 1) {
            if (nv > cap_vertices || ne > cap_edges) {
                *n_vertices = nv; *n_edges = ne;
                r360_set_error("g2o: capacity %d / %d < %d vertices / %d edges", cap_vertices, cap_edges, nv, ne);
                return -4;
            }
            if (fixed) memset(fixed, 0, sizeof(int) * (size_t)nv);
        }
        int line_no = 0, seen_v = 0, e = 0;
        size_t pos = 0;
        while (pos < text.size()) {
            size_t eol = text.find('\n', pos);
            if (eol == std::string::npos) eol = text.size();
            std::string line = text.substr(pos, eol - pos);
            pos = eol + 1;
            ++line_no;
            char* p = &line[0];
            while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
            if (*p == 0 || *p == '#') continue;
            char* tag = p;
            while (*p && *p != ' ' && *p != '\t' && *p != '\r') ++p;
            const std::string name(tag, p);
            double v[32];
            if (name == "VERTEX_SE3:QUAT") {
                if (!numbers(p, 8, v) || !is_integer(v[0])) { r360_set_error("g2o: %s:%d: short or malformed vertex line", path, line_no); return -2; }
                const int id = (int)v[0];
                if (v[4] == 0.0 && v[5] == 0.0 && v[6] == 0.0 && v[7] == 0.0) { r360_set_error("g2o: %s:%d: zero quaternion", path, line_no); return -2; }
                if (pass == 0) { ++nv; ids.push_back(id); }
                else {
                    if (id >= nv) { r360_set_error("g2o: %s:%d: vertex ids are not 0 .. n-1", path, line_no); return -2; }
                    if (poses) pose_of(v + 1, v + 4, poses + (size_t)id * 16);
                }
                ++seen_v;
            } else if (name == "FIX") {
                if (!numbers(p, 1, v) || !is_integer(v[0])) { r360_set_error("g2o: %s:%d: short or malformed FIX line", path, line_no); return -2; }
                if (seen_v == 0) { r360_set_error("g2o: %s:%d: FIX before the first vertex", path, line_no); return -2; }
                max_ref = std::max(max_ref, (int)v[0]);
                if (pass == 1) {
                    if ((int)v[0] >= nv) { r360_set_error("g2o: %s:%d: FIX names a missing vertex", path, line_no); return -2; }
                    if (fixed) fixed[(int)v[0]] = 1;
                }
            } else if (name == "EDGE_SE3:QUAT") {
                if (!numbers(p, 30, v) || !is_integer(v[0]) || !is_integer(v[1])) { r360_set_error("g2o: %s:%d: short or malformed edge line", path, line_no); return -2; }
                if (v[5] == 0.0 && v[6] == 0.0 && v[7] == 0.0 && v[8] == 0.0) { r360_set_error("g2o: %s:%d: zero quaternion", path, line_no); return -2; }
                max_ref = std::max(max_ref, std::max((int)v[0], (int)v[1]));
                if (pass == 0) ++ne;
                else {
                    if ((int)v[0] >= nv || (int)v[1] >= nv) { r360_set_error("g2o: %s:%d: the edge names a missing vertex", path, line_no); return -2; }
                    if (ij) { ij[2 * e] = (int)v[0]; ij[2 * e + 1] = (int)v[1]; }
                    if (rel) pose_of(v + 2, v + 5, rel + (size_t)e * 16);
                    if (info) {
                        int q = 9;
                        for (int r = 0; r < 6; ++r)
                            for (int c = r; c < 6; ++c, ++q) info[(size_t)e * 36 + c * 6 + r] = info[(size_t)e * 36 + r * 6 + c] = v[q];
                    }
                    ++e;
                }
            } else if (seen_v == 0) {
                r360_set_error("g2o: %s:%d: unknown tag '%s' before the first vertex", path, line_no, name.c_str());
                return -2;
            }   // a later unknown tag is skipped, as g2o does
        }
        if (pass == 0) {
            std::sort(ids.begin(), ids.end());
            for (int k = 0; k < nv; ++k)
                if (ids[k] != k) { r360_set_error("g2o: %s: vertex ids are not 0 .. n-1, each once", path); return -2; }
            if (max_ref >= nv) { r360_set_error("g2o: %s: a FIX or edge line names a missing vertex", path); return -2; }
        }
    }
    *n_vertices = nv;
    *n_edges = ne;
    return 0;
}
