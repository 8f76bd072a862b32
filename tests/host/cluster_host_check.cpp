// cluster_host_check.cpp — the host side of the cluster extraction without a GPU: the ranking tables
// (rgbd360_amd/csrc/host/cluster_rank.h) and the labelled PCD writer and reader (rgbd360_amd/csrc/host/io.cpp), built by
// tests/test_clusters_io.py with g++ and the address / undefined-behaviour sanitizers, no HIP runtime linked (the few
// runtime calls io.cpp's other entry points make are stubs that fail).  Usage: cluster_host_check <scratch dir>; prints
// "cluster host ok" and exits 0, or names the broken rule and exits 1.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "r360_internal.h"
#include "host/cluster_rank.h"

// ------------------------------------------------------------------ what io.cpp links against
static std::string g_error;
void r360_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
int ctx_wait(r360_ctx*) { return -1; }
void planes_join(r360_frame*) {}
extern "C" {
hipError_t hipGetDevice(int*) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
const char* hipGetErrorString(hipError_t) { return "no device"; }
hipError_t hipHostMalloc(void**, size_t, unsigned) { return hipErrorOutOfMemory; }
hipError_t hipHostFree(void*) { return hipSuccess; }
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipMalloc(void**, size_t) { return hipErrorOutOfMemory; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipErrorNoDevice; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipErrorNoDevice; }
}

static int g_errors = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            ++g_errors;                                                     \
        }                                                                   \
    } while (0)

static void check_ranking() {
    // sizes 2, 5000, 2, 4096, 1 at roots 0, 7, 3, 9, 4: by size descending, ties by root ascending
    const ClusterRankRec rec[5] = {{0, 2}, {7, 5000}, {3, 2}, {9, 4096}, {4, 1}};
    std::vector<int> rank_root;
    std::vector<unsigned> off, cpre;
    const size_t m = cluster_rank_tables(rec, 5, 4096, rank_root, off, cpre);
    EXPECT(m == 9101);
    EXPECT((rank_root == std::vector<int>{7, 9, 0, 3, 4}));
    EXPECT((off == std::vector<unsigned>{0, 5000, 9096, 9098, 9100, 9101}));
    EXPECT((cpre == std::vector<unsigned>{0, 2, 3, 4, 5, 6}));
    EXPECT(cluster_rank_tables(nullptr, 0, 4096, rank_root, off, cpre) == 0);
    EXPECT(rank_root.empty() && off == std::vector<unsigned>{0} && cpre == std::vector<unsigned>{0});
    // many equal sizes in descending root order come back ascending
    std::vector<ClusterRankRec> many;
    for (int k = 0; k < 1000; ++k) many.push_back({999 - k, 3});
    EXPECT(cluster_rank_tables(many.data(), many.size(), 4096, rank_root, off, cpre) == 3000);
    for (int k = 0; k < 1000; ++k) EXPECT(rank_root[k] == k && off[k] == 3u * k && cpre[k] == (unsigned)k);
}

static void check_pcd(const std::string& dir) {
    const size_t n = 257;
    std::vector<float> xyz(3 * n);
    std::vector<uint32_t> rgba(n);
    std::vector<int> labels(n);
    for (size_t i = 0; i < n; ++i) {
        xyz[3 * i] = 0.1f * (float)i; xyz[3 * i + 1] = -1.0f / (float)(i + 1); xyz[3 * i + 2] = (i % 7 == 0) ? NAN : 3.25f;
        rgba[i] = 0xff000000u | (uint32_t)(i * 2654435761u);
        labels[i] = (i % 5 == 0) ? -1 : (int)(i % 11);
    }
    for (int mode = 0; mode < 3; ++mode) {
        const std::string path = dir + "/labels_" + std::to_string(mode) + ".pcd";
        EXPECT(r360_pcd_write_labels(path.c_str(), xyz.data(), rgba.data(), labels.data(), n, mode) == 0);
        size_t m = 0;
        EXPECT(r360_pcd_read_labels(path.c_str(), nullptr, nullptr, nullptr, 0, &m) == 0 && m == n);
        std::vector<float> x2(3 * n);
        std::vector<uint32_t> c2(n);
        std::vector<int> l2(n);
        EXPECT(r360_pcd_read_labels(path.c_str(), x2.data(), c2.data(), l2.data(), n, &m) == 0 && m == n);
        EXPECT(l2 == labels && c2 == rgba);
        // ascii prints coordinates with eight digits, as savePCDFile does; the binary modes keep the bits
        bool same = true;
        for (size_t i = 0; i < 3 * n; ++i)
            same = same && ((std::isnan(xyz[i]) && std::isnan(x2[i])) ||
                            (mode == 0 ? std::fabs(xyz[i] - x2[i]) <= 1e-7f * std::fabs(xyz[i]) : xyz[i] == x2[i]));
        EXPECT(same);
        // a smaller capacity reads the first points and writes nothing beyond them
        std::vector<int> l3(10, 12345);
        EXPECT(r360_pcd_read_labels(path.c_str(), nullptr, nullptr, l3.data(), 9, &m) == 0 && m == n);
        EXPECT(l3[9] == 12345 && std::equal(l3.begin(), l3.begin() + 9, labels.begin()));
        // the plain reader takes the file too
        int w = 0, h = 0;
        EXPECT(r360_pcd_read(path.c_str(), x2.data(), c2.data(), n, &m, &w, &h) == 0 && m == n && w == (int)n && h == 1);
    }
    // no label field: the label reader refuses, whatever it is asked to return
    const std::string plain = dir + "/plain.pcd";
    EXPECT(r360_pcd_write(plain.c_str(), xyz.data(), rgba.data(), (int)n, 1, 1) == 0);
    size_t m = 0;
    EXPECT(r360_pcd_read_labels(plain.c_str(), nullptr, nullptr, nullptr, 0, &m) < 0);
    EXPECT(g_error.find("no label field") != std::string::npos);
    // empty cloud, NULL labels and colours
    const std::string empty = dir + "/empty.pcd";
    EXPECT(r360_pcd_write_labels(empty.c_str(), nullptr, nullptr, nullptr, 0, 1) == 0);
    EXPECT(r360_pcd_read_labels(empty.c_str(), nullptr, nullptr, nullptr, 0, &m) == 0 && m == 0);
    const std::string bare = dir + "/bare.pcd";
    EXPECT(r360_pcd_write_labels(bare.c_str(), xyz.data(), nullptr, nullptr, n, 0) == 0);
    std::vector<int> l4(n, 7);
    EXPECT(r360_pcd_read_labels(bare.c_str(), nullptr, nullptr, l4.data(), n, &m) == 0 && l4 == std::vector<int>(n, 0));
    EXPECT(r360_pcd_write_labels(nullptr, xyz.data(), nullptr, nullptr, n, 0) == -2);
    EXPECT(r360_pcd_write_labels(bare.c_str(), xyz.data(), nullptr, nullptr, n, 3) == -2);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <scratch dir>\n", argv[0]); return 2; }
    check_ranking();
    check_pcd(argv[1]);
    if (g_errors) return 1;
    std::printf("cluster host ok\n");
    return 0;
}
