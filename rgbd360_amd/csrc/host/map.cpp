// map.cpp — FilterPointCloud::filterVoxel (pcl::VoxelGrid restated from PCL 1.7, unpinned) on the GPU and the
// context's global map: globalMap += cloud; filter.filterVoxel(globalMap) of SLAM/SphereGraphSLAM.cpp:136-137,
// :208-209 with the map resident in HBM.  Kernels: kernels/map_kernels.hip; semantics, the quantum and the supported
// domain: DESIGN.md §5b.  Every device buffer here is a plain pointer in the r360_ctx's MapState, grown on demand
// and freed by r360_ctx_destroy: there is no handle type and no static owner.
#include <cmath>
#include <cstring>

#include "../r360_internal.h"

namespace {

// frees `p` (after the stream has drained, so no enqueued pass still uses it) and allocates `need` items
template <class T>
int regrow(r360_ctx* ctx, T*& p, size_t& cap, size_t need, bool zero, bool geometric = true) {
    if (need <= cap) return 0;
    size_t want = std::max<size_t>(need, 1024);
    // geometric: a growing map does not reallocate per frame
    if (geometric && cap && want < cap + cap / 2) want = cap + cap / 2;
    if (p) {
        if (ctx_wait(ctx)) return -1;
        R360_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
    }
    R360_HIP(hipMalloc(&p, sizeof(T) * want));
    if (zero) R360_HIP(hipMemsetAsync(p, 0, sizeof(T) * want, ctx->stream));
    cap = want;
    return 0;
}

int ensure_hdr(r360_ctx* ctx) {
    MapState& M = ctx->vmap;
    if (!M.d_hdr) R360_HIP(hipMalloc(&M.d_hdr, sizeof(MapHdr)));
    if (!M.h_hdr) R360_HIP(hipHostMalloc(&M.h_hdr, sizeof(MapHdr), hipHostMallocDefault));
    return 0;
}

int read_hdr(r360_ctx* ctx) {
    MapState& M = ctx->vmap;
    R360_HIP(hipMemcpyAsync(M.h_hdr, M.d_hdr, sizeof(MapHdr), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

float ord2f(unsigned e) {
    const unsigned u = (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// The voxel grid of pts[0 .. n) into out (room for n points).  0 with *m points, 1 when PCL's size guard refuses the
// leaf (nothing written), < 0 on error.  Synchronous.
int voxel_run(r360_ctx* ctx, const uint4* pts, size_t n, float leaf, uint4* out, size_t out_cap, size_t* m) {
    MapState& M = ctx->vmap;
    hipStream_t st = ctx->stream;
    *m = 0;
    const float inv = 1.0f / leaf;
    if (ensure_hdr(ctx)) return -1;
    if (launch_map_bounds(st, pts, n, M.d_hdr)) return -1;
    if (read_hdr(ctx)) return -1;
    const unsigned long long count = M.h_hdr->count;
    if (count == 0) return 0;
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) { mn[k] = ord2f(M.h_hdr->mn[k]); mx[k] = ord2f(M.h_hdr->mx[k]); }
    // PCL 1.7 voxel_grid.hpp: dx = (int64)((max - min) * inv) + 1 per axis in float; dx*dy*dz > INT32_MAX -> refuse
    __int128 cells_est = 1;
    for (int k = 0; k < 3; ++k) {
        const float d = (mx[k] - mn[k]) * inv;
        if (!(d < 4.0e18f)) return 1;          // also an infinite or NaN product
        cells_est *= (__int128)((long long)d + 1);
    }
    if (cells_est > (__int128)INT32_MAX) return 1;
    // supported domain: voxel indices that fit an int with room to spare, and coordinate sums that cannot overflow
    float maxabs = 0.f;
    MapGrid G;
    G.inv = inv;
    long long ext[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = floorf(mn[k] * inv), hi = floorf(mx[k] * inv);
        if (!(fabsf(lo) < 1073741824.0f && fabsf(hi) < 1073741824.0f)) {
            r360_set_error("voxel grid: voxel index beyond 2^30 (coordinate %g at leaf %g is outside the supported domain)",
                           (double)(fabsf(lo) > fabsf(hi) ? mn[k] : mx[k]), (double)leaf);
            return -3;
        }
        G.minb[k] = (int)lo;
        ext[k] = (long long)hi - (long long)lo + 1;
        maxabs = std::max(maxabs, std::max(fabsf(mn[k]), fabsf(mx[k])));
    }
    // each term is at most ceil(maxabs) * 2^24 + 1 in magnitude; count terms must stay below 2^62
    if ((std::ceil((double)maxabs) * 16777216.0 + 1.0) * (double)count >= 4611686018427387904.0) {
        r360_set_error("voxel grid: %llu points with |coordinate| up to %g m would overflow the fixed-point sums "
                       "(supported: ceil(max |coordinate|) * 2^24 * points < 2^62)", count, (double)maxabs);
        return -3;
    }
    // the grid from the floors can be one voxel wider per axis than PCL's estimate: the index must still fit 31 bits
    const __int128 cells128 = (__int128)ext[0] * ext[1] * ext[2];
    if (cells128 > (__int128)INT32_MAX) return 1;
    const size_t cells = (size_t)cells128;
    G.dx = (unsigned)ext[0];
    G.dy = (unsigned)ext[1];
    const size_t occupied_max = std::min<size_t>((size_t)count, cells);
    if (out_cap < occupied_max) { r360_set_error("voxel grid: internal output buffer too small"); return -1; }
    size_t cap = 1024;
    while (cap < 2 * occupied_max) cap <<= 1;
    // the table's size stays a power of two (the probe mask), and it is zero whenever no call is running
    if (regrow(ctx, M.table, M.table_cap, cap, true, false) || regrow(ctx, M.list, M.list_cap, M.table_cap / 2, false, false))
        return -1;
    const size_t nwords = (cells + 31) / 32, nb = (nwords + R360_MAP_SCAN_BLOCK - 1) / R360_MAP_SCAN_BLOCK;
    if (regrow(ctx, M.bitmap, M.bitmap_cap, nwords, false) || regrow(ctx, M.wprefix, M.wprefix_cap, nwords, false) ||
        regrow(ctx, M.bsum, M.bsum_cap, nb, false))
        return -1;
    R360_HIP(hipMemsetAsync(M.bitmap, 0, sizeof(unsigned) * nwords, st));
    if (launch_map_insert(st, pts, n, G, M.table, M.table_cap, M.bitmap, M.list, M.d_hdr)) return -1;
    if (launch_map_scan(st, M.bitmap, nwords, M.bsum, M.wprefix)) return -1;
    if (launch_map_finalise(st, pts, n, M.table, M.table_cap, M.list, M.bitmap, nwords, M.wprefix, M.d_hdr, out, out_cap))
        return -1;
    if (read_hdr(ctx)) return -1;
    if (M.h_hdr->err || M.h_hdr->m > occupied_max) {
        // cannot happen with a table at most half full; leave a clean table behind all the same
        hipMemsetAsync(M.table, 0, sizeof(MapCell) * M.table_cap, st);
        ctx_wait(ctx);
        r360_set_error("voxel grid: internal error (flags %u, %u voxels)", M.h_hdr->err, M.h_hdr->m);
        return -1;
    }
    *m = M.h_hdr->m;
    return 0;
}

int check_cloud_args(r360_ctx* ctx, const float* xyz, size_t n, float leaf) {
    CHECK_ARG(ctx, "null ctx");
    CHECK_ARG(n == 0 || xyz, "null xyz");
    CHECK_ARG(n <= (size_t)1 << 30, "more than 2^30 points");
    CHECK_ARG(std::isfinite(leaf) && leaf > 0.f && std::isfinite(1.0f / leaf) && 1.0f / leaf > 0.f,
              "leaf must be positive and finite, with a finite 1 / leaf");
    return 0;
}

// host arrays -> packed points at dst[0 .. n)
int upload_cloud(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, uint4* dst) {
    MapState& M = ctx->vmap;
    if (n == 0) return 0;
    if (regrow(ctx, M.up_xyz, M.up_xyz_cap, 3 * n, false) || regrow(ctx, M.up_rgba, M.up_rgba_cap, n, false)) return -1;
    R360_HIP(hipMemcpyAsync(M.up_xyz, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    if (rgba) R360_HIP(hipMemcpyAsync(M.up_rgba, rgba, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    return launch_map_pack_host(ctx->stream, M.up_xyz, rgba ? M.up_rgba : nullptr, n, dst);
}

// packed points src[0 .. m) -> host arrays
int download_cloud(r360_ctx* ctx, const uint4* src, size_t m, float* xyz, uint32_t* rgba) {
    MapState& M = ctx->vmap;
    if (m == 0) return 0;
    if (regrow(ctx, M.up_xyz, M.up_xyz_cap, 3 * m, false) || regrow(ctx, M.up_rgba, M.up_rgba_cap, m, false)) return -1;
    if (launch_map_unpack(ctx->stream, src, m, M.up_xyz, M.up_rgba)) return -1;
    if (xyz) R360_HIP(hipMemcpyAsync(xyz, M.up_xyz, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (rgba) R360_HIP(hipMemcpyAsync(rgba, M.up_rgba, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

// room for map_n + extra points in the map's current buffer (contents kept) and in the other one
int map_reserve(r360_ctx* ctx, size_t extra) {
    MapState& M = ctx->vmap;
    const size_t need = M.map_n + extra;
    if (need > M.map_cap[M.cur]) {
        const size_t want = std::max<size_t>(std::max<size_t>(need, 1024), M.map_cap[M.cur] + M.map_cap[M.cur] / 2);
        uint4* p = nullptr;
        R360_HIP(hipMalloc(&p, sizeof(uint4) * want));
        if (M.map_n) {
            const hipError_t e = hipMemcpyAsync(p, M.map[M.cur], sizeof(uint4) * M.map_n, hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) { hipFree(p); r360_set_error("map copy -> %s", hipGetErrorString(e)); return -1; }
        }
        if (ctx_wait(ctx)) { hipFree(p); return -1; }
        if (M.map[M.cur]) hipFree(M.map[M.cur]);
        M.map[M.cur] = p;
        M.map_cap[M.cur] = want;
    }
    return regrow(ctx, M.map[1 - M.cur], M.map_cap[1 - M.cur], need, false);
}

// map <- voxel(map ++ the `extra` points already packed behind it)
int map_commit(r360_ctx* ctx, size_t extra, float leaf) {
    MapState& M = ctx->vmap;
    size_t m = 0;
    const int rc = voxel_run(ctx, M.map[M.cur], M.map_n + extra, leaf, M.map[1 - M.cur], M.map_cap[1 - M.cur], &m);
    if (rc != 0) return rc;   // the guard's soft failure and errors leave the map as it was
    M.cur = 1 - M.cur;
    M.map_n = m;
    return 0;
}

}  // namespace

void map_state_free(MapState& M) {
    hipFree(M.d_hdr); hipHostFree(M.h_hdr);
    hipFree(M.table); hipFree(M.list); hipFree(M.bitmap); hipFree(M.wprefix); hipFree(M.bsum);
    hipFree(M.up_xyz); hipFree(M.up_rgba); hipFree(M.in); hipFree(M.out);
    hipFree(M.map[0]); hipFree(M.map[1]);
    M = MapState();
}

extern "C" int r360_cloud_filter_voxel(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, float leaf,
                                       float* out_xyz, uint32_t* out_rgba, size_t cap, size_t* n_out) {
    if (int rc = check_cloud_args(ctx, xyz, n, leaf)) return rc;
    CHECK_ARG(n_out && (n == 0 || out_xyz), "null output");
    *n_out = 0;
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    MapState& M = ctx->vmap;
    if (regrow(ctx, M.in, M.in_cap, n, false) || regrow(ctx, M.out, M.out_cap, n, false)) return -1;
    if (upload_cloud(ctx, xyz, rgba, n, M.in)) return -1;
    size_t m = 0;
    const int rc = voxel_run(ctx, M.in, n, leaf, M.out, M.out_cap, &m);
    if (rc < 0) return rc;
    if (rc == 1) {   // PCL: "Leaf size is too small for the input dataset": the output is the input
        *n_out = n;
        if (cap < n) { r360_set_error("voxel grid: output capacity %zu < %zu points", cap, n); return -4; }
        if (out_xyz != xyz) memmove(out_xyz, xyz, sizeof(float) * 3 * n);
        if (rgba && out_rgba && out_rgba != rgba) memmove(out_rgba, rgba, sizeof(uint32_t) * n);
        return 1;
    }
    *n_out = m;
    if (cap < m) { r360_set_error("voxel grid: output capacity %zu < %zu voxels", cap, m); return -4; }
    return download_cloud(ctx, M.out, m, out_xyz, out_rgba);
}

extern "C" int r360_ctx_map_reset(r360_ctx* ctx) {
    CHECK_ARG(ctx, "null ctx");
    ctx->vmap.map_n = 0;
    return 0;
}

extern "C" int r360_ctx_map_size(r360_ctx* ctx, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    *n = ctx->vmap.map_n;
    return 0;
}

extern "C" int r360_ctx_map_add_cloud(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, float leaf) {
    if (int rc = check_cloud_args(ctx, xyz, n, leaf)) return rc;
    MapState& M = ctx->vmap;
    CHECK_ARG(M.map_n + n <= (size_t)1 << 30, "more than 2^30 points");
    if (M.map_n + n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    if (map_reserve(ctx, n)) return -1;
    if (upload_cloud(ctx, xyz, rgba, n, M.map[M.cur] + M.map_n)) return -1;
    return map_commit(ctx, n, leaf);
}

// the host chain on a loaded sphereCloud (already in the rig frame): the Euclidean box, then the pose, uncontracted
#pragma clang fp contract(off)
static void host_chain(const SphereCloudHost& sc, const float* m, float x_min, float x_max, float box,
                       std::vector<float>& xyz, std::vector<uint32_t>& rgba) {
    const size_t n = sc.rgba.size();
    xyz.reserve(3 * n);
    rgba.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const float x = sc.xyz[3 * i], y = sc.xyz[3 * i + 1], z = sc.xyz[3 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
        if (!(x >= x_min && x <= x_max && y >= -box && y <= box && z >= -box && z <= box)) continue;
        for (int k = 0; k < 3; ++k) {
            float a = m[k] * x;
            a = a + m[4 + k] * y;
            a = a + m[8 + k] * z;
            xyz.push_back(a + m[12 + k]);
        }
        rgba.push_back(sc.rgba[i]);
    }
}
#pragma clang fp contract(on)

extern "C" int r360_ctx_map_add_frame(r360_ctx* ctx, r360_frame* f, const float pose[16], float x_min, float x_max,
                                      float box, float leaf) {
    CHECK_ARG(ctx && f && pose, "null arg");
    if (int rc = check_cloud_args(ctx, nullptr, 0, leaf)) return rc;
    for (int k = 0; k < 16; ++k) CHECK_ARG(std::isfinite(pose[k]), "non-finite pose");
    if (f->sphere_cloud) {   // a cloud set by loadCloud lives on the host
        std::vector<float> xyz;
        std::vector<uint32_t> rgba;
        host_chain(*f->sphere_cloud, pose, x_min, x_max, box, xyz, rgba);
        return r360_ctx_map_add_cloud(ctx, xyz.data(), rgba.data(), rgba.size(), leaf);
    }
    CHECK_ARG(f->built & R360_BUILD_CLOUD, "no sphere cloud: build the frame with R360_BUILD_CLOUD or load one (loadCloud)");
    CHECK_ARG(f->ctx && f->ctx->device == ctx->device, "the frame lives on another device");
    if (bind_device(ctx->device)) return -1;
    planes_join(f);   // a plane queue builds the cloud on its own stream: the frame's assembly has waited for it
    const PlaneBufs& P = f->pl;
    CHECK_ARG(P.cloud && P.rgb && P.w > 0 && P.h > 0, "the frame has no cloud buffers");
    const size_t per = (size_t)P.w * P.h, n = 8 * per;
    MapState& M = ctx->vmap;
    CHECK_ARG(M.map_n + n <= (size_t)1 << 30, "more than 2^30 points");
    if (map_reserve(ctx, n)) return -1;
    r360_frame* fr[1] = {f};
    if (ctx_wait_frames(ctx, fr, 1)) return -1;   // a frame of another context: wait for its stream's work so far
    MapRig rig;
    memcpy(rig.rt, f->calib->rt, sizeof rig.rt);
    MapPose T;
    memcpy(T.m, pose, sizeof T.m);
    if (launch_map_pack_frame(ctx->stream, P.cloud, P.rgb, per, rig, T, x_min, x_max, box, M.map[M.cur] + M.map_n)) return -1;
    return map_commit(ctx, n, leaf);
}

extern "C" int r360_ctx_map_download(r360_ctx* ctx, float* xyz, uint32_t* rgba, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    MapState& M = ctx->vmap;
    *n = M.map_n;
    if (M.map_n == 0 || (!xyz && !rgba)) return 0;
    if (cap < M.map_n) { r360_set_error("map download: capacity %zu < %zu points", cap, M.map_n); return -4; }
    if (bind_device(ctx->device)) return -1;
    return download_cloud(ctx, M.map[M.cur], M.map_n, xyz, rgba);
}
