// map.cpp — FilterPointCloud::filterVoxel (pcl::VoxelGrid restated from PCL 1.7, unpinned) on the GPU and the
// context's global map: globalMap += cloud; filter.filterVoxel(globalMap) of SLAM/SphereGraphSLAM.cpp:136-137,
// :208-209 with the map resident in HBM.  Kernels: kernels/map_kernels.hip; semantics, the quantum and the supported
// domain: DESIGN.md §5b.  Every device buffer here is a DevBuf / PinnedBuf member of the r360_ctx's MapState (devmem.h),
// grown on demand by the arithmetic below and freed with the context: there is no handle type and no static owner.
#include <cmath>
#include <cstring>

#include "../r360_internal.h"

namespace {

// what a buffer of `cap` items grows to for `need`: a 1024-item floor, and half as much again, so that a growing map
// does not reallocate per frame
size_t stepped(size_t cap, size_t need) {
    return need <= cap ? cap : std::max(std::max<size_t>(need, 1024), cap + cap / 2);
}

int ensure_hdr(r360_ctx* ctx) {
    MapState& M = ctx->vmap;
    return M.d_hdr.reserve(ctx, 1) || M.h_hdr.reserve(ctx, 1) ? -1 : 0;
}

int read_hdr(r360_ctx* ctx) {
    MapState& M = ctx->vmap;
    R360_HIP(hipMemcpyAsync(M.h_hdr.get(), M.d_hdr.get(), sizeof(MapHdr), hipMemcpyDeviceToHost, ctx->stream));
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
    if (launch_map_bounds(st, pts, n, M.d_hdr.get())) return -1;
    if (read_hdr(ctx)) return -1;
    const MapHdr& H = *M.h_hdr.get();
    const unsigned long long count = H.count;
    if (count == 0) return 0;
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) { mn[k] = ord2f(H.mn[k]); mx[k] = ord2f(H.mx[k]); }
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
    if (M.table.reserve_zeroed(ctx, cap, st) || M.list.reserve(ctx, std::max<size_t>(M.table.cap() / 2, 1024))) return -1;
    const size_t nwords = (cells + 31) / 32, nb = (nwords + R360_MAP_SCAN_BLOCK - 1) / R360_MAP_SCAN_BLOCK;
    if (M.bitmap.reserve(ctx, stepped(M.bitmap.cap(), nwords)) || M.wprefix.reserve(ctx, stepped(M.wprefix.cap(), nwords)) ||
        M.bsum.reserve(ctx, stepped(M.bsum.cap(), nb)))
        return -1;
    R360_HIP(hipMemsetAsync(M.bitmap.get(), 0, sizeof(unsigned) * nwords, st));
    if (launch_map_insert(st, pts, n, G, M.table.get(), M.table.cap(), M.bitmap.get(), M.list.get(), M.d_hdr.get())) return -1;
    if (launch_map_scan(st, M.bitmap.get(), nwords, M.bsum.get(), M.wprefix.get())) return -1;
    if (launch_map_finalise(st, pts, n, M.table.get(), M.table.cap(), M.list.get(), M.bitmap.get(), nwords, M.wprefix.get(),
                            M.d_hdr.get(), out, out_cap))
        return -1;
    if (read_hdr(ctx)) return -1;
    if (H.err || H.m > occupied_max) {
        // cannot happen with a table at most half full; leave a clean table behind all the same
        hipMemsetAsync(M.table.get(), 0, sizeof(MapCell) * M.table.cap(), st);
        ctx_wait(ctx);
        r360_set_error("voxel grid: internal error (flags %u, %u voxels)", H.err, H.m);
        return -1;
    }
    *m = H.m;
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
    if (M.up_xyz.reserve(ctx, stepped(M.up_xyz.cap(), 3 * n)) || M.up_rgba.reserve(ctx, stepped(M.up_rgba.cap(), n))) return -1;
    R360_HIP(hipMemcpyAsync(M.up_xyz.get(), xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    if (rgba) R360_HIP(hipMemcpyAsync(M.up_rgba.get(), rgba, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    return launch_map_pack_host(ctx->stream, M.up_xyz.get(), rgba ? M.up_rgba.get() : nullptr, n, dst);
}

// packed points src[0 .. m) -> host arrays
int download_cloud(r360_ctx* ctx, const uint4* src, size_t m, float* xyz, uint32_t* rgba) {
    MapState& M = ctx->vmap;
    if (m == 0) return 0;
    if (M.up_xyz.reserve(ctx, stepped(M.up_xyz.cap(), 3 * m)) || M.up_rgba.reserve(ctx, stepped(M.up_rgba.cap(), m))) return -1;
    if (launch_map_unpack(ctx->stream, src, m, M.up_xyz.get(), M.up_rgba.get())) return -1;
    if (xyz) R360_HIP(hipMemcpyAsync(xyz, M.up_xyz.get(), sizeof(float) * 3 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (rgba) R360_HIP(hipMemcpyAsync(rgba, M.up_rgba.get(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_wait(ctx);
}

// room for map_n + extra points in the map's current buffer (contents kept) and in the other one
int map_reserve(r360_ctx* ctx, size_t extra) {
    MapState& M = ctx->vmap;
    const size_t need = M.map_n + extra;
    DevBuf<uint4>& cur = M.map[M.cur];
    if (need > cur.cap()) {   // a fresh buffer, the map copied into it on the stream, then it takes the old one's place
        DevBuf<uint4> grown;
        if (grown.reserve(nullptr, stepped(cur.cap(), need))) return -1;
        if (M.map_n)
            R360_HIP(hipMemcpyAsync(grown.get(), cur.get(), sizeof(uint4) * M.map_n, hipMemcpyDeviceToDevice, ctx->stream));
        if (ctx_wait(ctx)) return -1;
        cur = std::move(grown);
    }
    DevBuf<uint4>& other = M.map[1 - M.cur];
    return other.reserve(ctx, stepped(other.cap(), need));
}

// map <- voxel(map ++ the `extra` points already packed behind it)
int map_commit(r360_ctx* ctx, size_t extra, float leaf) {
    MapState& M = ctx->vmap;
    size_t m = 0;
    const int rc = voxel_run(ctx, M.map[M.cur].get(), M.map_n + extra, leaf, M.map[1 - M.cur].get(), M.map[1 - M.cur].cap(), &m);
    if (rc != 0) return rc;   // the guard's soft failure and errors leave the map as it was
    M.cur = 1 - M.cur;
    M.map_n = m;
    return 0;
}

}  // namespace

extern "C" int r360_cloud_filter_voxel(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, float leaf,
                                       float* out_xyz, uint32_t* out_rgba, size_t cap, size_t* n_out) {
    if (int rc = check_cloud_args(ctx, xyz, n, leaf)) return rc;
    CHECK_ARG(n_out && (n == 0 || out_xyz), "null output");
    *n_out = 0;
    if (n == 0) return 0;
    if (bind_device(ctx->device)) return -1;
    MapState& M = ctx->vmap;
    if (M.in.reserve(ctx, stepped(M.in.cap(), n)) || M.out.reserve(ctx, stepped(M.out.cap(), n))) return -1;
    if (upload_cloud(ctx, xyz, rgba, n, M.in.get())) return -1;
    size_t m = 0;
    const int rc = voxel_run(ctx, M.in.get(), n, leaf, M.out.get(), M.out.cap(), &m);
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
    return download_cloud(ctx, M.out.get(), m, out_xyz, out_rgba);
}

extern "C" int r360_ctx_map_reset(r360_ctx* ctx) {
    CHECK_ARG(ctx, "null ctx");
    ctx->vmap.map_n = 0;
    ctx->map_changed();
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
    if (upload_cloud(ctx, xyz, rgba, n, M.map[M.cur].get() + M.map_n)) return -1;
    ctx->map_changed();
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
    CHECK_ARG(P.v.cloud && P.v.rgb && P.w > 0 && P.h > 0, "the frame has no cloud buffers");
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
    if (launch_map_pack_frame(ctx->stream, P.v.cloud, P.v.rgb, per, rig, T, x_min, x_max, box, M.map[M.cur].get() + M.map_n))
        return -1;
    ctx->map_changed();
    return map_commit(ctx, n, leaf);
}

extern "C" int r360_ctx_map_download(r360_ctx* ctx, float* xyz, uint32_t* rgba, size_t cap, size_t* n) {
    CHECK_ARG(ctx && n, "null arg");
    MapState& M = ctx->vmap;
    *n = M.map_n;
    if (M.map_n == 0 || (!xyz && !rgba)) return 0;
    if (cap < M.map_n) { r360_set_error("map download: capacity %zu < %zu points", cap, M.map_n); return -4; }
    if (bind_device(ctx->device)) return -1;
    return download_cloud(ctx, M.map[M.cur].get(), M.map_n, xyz, rgba);
}
