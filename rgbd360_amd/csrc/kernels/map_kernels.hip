// map_kernels.hip — pcl::VoxelGrid (FilterPointCloud::filterVoxel, SLAM/SphereGraphSLAM.cpp:137, :209) and the map
// step's fused front end on gfx950.  Semantics and design: DESIGN.md §5b; the numpy statement is
// tests/test_map.py::voxel_model plus the guard of tests/test_voxel_host.py.
//
//   k_map_pack_host / k_map_pack_frame   the input as 16-byte points {x, y, z bits, rgba}; the frame form applies
//                                        Rt_[sensor], the Euclidean box and the pose on the way
//   k_map_bounds                         min / max / count of the finite points (wave reduction, then integer atomics)
//   k_map_insert                         per workgroup an LDS table pre-aggregates equal voxels of a 512-point tile,
//                                        then one claim (atomicCAS) and one set of integer adds per distinct voxel
//   k_map_scan_*                         exclusive prefix of the occupancy bitmap's popcounts: the output order
//   k_map_finalise                       one output point per claimed cell at its rank; the cell is zeroed again
//
// Every sum is an integer (coordinates in 2^-24 m fixed point, 64-bit), so the result does not depend on the order
// in which points arrive: no float atomics here (the Makefile also keeps -munsafe-fp-atomics off this file).
#include "../r360_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int TILE = 512;          // points per LDS table fill
constexpr int LSLOTS = 1024;       // LDS table slots: never more than half full
constexpr unsigned NANBITS = 0x7fc00000u;

__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
// float bits -> unsigned with the same order (and back on the host, map.cpp)
__device__ __forceinline__ unsigned f2ord(unsigned u) { return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
__device__ __forceinline__ unsigned mix32(unsigned h) {   // murmur3's finaliser
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__global__ void __launch_bounds__(TPB) k_map_pack_host(const float* __restrict__ xyz, const uint32_t* __restrict__ rgba,
                                                       size_t n, uint4* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        uint4 p;
        p.x = __float_as_uint(xyz[3 * i]); p.y = __float_as_uint(xyz[3 * i + 1]); p.z = __float_as_uint(xyz[3 * i + 2]);
        p.w = rgba ? rgba[i] : 0u;
        out[i] = p;
    }
}

// m(k,0)*x + m(k,1)*y + m(k,2)*z + m(k,3), left to right (the file is compiled with -ffp-contract=off), as
// host/io.cpp and r360::transformPointCloud write it
__device__ __forceinline__ void xform(const float* m, float& x, float& y, float& z) {
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float a = m[k] * x;
        a = a + m[4 + k] * y;
        a = a + m[8 + k] * z;
        o[k] = a + m[12 + k];
    }
    x = o[0]; y = o[1]; z = o[2];
}

// The map step on a frame's per-sensor clouds: Rt_[sensor] (non-finite points stay), the closed Euclidean box (drops
// them), the pose.  A dropped point leaves a NaN, which the later passes skip.
__global__ void __launch_bounds__(TPB) k_map_pack_frame(const float4* __restrict__ cloud, const uchar4* __restrict__ rgb,
                                                        size_t per, MapRig rig, MapPose pose, float x_min, float x_max,
                                                        float box, uint4* __restrict__ out) {
    const size_t n = 8 * per;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const float4 c = cloud[i];
        const uchar4 q = rgb[i];
        float x = c.x, y = c.y, z = c.z;
        const bool fin = finite_bits(__float_as_uint(x)) && finite_bits(__float_as_uint(y)) && finite_bits(__float_as_uint(z));
        bool keep = false;
        if (fin) {
            xform(rig.rt[i / per], x, y, z);
            keep = finite_bits(__float_as_uint(x)) && finite_bits(__float_as_uint(y)) && finite_bits(__float_as_uint(z)) &&
                   x >= x_min && x <= x_max && y >= -box && y <= box && z >= -box && z <= box;
            if (keep) xform(pose.m, x, y, z);
        }
        uint4 p;
        p.x = keep ? __float_as_uint(x) : NANBITS; p.y = __float_as_uint(y); p.z = __float_as_uint(z);
        p.w = uint32_t(q.z) | uint32_t(q.y) << 8 | uint32_t(q.x) << 16 | uint32_t(q.w) << 24;
        out[i] = p;
    }
}

__global__ void k_map_hdr_init(MapHdr* hdr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int k = 0; k < 3; ++k) { hdr->mn[k] = 0xffffffffu; hdr->mx[k] = 0u; }
        hdr->count = 0; hdr->m = 0; hdr->err = 0; hdr->pad[0] = hdr->pad[1] = 0;
    }
}

__global__ void __launch_bounds__(TPB) k_map_bounds(const uint4* __restrict__ pts, size_t n, MapHdr* hdr) {
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, cnt = 0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const uint4 p = pts[i];
        if (!(finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z))) continue;
        const unsigned e[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], e[k]); mx[k] = max(mx[k], e[k]); }
        ++cnt;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = min(mn[k], (unsigned)__shfl_xor((int)mn[k], d));
            mx[k] = max(mx[k], (unsigned)__shfl_xor((int)mx[k], d));
        }
        cnt += (unsigned)__shfl_xor((int)cnt, d);
    }
    // the waves' results meet in LDS: one set of atomics per workgroup (every workgroup adds to the same seven words)
    __shared__ unsigned w_mn[TPB / 64][3], w_mx[TPB / 64][3], w_cnt[TPB / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { w_mn[wave][k] = mn[k]; w_mx[wave][k] = mx[k]; }
        w_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / 64; ++w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], w_mn[w][k]); mx[k] = max(mx[k], w_mx[w][k]); }
            cnt += w_cnt[w];
        }
        if (cnt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(&hdr->mn[k], mn[k]); atomicMax(&hdr->mx[k], mx[k]); }
            atomicAdd(&hdr->count, (unsigned long long)cnt);
        }
    }
}

__global__ void __launch_bounds__(TPB) k_map_insert(const uint4* __restrict__ pts, size_t n, MapGrid G,
                                                    MapCell* __restrict__ table, unsigned mask,
                                                    unsigned* __restrict__ bitmap, unsigned* __restrict__ list,
                                                    unsigned list_cap, MapHdr* hdr) {
    __shared__ unsigned l_key[LSLOTS], l_cnt[LSLOTS], l_idx[LSLOTS], l_c[3][LSLOTS];
    __shared__ unsigned long long l_s[3][LSLOTS];
    __shared__ unsigned l_claim[TILE], l_nclaim, l_base;   // cells this tile claimed; their range in the list
    const size_t ntiles = (n + TILE - 1) / TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int s = threadIdx.x; s < LSLOTS; s += TPB) {
            l_key[s] = 0; l_cnt[s] = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { l_c[k][s] = 0; l_s[k][s] = 0; }
        }
        if (threadIdx.x == 0) l_nclaim = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TILE / TPB; ++j) {
            const size_t i = tile * TILE + (size_t)j * TPB + threadIdx.x;
            if (i >= n) continue;
            const uint4 p = pts[i];
            if (!(finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z))) continue;
            const float x = __uint_as_float(p.x), y = __uint_as_float(p.y), z = __uint_as_float(p.z);
            const unsigned vi = (unsigned)((int)floorf(x * G.inv) - G.minb[0]);
            const unsigned vj = (unsigned)((int)floorf(y * G.inv) - G.minb[1]);
            const unsigned vk = (unsigned)((int)floorf(z * G.inv) - G.minb[2]);
            const unsigned k1 = vi + vj * G.dx + vk * G.dx * G.dy + 1u;
            unsigned h = mix32(k1) & (LSLOTS - 1);
            for (;;) {   // at most TILE of the LSLOTS slots are ever taken: a free or equal slot is always met
                const unsigned old = atomicCAS(&l_key[h], 0u, k1);
                if (old == 0u) l_idx[h] = (unsigned)i;
                if (old == 0u || old == k1) break;
                h = (h + 1) & (LSLOTS - 1);
            }
            atomicAdd(&l_cnt[h], 1u);
            atomicAdd(&l_s[0][h], (unsigned long long)__double2ll_rn((double)x * 16777216.0));
            atomicAdd(&l_s[1][h], (unsigned long long)__double2ll_rn((double)y * 16777216.0));
            atomicAdd(&l_s[2][h], (unsigned long long)__double2ll_rn((double)z * 16777216.0));
            atomicAdd(&l_c[0][h], (p.w >> 16) & 255u);
            atomicAdd(&l_c[1][h], (p.w >> 8) & 255u);
            atomicAdd(&l_c[2][h], p.w & 255u);
        }
        __syncthreads();
        for (int s = threadIdx.x; s < LSLOTS; s += TPB) {
            const unsigned k1 = l_key[s];
            if (!k1) continue;
            unsigned h = mix32(k1) & mask;
            bool done = false;
            for (unsigned probe = 0; probe <= mask && !done; ++probe) {
                const unsigned old = atomicCAS(&table[h].key1, 0u, k1);
                if (old == 0u) {
                    table[h].idx = l_idx[s];
                    const unsigned key = k1 - 1u;
                    atomicOr(&bitmap[key >> 5], 1u << (key & 31u));
                    l_claim[atomicAdd(&l_nclaim, 1u) & (TILE - 1)] = h;   // at most TILE distinct voxels per tile
                }
                if (old == 0u || old == k1) {
                    atomicAdd(&table[h].cnt, l_cnt[s]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        atomicAdd(&table[h].s[k], l_s[k][s]);
                        atomicAdd(&table[h].c[k], (unsigned long long)l_c[k][s]);
                    }
                    done = true;
                } else {
                    h = (h + 1) & mask;
                }
            }
            if (!done) atomicOr(&hdr->err, 2u);
        }
        __syncthreads();
        const unsigned nclaim = min(l_nclaim, (unsigned)TILE);
        if (threadIdx.x == 0 && nclaim) l_base = atomicAdd(&hdr->m, nclaim);
        __syncthreads();
        for (unsigned c = threadIdx.x; c < nclaim; c += TPB) {
            const unsigned slot = l_base + c;
            if (slot < list_cap) list[slot] = l_claim[c];
            else atomicOr(&hdr->err, 1u);
        }
        __syncthreads();
    }
}

// exclusive scan of one value per thread over the workgroup; *total: the workgroup's sum
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* wsum, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();   // wsum may still be read from the previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    *total = tot;
    return off + inc - v;
}

__global__ void __launch_bounds__(TPB) k_map_scan_reduce(const unsigned* __restrict__ bitmap, size_t nwords,
                                                         unsigned* __restrict__ bsum) {
    __shared__ unsigned wsum[TPB / 64];
    const size_t base = (size_t)blockIdx.x * R360_MAP_SCAN_BLOCK;
    unsigned v = 0;
    for (size_t j = threadIdx.x; j < R360_MAP_SCAN_BLOCK; j += TPB)
        if (base + j < nwords) v += __popc(bitmap[base + j]);
    unsigned total;
    block_excl_scan(v, wsum, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TPB) k_map_scan_top(unsigned* bsum, size_t nb) {
    __shared__ unsigned wsum[TPB / 64];
    unsigned carry = 0;
    for (size_t base = 0; base < nb; base += TPB) {
        const size_t i = base + threadIdx.x;
        const unsigned v = i < nb ? bsum[i] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(v, wsum, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(TPB) k_map_scan_apply(const unsigned* __restrict__ bitmap, size_t nwords,
                                                        const unsigned* __restrict__ bsum, unsigned* __restrict__ wprefix) {
    __shared__ unsigned wsum[TPB / 64];
    const size_t base = (size_t)blockIdx.x * R360_MAP_SCAN_BLOCK;
    unsigned carry = bsum[blockIdx.x];
    for (size_t j = 0; j < R360_MAP_SCAN_BLOCK; j += TPB) {
        const size_t w = base + j + threadIdx.x;
        const unsigned v = w < nwords ? __popc(bitmap[w]) : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(v, wsum, &total);
        if (w < nwords) wprefix[w] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(TPB) k_map_finalise(const uint4* __restrict__ pts, size_t n, MapCell* __restrict__ table,
                                                      unsigned mask, const unsigned* __restrict__ list, unsigned list_cap,
                                                      const unsigned* __restrict__ bitmap, size_t nwords,
                                                      const unsigned* __restrict__ wprefix, MapHdr* hdr,
                                                      uint4* __restrict__ out, size_t out_cap) {
    const unsigned m = min(hdr->m, list_cap);
    for (size_t t = (size_t)blockIdx.x * TPB + threadIdx.x; t < m; t += (size_t)gridDim.x * TPB) {
        const unsigned h = list[t] & mask;
        const MapCell c = table[h];
        uint4* cell = reinterpret_cast<uint4*>(&table[h]);
        const uint4 zero = make_uint4(0, 0, 0, 0);
        cell[0] = zero; cell[1] = zero; cell[2] = zero; cell[3] = zero;
        if (c.key1 == 0u || c.cnt == 0u) { atomicOr(&hdr->err, 4u); continue; }
        const unsigned key = c.key1 - 1u, w = key >> 5;
        if (w >= nwords) { atomicOr(&hdr->err, 8u); continue; }
        const size_t pos = (size_t)wprefix[w] + __popc(bitmap[w] & ((1u << (key & 31u)) - 1u));
        if (pos >= out_cap) { atomicOr(&hdr->err, 8u); continue; }
        uint4 o;
        if (c.cnt == 1u && c.idx < n) {   // the singleton rule: the point's own bits
            const uint4 p = pts[c.idx];
            o.x = p.x; o.y = p.y; o.z = p.z;
        } else {
            const double inv_n = (double)c.cnt;
            o.x = __float_as_uint((float)((double)(long long)c.s[0] * R360_VOXEL_QUANTUM / inv_n));
            o.y = __float_as_uint((float)((double)(long long)c.s[1] * R360_VOXEL_QUANTUM / inv_n));
            o.z = __float_as_uint((float)((double)(long long)c.s[2] * R360_VOXEL_QUANTUM / inv_n));
        }
        const unsigned long long cn = c.cnt;
        o.w = (unsigned)(c.c[0] / cn) << 16 | (unsigned)(c.c[1] / cn) << 8 | (unsigned)(c.c[2] / cn);
        out[pos] = o;
    }
}

__global__ void __launch_bounds__(TPB) k_map_unpack(const uint4* __restrict__ pts, size_t m, float* __restrict__ xyz,
                                                    uint32_t* __restrict__ rgba) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < m; i += (size_t)gridDim.x * TPB) {
        const uint4 p = pts[i];
        xyz[3 * i] = __uint_as_float(p.x); xyz[3 * i + 1] = __uint_as_float(p.y); xyz[3 * i + 2] = __uint_as_float(p.z);
        if (rgba) rgba[i] = p.w;
    }
}

inline int grid_for(size_t items, size_t per_block, int cap) {
    const size_t b = (items + per_block - 1) / per_block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

}  // namespace

int launch_map_pack_host(hipStream_t st, const float* xyz, const uint32_t* rgba, size_t n, uint4* out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_map_pack_host, dim3(grid_for(n, TPB, 4096)), dim3(TPB), 0, st, xyz, rgba, n, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_pack_frame(hipStream_t st, const float4* cloud, const uchar4* rgb, size_t per_sensor, const MapRig& rig,
                          const MapPose& pose, float x_min, float x_max, float box, uint4* out) {
    if (per_sensor == 0) return 0;
    hipLaunchKernelGGL(k_map_pack_frame, dim3(grid_for(8 * per_sensor, TPB, 4096)), dim3(TPB), 0, st, cloud, rgb, per_sensor,
                       rig, pose, x_min, x_max, box, out);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_bounds(hipStream_t st, const uint4* pts, size_t n, MapHdr* hdr) {
    hipLaunchKernelGGL(k_map_hdr_init, dim3(1), dim3(64), 0, st, hdr);
    R360_HIP(hipGetLastError());
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_map_bounds, dim3(grid_for(n, 8 * TPB, 2048)), dim3(TPB), 0, st, pts, n, hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_insert(hipStream_t st, const uint4* pts, size_t n, const MapGrid& G, MapCell* table, size_t table_cap,
                      unsigned* bitmap, unsigned* list, MapHdr* hdr) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_map_insert, dim3(grid_for(n, TILE, 4096)), dim3(TPB), 0, st, pts, n, G, table,
                       (unsigned)(table_cap - 1), bitmap, list, (unsigned)(table_cap / 2), hdr);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_scan(hipStream_t st, const unsigned* bitmap, size_t nwords, unsigned* bsum, unsigned* wprefix) {
    if (nwords == 0) return 0;
    const size_t nb = (nwords + R360_MAP_SCAN_BLOCK - 1) / R360_MAP_SCAN_BLOCK;
    hipLaunchKernelGGL(k_map_scan_reduce, dim3((unsigned)nb), dim3(TPB), 0, st, bitmap, nwords, bsum);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_map_scan_top, dim3(1), dim3(TPB), 0, st, bsum, nb);
    R360_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_map_scan_apply, dim3((unsigned)nb), dim3(TPB), 0, st, bitmap, nwords, bsum, wprefix);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_finalise(hipStream_t st, const uint4* pts, size_t n, MapCell* table, size_t table_cap,
                        const unsigned* list, const unsigned* bitmap, size_t nwords, const unsigned* wprefix, MapHdr* hdr,
                        uint4* out, size_t out_cap) {
    hipLaunchKernelGGL(k_map_finalise, dim3(grid_for(std::min(n, table_cap / 2), TPB, 4096)), dim3(TPB), 0, st, pts, n,
                       table, (unsigned)(table_cap - 1), list, (unsigned)(table_cap / 2), bitmap, nwords, wprefix, hdr, out, out_cap);
    R360_HIP(hipGetLastError());
    return 0;
}

int launch_map_unpack(hipStream_t st, const uint4* pts, size_t m, float* xyz, uint32_t* rgba) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_map_unpack, dim3(grid_for(m, TPB, 4096)), dim3(TPB), 0, st, pts, m, xyz, rgba);
    R360_HIP(hipGetLastError());
    return 0;
}
