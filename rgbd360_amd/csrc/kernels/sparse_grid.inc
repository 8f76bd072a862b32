// sparse_grid.inc — the device side of the sparse cell grid that k_out_cells / k_out_scan_* / k_out_scatter build
// (kernels/outlier_kernels.hip, DESIGN.md §5b-2): the cell keys, the lookup of an occupied cell and the lower bound of
// the distance to a neighbouring cell.  Included inside the anonymous namespace of the kernel files that walk the grid
// (outlier_kernels.hip, normal_kernels.hip).
constexpr unsigned NOSLOT = 0xffffffffu;
constexpr unsigned long long OCCUPIED = 1ull << 63;

__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ unsigned long long mix64(unsigned long long h) {   // murmur3's 64-bit finaliser
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}
// a cell's coordinates (each in [0, 2^21)) as a non-zero key
__device__ __forceinline__ unsigned long long cell_key(long long cx, long long cy, long long cz) {
    return OCCUPIED | (unsigned long long)cz << 42 | (unsigned long long)cy << 21 | (unsigned long long)cx;
}
__device__ __forceinline__ bool cell_in_range(long long c) { return c >= 0 && c < (1ll << 21); }

// the occupied cell with this key: its slot, or NOSLOT
__device__ __forceinline__ unsigned find_cell(const unsigned long long* __restrict__ keys, unsigned mask, unsigned long long key) {
    unsigned h = (unsigned)mix64(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long k = keys[h];
        if (k == key) return h;
        if (k == 0ull) return NOSLOT;
        h = (h + 1) & mask;
    }
    return NOSLOT;
}

// lower bound, in cell edges, of the distance along one axis from a point at fraction u of its cell to the cell o
// cells away; the 1e-6 of slack is far above what the rounding of x / ec can move a point across a cell face
__device__ __forceinline__ double axis_gap(int o, double u) {
    const double g = o < 0 ? u + (double)(-o - 1) : (o > 0 ? (double)(o - 1) + (1.0 - u) : 0.0);
    return fmax(g - 1.0e-6, 0.0);
}
