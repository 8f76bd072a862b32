// cloud_filter.cpp — FilterPointCloud::filterEuclidean (include/FilterPointCloud.h: three pcl::PassThrough filters;
// SLAM/SphereGraphSLAM.cpp:116, :193) on the host, restated from PCL 1.7 (unpinned: PCL is not available here).
#include <cmath>

#include "../r360_internal.h"

// Keeps, in order, the points with finite x, y, z inside the closed box [x_min, x_max] x [-box, box]^2 (float
// compares).  out_* may be the inputs (filtering in place): a point is read before its slot can be written.
extern "C" int r360_cloud_filter_euclidean(const float* xyz, const uint32_t* rgba, size_t n, float x_min, float x_max,
                                           float box, float* out_xyz, uint32_t* out_rgba, size_t* n_out) {
    CHECK_ARG((n == 0 || (xyz && out_xyz)) && n_out, "null arg");
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
        if (!(x >= x_min && x <= x_max && y >= -box && y <= box && z >= -box && z <= box)) continue;
        const uint32_t c = rgba ? rgba[i] : 0u;
        out_xyz[3 * k] = x; out_xyz[3 * k + 1] = y; out_xyz[3 * k + 2] = z;
        if (rgba && out_rgba) out_rgba[k] = c;
        ++k;
    }
    *n_out = k;
    return 0;
}
