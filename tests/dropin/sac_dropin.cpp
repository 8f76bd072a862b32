// Drop-in check of the RANSAC plane segmentation in the order a PCL user writes it, against the façade through
// include/rgbd360/compat.h: PCL's planar-segmentation sequence (ModelCoefficients coefficients; PointIndices inliers;
// SACSegmentation seg; seg.setOptimizeCoefficients(true); seg.setModelType(SACMODEL_PLANE);
// seg.setMethodType(SAC_RANSAC); seg.setDistanceThreshold(t); seg.setInputCloud(cloud); seg.segment(inliers,
// coefficients)), then the constrained models, then PCL's cluster-extraction recipe on the map resident on the GPU:
// planes off (r360::GlobalMap360::segmentPlanes / removePlanes), clusters on the rest.  The cloud is a floor of 1200
// points and a wall of 900 that meet along an edge, a detached blob of 144 and five strays, so the answers are known.
//   usage: sac_dropin [file.pcd]
#include <rgbd360/compat.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace std;

static bool near4(const ModelCoefficients& c, float a, float b, float cc, float d) {
    return c.values.size() == 4 && fabs(c.values[0] - a) < 1e-5f && fabs(c.values[1] - b) < 1e-5f &&
           fabs(c.values[2] - cc) < 1e-5f && fabs(c.values[3] - d) < 1e-5f;
}

int main(int argc, char** argv) {
    const string file = argc > 1 ? argv[1] : "/tmp/sac_dropin.pcd";

    r360::PointCloud cloud;             // 6 cm spacing: at most one point per 5 cm voxel
    auto add = [&](float x, float y, float z, uint32_t colour) {
        cloud.xyz.insert(cloud.xyz.end(), {x, y, z});
        cloud.rgba.push_back(colour);
    };
    for (int i = 0; i < 30; ++i)
        for (int j = 1; j <= 40; ++j) {
            const float a = 0.06f * float(i) + 0.01f, b = 0.06f * float(j) + 0.01f;
            if (j <= 30) add(0.f, a, b, 0xff0000u);       // wall in x = 0: 900 points
            add(b, a, 0.f, 0x00ff00u);                    // floor in z = 0: 1200 points
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j)
            for (int k = 0; k < 4; ++k)                   // a detached blob of 144 points, 1 m above the floor
                add(1.f + 0.06f * float(i), 1.f + 0.06f * float(j), 1.f + 0.06f * float(k), 0x0000ffu);
    for (int s = 0; s < 5; ++s) add(3.f + float(s), -2.f, 2.f, 0xffffffu);   // strays, 1 m apart
    cloud.width = int(cloud.rgba.size());
    cloud.height = 1;

    ModelCoefficients coefficients;
    PointIndices inliers;
    SACSegmentation seg;
    seg.setOptimizeCoefficients(true);
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.01);
    seg.setInputCloud(cloud);
    seg.segment(inliers, coefficients);
    cout << "plane: " << inliers.indices.size() << " inliers after " << seg.getPlaneInfo().evaluated << " hypotheses\n";
    bool ok = inliers.indices.size() == 1200 && near4(coefficients, 0.f, 0.f, 1.f, 0.f);
    for (size_t k = 1; k < inliers.indices.size(); ++k) ok = ok && inliers.indices[k - 1] < inliers.indices[k];
    for (int i : inliers.indices) ok = ok && cloud.xyz[3 * size_t(i) + 2] == 0.f;
    cout << "coefficients " << (ok ? "as expected" : "WRONG") << "\n";

    seg.setModelType(SACMODEL_PERPENDICULAR_PLANE);     // the plane whose normal is the axis: the wall
    seg.setAxis(1.f, 0.f, 0.f);
    seg.setEpsAngle(0.1);
    seg.segment(inliers, coefficients);
    cout << "perpendicular to x: " << inliers.indices.size() << " inliers\n";
    const bool perp = inliers.indices.size() == 900 && near4(coefficients, 1.f, 0.f, 0.f, 0.f);
    seg.setModelType(SACMODEL_PARALLEL_PLANE);          // a plane parallel to the axis: the floor again
    seg.segment(inliers, coefficients);
    cout << "parallel to x: " << inliers.indices.size() << " inliers\n";
    const bool par = inliers.indices.size() == 1200;
    bool threw = false;
    try {
        seg.setModelType(5);                            // a sphere in PCL
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    cout << "other models " << (threw ? "refused" : "ACCEPTED") << "\n";

    // the recipe on the device-resident map: the cloud has one point per voxel, so the map holds the same points
    r360::GlobalMap360 deviceMap;
    deviceMap.add(cloud);
    r360_sac_params params;
    r360_sac_default_params(&params);
    params.distance_threshold = 0.01f;
    r360_sac_stats st;
    deviceMap.segmentPlanes(params, false, &st);
    vector<r360_sac_plane> planes;
    vector<int> planeLabels;
    deviceMap.getPlanes(planes);
    deviceMap.getPlaneLabels(planeLabels);
    cout << "device map: " << st.n_in << " points, " << st.n_planes << " planes";
    for (const r360_sac_plane& p : planes) cout << " " << p.size;
    cout << "\n";
    const bool mapped = st.n_planes == 2 && planes.size() == 2 && planes[0].size == 1200 && planes[1].size == 900 &&
                        st.n_in_planes == 2100 && planeLabels.size() == cloud.size();

    deviceMap.savePCDPlaneLabels(file, 1);
    r360::PointCloud mapCloud;
    deviceMap.download(mapCloud);
    vector<float> xyz(3 * mapCloud.size());
    vector<uint32_t> rgba(mapCloud.size());
    vector<int> labels(mapCloud.size());
    size_t n = 0;
    const int rc = r360_pcd_read_labels(file.c_str(), xyz.data(), rgba.data(), labels.data(), mapCloud.size(), &n);
    const bool file_ok = rc == 0 && n == mapCloud.size() && labels == planeLabels;
    cout << "file " << file << ": " << n << " points " << (file_ok ? "read back" : "DIFFER") << "\n";
    std::remove(file.c_str());

    deviceMap.removePlanes(params, false, &st);
    bool refused = false;
    try {
        deviceMap.getPlaneLabels(planeLabels);
    } catch (const std::exception&) {
        refused = true;
    }
    cout << "planes removed: " << deviceMap.size() << " points left, plane labels " << (refused ? "refused" : "STILL THERE")
         << "\n";
    r360_cluster_params cparams;
    r360_cluster_default_params(&cparams);
    r360_cluster_stats cst;
    deviceMap.cluster(cparams, false, &cst);
    cout << "clusters on the rest: " << cst.n_clusters << " of " << cst.n_clustered << " points\n";
    const bool recipe = deviceMap.size() == 149 && refused && cst.n_clusters == 1 && cst.n_clustered == 144;
    return ok && perp && par && threw && mapped && file_ok && recipe ? 0 : 3;
}
