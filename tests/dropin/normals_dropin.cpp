// Drop-in check of the normal estimation in the order a PCL user writes it, against the façade through
// include/rgbd360/compat.h: NormalEstimation ne; ne.setInputCloud(cloud); ne.setKSearch(k) or ne.setRadiusSearch(r);
// ne.setViewPoint(x, y, z); ne.compute(normals).  The cloud is a wall and a floor sampled on a grid, so the answers are
// known: the wall's normals are +-x, the floor's +-z, each turned towards the viewpoint.  The same estimation then runs
// on the map resident on the GPU (r360::GlobalMap360::estimateNormals), is compared with the cloud's, and goes through
// a PointXYZRGBNormal file.
//   usage: normals_dropin [file.pcd]
#include <rgbd360/compat.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace std;

int main(int argc, char** argv) {
    const string file = argc > 1 ? argv[1] : "/tmp/normals_dropin.pcd";

    r360::PointCloud cloud;             // a wall in x = 0 and a floor in z = 0, 6 cm spacing: at most one point per 5 cm voxel
    for (int i = 0; i < 40; ++i)
        for (int j = 1; j <= 40; ++j) {
            const float a = 0.06f * float(i) + 0.01f, b = 0.06f * float(j) + 0.01f;
            cloud.xyz.insert(cloud.xyz.end(), {0.f, a, b});          // wall
            cloud.rgba.push_back(0xff0000u);
            cloud.xyz.insert(cloud.xyz.end(), {b, a, 0.f});          // floor
            cloud.rgba.push_back(0x00ff00u);
        }
    cloud.width = int(cloud.rgba.size());
    cloud.height = 1;

    NormalEstimation ne;
    r360::PointCloudNormal normals, byRadius, both;
    ne.setInputCloud(cloud);
    ne.setKSearch(9);
    ne.setViewPoint(1.f, 1.f, 1.f);
    ne.compute(normals);
    cout << "k search 9: " << normals.size() << " normals, " << ne.stats().n_short << " short, "
         << double(ne.stats().sum_neighbors) / double(ne.stats().n_finite) << " neighbours on average\n";

    NormalEstimation ne2;
    ne2.setInputCloud(cloud);
    ne2.setRadiusSearch(0.1);
    ne2.setViewPoint(1.f, 1.f, 1.f);
    ne2.compute(byRadius);
    cout << "radius search 0.1: " << byRadius.size() << " normals, " << ne2.stats().n_short << " short\n";

    ne2.setKSearch(20);                 // both: at most 20 points within 0.1 m
    ne2.compute(both);

    // away from the edge where wall and floor meet every normal is its surface's, towards (1, 1, 1)
    bool ok = normals.size() == cloud.size() && byRadius.size() == cloud.size() && both.size() == cloud.size();
    size_t checked = 0;
    for (size_t p = 0; ok && p < cloud.size(); ++p) {
        const bool wall = cloud.rgba[p] == 0xff0000u;
        const float away = wall ? cloud.xyz[3 * p + 2] : cloud.xyz[3 * p];
        if (away < 0.3f) continue;
        for (const r360::PointCloudNormal* n : {&normals, &byRadius, &both}) {
            const float* v = &n->normals[3 * p];
            const float want[3] = {wall ? 1.f : 0.f, 0.f, wall ? 0.f : 1.f};
            for (int c = 0; c < 3; ++c) ok = ok && std::fabs(v[c] - want[c]) < 1e-5f;
            ok = ok && std::fabs(n->curvature[p]) < 1e-9f;
        }
        ++checked;
    }
    cout << "surface normals " << (ok ? "as expected" : "WRONG") << " on " << checked << " points\n";

    // the same on the device-resident map: the cloud has one point per voxel, so the map holds the same points
    r360::GlobalMap360 deviceMap;
    deviceMap.add(cloud);
    r360_normal_params params;
    r360_normal_default_params(&params);
    params.k = 9;
    params.radius = 0.5f;
    r360_normal_stats st;
    deviceMap.estimateNormals(params, vector<float>{1.f, 1.f, 1.f}, &st);
    r360::PointCloud mapCloud;
    r360::PointCloudNormal mapNormals;
    deviceMap.download(mapCloud);
    deviceMap.getNormals(mapNormals);
    NormalEstimation ne3;
    ne3.setInputCloud(mapCloud);
    ne3.setKSearch(9);
    ne3.setViewPoint(1.f, 1.f, 1.f);
    r360::PointCloudNormal again;
    ne3.compute(again);
    const bool same = mapNormals.size() == mapCloud.size() && st.n_in == mapCloud.size() && again.size() == mapNormals.size() &&
                      memcmp(again.normals.data(), mapNormals.normals.data(), sizeof(float) * again.normals.size()) == 0 &&
                      memcmp(again.curvature.data(), mapNormals.curvature.data(), sizeof(float) * again.curvature.size()) == 0;
    cout << "device map: " << mapCloud.size() << " points, normals " << (same ? "identical" : "DIFFER") << "\n";

    deviceMap.savePCDNormals(file, 1);
    vector<float> xyz(3 * mapCloud.size()), nrm(3 * mapCloud.size()), curv(mapCloud.size());
    vector<uint32_t> rgba(mapCloud.size());
    size_t n = 0;
    const int rc = r360_pcd_read_normals(file.c_str(), xyz.data(), rgba.data(), nrm.data(), curv.data(), mapCloud.size(), &n);
    const bool file_ok = rc == 0 && n == mapCloud.size() &&
                         memcmp(nrm.data(), mapNormals.normals.data(), sizeof(float) * nrm.size()) == 0 &&
                         memcmp(xyz.data(), mapCloud.xyz.data(), sizeof(float) * xyz.size()) == 0;
    cout << "file " << file << ": " << n << " points " << (file_ok ? "read back" : "DIFFER") << "\n";
    std::remove(file.c_str());

    // a changed map has no normals any more
    deviceMap.add(cloud);
    bool threw = false;
    try {
        deviceMap.getNormals(mapNormals);
    } catch (const std::exception&) {
        threw = true;
    }
    cout << "normals after the map changed: " << (threw ? "refused" : "STILL THERE") << "\n";
    return ok && same && file_ok && threw ? 0 : 3;
}
