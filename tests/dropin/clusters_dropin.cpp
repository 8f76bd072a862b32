// Drop-in check of the Euclidean cluster extraction in the order a PCL user writes it, against the façade through
// include/rgbd360/compat.h: EuclideanClusterExtraction ec; ec.setClusterTolerance(t); ec.setMinClusterSize(a);
// ec.setMaxClusterSize(b); ec.setInputCloud(cloud); ec.extract(cluster_indices).  The cloud is a wall and a floor that
// meet along an edge, a detached blob and a few stray points, so the answers are known: one large cluster and the blob,
// the strays rejected; with the normals (the extension setInputNormals / setEpsAngle) the wall and the floor part.  The
// same extraction then runs on the map resident on the GPU (r360::GlobalMap360::cluster), is compared with the cloud's,
// goes through a PointXYZRGBL file, and removeSmallClusters drops what belongs to no cluster.
//   usage: clusters_dropin [file.pcd]
#include <rgbd360/compat.h>

#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace std;

int main(int argc, char** argv) {
    const string file = argc > 1 ? argv[1] : "/tmp/clusters_dropin.pcd";

    r360::PointCloud cloud;             // 6 cm spacing: at most one point per 5 cm voxel
    r360::PointCloudNormal normals;
    auto add = [&](float x, float y, float z, float nx, float ny, float nz, uint32_t colour) {
        cloud.xyz.insert(cloud.xyz.end(), {x, y, z});
        cloud.rgba.push_back(colour);
        normals.normals.insert(normals.normals.end(), {nx, ny, nz});
        normals.curvature.push_back(0.f);
    };
    for (int i = 0; i < 30; ++i)
        for (int j = 1; j <= 30; ++j) {
            const float a = 0.06f * float(i) + 0.01f, b = 0.06f * float(j) + 0.01f;
            add(0.f, a, b, 1.f, 0.f, 0.f, 0xff0000u);     // wall in x = 0
            add(b, a, 0.f, 0.f, 0.f, 1.f, 0x00ff00u);     // floor in z = 0
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j)
            for (int k = 0; k < 4; ++k)                   // a detached blob of 144 points, 1 m above the floor
                add(1.f + 0.06f * float(i), 1.f + 0.06f * float(j), 1.f + 0.06f * float(k), 0.f, 1.f, 0.f, 0x0000ffu);
    for (int s = 0; s < 5; ++s) add(3.f + float(s), -2.f, 2.f, 0.f, 0.f, 1.f, 0xffffffu);   // strays, 1 m apart
    cloud.width = int(cloud.rgba.size());
    cloud.height = 1;

    vector<PointIndices> cluster_indices;
    EuclideanClusterExtraction ec;
    ec.setClusterTolerance(0.1);
    ec.setMinClusterSize(100);
    ec.setMaxClusterSize(25000);
    ec.setInputCloud(cloud);
    ec.extract(cluster_indices);
    cout << "plain: " << cluster_indices.size() << " clusters of " << ec.stats().n_components << " components";
    for (const PointIndices& c : cluster_indices) cout << " " << c.indices.size();
    cout << "\n";
    bool ok = cluster_indices.size() == 2 && cluster_indices[0].indices.size() == 1800 &&
              cluster_indices[1].indices.size() == 144 && ec.stats().n_components == 7 && ec.stats().n_clustered == 1944;
    // members ascend, and the records describe them
    for (const PointIndices& c : cluster_indices)
        for (size_t k = 1; k < c.indices.size(); ++k) ok = ok && c.indices[k - 1] < c.indices[k];
    const vector<r360_cluster_info>& info = ec.getClusterInfo();
    ok = ok && info.size() == 2 && info[0].size == 1800 && info[0].root == 0 && info[1].size == 144 &&
         info[1].min[0] == 1.f && info[1].max[2] == 1.f + 0.06f * 3.f;
    cout << "records " << (ok ? "as expected" : "WRONG") << "\n";

    ec.setInputNormals(normals);        // extension: pcl::extractEuclideanClusters(cloud, normals, ...)
    ec.setEpsAngle(0.2);
    vector<PointIndices> smooth;
    ec.extract(smooth);
    cout << "with normals: " << smooth.size() << " clusters";
    for (const PointIndices& c : smooth) cout << " " << c.indices.size();
    cout << "\n";
    const bool parted = smooth.size() == 3 && smooth[0].indices.size() == 900 && smooth[1].indices.size() == 900 &&
                        smooth[2].indices.size() == 144 && smooth[0].indices[0] == 0 && smooth[1].indices[0] == 1;

    // the same on the device-resident map: the cloud has one point per voxel, so the map holds the same points
    r360::GlobalMap360 deviceMap;
    deviceMap.add(cloud);
    r360_cluster_params params;
    r360_cluster_default_params(&params);
    params.max_size = 25000;
    r360_cluster_stats st;
    deviceMap.cluster(params, false, &st);
    r360::PointCloud mapCloud;
    vector<int> mapLabels;
    vector<r360_cluster_info> mapClusters;
    deviceMap.download(mapCloud);
    deviceMap.getLabels(mapLabels);
    deviceMap.getClusters(mapClusters);
    EuclideanClusterExtraction ec2;
    ec2.setClusterTolerance(params.tolerance);
    ec2.setMinClusterSize(params.min_size);
    ec2.setMaxClusterSize(params.max_size);
    ec2.setInputCloud(mapCloud);
    vector<PointIndices> again;
    ec2.extract(again);
    const bool same = mapLabels.size() == mapCloud.size() && st.n_in == mapCloud.size() && st.n_clusters == 2 &&
                      mapLabels == ec2.getLabels() && mapClusters.size() == ec2.getClusterInfo().size() &&
                      memcmp(mapClusters.data(), ec2.getClusterInfo().data(), sizeof(r360_cluster_info) * mapClusters.size()) == 0;
    cout << "device map: " << mapCloud.size() << " points, " << st.n_clusters << " clusters, labels and records "
         << (same ? "identical" : "DIFFER") << "\n";

    deviceMap.savePCDLabels(file, 1);
    vector<float> xyz(3 * mapCloud.size());
    vector<uint32_t> rgba(mapCloud.size());
    vector<int> labels(mapCloud.size());
    size_t n = 0;
    const int rc = r360_pcd_read_labels(file.c_str(), xyz.data(), rgba.data(), labels.data(), mapCloud.size(), &n);
    const bool file_ok = rc == 0 && n == mapCloud.size() && labels == mapLabels &&
                         memcmp(xyz.data(), mapCloud.xyz.data(), sizeof(float) * xyz.size()) == 0;
    cout << "file " << file << ": " << n << " points " << (file_ok ? "read back" : "DIFFER") << "\n";
    std::remove(file.c_str());

    // what belongs to no cluster goes; the map then has no labels any more
    deviceMap.removeSmallClusters(params, false, &st);
    const bool removed = deviceMap.size() == 1944 && st.n_clustered == 1944;
    bool threw = false;
    try {
        deviceMap.getLabels(mapLabels);
    } catch (const std::exception&) {
        threw = true;
    }
    cout << "small clusters removed: " << deviceMap.size() << " points left, labels " << (threw ? "refused" : "STILL THERE") << "\n";
    return ok && parted && same && file_ok && removed && threw ? 0 : 3;
}
