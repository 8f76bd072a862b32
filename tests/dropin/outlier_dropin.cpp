// Drop-in check of the outlier filters in the order a PCL user writes them after a voxel grid, against the façade through
// include/rgbd360/compat.h: filter.filterVoxel(cloud), then filter.filterStatistical(cloud) (pcl::StatisticalOutlierRemoval
// with setMeanK / setStddevMulThresh) and filter.filterRadius(cloud) (pcl::RadiusOutlierRemoval with setRadiusSearch /
// setMinNeighborsInRadius), each with its default arguments and with explicit ones.  The same radius filter then runs on
// the map resident on the GPU (r360::GlobalMap360::removeOutliers), and the two results are compared.
//   usage: outlier_dropin <dir with sphere_images_<n>.bin> <first frame> <n frames>
#include <rgbd360/compat.h>

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace std;

int main(int argc, char** argv) {
    if (argc < 4) {
        cerr << "usage: " << argv[0] << " <dir> <first frame> <n frames>\n";
        return 1;
    }
    const string dir = argv[1];
    const int first = atoi(argv[2]), count = atoi(argv[3]);

    Calib360 calib;
    calib.loadExtrinsicCalibration();
    calib.loadIntrinsicCalibration();

    FilterPointCloud filter;            // voxelSize 0.05, euclideanBox 4.0
    r360::PointCloud globalMap;
    r360::GlobalMap360 deviceMap;       // the default context's map, same voxel size and box

    vector<unique_ptr<Frame360> > keyframes;
    Eigen::Matrix4f currentPose = Eigen::Matrix4f::Identity();
    for (int n = first; n < first + count; ++n) {
        const string file = mrpt::format("%s/sphere_images_%d.bin", dir.c_str(), n);
        if (!fexists(file.c_str())) break;
        keyframes.emplace_back(new Frame360(&calib));
        Frame360& keyframe = *keyframes.back();
        keyframe.loadFrame(file);
        keyframe.undistort();
        keyframe.buildSphereCloud();

        r360::PointCloud sphereCloud, posedCloud;
        keyframe.sphereCloud(sphereCloud);
        filter.filterEuclidean(sphereCloud);
        r360::transformPointCloud(sphereCloud, posedCloud, currentPose);
        globalMap += posedCloud;
        filter.filterVoxel(globalMap);
        deviceMap.add(keyframe, currentPose);
        currentPose(1, 3) += 0.25f;     // a stand-in for the tracked motion
    }
    cout << "map " << globalMap.size() << " points, device map " << deviceMap.size() << " points\n";

    // voxel grid, then the statistical filter: the defaults, then explicit arguments with the statistics
    r360::PointCloud sor = globalMap;
    filter.filterStatistical(sor);
    cout << "statistical (20, 1, 0.5): " << globalMap.size() << " -> " << sor.size() << " points\n";
    r360::PointCloud sor2 = globalMap;
    r360_outlier_stats st;
    filter.filterStatistical(sor2, 8, 2.f, 0.5f, &st);
    cout << "statistical (8, 2, 0.5): " << st.n_in << " -> " << sor2.size() << " points, " << st.n_short << " short, mean "
         << st.mean << " stddev " << st.stddev << " threshold " << st.threshold << "\n";

    // voxel grid, then the radius filter
    r360::PointCloud rad = globalMap;
    filter.filterRadius(rad);
    cout << "radius (0.15, 5): " << globalMap.size() << " -> " << rad.size() << " points\n";
    r360::PointCloud rad2 = globalMap;
    filter.filterRadius(rad2, 0.3f, 1);
    cout << "radius (0.3, 1): " << globalMap.size() << " -> " << rad2.size() << " points\n";

    // the same radius filter on the map where it lies
    r360_outlier_params params;
    r360_outlier_default_params(&params);
    params.kind = R360_OUTLIER_RADIUS;
    deviceMap.removeOutliers(params, &st);
    r360::PointCloud fromDevice;
    deviceMap.download(fromDevice);
    cout << "device map cleaned: " << st.n_in << " -> " << fromDevice.size() << " points\n";
    const bool ordered = sor.size() <= globalMap.size() && sor2.size() <= globalMap.size() && rad.size() <= rad2.size() &&
                         rad2.size() <= globalMap.size() && st.n_removed == st.n_in - fromDevice.size();
    const bool same = fromDevice.size() == rad.size() &&
                      (rad.empty() || (memcmp(fromDevice.xyz.data(), rad.xyz.data(), sizeof(float) * rad.xyz.size()) == 0 &&
                                       memcmp(fromDevice.rgba.data(), rad.rgba.data(), sizeof(uint32_t) * rad.rgba.size()) == 0));
    cout << "maps " << (same && ordered ? "identical" : "DIFFER") << "\n";
    return same && ordered ? 0 : 3;
}
