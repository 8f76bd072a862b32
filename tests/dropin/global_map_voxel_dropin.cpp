// Drop-in check of the whole map step of a SphereGraphSLAM-style driver (SLAM/SphereGraphSLAM.cpp:95-137, :193-209),
// written against the façade through include/rgbd360/compat.h: a FilterPointCloud with the reference's constructor
// defaults, filterEuclidean on each keyframe's sphere cloud, transformPointCloud by the keyframe's pose,
// globalMap += the result, filter.filterVoxel(globalMap).  The same step with the map resident on the GPU
// (r360::GlobalMap360) runs beside it, and the two maps are compared at the end.
//   usage: global_map_voxel_dropin <dir with sphere_images_<n>.bin> <first frame> <n frames> [out.pcd]
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
        cerr << "usage: " << argv[0] << " <dir> <first frame> <n frames> [out.pcd]\n";
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

        // the reference's sequence on the host cloud
        r360::PointCloud sphereCloud, posedCloud;
        keyframe.sphereCloud(sphereCloud);
        filter.filterEuclidean(sphereCloud);
        r360::transformPointCloud(sphereCloud, posedCloud, currentPose);
        globalMap += posedCloud;
        filter.filterVoxel(globalMap);

        // the same step without leaving the GPU
        deviceMap.add(keyframe, currentPose);

        cout << "keyframe " << n << ": " << sphereCloud.size() << " points in the box, map " << globalMap.size()
             << " points, device map " << deviceMap.size() << " points\n";
        currentPose(1, 3) += 0.25f;     // a stand-in for the tracked motion
    }
    r360::PointCloud fromDevice;
    deviceMap.download(fromDevice);
    const bool same = fromDevice.size() == globalMap.size() &&
                      (globalMap.empty() ||
                       (memcmp(fromDevice.xyz.data(), globalMap.xyz.data(), sizeof(float) * globalMap.xyz.size()) == 0 &&
                        memcmp(fromDevice.rgba.data(), globalMap.rgba.data(), sizeof(uint32_t) * globalMap.rgba.size()) == 0));
    cout << "maps " << (same ? "identical" : "DIFFER") << "\n";
    if (argc > 4 && !globalMap.empty())
        r360::check(r360_pcd_write(argv[4], globalMap.xyz.data(), globalMap.rgba.data(), globalMap.width, globalMap.height, 1),
                    "r360_pcd_write");
    return same ? 0 : 3;
}
