// Drop-in check of the host part of the map step of a SphereGraphSLAM-style driver (SLAM/SphereGraphSLAM.cpp:95-137,
// :193-209), written against the façade through include/rgbd360/compat.h: a FilterPointCloud with the reference's
// constructor defaults, filterEuclidean on each keyframe's sphere cloud, transformPointCloud by the keyframe's
// pose, globalMap += the result.  (The voxel-grid step, filterVoxel, has no counterpart in the library yet.)
//   usage: global_map_dropin <dir with sphere_images_<n>.bin> <first frame> <n frames> [out.pcd]
#include <rgbd360/compat.h>

#include <cstdlib>
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

        // download, box filter in the rig frame, pose, append
        r360::PointCloud sphereCloud, posedCloud;
        keyframe.sphereCloud(sphereCloud);
        filter.filterEuclidean(sphereCloud);
        r360::transformPointCloud(sphereCloud, posedCloud, currentPose);
        globalMap += posedCloud;

        cout << "keyframe " << n << ": " << sphereCloud.size() << " points in the box, map " << globalMap.size()
             << " points\n";
        currentPose(1, 3) += 0.25f;     // a stand-in for the tracked motion
    }
    if (argc > 4 && !globalMap.empty())
        r360::check(r360_pcd_write(argv[4], globalMap.xyz.data(), globalMap.rgba.data(), globalMap.width, globalMap.height, 1),
                    "r360_pcd_write");
    return 0;
}
