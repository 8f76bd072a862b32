// Drop-in check of the Generalized-ICP call sequence of a RegisterPairRGBD360-style driver
// (Registration/RegisterPairRGBD360.cpp:109-149), written against the façade through include/rgbd360/compat.h: the
// four setters with the driver's values, a FilterPointCloud of leaf 0.1 on both sphere clouds, the second frame as
// source and the first as target, an identity guess, then the final transformation beside the PbMap pose.
//   usage: gicp_dropin [frame1.bin frame2.bin]      (default: the shipped sample pair)
#include <rgbd360/compat.h>

#include <cmath>
#include <iostream>
#include <string>

using namespace std;

int main(int argc, char** argv) {
    const string root = PROJECT_SOURCE_PATH;
    const string file1 = argc > 2 ? argv[1] : root + "/samples/sphere_images_1.bin";
    const string file2 = argc > 2 ? argv[2] : root + "/samples/sphere_images_10.bin";
    if (!fexists(file1.c_str()) || !fexists(file2.c_str())) {
        cerr << "missing " << file1 << " or " << file2 << "\n";
        return 1;
    }

    Calib360 calib;
    calib.loadExtrinsicCalibration();
    calib.loadIntrinsicCalibration();

    Frame360 frame360_1(&calib), frame360_2(&calib);
    frame360_1.loadFrame(file1);
    frame360_1.undistort();
    frame360_1.buildSphereCloud();
    frame360_1.getPlanes();
    frame360_2.loadFrame(file2);
    frame360_2.undistort();
    frame360_2.buildSphereCloud();
    frame360_2.getPlanes();

    RegisterRGBD360 registerer(mrpt::format("%s/config_files/configLocaliser_sphericalOdometry.ini", PROJECT_SOURCE_PATH));
    registerer.RegisterPbMap(&frame360_1, &frame360_2, 25, RegisterRGBD360::PLANAR_3DoF);

    GeneralizedIterativeClosestPoint icp;
    icp.setMaxCorrespondenceDistance(0.4);
    icp.setMaximumIterations(10);
    icp.setTransformationEpsilon(1e-9);
    icp.setRANSACOutlierRejectionThreshold(0.1);

    r360::PointCloud cloud1, cloud2;
    frame360_1.sphereCloud(cloud1);
    frame360_2.sphereCloud(cloud2);
    FilterPointCloud filter(0.1);
    filter.filterVoxel(cloud1);
    filter.filterVoxel(cloud2);

    icp.setInputSource(cloud2);
    icp.setInputTarget(cloud1);
    r360::PointCloud alignedICP;
    Eigen::Matrix4f initRigidTransf = Eigen::Matrix4f::Identity();
    icp.align(alignedICP, initRigidTransf);

    cout << "clouds " << cloud2.size() << " -> " << cloud1.size() << " points, aligned " << alignedICP.size() << "\n";
    cout << "has converged:" << icp.hasConverged() << " score: " << icp.getFitnessScore() << "\n";
    Eigen::Matrix4f icpTransformation = icp.getFinalTransformation();
    cout << "ICP transformation:\n" << icpTransformation << endl << "PbMap-Registration\n" << registerer.getPose() << endl;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(icpTransformation(r, c))) return 3;
    return alignedICP.size() == cloud2.size() ? 0 : 3;
}
