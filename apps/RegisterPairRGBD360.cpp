// RegisterPairRGBD360 — the reference's Registration/RegisterPairRGBD360.cpp:60-149 over the MI355X
// library: load two Frame360 archives, undistort, build the sphere cloud and the PbMap, register the
// PbMaps (25 planes, PLANAR_3DoF) and print the matched planes and the pose; then the Generalized-ICP
// alignment of the two voxel-filtered sphere clouds (:109-149: leaf 0.1, source = frame 2, target =
// frame 1, identity guess) and its transformation beside the PbMap pose.  The PCL viewers of the
// reference are not reproduced.
//   usage: RegisterPairRGBD360 <frame1.bin> <frame2.bin> [calib_dir]
#include <rgbd360/rgbd360.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <frame1.bin> <frame2.bin> [calib_dir]\n", argv[0]);
        return 1;
    }
    const std::string calib_dir = argc > 3 ? argv[3] : std::string(RGBD360_DATA_DIR) + "/calib";
    try {
        r360::Context ctx(0);
        r360::Calib360 calib(ctx);                                   // QVGA sensors (Calib360.h:73-77)
        calib.loadExtrinsicCalibration(calib_dir + "/Extrinsics");
        calib.loadIntrinsicCalibration(calib_dir + "/Intrinsics");
        std::printf("Create sphere 1\n");
        r360::Frame360 frame360_1(&calib);
        frame360_1.loadFrame(argv[1]);
        frame360_1.undistort();
        frame360_1.buildSphereCloud();
        frame360_1.getPlanes();
        std::printf("Create sphere 2\n");
        r360::Frame360 frame360_2(&calib);
        frame360_2.loadFrame(argv[2]);
        frame360_2.undistort();
        frame360_2.buildSphereCloud();
        frame360_2.getPlanes();
        r360::RegisterRGBD360 registerer(ctx, std::string(RGBD360_DATA_DIR) + "/config_files/configLocaliser_sphericalOdometry.ini");
        const bool good = registerer.RegisterPbMap(&frame360_1, &frame360_2, 25, r360::RegisterRGBD360::PLANAR_3DoF);
        std::printf("planes %zu / %zu, registration %s\n", frame360_1.planes.size(), frame360_2.planes.size(),
                    good ? "good" : "insufficient");
        for (const auto& kv : registerer.getMatchedPlanes()) std::printf("%u %u\n", kv.first, kv.second);
        const r360::Matrix4f P = registerer.getPose();
        std::printf("Distance %g\nPose\n", std::sqrt(P(0, 3) * P(0, 3) + P(1, 3) * P(1, 3) + P(2, 3) * P(2, 3)));
        for (int r = 0; r < 4; ++r) std::printf("%10.6f %10.6f %10.6f %10.6f\n", P(r, 0), P(r, 1), P(r, 2), P(r, 3));

        // ICP alignment (:109-149)
        const auto t0 = std::chrono::steady_clock::now();
        r360::GeneralizedIterativeClosestPoint icp(ctx);
        icp.setMaxCorrespondenceDistance(0.4);
        icp.setMaximumIterations(10);
        icp.setTransformationEpsilon(1e-9);
        icp.setRANSACOutlierRejectionThreshold(0.1);
        // filter the point clouds and remove the NaN points
        r360::PointCloud cloud_1, cloud_2, alignedICP;
        frame360_1.sphereCloud(cloud_1);
        frame360_2.sphereCloud(cloud_2);
        r360::FilterPointCloud filter(ctx, 0.1f);
        filter.filterVoxel(cloud_1);
        filter.filterVoxel(cloud_2);
        icp.setInputSource(cloud_2);
        icp.setInputTarget(cloud_1);
        icp.align(alignedICP, r360::Matrix4f::Identity());
        std::printf("ICP took %g\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        std::printf("has converged:%d score: %g (%zu -> %zu points)\n", int(icp.hasConverged()), icp.getFitnessScore(),
                    cloud_2.size(), cloud_1.size());
        const r360::Matrix4f T = icp.getFinalTransformation();
        std::printf("ICP transformation:\n");
        for (int r = 0; r < 4; ++r) std::printf("%10.6f %10.6f %10.6f %10.6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
        std::printf("PbMap-Registration\n");
        for (int r = 0; r < 4; ++r) std::printf("%10.6f %10.6f %10.6f %10.6f\n", P(r, 0), P(r, 1), P(r, 2), P(r, 3));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return 0;
}
