// Drop-in check (compile only): the reference's topological-map call sites — SLAM/KFsphere_SLAM.cpp:560-744 and
// SLAM/SphereGraphSLAM.cpp:82-129, 160-242 — against the façade through include/rgbd360/compat.h with
// RGBD360_COMPAT_MAP360, under the substitutions INTEGRATION.md lists:
//   topologicalMap.vSSO.push_back(CMatrix(1,1)); vSSO[area](0,0) = 0        -> topologicalMap.addKeyframe(area)
//   vSSO[area].setSize(n+1, n+1); vSSO[area](n, n) = 0   (:164-166)          -> topologicalMap.addKeyframe(area)
//   vSSO[area](i, j) = vSSO[area](j, i) = sso   (:215, KFsphere_SLAM.cpp:613) -> topologicalMap.addConnection(kf_i, kf_j, sso)
//   vSSO[area].setSize(n, n)   (the not-registered branch, :236)             -> topologicalMap.dropLastKeyframe()
// Everything else is the reference's sequence: Map.addKeyframe, frame360->id / node, mmConnectionKFs, addConnection of
// a loop closure's SSO, Partitioner() every fourth keyframe, the Places print-out, Relocalizer360::relocalize.
#define RGBD360_COMPAT_MAP360
#include <rgbd360/compat.h>

#include <iostream>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#define MAX_MATCH_PLANES 25

using namespace std;

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const string path_dataset = argv[1];
    unsigned frame = unsigned(atoi(argv[2]));
    const int selectSample = 2;

    Calib360 calib;
    calib.loadExtrinsicCalibration();
    calib.loadIntrinsicCalibration();

    Map360 Map;
    TopologicalMap360 topologicalMap(Map);       // SphereGraphSLAM.cpp:83
    Relocalizer360 relocalizer(Map);
    RegisterRGBD360 registerer(mrpt::format("%s/config_files/configLocaliser_sphericalOdometry.ini", PROJECT_SOURCE_PATH));

    unsigned frameOrder = 0;
    string fileName = path_dataset + mrpt::format("/sphere_images_%d.bin", frame);
    Frame360* frame360 = new Frame360(&calib);
    frame360->loadFrame(fileName);
    frame360->undistort();
    frame360->buildSphereCloud();
    frame360->getPlanes();
    frame360->id = frameOrder;
    frame360->node = Map.currentArea;
    Eigen::Matrix4f currentPose = Eigen::Matrix4f::Identity();
    Map.addKeyframe(frame360, currentPose);      // :118
    topologicalMap.addKeyframe(Map.currentArea); // :123-129
    unsigned nearestKF = frameOrder;

    frame += selectSample;
    fileName = path_dataset + mrpt::format("/sphere_images_%d.bin", frame);
    while (fexists(fileName.c_str())) {
        frame360 = new Frame360(&calib);
        frame360->loadFrame(fileName);
        frame360->undistort();
        frame360->buildSphereCloud();
        frame360->getPlanes();
        frame += selectSample;
        fileName = path_dataset + mrpt::format("/sphere_images_%d.bin", frame);

        ++frameOrder;
        frame360->id = frameOrder;
        frame360->node = Map.currentArea;
        int newLocalFrameID = int(Map.vsAreas[Map.currentArea].size());
        Map.addKeyframe(frame360, currentPose);
        topologicalMap.addKeyframe(Map.currentArea);   // :164-166

        const unsigned compareSphereId = nearestKF;
        bool bGoodRegistration = registerer.RegisterPbMap(Map.vpSpheres[compareSphereId], frame360, MAX_MATCH_PLANES,
                                                          RegisterRGBD360::PLANAR_ODOMETRY_3DoF);
        if (bGoodRegistration && registerer.getMatchedPlanes().size() >= 6) {
            currentPose = currentPose * registerer.getPose();
            Map.vOptimizedPoses.back() = currentPose;
            Map.mmConnectionKFs[frameOrder][compareSphereId] =
                std::pair<Eigen::Matrix4f, Eigen::Matrix<float, 6, 6> >(registerer.getPose(), registerer.getInfoMat());
            float sso = registerer.getAreaMatched() / registerer.areaSource;
            cout << "Add tracking SSO: " << newLocalFrameID << " " << compareSphereId << endl;
            topologicalMap.addConnection(frameOrder, compareSphereId, sso);   // :215
            nearestKF = frameOrder;
        } else {
            cout << "No registration available\n";
            topologicalMap.dropLastKeyframe();   // :232-242
            Map.vpSpheres.pop_back();
            Map.vTrajectoryPoses.pop_back();
            Map.vOptimizedPoses.pop_back();
            --frameOrder;
            delete frame360;
            int relocKF = relocalizer.relocalize(Map.vpSpheres.back());
            if (relocKF >= 0)
                cout << "relocalized wrt " << relocalizer.relocKF << " " << relocalizer.rigidTransf(0, 3) << " "
                     << relocalizer.informationM(0, 0) << endl;
            continue;
        }

        // Visibility divission (Normalized-cut), KFsphere_SLAM.cpp:710-740
        if (newLocalFrameID % 4 == 0) {
            std::vector<unsigned> vicinityKFs;
            std::vector<float> SSO = topologicalMap.getVicinitySSO(&vicinityKFs);
            cout << "SSO of " << vicinityKFs.size() << " keyframes, " << SSO.size() << " entries\n";
            topologicalMap.Partitioner();
            cout << "\tPlaces\n";
            for (unsigned node = 0; node < Map.vsNeighborAreas.size(); node++) {
                cout << "\t" << node << ":";
                for (set<unsigned>::iterator it = Map.vsNeighborAreas[node].begin(); it != Map.vsNeighborAreas[node].end(); it++)
                    cout << " " << *it;
                cout << endl;
            }
            for (unsigned node = 0; node < Map.vsAreas.size(); node++)
                cout << "area " << node << " representative " << Map.vSelectedKFs[node] << endl;
        }
    }
    for (unsigned i = 0; i < Map.vpSpheres.size(); i++) {
        cout << "keyframe " << Map.vpSpheres[i]->id << " submap " << Map.vpSpheres[i]->node << endl;
        delete Map.vpSpheres[i];
    }
    return 0;
}
