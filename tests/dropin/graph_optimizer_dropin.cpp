// The reference's GraphOptimizer call sites, written as SLAM/KFsphere_SLAM.cpp (:263-265, :541-550, :630, :679, :689,
// :705) and include/LoopClosure360.h (:89-91, :318) write them, through include/rgbd360/compat.h with g++ alone.
//
//   graph_optimizer_dropin <graph.txt> [out.g2o]
//
// graph.txt holds float values: "V <16 column-major pose entries>" per keyframe in order, then
// "E <from> <to> <16 column-major relative pose entries> <36 information entries>" per connection.  The program
// replays them the way the SLAM loop does (a vertex per keyframe, the edge from its nearest keyframe, then the
// further connections), optimises, and prints "pose <k> <16 floats>" per optimised pose.
#include <rgbd360/compat.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <vector>

struct Map360 {
    std::vector<Eigen::Matrix4f, Eigen::aligned_allocator<Eigen::Matrix4f> > vOptimizedPoses;
    std::map<unsigned, std::map<unsigned, std::pair<Eigen::Matrix4f, Eigen::Matrix<float, 6, 6> > > > mmConnectionKFs;
};

// LoopClosure360.h:52-60, 83-94: the loop closer owns an optimiser and seeds it with the identity
class LoopClosure360 {
  public:
    GraphOptimizer optimizer;
    LoopClosure360() {
        optimizer.setRigidTransformationType(GraphOptimizer::SixDegreesOfFreedom);
        Eigen::Matrix4d firstPose = Eigen::Matrix4d::Identity();
        optimizer.addVertex(firstPose);  // Set the first pose to the Identity
    }
    // LoopClosure360.h:314-321
    void addLoop(int compareLocalIdx, int newFrameID, Eigen::Matrix4f relativePose, Eigen::Matrix<float, 6, 6> informationMatrix,
                 Map360& Map) {
        optimizer.addEdge(compareLocalIdx, newFrameID, relativePose.cast<double>(), informationMatrix.cast<double>());
        Map.mmConnectionKFs[newFrameID][compareLocalIdx] =
            std::pair<Eigen::Matrix4f, Eigen::Matrix<float, 6, 6> >(relativePose, informationMatrix);
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        std::cerr << "usage: graph_optimizer_dropin <graph.txt> [out.g2o]\n";
        return 2;
    }
    std::vector<Eigen::Matrix4f> keyframePoses;
    struct Connection { int from, to; std::pair<Eigen::Matrix4f, Eigen::Matrix<float, 6, 6> > geomConnection; };
    std::vector<Connection> vConnections;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "V") {
            Eigen::Matrix4f T;
            for (int k = 0; k < 16; ++k) ss >> T.data()[k];
            keyframePoses.push_back(T);
        } else if (tag == "E") {
            Connection c;
            ss >> c.from >> c.to;
            for (int k = 0; k < 16; ++k) ss >> c.geomConnection.first.data()[k];
            for (int k = 0; k < 36; ++k) ss >> c.geomConnection.second.data()[k];
            vConnections.push_back(c);
        }
        if (!ss) {
            std::cerr << "malformed line: " << line << "\n";
            return 2;
        }
    }
    if (keyframePoses.empty()) return 2;

    Map360 Map;
    // KFsphere_SLAM.cpp:263-265
    Eigen::Matrix4f currentPose = keyframePoses[0];
    GraphOptimizer optimizer;
    optimizer.setRigidTransformationType(GraphOptimizer::SixDegreesOfFreedom);
    std::cout << "Added vertex: " << optimizer.addVertex(currentPose.cast<double>()) << std::endl;
    bool bHasNewLC = false;

    for (size_t kf = 1; kf < keyframePoses.size(); ++kf) {
        // :540-544: the new keyframe's vertex and the edge from its nearest keyframe
        currentPose = keyframePoses[kf];
        std::cout << "Added vertex: " << optimizer.addVertex(currentPose.cast<double>()) << std::endl;
        for (size_t link = 0; link < vConnections.size(); ++link) {
            if (vConnections[link].to != int(kf) && vConnections[link].from != int(kf)) continue;
            if (std::max(vConnections[link].to, vConnections[link].from) != int(kf)) continue;
            const unsigned frameOrder = unsigned(vConnections[link].to);
            // :630
            optimizer.addEdge(vConnections[link].from, unsigned(frameOrder), vConnections[link].geomConnection.first.cast<double>(),
                              vConnections[link].geomConnection.second.cast<double>());
            Map.mmConnectionKFs[frameOrder][vConnections[link].from] = vConnections[link].geomConnection;
            if (vConnections[link].to - vConnections[link].from != 1) bHasNewLC = true;
        }
    }
    if (bHasNewLC) {
        // :679, :689, :705
        optimizer.optimizeGraph();
        optimizer.getPoses(Map.vOptimizedPoses);
        currentPose = Map.vOptimizedPoses.back();
        bHasNewLC = false;
    } else {
        optimizer.getPoses(Map.vOptimizedPoses);
    }
    std::cout << "status " << optimizer.stats().status << " iterations " << optimizer.stats().iterations << " F "
              << optimizer.stats().F_initial << " -> " << optimizer.stats().F_final << "\n";
    for (size_t j = 0; j < Map.vOptimizedPoses.size(); j++) {
        std::printf("pose %zu", j);
        for (int k = 0; k < 16; ++k) std::printf(" %.9g", Map.vOptimizedPoses[j].data()[k]);
        std::printf("\n");
    }
    if (argc > 2) optimizer.saveGraph(argv[2]);

    // the loop closer's own optimiser, seeded with the identity (LoopClosure360.h:89-91) and fed one loop (:318)
    LoopClosure360 loopCloser;
    Eigen::Matrix4d second = Eigen::Matrix4d::Identity();
    second(0, 3) = 1.0;
    loopCloser.optimizer.addVertex(second);
    Eigen::Matrix4f rel = Eigen::Matrix4f::Identity();
    rel(0, 3) = 1.1f;
    loopCloser.addLoop(0, 1, rel, Eigen::Matrix<float, 6, 6>::Identity(), Map);
    loopCloser.optimizer.optimizeGraph();
    loopCloser.optimizer.getPoses(Map.vOptimizedPoses);
    std::printf("loop closer: x = %.6f\n", Map.vOptimizedPoses.back()(0, 3));

    bool threw = false;
    try {
        optimizer.setRigidTransformationType(GraphOptimizer::ThreeDegreesOfFreedom);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    std::cout << "ThreeDegreesOfFreedom " << (threw ? "throws" : "accepted") << "\n";
    return threw ? 0 : 1;
}
