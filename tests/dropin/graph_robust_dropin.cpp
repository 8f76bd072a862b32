// A loop closer that does not trust its loop edges, written against GraphOptimizer as a g2o user would write it
// (setRobustKernel per edge, chi2 per edge, dropping an edge), through include/rgbd360/compat.h with g++ alone.
//
//   graph_robust_dropin <graph.txt>
//
// graph.txt is graph_optimizer_dropin's, float values: "V <16 column-major pose entries>" per keyframe in order, then
// "E <from> <to> <16 column-major relative pose entries> <36 information entries>" per connection, in edge order.
// The program gives every loop edge (to - from != 1) a Cauchy kernel of width 3 and leaves the chain quadratic,
// optimises, prints "edge <k> chi2 <c> weight <w>" per edge and "wrong edge <k>" for the largest chi2, deactivates
// that edge, makes the others quadratic again, optimises once more and prints "pose <k> <16 values>" per keyframe.
#include <rgbd360/compat.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) {
        std::cerr << "usage: graph_robust_dropin <graph.txt>\n";
        return 2;
    }
    GraphOptimizer optimizer;
    optimizer.setRigidTransformationType(GraphOptimizer::SixDegreesOfFreedom);
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "V") {
            Eigen::Matrix4f T;                       // float, as the reference's callers hold their poses
            for (int k = 0; k < 16; ++k) ss >> T.data()[k];
            optimizer.addVertex(T.cast<double>());
        } else if (tag == "E") {
            int from, to;
            Eigen::Matrix4f Z;
            Eigen::Matrix<float, 6, 6> info;
            ss >> from >> to;
            for (int k = 0; k < 16; ++k) ss >> Z.data()[k];
            for (int k = 0; k < 36; ++k) ss >> info.data()[k];
            // the kernel of the edges added from now on: loop edges robust, the chain quadratic
            if (to - from != 1) optimizer.setRobustKernel(R360_GRAPH_KERNEL_CAUCHY, 3.0);
            else optimizer.setRobustKernel(R360_GRAPH_KERNEL_NONE);
            optimizer.addEdge(from, to, Z.cast<double>(), info.cast<double>());
        }
        if (!ss) {
            std::cerr << "malformed line: " << line << "\n";
            return 2;
        }
    }
    const int m = optimizer.numEdges();
    if (m == 0) return 2;
    optimizer.optimizeGraph();
    std::printf("status %d iterations %d F %.9g -> %.9g\n", optimizer.stats().status, optimizer.stats().iterations,
                optimizer.stats().F_initial, optimizer.stats().F_final);

    std::vector<double> chi2, weight;
    optimizer.getEdgeChi2(chi2, &weight);
    int worst = 0;
    for (int k = 0; k < m; ++k) {
        std::printf("edge %d chi2 %.9g weight %.9g\n", k, chi2[k], weight[k]);
        if (chi2[k] > chi2[worst]) worst = k;
    }
    std::printf("wrong edge %d\n", worst);

    optimizer.setEdgeActive(worst, false);
    for (int k = 0; k < m; ++k) optimizer.setEdgeRobustKernel(k, R360_GRAPH_KERNEL_NONE);
    optimizer.optimizeGraph();
    std::printf("status %d iterations %d F %.9g -> %.9g\n", optimizer.stats().status, optimizer.stats().iterations,
                optimizer.stats().F_initial, optimizer.stats().F_final);
    optimizer.getEdgeChi2(chi2);
    std::printf("dropped edge %d chi2 %.9g\n", worst, chi2[worst]);
    std::vector<Eigen::Matrix4f, Eigen::aligned_allocator<Eigen::Matrix4f> > poses;
    optimizer.getPoses(poses);
    for (size_t j = 0; j < poses.size(); j++) {
        std::printf("pose %zu", j);
        for (int k = 0; k < 16; ++k) std::printf(" %.9g", poses[j].data()[k]);
        std::printf("\n");
    }
    return 0;
}
