// KFsphereSLAM — apps/KFsphereTracking.cpp's front end plus the back half of the reference's SLAM/KFsphere_SLAM.cpp,
// written against the façade (include/rgbd360/rgbd360.h):
//   * every new keyframe adds a vertex at the chained pose (:541) and the dense edge from the keyframe it was
//     tracked against (:544: the dense pose and align360.getHessian(), unchanged), and the PbMap edge under the
//     reference's test (:547-550: good tracking, at least 4 matched planes, more than 6 m2 matched, within 5 degrees
//     and 0.1 m of the dense pose; registerer.getInfoMat());
//   * the keyframe is then registered against the earlier keyframes within 5 m (LoopClosure360.h:294) that lie at
//     least --min-gap keyframes back (default 3): RegisterPbMap, more than minMatchesThreshold = 5 matched planes and
//     more than areaThreshold = 15 m2 (:114-115, :298), the dense refinement from the PbMap pose (:306-313) and
//     avDepthResidual < 2.0 (:316; assigned only by the occlusion variants, so the test applies with occlusion 1 / 2);
//     a loop edge carries the refined pose and align360.getHessian() (:318);
//   * the graph is optimised whenever a loop edge was added (:679), the optimised poses replace the chain's
//     (:689, :705) and tracking goes on from the optimised pose of the last keyframe.
// At the end: the chained and the optimised keyframe poses, in synthetic mode each one's distance from the path
// (r360_synth_path_pose), and the global map fused twice (r360_ctx_map_add_frame), at the chained and at the
// optimised poses, with both sizes.
// With --submaps the topological map of KFsphere_SLAM.cpp goes along (r360::Map360 / TopologicalMap360): every keyframe
// joins the current area, every accepted tracking or loop connection enters the SSO table with align360.SSO (:402,
// :443, :613-628), Partitioner() runs when the keyframe's index in its area is a multiple of 4 (:710-717) and the
// "Places" lines follow (:733-740); at the end a line per area gives its keyframes and its representative.  Without
// the flag nothing of this runs or prints.
// The reference optimises with every loop edge at full quadratic weight; three flags go beyond it:
// --robust huber:D | cauchy:D gives the loop edges a robust kernel (the chain and PbMap edges stay quadratic),
// --reject-chi2 T deactivates after each optimisation the loop edges whose chi2 exceeds T and optimises again, and
// --false-loop I,J adds, with keyframe J, a loop edge I -> J whose measurement is the keyframes' current relative pose
// composed with a fixed wrong transform (0.4 rad about y, (1.0, -0.7, 0.5) m) at J's dense Hessian.  With any of them
// every optimisation is followed by a "loop edge I J chi2 X weight W" line per loop edge; without them the output is
// what it was.
// --clean-map sor:K,MUL[,D] | radius:R,N filters the final map, fused at the optimised poses, where it lies on the GPU
// (r360::GlobalMap360::removeOutliers: pcl::StatisticalOutlierRemoval with meanK K, multiplier MUL and a search bound of
// D m, 0.5 by default, or pcl::RadiusOutlierRemoval) and prints one more line, "map cleaned: <before> -> <after> points
// (<short> short)"; without the flag the output is what it was.
// --map-normals K,R estimates the final map's normals and curvature where it lies (r360::GlobalMap360::estimateNormals:
// pcl::NormalEstimation over at most K points within R m, turned towards the nearest optimised keyframe position), after
// --clean-map if given, and prints one more line, "map normals: <points> points, <short> short, <mean> neighbours on
// average".  --save-map file.pcd writes the final map (binary), with its normals when they were estimated.
// --clean-map cluster:TOL,MIN is the third kind: r360::GlobalMap360::removeSmallClusters keeps the connected components of
// "closer than TOL m" with at least MIN points (pcl::EuclideanClusterExtraction), and the line reads "map cleaned:
// <before> -> <after> points (<components> components, <kept> kept)".  --map-clusters TOL,MIN[,ANGLE_DEG] clusters the
// final map where it lies (r360::GlobalMap360::cluster), after --clean-map; with an angle it is the normal-aware form on
// the normals of --map-normals, which it then requires and follows.  It prints one more line, "map clusters: <points>
// points, <components> components, <clusters> kept, largest <size>".  --save-clusters file.pcd writes the labelled map
// (binary, x y z rgba label).
// --map-planes DIST,MIN[,MAX] peels the final map's RANSAC planes where it lies (r360::GlobalMap360::segmentPlanes:
// pcl::SACSegmentation's plane search with distance threshold DIST m, planes of at least MIN points, at most MAX of
// them, 8 by default), after --clean-map and --map-normals; with --map-normals an inlier's normal must also agree with
// the plane's.  It prints one more line, "map planes: <points> points, <planes> planes, <in planes> points in planes,
// largest <size>".  --save-planes file.pcd writes the map labelled by plane (binary, x y z rgba label).  --remove-planes
// then drops the plane points (r360::GlobalMap360::removePlanes) before --map-clusters, which so reports the objects
// rather than the room; the removal invalidates the normals, so it is refused together with an angle in --map-clusters,
// and --save-map then writes what is left without normals.
//   usage: KFsphereSLAM --synthetic-frames a,b,c,... [occlusion] [--min-gap G] [--kf-dist D] [--save graph.g2o] [--submaps]
//                       [--robust huber:D | cauchy:D] [--reject-chi2 T] [--false-loop I,J] [--clean-map sor:K,MUL[,D] | radius:R,N]
//                       [--map-normals K,R] [--save-map file.pcd] [--map-clusters TOL,MIN[,ANGLE_DEG]] [--save-clusters file.pcd]
//                       [--map-planes DIST,MIN[,MAX]] [--save-planes file.pcd] [--remove-planes]
//                       (--clean-map also takes cluster:TOL,MIN)
//          KFsphereSLAM --synthetic <n_frames> [occlusion] ...
//          KFsphereSLAM <dir with sphere_images_<n>.bin> <first> <step> [occlusion] ...
#include <rgbd360/rgbd360.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

static bool fexists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

typedef r360::Matrix4f Matrix4f;

static float translationNorm(const Matrix4f& T) {
    return std::sqrt(T(0, 3) * T(0, 3) + T(1, 3) * T(1, 3) + T(2, 3) * T(2, 3));
}
// Miscellaneous.h:127-149: the angle (degrees) and the distance between two poses
static float diffRotation(const Matrix4f& a, const Matrix4f& b) {
    float tr = 0.f;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) tr += a(r, c) * b(r, c);
    const float cs = std::fmax(-1.f, std::fmin(1.f, (tr - 1.f) / 2.f));
    return std::acos(cs) * 180.f / 3.14159265359f;
}
static float difTranslation(const Matrix4f& a, const Matrix4f& b) { return translationNorm(a.inverse() * b); }

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    int min_gap = 3;
    float kf_dist = 0.4f;
    std::string save, frames_arg;
    int n_synth = 0;
    bool synthetic = false, submaps = false;
    int robust_kind = R360_GRAPH_KERNEL_NONE;            // --robust: the loop edges' kernel
    double robust_delta = 1.0;
    double reject_chi2 = -1.0;                           // --reject-chi2: < 0 = off
    int false_from = -1, false_to = -1;                  // --false-loop
    bool bad_arg = false;
    bool clean_map = false;                              // --clean-map
    r360_outlier_params clean;
    r360_outlier_default_params(&clean);
    bool map_normals = false;                            // --map-normals
    r360_normal_params normal_prm;
    r360_normal_default_params(&normal_prm);
    std::string save_map;                                // --save-map
    bool clean_clusters = false;                         // --clean-map cluster:TOL,MIN
    r360_cluster_params clean_clu;
    r360_cluster_default_params(&clean_clu);
    bool map_clusters = false, cluster_normals = false;  // --map-clusters, with an angle
    r360_cluster_params cluster_prm;
    r360_cluster_default_params(&cluster_prm);
    std::string save_clusters;                           // --save-clusters
    bool map_planes = false, remove_planes = false;      // --map-planes, --remove-planes
    r360_sac_params plane_prm;
    r360_sac_default_params(&plane_prm);
    std::string save_planes;                             // --save-planes
    for (int k = 1; k < argc; ++k) {
        const std::string a = argv[k];
        if (a == "--clean-map" && k + 1 < argc) {
            const std::string v = argv[++k];
            clean_map = true;
            if (v.compare(0, 4, "sor:") == 0) {
                clean.kind = R360_OUTLIER_STATISTICAL;
                const int got = std::sscanf(v.c_str() + 4, "%d,%f,%f", &clean.mean_k, &clean.stddev_mul, &clean.max_dist);
                bad_arg = bad_arg || got < 2;
            } else if (v.compare(0, 7, "radius:") == 0) {
                clean.kind = R360_OUTLIER_RADIUS;
                bad_arg = bad_arg || std::sscanf(v.c_str() + 7, "%f,%d", &clean.radius, &clean.min_neighbors) != 2;
            } else if (v.compare(0, 8, "cluster:") == 0) {
                clean_clusters = true;
                bad_arg = bad_arg || std::sscanf(v.c_str() + 8, "%f,%d", &clean_clu.tolerance, &clean_clu.min_size) != 2;
            } else {
                bad_arg = true;
            }
            continue;
        }
        if (a == "--robust" && k + 1 < argc) {
            const std::string v = argv[++k];
            const size_t colon = v.find(':');
            const std::string name = v.substr(0, colon);
            robust_kind = name == "huber" ? R360_GRAPH_KERNEL_HUBER : name == "cauchy" ? R360_GRAPH_KERNEL_CAUCHY : -1;
            robust_delta = colon == std::string::npos ? 0.0 : std::atof(v.c_str() + colon + 1);
            bad_arg = bad_arg || robust_kind < 0 || !(robust_delta > 0.0);
        } else if (a == "--reject-chi2" && k + 1 < argc) {
            reject_chi2 = std::atof(argv[++k]);
            bad_arg = bad_arg || !(reject_chi2 >= 0.0);
        } else if (a == "--false-loop" && k + 1 < argc) {
            bad_arg = bad_arg || std::sscanf(argv[++k], "%d,%d", &false_from, &false_to) != 2 || false_from < 0 ||
                      false_to <= false_from;
        }
        else if (a == "--min-gap" && k + 1 < argc) min_gap = std::atoi(argv[++k]);
        else if (a == "--kf-dist" && k + 1 < argc) kf_dist = float(std::atof(argv[++k]));
        else if (a == "--save" && k + 1 < argc) save = argv[++k];
        else if (a == "--save-map" && k + 1 < argc) save_map = argv[++k];
        else if (a == "--map-normals" && k + 1 < argc) {
            map_normals = true;
            bad_arg = bad_arg || std::sscanf(argv[++k], "%d,%f", &normal_prm.k, &normal_prm.radius) != 2;
        }
        else if (a == "--save-clusters" && k + 1 < argc) save_clusters = argv[++k];
        else if (a == "--map-clusters" && k + 1 < argc) {
            map_clusters = true;
            float deg = 0.f;
            const int got = std::sscanf(argv[++k], "%f,%d,%f", &cluster_prm.tolerance, &cluster_prm.min_size, &deg);
            bad_arg = bad_arg || got < 2;
            if (got == 3) {
                cluster_normals = true;
                cluster_prm.eps_angle = deg * 3.14159265359f / 180.f;
            }
        }
        else if (a == "--save-planes" && k + 1 < argc) save_planes = argv[++k];
        else if (a == "--remove-planes") remove_planes = true;
        else if (a == "--map-planes" && k + 1 < argc) {
            map_planes = true;
            const int got = std::sscanf(argv[++k], "%f,%d,%d", &plane_prm.distance_threshold, &plane_prm.min_inliers,
                                        &plane_prm.max_planes);
            bad_arg = bad_arg || got < 2;
        }
        else if (a == "--submaps") submaps = true;
        else if (a == "--synthetic-frames" && k + 1 < argc) { frames_arg = argv[++k]; synthetic = true; }
        else if (a == "--synthetic" && k + 1 < argc) { n_synth = std::atoi(argv[++k]); synthetic = true; }
        else pos.push_back(a);
    }
    std::vector<int> order;                              // the frames to read, in order
    for (size_t p = 0; p < frames_arg.size();) {
        size_t q = frames_arg.find(',', p);
        if (q == std::string::npos) q = frames_arg.size();
        order.push_back(std::atoi(frames_arg.substr(p, q - p).c_str()));
        p = q + 1;
    }
    for (int k = 0; k < n_synth && frames_arg.empty(); ++k) order.push_back(k);
    bad_arg = bad_arg || (cluster_normals && !map_normals) || (!save_clusters.empty() && !map_clusters);
    bad_arg = bad_arg || ((remove_planes || !save_planes.empty()) && !map_planes) || (remove_planes && cluster_normals);
    if (bad_arg || (synthetic && order.empty()) || (!synthetic && pos.size() < 3)) {
        std::fprintf(stderr, "usage: %s --synthetic-frames a,b,c,... [occlusion] | --synthetic <n> [occlusion] | <dir> <first> <step> "
                             "[occlusion]   [--min-gap G] [--kf-dist D] [--save graph.g2o] [--submaps]\n"
                             "       [--robust huber:D | cauchy:D] [--reject-chi2 T] [--false-loop I,J] [--clean-map sor:K,MUL[,D] | radius:R,N]\n"
                             "       [--map-normals K,R] [--save-map file.pcd] [--map-clusters TOL,MIN[,ANGLE_DEG]] [--save-clusters file.pcd]\n"
                             "       [--map-planes DIST,MIN[,MAX]] [--save-planes file.pcd] [--remove-planes]\n"
                             "  --robust       loop edges get the kernel, of width D on sqrt(chi2); chain and PbMap edges stay quadratic\n"
                             "  --reject-chi2  after each optimisation loop edges with chi2 > T are deactivated and the graph is optimised again\n"
                             "  --false-loop   when keyframe J is added, also add a wrong loop edge I -> J (demonstration)\n"
                             "  With any of the three, 'loop edge I J chi2 X weight W' is printed per loop edge after every optimisation\n"
                             "  (--reject-chi2 inf prints and rejects nothing).  The dense Hessians are not calibrated information\n"
                             "  matrices, so chi2 has no unit scale: choose D and T from these printed values.\n"
                             "  --clean-map    the final map at the optimised poses through the statistical (sor:meanK,multiplier[,bound in m])\n"
                             "                 or the radius (radius:R in m,min neighbours) outlier filter, on the GPU\n"
                             "  --map-normals  normals and curvature of the final map from at most K points within R m, turned towards the\n"
                             "                 nearest keyframe position, on the GPU (after --clean-map)\n"
                             "  --save-map     the final map as a binary PCD file, with the normals when they were estimated\n"
                             "  --clean-map cluster:TOL,MIN  keeps the connected components of 'closer than TOL m' with at least MIN points\n"
                             "  --map-clusters the final map's Euclidean clusters (tolerance in m, least size), after --clean-map; with an angle\n"
                             "                 in degrees two neighbours' normals must also agree within it (needs --map-normals)\n"
                             "  --save-clusters  the clustered map as a binary PCD file with a label field (needs --map-clusters)\n"
                             "  --map-planes   the final map's RANSAC planes (distance threshold in m, least size, at most MAX planes, 8 by\n"
                             "                 default), after --clean-map and --map-normals; with --map-normals an inlier's normal must agree\n"
                             "  --save-planes  the map labelled by plane as a binary PCD file with a label field (needs --map-planes)\n"
                             "  --remove-planes  drops the plane points before --map-clusters (needs --map-planes; not with an angle in\n"
                             "                 --map-clusters: the removal invalidates the normals)\n", argv[0]);
        return 1;
    }
    const bool edge_report = robust_kind != R360_GRAPH_KERNEL_NONE || reject_chi2 >= 0.0 || false_from >= 0;
    const std::string dir = synthetic ? "" : pos[0];
    const int first = synthetic ? 0 : std::atoi(pos[1].c_str()), step = synthetic ? 1 : std::atoi(pos[2].c_str());
    const size_t occ_at = synthetic ? 0 : 3;
    const int occlusion = pos.size() > occ_at ? std::atoi(pos[occ_at].c_str()) : 1;
    const float selectKF_ICPdist = 0.9f;                 // KFsphere_SLAM.cpp:388
    const size_t minMatchesThreshold = 5;                // LoopClosure360.h:114-115
    const float areaThreshold = 15.0f;
    try {
        r360::Context ctx(0);
        r360::Calib360 calib(ctx, synthetic ? 480 : 240, synthetic ? 640 : 320);
        calib.loadExtrinsicCalibration(std::string(RGBD360_DATA_DIR) + "/calib/Extrinsics");
        if (!synthetic) calib.loadIntrinsicCalibration(std::string(RGBD360_DATA_DIR) + "/calib/Intrinsics");
        r360::RegisterRGBD360 registerer(ctx, std::string(RGBD360_DATA_DIR) + "/config_files/configLocaliser_sphericalOdometry.ini");
        r360::RegisterPhotoICP align360(ctx);
        align360.setNumPyr(5);
        align360.useSaliency(false);
        align360.setVisualization(false);
        align360.setGrayVariance(3.f / 255);
        const float angleOffset = 157.5f;
        Matrix4f rotOffset, rotOffsetInv;
        rotOffset(1, 1) = rotOffset(2, 2) = std::cos(angleOffset * 3.14159265359 / 180);
        rotOffset(1, 2) = std::sin(angleOffset * 3.14159265359 / 180);
        rotOffset(2, 1) = -rotOffset(1, 2);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) rotOffsetInv(r, c) = rotOffset(c, r);

        const uint32_t seed = 360u << 16;
        std::vector<uint8_t> bgr;
        std::vector<uint16_t> depth;
        // the n-th frame of the run; *id = its path index (synthetic) or file number
        auto load = [&](r360::Frame360& f, size_t n, int* id) -> bool {
            if (synthetic) {
                if (n >= order.size()) return false;
                *id = order[n];
                float P[16];
                r360_synth_path_pose(seed, *id, P);
                bgr.resize(size_t(8) * 480 * 640 * 3);
                depth.resize(size_t(8) * 480 * 640);
                r360::check(r360_synth_frame(calib.get(), seed, P, bgr.data(), depth.data()), "synth_frame");
                f.upload(bgr.data(), depth.data());
                return true;
            }
            *id = first + int(n) * step;
            const std::string path = dir + "/sphere_images_" + std::to_string(*id) + ".bin";
            if (!fexists(path)) return false;
            f.loadFrame(path);
            return true;
        };

        // KFsphere_SLAM.cpp:263-265
        r360::GraphOptimizer optimizer(ctx);
        optimizer.setRigidTransformationType(r360::GraphOptimizer::SixDegreesOfFreedom);
        std::vector<std::unique_ptr<r360::Frame360> > kfs;
        std::vector<int> kfId;
        std::vector<Matrix4f> chainPose;                 // the raw product of dense poses
        std::vector<Matrix4f> vOptimizedPoses;           // Map.vOptimizedPoses: the chain until a loop closes
        int id = 0;
        kfs.emplace_back(new r360::Frame360(&calib));
        if (!load(*kfs.back(), 0, &id)) { std::fprintf(stderr, "no first frame\n"); return 3; }
        kfs.back()->getPlanes();
        kfs.back()->stitchSphericalImage();
        kfId.push_back(id);
        Matrix4f currentPose = Matrix4f::Identity();
        chainPose.push_back(currentPose);
        vOptimizedPoses.push_back(currentPose);
        std::printf("Added vertex: %d\n", optimizer.addVertex(currentPose.cast<double>()));
        // KFsphere_SLAM.cpp:259-260, 330-337: the map and its topological arrangement
        r360::Map360 Map;
        std::unique_ptr<r360::TopologicalMap360> topologicalMap;
        if (submaps) {
            topologicalMap.reset(new r360::TopologicalMap360(Map, ctx));
            Map.vpSpheres.push_back(kfs.back().get());
            topologicalMap->addKeyframe(Map.currentArea);
        }
        Matrix4f rigidTransf_dense_ref = Matrix4f::Identity();
        int loops = 0, optimisations = 0;
        double F_first = 0.0, F_last = 0.0;
        // the loop edges by their index in the graph: the ones that may carry a kernel and may be rejected
        struct LoopEdge { int edge, from, to; bool active; double chi2; };
        std::vector<LoopEdge> loopEdges;
        auto addLoopEdge = [&](int from, int to, const Matrix4f& rel, const r360::Matrix6f& info) {
            const int edge = optimizer.numEdges();
            optimizer.addEdge(from, to, rel.cast<double>(), info.cast<double>());
            if (robust_kind != R360_GRAPH_KERNEL_NONE) optimizer.setEdgeRobustKernel(edge, robust_kind, robust_delta);
            loopEdges.push_back(LoopEdge{edge, from, to, true, 0.0});
        };
        auto optimise = [&]() {                          // :679-705
            optimizer.optimizeGraph();
            optimizer.getPoses(vOptimizedPoses);
            currentPose = vOptimizedPoses.back();
            const r360_graph_stats& st = optimizer.stats();
            if (optimisations++ == 0) F_first = st.F_initial;
            F_last = st.F_final;
            std::printf("Optimize graph SLAM %zu: status %d iterations %d cost %.9g -> %.9g\n", kfs.size(), st.status, st.iterations,
                        st.F_initial, st.F_final);
            if (!edge_report) return;
            std::vector<double> chi2, weight;
            optimizer.getEdgeChi2(chi2, &weight);
            for (LoopEdge& le : loopEdges) {
                le.chi2 = chi2[le.edge];
                std::printf("loop edge %d %d chi2 %.9g weight %.9g\n", le.from, le.to, le.chi2, weight[le.edge]);
            }
        };
        for (size_t n = 1;; ++n) {
            std::unique_ptr<r360::Frame360> frame(new r360::Frame360(&calib));
            if (!load(*frame, n, &id)) break;
            frame->getPlanes();
            frame->stitchSphericalImage();
            r360::Frame360* kf = kfs.back().get();
            const int nearestKF = int(kfs.size()) - 1;
            const bool bGoodTracking = registerer.RegisterPbMap(kf, frame.get(), 25, r360::RegisterRGBD360::PLANAR_3DoF);
            Matrix4f trackedPosePbMap = registerer.getPose();
            const size_t trackedMatches = registerer.getMatchedPlanes().size();
            const float trackedArea = registerer.getAreaMatched();
            const r360::Matrix6f trackedInfo = bGoodTracking ? registerer.getInfoMat() : r360::Matrix6f::Identity();
            if (bGoodTracking) rigidTransf_dense_ref = rotOffset * trackedPosePbMap * rotOffsetInv;
            align360.setTargetFrame(kf->sphereRGB, kf->sphereDepth);
            align360.setSourceFrame(frame->sphereRGB, frame->sphereDepth);
            const bool ok = align360.alignFrames360(rigidTransf_dense_ref, r360::RegisterPhotoICP::PHOTO_DEPTH, occlusion);
            rigidTransf_dense_ref = align360.getOptimalPose();
            Matrix4f rigidTransf_dense = rotOffsetInv * rigidTransf_dense_ref * rotOffset;
            const r360::Matrix6f hessian = align360.getHessian();
            const float candidateKF_sso = align360.SSO;  // :402
            const float dist = translationNorm(rigidTransf_dense);
            std::printf("frame %d: PbMap %s matches %zu area %.3f; dense %s dist %.3f residuals %.5f %.5f\n", id,
                        bGoodTracking ? "ok" : "failed", trackedMatches, trackedArea, ok ? "ok" : "ILL-POSED", dist,
                        align360.avPhotoResidual, align360.avDepthResidual);
            const bool far = dist > kf_dist || (occlusion && !(align360.avDepthResidual < selectKF_ICPdist));
            if (!far || !ok) continue;

            // a new keyframe (:536-550)
            chainPose.push_back(chainPose.back() * rigidTransf_dense);
            currentPose = currentPose * rigidTransf_dense;
            const int newFrameID = optimizer.addVertex(currentPose.cast<double>());
            std::printf("Added vertex: %d (frame %d)\n", newFrameID, id);
            optimizer.addEdge(nearestKF, newFrameID, rigidTransf_dense.cast<double>(), hessian.cast<double>());
            if (bGoodTracking && trackedMatches >= 4 && trackedArea > 6)
                if (diffRotation(trackedPosePbMap, rigidTransf_dense) < 5 && difTranslation(trackedPosePbMap, rigidTransf_dense) < 0.1) {
                    optimizer.addEdge(nearestKF, newFrameID, trackedPosePbMap.cast<double>(), trackedInfo.cast<double>());
                    std::printf("Added addEdge PbMap %d %d\n", nearestKF, newFrameID);
                }
            kfs.push_back(std::move(frame));
            kfId.push_back(id);
            vOptimizedPoses.push_back(currentPose);
            rigidTransf_dense_ref = Matrix4f::Identity();
            r360::Frame360* newKF = kfs.back().get();
            int newLocalFrameID = 0;
            if (submaps) {                               // :566-615
                newLocalFrameID = int(Map.vsAreas[Map.currentArea].size());
                Map.vpSpheres.push_back(newKF);
                topologicalMap->addKeyframe(Map.currentArea);
                topologicalMap->addConnection(unsigned(newFrameID), unsigned(nearestKF), candidateKF_sso);
                std::printf("SSO is %.6f\n", candidateKF_sso);
            }

            // loop closure against the earlier keyframes (LoopClosure360.h:290-321)
            bool bHasNewLC = false;
            for (int compareLocalIdx = 0; compareLocalIdx + min_gap <= newFrameID; ++compareLocalIdx) {
                Matrix4f relativePose = vOptimizedPoses[compareLocalIdx].inverse() * currentPose;
                const float distance = translationNorm(relativePose);
                if (!(distance < 5.f)) continue;
                const bool bGoodRegistration =
                    registerer.RegisterPbMap(kfs[compareLocalIdx].get(), newKF, 25, r360::RegisterRGBD360::PLANAR_3DoF);
                std::printf("Check loop closure between %d and %d: %s matches %zu area %.3f\n", newFrameID, compareLocalIdx,
                            bGoodRegistration ? "ok" : "failed", registerer.getMatchedPlanes().size(), registerer.getAreaMatched());
                if (!(bGoodRegistration && registerer.getMatchedPlanes().size() > minMatchesThreshold &&
                      registerer.getAreaMatched() > areaThreshold))
                    continue;
                relativePose = registerer.getPose();
                align360.setTargetFrame(kfs[compareLocalIdx]->sphereRGB, kfs[compareLocalIdx]->sphereDepth);
                align360.setSourceFrame(newKF->sphereRGB, newKF->sphereDepth);
                const Matrix4f initTransf_dense = rotOffset * relativePose * rotOffsetInv;
                const bool lok = align360.alignFrames360(initTransf_dense, r360::RegisterPhotoICP::PHOTO_DEPTH, occlusion);
                relativePose = rotOffsetInv * align360.getOptimalPose() * rotOffset;
                const r360::Matrix6f informationMatrix = align360.getHessian();
                if (lok && (!occlusion || align360.avDepthResidual < 2.0)) {
                    addLoopEdge(compareLocalIdx, newFrameID, relativePose, informationMatrix);
                    std::printf("LC Add edge between %d and %d (residual %.5f)\n", compareLocalIdx, newFrameID, align360.avDepthResidual);
                    if (submaps) topologicalMap->addConnection(unsigned(newFrameID), unsigned(compareLocalIdx), align360.SSO);   // :628
                    bHasNewLC = true;
                    ++loops;
                }
            }
            if (newFrameID == false_to && false_from < newFrameID) {   // --false-loop: a wrong pair that passed the matcher
                Matrix4f wrong = Matrix4f::Identity();   // 0.4 rad about y, then (1.0, -0.7, 0.5) m
                wrong(0, 0) = wrong(2, 2) = std::cos(0.4f);
                wrong(0, 2) = std::sin(0.4f);
                wrong(2, 0) = -wrong(0, 2);
                wrong(0, 3) = 1.0f; wrong(1, 3) = -0.7f; wrong(2, 3) = 0.5f;
                const Matrix4f relativePose = vOptimizedPoses[false_from].inverse() * currentPose * wrong;
                addLoopEdge(false_from, newFrameID, relativePose, hessian);
                std::printf("LC Add false edge between %d and %d\n", false_from, newFrameID);
                bHasNewLC = true;
                ++loops;
            }
            if (bHasNewLC) {                             // :679-705
                optimise();
                bool rejected = false;
                if (reject_chi2 >= 0.0)
                    for (LoopEdge& le : loopEdges)
                        if (le.active && le.chi2 > reject_chi2) {
                            optimizer.setEdgeActive(le.edge, false);
                            le.active = false;
                            rejected = true;
                            std::printf("LC reject edge between %d and %d chi2 %.9g\n", le.from, le.to, le.chi2);
                        }
                if (rejected) optimise();
            }
            if (submaps && newLocalFrameID % 4 == 0) {   // Visibility division (Normalized-cut), :710-740
                topologicalMap->Partitioner();
                std::printf("\tPlaces\n");
                for (size_t node = 0; node < Map.vsNeighborAreas.size(); ++node) {
                    std::printf("\t%zu:", node);
                    for (unsigned nb : Map.vsNeighborAreas[node]) std::printf(" %u", nb);
                    std::printf("\n");
                }
            }
        }
        if (submaps)
            for (size_t node = 0; node < Map.vsAreas.size(); ++node) {
                std::printf("area %zu: keyframes", node);
                for (unsigned k : Map.vsAreas[node]) std::printf(" %u", k);
                std::printf(" representative %u%s\n", Map.vSelectedKFs[node], node == Map.currentArea ? " current" : "");
            }

        std::printf("%zu keyframes, %d loop edges, %d optimisations", kfs.size(), loops, optimisations);
        if (optimisations) std::printf(", cost %.9g -> %.9g", F_first, F_last);
        std::printf("\n");
        Matrix4f P0inv = Matrix4f::Identity();
        if (synthetic) {
            Matrix4f P0;
            r360_synth_path_pose(seed, kfId[0], P0.data());
            P0inv = P0.inverse();
        }
        double worstChain = 0, worstOpt = 0;
        for (size_t k = 0; k < kfs.size(); ++k) {
            const Matrix4f& C = chainPose[k];
            const Matrix4f& O = vOptimizedPoses[k];
            std::printf("keyframe %zu frame %d chain %.9g %.9g %.9g optimised %.9g %.9g %.9g", k, kfId[k], C(0, 3), C(1, 3), C(2, 3),
                        O(0, 3), O(1, 3), O(2, 3));
            if (synthetic) {
                Matrix4f P;
                r360_synth_path_pose(seed, kfId[k], P.data());
                const Matrix4f truth = P0inv * P;
                const float dc = difTranslation(truth, C), dopt = difTranslation(truth, O);
                worstChain = std::fmax(worstChain, dc);
                worstOpt = std::fmax(worstOpt, dopt);
                std::printf(" from path %.4f %.4f", dc, dopt);
            }
            bool same = true;
            for (int e = 0; e < 16; ++e) same = same && C.data()[e] == O.data()[e];
            std::printf(" %s\n", same ? "same" : "moved");
        }
        if (synthetic) std::printf("worst distance from the path: chain %.4f m, optimised %.4f m\n", worstChain, worstOpt);

        // the global map, fused at the chained and at the optimised poses
        r360::GlobalMap360 map(ctx, 0.05f, 4.0f);
        size_t sizes[2] = {0, 0};
        for (int which = 0; which < 2; ++which) {
            map.reset();
            for (size_t k = 0; k < kfs.size(); ++k) map.add(*kfs[k], which ? vOptimizedPoses[k] : chainPose[k]);
            sizes[which] = map.size();
        }
        std::printf("global map: %zu points at the chained poses, %zu at the optimised poses\n", sizes[0], sizes[1]);
        if (clean_map && clean_clusters) {
            r360_cluster_stats st;
            map.removeSmallClusters(clean_clu, false, &st);
            std::printf("map cleaned: %zu -> %zu points (%zu components, %zu kept)\n", sizes[1], map.size(), st.n_components,
                        st.n_clusters);
        } else if (clean_map) {   // the map holds the fusion at the optimised poses
            r360_outlier_stats st;
            map.removeOutliers(clean, &st);
            std::printf("map cleaned: %zu -> %zu points (%zu short)\n", sizes[1], map.size(), st.n_short);
        }
        if (map_normals) {   // the viewpoints: where the keyframes stood, at the optimised poses
            std::vector<float> views;
            for (size_t k = 0; k < kfs.size(); ++k)
                for (int r = 0; r < 3; ++r) views.push_back(vOptimizedPoses[k](r, 3));
            r360_normal_stats st;
            map.estimateNormals(normal_prm, views, &st);
            std::printf("map normals: %zu points, %zu short, %.3f neighbours on average\n", st.n_in, st.n_short,
                        st.n_finite ? double(st.sum_neighbors) / double(st.n_finite) : 0.0);
        }
        if (map_planes) {
            r360_sac_stats st;
            map.segmentPlanes(plane_prm, map_normals, &st);
            std::vector<r360_sac_plane> planes;
            map.getPlanes(planes);
            int largest = 0;
            for (const r360_sac_plane& p : planes) largest = std::max(largest, p.size);
            std::printf("map planes: %zu points, %zu planes, %zu points in planes, largest %d\n", st.n_in, st.n_planes,
                        st.n_in_planes, largest);
            if (!save_planes.empty()) map.savePCDPlaneLabels(save_planes, 1);
            if (remove_planes) map.removePlanes(plane_prm, map_normals);
        }
        if (map_clusters) {
            r360_cluster_stats st;
            map.cluster(cluster_prm, cluster_normals, &st);
            std::vector<r360_cluster_info> clusters;
            map.getClusters(clusters);
            std::printf("map clusters: %zu points, %zu components, %zu kept, largest %d\n", st.n_in, st.n_components,
                        st.n_clusters, clusters.empty() ? 0 : clusters[0].size);
            if (!save_clusters.empty()) map.savePCDLabels(save_clusters, 1);
        }
        if (!save_map.empty()) {
            if (map_normals && !remove_planes) {
                map.savePCDNormals(save_map, 1);
            } else {
                r360::PointCloud cloud;
                map.download(cloud);
                if (r360_pcd_write(save_map.c_str(), cloud.xyz.data(), cloud.rgba.data(), int(cloud.size()), 1, 1))
                    throw std::runtime_error("cannot write " + save_map);
            }
        }
        if (!save.empty()) optimizer.saveGraph(save);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return 0;
}
