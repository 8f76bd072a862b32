// rgbd360/rgbd360.h — C++ façade of librgbd360_hip.so with the reference's class names and method
// signatures for the registration hot path:
//
//   Calib360          include/Calib360.h:44-132
//   Frame360          include/Frame360.h:93-1150   loadFrame / undistort / stitchSphericalImage /
//                                                  buildSphereCloud / getPlanes / planes
//   RegisterPhotoICP  include/RegisterPhotoICP.h   setters :224-269, setSourceFrame/setTargetFrame
//                                                  :480-516, alignFrames360 :4519, getOptimalPose :273,
//                                                  getHessian/getGradient :279-288
//   RegisterRGBD360   include/RegisterRGBD360.h    ctor(ini) :97, setReference/setTarget :111/:161,
//                                                  RegisterPbMap :276, getPose :199, getCovMat :208,
//                                                  getInfoMat :219, calcEntropy :230, getMatchedPlanes :242,
//                                                  getAreaMatched :251, areaSource/areaTarget :91-94,
//                                                  RegisterDensePhotoICP :344, trackingScore :526,
//                                                  Register() = OdometryKeyFrame360.cpp:205-254
//   BatchRegistration  many independent pair registrations on one GPU (§8f-4): SphereGraphSLAM's
//                      tracking loop (SLAM/SphereGraphSLAM.cpp:169-231) and LoopClosure360's candidate
//                      checks (include/LoopClosure360.h:280-366)
//
// Header-only; every body is a call into the C-ABI (include/rgbd360_hip.h).  Matrices are the
// column-major Eigen layout; r360::Matrix4f / Matrix6f are minimal stand-ins with Eigen's (row, col)
// accessors and data() — define RGBD360_WITH_EIGEN to use Eigen::Matrix4f / Matrix<float,6,6>.
// Differences from the reference surface, all forced by the GPU-resident design:
//   * images are r360::Mat (rows, cols, channels, bytes) instead of cv::Mat.  Frame360::sphereRGB /
//     sphereDepth are views of the frame's sphere in HBM: RegisterPhotoICP::setSourceFrame(
//     frame->sphereRGB, frame->sphereDepth) uses the frame's device pyramid without a copy; other images
//     are uploaded and pyramided on the GPU (r360_frame_set_sphere);
//   * objects are bound to an r360::Context (one GPU + HIP stream); errors throw r360::Error.  The constructors with
//     the reference's signatures (Calib360(Resolution), RegisterPhotoICP(), RegisterRGBD360(configFile)) bind to
//     r360::default_context(): one context per host thread on device $R360_DEVICE (default 0), created on first
//     use.  include/rgbd360/compat.h brings the class names into the global namespace for unchanged call sites.
#pragma once
#include <rgbd360_hip.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <ostream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef RGBD360_WITH_EIGEN
#include <Eigen/Dense>
#endif

namespace r360 {

struct Error : std::runtime_error {
    explicit Error(const std::string& what) : std::runtime_error(what + ": " + r360_last_error()) {}
};
inline int check(int rc, const char* what) {
    if (rc < 0) throw Error(what);
    return rc;
}

#ifdef RGBD360_WITH_EIGEN
typedef Eigen::Matrix4f Matrix4f;
typedef Eigen::Matrix<float, 6, 6> Matrix6f;
typedef Eigen::Matrix4d Matrix4d;
typedef Eigen::Matrix<double, 6, 6> Matrix6d;
#else
template <typename T, int N>
struct MatrixOf;                        // the stand-in of Eigen::Matrix<T, N, N>: what cast<T>() returns
template <int N>
struct MatrixNf {                       // column-major, Eigen's (row, col) and data()
    float v[N * N];
    // currentPose.cast<double>() (KFsphere_SLAM.cpp:265, 541-550; LoopClosure360.h:318)
    template <typename T>
    typename MatrixOf<T, N>::type cast() const {
        typename MatrixOf<T, N>::type o;
        for (int i = 0; i < N * N; ++i) o.v[i] = T(v[i]);
        return o;
    }
    MatrixNf() { for (int i = 0; i < N * N; ++i) v[i] = (i % (N + 1) == 0) ? 1.f : 0.f; }
    static MatrixNf Identity() { return MatrixNf(); }
    float& operator()(int r, int c) { return v[c * N + r]; }
    float operator()(int r, int c) const { return v[c * N + r]; }
    float* data() { return v; }
    const float* data() const { return v; }
    MatrixNf operator*(const MatrixNf& b) const {
        MatrixNf o;
        for (int c = 0; c < N; ++c)
            for (int r = 0; r < N; ++r) {
                float acc = (*this)(r, 0) * b(0, c);
                for (int k = 1; k < N; ++k) acc += (*this)(r, k) * b(k, c);
                o(r, c) = acc;
            }
        return o;
    }
    // inverse by Gauss-Jordan elimination with partial pivoting in double (Eigen's Matrix4f::inverse() uses
    // cofactors in float: the two agree to float rounding)
    MatrixNf inverse() const {
        double A[N][2 * N];
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < 2 * N; ++c) A[r][c] = c < N ? (*this)(r, c) : (c - N == r ? 1.0 : 0.0);
        for (int k = 0; k < N; ++k) {
            int p = k;
            for (int r = k + 1; r < N; ++r) if (std::fabs(A[r][k]) > std::fabs(A[p][k])) p = r;
            for (int c = 0; c < 2 * N; ++c) { const double t = A[k][c]; A[k][c] = A[p][c]; A[p][c] = t; }
            const double piv = A[k][k];
            for (int c = 0; c < 2 * N; ++c) A[k][c] /= piv;
            for (int r = 0; r < N; ++r)
                if (r != k) { const double f = A[r][k]; for (int c = 0; c < 2 * N; ++c) A[r][c] -= f * A[k][c]; }
        }
        MatrixNf o;
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) o(r, c) = float(A[r][c + N]);
        return o;
    }
    // block(r0, c0, rows, cols) as a read-only view with Eigen's norm() (e.g. the translation's length,
    // rigidTransf.block(0,3,3,1).norm(), OdometryRGBD360.cpp:228)
    struct Block {
        const MatrixNf* m;
        int r0, c0, rows, cols;
        float operator()(int r, int c) const { return (*m)(r0 + r, c0 + c); }
        float norm() const {
            float s = 0.f;
            for (int c = 0; c < cols; ++c)
                for (int r = 0; r < rows; ++r) s += (*this)(r, c) * (*this)(r, c);
            return std::sqrt(s);
        }
    };
    Block block(int r0, int c0, int rows, int cols) const { return Block{this, r0, c0, rows, cols}; }
};
template <int N>
inline std::ostream& operator<<(std::ostream& os, const MatrixNf<N>& m) {
    for (int r = 0; r < N; ++r) {
        for (int c = 0; c < N; ++c) os << (c ? " " : "") << m(r, c);
        if (r + 1 < N) os << "\n";
    }
    return os;
}
// scalar * matrix (e.g. registerer.getAreaMatched() * registerer.getInfoMat(), KFsphere_SLAM.cpp:454)
template <int N>
inline MatrixNf<N> operator*(float s, const MatrixNf<N>& m) {
    MatrixNf<N> o;
    for (int i = 0; i < N * N; ++i) o.v[i] = s * m.v[i];
    return o;
}
// Eigen::Matrix<double, N, N> as the graph optimiser takes it: storage, (row, col), data() and cast
template <int N>
struct MatrixNd {
    double v[N * N];
    MatrixNd() { for (int i = 0; i < N * N; ++i) v[i] = (i % (N + 1) == 0) ? 1.0 : 0.0; }
    static MatrixNd Identity() { return MatrixNd(); }
    double& operator()(int r, int c) { return v[c * N + r]; }
    double operator()(int r, int c) const { return v[c * N + r]; }
    double* data() { return v; }
    const double* data() const { return v; }
    template <typename T>
    typename MatrixOf<T, N>::type cast() const {
        typename MatrixOf<T, N>::type o;
        for (int i = 0; i < N * N; ++i) o.v[i] = T(v[i]);
        return o;
    }
};
template <int N>
inline std::ostream& operator<<(std::ostream& os, const MatrixNd<N>& m) {
    for (int r = 0; r < N; ++r) {
        for (int c = 0; c < N; ++c) os << (c ? " " : "") << m(r, c);
        if (r + 1 < N) os << "\n";
    }
    return os;
}
template <int N> struct MatrixOf<float, N> { typedef MatrixNf<N> type; };
template <int N> struct MatrixOf<double, N> { typedef MatrixNd<N> type; };
typedef MatrixNf<4> Matrix4f;
typedef MatrixNf<6> Matrix6f;
typedef MatrixNd<4> Matrix4d;
typedef MatrixNd<6> Matrix6d;
#endif

class Frame360;

// Host image (cv::Mat stand-in: CV_8UC3 BGR sphereRGB, CV_16UC1 range-mm sphereDepth).  A Mat whose `frame`
// is set is a view of that Frame360's sphere in HBM (no host pixels until Frame360::downloadSphere()).
struct Mat {
    int rows = 0, cols = 0, channels = 1, elem = 1;   // elem: bytes per channel
    std::vector<uint8_t> bytes;
    const Frame360* frame = nullptr;
    Mat() = default;
    Mat(int r, int c, int ch, int e) : rows(r), cols(c), channels(ch), elem(e), bytes(size_t(r) * c * ch * e) {}
    uint8_t* data() { return bytes.data(); }
    const uint8_t* data() const { return bytes.data(); }
    bool empty() const { return rows == 0 || cols == 0; }
};

// Host point cloud (pcl::PointCloud<pcl::PointXYZRGBA> stand-in): xyz triples and PointXYZRGBA-packed colours
// (b | g<<8 | r<<16 | a<<24); organised when height > 1.
struct PointCloud {
    std::vector<float> xyz;             // [size][3]
    std::vector<uint32_t> rgba;         // [size]
    int width = 0, height = 0;
    size_t size() const { return rgba.size(); }
    bool empty() const { return rgba.empty(); }
    // n points, unorganised (what a filter leaves)
    void resize(size_t n) {
        xyz.resize(3 * n);
        rgba.resize(n);
        width = int(n);
        height = 1;
    }
    void clear() { resize(0); }
    // concatenation: the result is unorganised, as pcl::PointCloud::operator+= leaves it
    PointCloud& operator+=(const PointCloud& o) {
        xyz.insert(xyz.end(), o.xyz.begin(), o.xyz.end());
        rgba.insert(rgba.end(), o.rgba.begin(), o.rgba.end());
        width = int(rgba.size());
        height = 1;
        return *this;
    }
};

// Normals and curvature of a cloud, row for row (the normal_x / normal_y / normal_z / curvature of
// pcl::PointCloud<pcl::Normal>): NaN where the point was dropped or had fewer than three neighbours.
struct PointCloudNormal {
    std::vector<float> normals;         // [size][3]
    std::vector<float> curvature;       // [size]
    size_t size() const { return curvature.size(); }
    bool empty() const { return curvature.empty(); }
    void resize(size_t n) {
        normals.resize(3 * n);
        curvature.resize(n);
    }
};

// One cluster's member rows of the input cloud, ascending (pcl::PointIndices).
struct PointIndices {
    std::vector<int> indices;
};

// A model's coefficients (pcl::ModelCoefficients): a plane's a, b, c, d with a x + b y + c z + d = 0 and |abc| = 1.
struct ModelCoefficients {
    std::vector<float> values;
};

// pcl::SacModel / the sample-consensus methods SACSegmentation takes: the three plane models and RANSAC.  The other
// enumerators of PCL have no counterpart; SACSegmentation throws on any other number.
enum SacModel { SACMODEL_PLANE = 0, SACMODEL_PARALLEL_PLANE = 15, SACMODEL_PERPENDICULAR_PLANE = 9 };
enum { SAC_RANSAC = 0 };

class Context {
  public:
    explicit Context(int device = 0) { check(r360_ctx_create(device, &h_), "r360_ctx_create"); }
    ~Context() { r360_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    r360_ctx* get() const { return h_; }
    void sync() { check(r360_ctx_sync(h_), "r360_ctx_sync"); }
  private:
    r360_ctx* h_ = nullptr;
};

// The default contexts of the reference-signature constructors: one per host thread (its own HIP stream), on device
// $R360_DEVICE (default 0), created on first use.  A thread's default context lives as long as its thread or the
// last object built on it, whichever is longer: Calib360(Resolution) and the frames built on it hold a reference, so
// frames built on one thread stay valid after it exits.  RegisterRGBD360(configFile) and RegisterPhotoICP() hold
// no context of their own: each call runs on the CALLING thread's default context, so an object constructed on one
// thread and used on another (LoopClosure360's registerer, constructed by the main thread and used by its loop
// thread, LoopClosure360.h:83-94, 297) never shares a context between threads.  Frames are shared freely: a
// registration on another thread's context waits for the frames' builds on their own streams.
inline int default_device() {
    const char* e = std::getenv("R360_DEVICE");
    return e ? std::atoi(e) : 0;
}
inline const std::shared_ptr<Context>& default_context_ptr() {
    thread_local std::shared_ptr<Context> ctx = std::make_shared<Context>(default_device());
    return ctx;
}
inline Context& default_context() { return *default_context_ptr(); }

// printf-style std::string (the callers' mrpt::format for file names)
inline std::string format(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char buf[4096];
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return std::string(buf);
}
inline std::string data_dir() { return r360_data_dir(); }

// ------------------------------------------------------------------ Calib360
class Calib360 {
  public:
    // Resolution mode of the device (Calib360.h:62-67): per-sensor images of 480/res x 640/res
    enum Resolution { VGA = 1, QVGA = 2, QQVGA = 4 };
    // Calib360(Resolution res = QVGA) (Calib360.h:70), on the thread's default context
    explicit Calib360(Resolution res = QVGA) : Calib360(default_context(), 480 / int(res), 640 / int(res)) {
        keep_ = default_context_ptr();
    }
    // rows x cols per sensor (the reference's QVGA default, Calib360.h:73-77)
    explicit Calib360(Context& ctx, int rows = 240, int cols = 320) : ctx_(ctx) {
        check(r360_calib_create(ctx.get(), rows, cols, &h_), "r360_calib_create");
        resolution = Resolution(cols > 0 && 640 % cols == 0 ? 640 / cols : 0);
    }
    ~Calib360() { r360_calib_destroy(h_); }
    Calib360(const Calib360&) = delete;
    Calib360& operator=(const Calib360&) = delete;
    // "" = the shipped calibration (data/calib/Extrinsics), as the reference's default argument (Calib360.h:122-125)
    void loadExtrinsicCalibration(const std::string& dir = "") {
        check(r360_calib_load_extrinsics(h_, dir.c_str()), "loadExtrinsicCalibration");
    }
    // "" = data/calib/Intrinsics (Calib360.h:104-107)
    void loadIntrinsicCalibration(const std::string& dir = "") {
        check(r360_calib_load_intrinsics(h_, dir.c_str()), "loadIntrinsicCalibration");
    }
    Resolution resolution;
    Matrix4f getRt_id(int sensor_id) const {
        float rt[128];
        check(r360_calib_get_extrinsics(h_, rt, nullptr, nullptr), "getRt_id");
        Matrix4f m;
        std::memcpy(m.data(), rt + 16 * sensor_id, sizeof(float) * 16);
        return m;
    }
    r360_calib* get() const { return h_; }
    Context& ctx() const { return ctx_; }
    // the default context this calibration was built on (null for an explicit Context)
    const std::shared_ptr<Context>& keepAlive() const { return keep_; }
  private:
    Context& ctx_;
    std::shared_ptr<Context> keep_;
    r360_calib* h_ = nullptr;
};

// ------------------------------------------------------------------ Frame360
struct Plane {                          // mrpt::pbmap::Plane fields used on the path
    float v3normal[3], v3center[3], d, areaHull, elongation, curvature, v3PpalDir[3], v3colorNrgb[3],
        dominantIntensity;
    unsigned id;
    int sensor;
    size_t n_inliers;
    std::vector<float> polygonContour;  // closed hull polygon, xyz triples
    std::string label;                  // Plane::label (labelization tools), kept by savePlanes
};

// mrpt::pbmap::PbMap as Frame360::planes holds it (Frame360.h:123): the planes in vPlanes (callers write
// frame360->planes.vPlanes[i], OnlineOdometryRGBD360.cpp:172,330); size() / operator[] / iteration forward to it
struct PbMap {
    std::vector<Plane> vPlanes;
    size_t size() const { return vPlanes.size(); }
    bool empty() const { return vPlanes.empty(); }
    Plane& operator[](size_t i) { return vPlanes[i]; }
    const Plane& operator[](size_t i) const { return vPlanes[i]; }
    std::vector<Plane>::iterator begin() { return vPlanes.begin(); }
    std::vector<Plane>::iterator end() { return vPlanes.end(); }
    std::vector<Plane>::const_iterator begin() const { return vPlanes.begin(); }
    std::vector<Plane>::const_iterator end() const { return vPlanes.end(); }
};

class Frame360 {
  public:
    explicit Frame360(Calib360* calib_) : calib(calib_), keep_(calib_->keepAlive()) {
        check(r360_frame_create(calib->ctx().get(), calib->get(), &h_), "r360_frame_create");
        int r, c, sr, sc;
        check(r360_frame_dims(h_, &r, &c, &sr, &sc), "r360_frame_dims");
        sphereRGB.rows = sphereDepth.rows = sr;
        sphereRGB.cols = sphereDepth.cols = sc;
        sphereRGB.channels = 3; sphereRGB.elem = 1;
        sphereDepth.channels = 1; sphereDepth.elem = 2;
        sphereRGB.frame = sphereDepth.frame = this;
    }
    ~Frame360() { r360_frame_destroy(h_); }
    Frame360(const Frame360&) = delete;
    Frame360& operator=(const Frame360&) = delete;

    void loadFrame(const std::string& path) { check(r360_frame_load_bin(h_, path.c_str()), "loadFrame"); }
    void upload(const uint8_t* bgr8, const uint16_t* depth8) { check(r360_frame_upload(h_, bgr8, depth8), "upload"); }
    void undistort() { check(r360_frame_build(h_, R360_BUILD_UNDISTORT), "undistort"); }
    void stitchSphericalImage() {
        std::lock_guard<std::mutex> lk(build_m_);
        check(r360_frame_build(h_, R360_BUILD_SPHERE | R360_BUILD_PYRAMID), "stitch");
    }
    void buildSphereCloud() { check(r360_frame_build(h_, R360_BUILD_UNDISTORT | R360_BUILD_CLOUD), "buildSphereCloud"); }
    void getPlanes() {
        check(r360_frame_build(h_, R360_BUILD_UNDISTORT | R360_BUILD_PLANES), "getPlanes");
        fetch_planes();
    }
    // getLocalPlanes (GetControlPlanes.cpp:345): getPlanes that also keeps each sensor's planes as they were before
    // groupPlanes, for ControlPlanes::collect
    void getLocalPlanes() {
        check(r360_frame_build(h_, R360_BUILD_UNDISTORT | R360_BUILD_PLANES | R360_BUILD_LOCAL_PLANES), "getLocalPlanes");
        fetch_planes();
    }
    // ---- keyframe persistence (Frame360.h:181-228, 312-345)
    void serialize(const std::string& fileName) { check(r360_frame_save_bin(h_, fileName.c_str()), "serialize"); }
    void setTimeStamp(uint64_t t) { check(r360_frame_set_timestamp(h_, t), "setTimeStamp"); }
    uint64_t timeStamp() const { uint64_t t = 0; check(r360_frame_get_timestamp(h_, &t), "timeStamp"); return t; }
    void loadCloud(const std::string& pointCloudPath) { check(r360_frame_load_cloud(h_, pointCloudPath.c_str()), "loadCloud"); }
    void loadPbMap(const std::string& pbmapPath) {
        check(r360_frame_load_pbmap(h_, pbmapPath.c_str()), "loadPbMap");
        fetch_planes();
    }
    void load_PbMap_Cloud(const std::string& pointCloudPath, const std::string& pbmapPath) {
        loadCloud(pointCloudPath);
        loadPbMap(pbmapPath);
    }
    void load_PbMap_Cloud(const std::string& path, unsigned index) {
        check(r360_frame_load_pbmap_cloud(h_, path.c_str(), index), "load_PbMap_Cloud");
        fetch_planes();
    }
    // labels edited in `planes` are written with the map
    void savePlanes(const std::string& pathPbMap) {
        push_labels();
        check(r360_frame_save_planes(h_, pathPbMap.c_str()), "savePlanes");
    }
    void save(const std::string& path, unsigned frame) {
        push_labels();
        check(r360_frame_save(h_, path.c_str(), frame), "save");
    }
    // sphereCloud as xyz triples + PointXYZRGBA-packed colours
    void sphereCloud(std::vector<float>& xyz, std::vector<uint32_t>& rgba, int& width, int& height) {
        check(r360_frame_get_sphere_cloud(h_, nullptr, nullptr, 0, &width, &height), "sphereCloud");
        const size_t n = size_t(width) * size_t(height);
        xyz.resize(3 * n);
        rgba.resize(n);
        check(r360_frame_get_sphere_cloud(h_, xyz.data(), rgba.data(), n, &width, &height), "sphereCloud");
    }
    void sphereCloud(PointCloud& cloud) { sphereCloud(cloud.xyz, cloud.rgba, cloud.width, cloud.height); }
    // Frame360::getPlanarArea (Frame360.h:157)
    float getPlanarArea() const {
        float a = 0.f;
        for (const Plane& p : planes) a += p.areaHull;
        return a;
    }
    // sphereRGB / sphereDepth (Frame360.h:104-107): views of the stitched sphere in HBM
    Mat sphereRGB, sphereDepth;
    // copies the sphere's pixels into sphereRGB / sphereDepth (they stay views of this frame)
    void downloadSphere() {
        ensureSpherePyramid();
        sphereRGB.bytes.resize(size_t(sphereRGB.rows) * sphereRGB.cols * 3);
        sphereDepth.bytes.resize(size_t(sphereDepth.rows) * sphereDepth.cols * 2);
        check(r360_frame_get_sphere(h_, sphereRGB.data(), reinterpret_cast<uint16_t*>(sphereDepth.data())),
              "downloadSphere");
    }
    PbMap planes;                       // the frame's PbMap (planes.vPlanes)
    Matrix4f pose;
    unsigned id = 0;
    unsigned node = 0;                  // topological node (submap) of the frame (Frame360.h:101)
    Calib360* calib;                    // the sensor calibration (Frame360.h:97)
    r360_frame* get() const { return h_; }
    // the stitched sphere and its pyramid, built once (stitchSphericalImage, or the first setSourceFrame /
    // setTargetFrame of the frame's sphere views, possibly from another thread)
    void ensureSpherePyramid() {
        std::lock_guard<std::mutex> lk(build_m_);
        unsigned built = 0;
        check(r360_frame_built(h_, &built), "r360_frame_built");
        const unsigned need = R360_BUILD_SPHERE | R360_BUILD_PYRAMID;   // the stitch reads the raw depth
        if ((built & need) != need) check(r360_frame_build(h_, need), "pyramid");
    }

  private:
    void push_labels() {
        for (size_t i = 0; i < planes.size(); ++i)
            check(r360_frame_set_plane_label(h_, int(i), planes[i].label.c_str()), "plane label");
    }
    void fetch_planes() {
        int n = 0;
        check(r360_frame_get_planes(h_, nullptr, 0, &n), "getPlanes");
        std::vector<r360_plane> raw(n > 0 ? n : 1);
        check(r360_frame_get_planes(h_, raw.data(), n, &n), "getPlanes");
        planes.vPlanes.clear();
        for (int i = 0; i < n; ++i) {
            const r360_plane& r = raw[i];
            Plane p;
            std::memcpy(p.v3normal, r.normal, sizeof p.v3normal);
            std::memcpy(p.v3center, r.center, sizeof p.v3center);
            std::memcpy(p.v3PpalDir, r.ppal, sizeof p.v3PpalDir);
            std::memcpy(p.v3colorNrgb, r.nrgb, sizeof p.v3colorNrgb);
            p.d = r.d; p.areaHull = r.area; p.elongation = r.elongation; p.curvature = r.curvature;
            p.dominantIntensity = r.intensity; p.id = unsigned(r.id); p.sensor = r.sensor;
            p.n_inliers = size_t(r.n_inliers);
            p.polygonContour.resize(3 * size_t(r.n_hull));
            int m = 0;
            check(r360_frame_get_plane_hull(h_, i, p.polygonContour.data(), r.n_hull, &m), "getPlanes");
            const int ll = r360_frame_get_plane_label(h_, i, nullptr, 0);
            if (ll > 0) {
                std::vector<char> buf(size_t(ll) + 1);
                r360_frame_get_plane_label(h_, i, buf.data(), ll + 1);
                p.label = buf.data();
            }
            planes.vPlanes.push_back(p);
        }
    }
    std::shared_ptr<Context> keep_;     // the default context the frame was built on (see default_context_ptr)
    std::mutex build_m_;
    r360_frame* h_ = nullptr;
};

// ------------------------------------------------------------------ RegisterPhotoICP
class RegisterPhotoICP {
  public:
    enum costFuncType { PHOTO_CONSISTENCY = 0, DEPTH_CONSISTENCY = 1, PHOTO_DEPTH = 2 };
    explicit RegisterPhotoICP(Context& ctx) : ctx_(&ctx) { r360_icp_default_params(&p_); }
    // RegisterPhotoICP() (RegisterPhotoICP.h:201): every call on the calling thread's default context
    RegisterPhotoICP() { r360_icp_default_params(&p_); }
    ~RegisterPhotoICP() {
        for (auto& o : own_) { r360_frame_destroy(o.frame); r360_calib_destroy(o.calib); }
    }
    RegisterPhotoICP(const RegisterPhotoICP&) = delete;
    RegisterPhotoICP& operator=(const RegisterPhotoICP&) = delete;
    void setNumPyr(int n) { p_.n_pyr = n; }
    void setMinDepth(float d) { p_.min_depth = d; }
    void setMaxDepth(float d) { p_.max_depth = d; }
    void setGrayVariance(float s) { p_.std_dev_photo = s; }   // sets stdDevPhoto (RegisterPhotoICP.h:242-245)
    void setDepthVariance(float s) { p_.std_dev_depth = s; }
    void useSaliency(bool b) {           // the sphere path never subsamples (the saliency code is commented out)
        if (b) throw std::invalid_argument("useSaliency(true) is not supported on the spherical path");
    }
    void setVisualization(bool) {}      // visualizeIterations: OpenCV windows, no display here
    void setSourceFrame(Frame360& f) { ensure_pyramid(f); src_ = f.get(); }
    void setTargetFrame(Frame360& f) { ensure_pyramid(f); trg_ = f.get(); }
    // setSourceFrame / setTargetFrame(cv::Mat& imgRGB, cv::Mat& imgDepth) (:480-516): a frame's own
    // sphereRGB / sphereDepth use its device pyramid; other images (BGR u8, range u16 mm) are uploaded
    void setSourceFrame(Mat& imgRGB, Mat& imgDepth) { src_ = sphere_frame(0, imgRGB, imgDepth); }
    void setTargetFrame(Mat& imgRGB, Mat& imgDepth) { trg_ = sphere_frame(1, imgRGB, imgDepth); }
    // benchmark timing mode: exactly K level-0 iterations (0 = reference schedule)
    void setFixedIterationsLevel0(int k) { p_.fixed_iters_level0 = k; }
    // returns false where the reference prints "ILL-POSED" and returns early (:4682-4690)
    bool alignFrames360(const Matrix4f& pose_guess = Matrix4f::Identity(), costFuncType method = PHOTO_CONSISTENCY,
                        int occlusion = 0) {
        float g[6];
        const int rc = check(r360_align360(ctx().get(), trg_, src_, pose_guess.data(), method, occlusion,
                                           &p_, relPose_.data(), hessian_.data(), g, &st_),
                             "alignFrames360");
        std::memcpy(gradient_, g, sizeof g);
        SSO = st_.sso;
        // the residual members keep their previous value unless the error function assigns them (:183-189)
        if (st_.residuals_set & 1) { avPhotoResidual = st_.av_photo_residual; avDepthResidual = st_.av_depth_residual; }
        if (st_.residuals_set & 2) avResidual = st_.av_residual;
        return rc == 0;
    }
    Matrix4f getOptimalPose() const { return relPose_; }
    Matrix6f getHessian() const { return hessian_; }
    const float* getGradient() const { return gradient_; }
    float SSO = 0.f;
    // public residual members (RegisterPhotoICP.h:183-189; uninitialised in the reference until assigned)
    float avResidual = std::numeric_limits<float>::quiet_NaN();
    double avPhotoResidual = std::numeric_limits<double>::quiet_NaN();
    double avDepthResidual = std::numeric_limits<double>::quiet_NaN();
    const r360_icp_stats& stats() const { return st_; }
    r360_icp_params& params() { return p_; }
  private:
    Context& ctx() const { return ctx_ ? *ctx_ : default_context(); }
    static void ensure_pyramid(Frame360& f) { f.ensureSpherePyramid(); }
    r360_frame* sphere_frame(int role, Mat& rgb, Mat& depth) {
        if (rgb.frame && rgb.frame == depth.frame) {       // the frame's own sphere views
            Frame360& f = const_cast<Frame360&>(*rgb.frame);
            ensure_pyramid(f);
            return f.get();
        }
        if (rgb.channels != 3 || rgb.elem != 1 || depth.channels != 1 || depth.elem != 2 || rgb.rows != depth.rows ||
            rgb.cols != depth.cols || rgb.bytes.size() < size_t(rgb.rows) * rgb.cols * 3 ||
            depth.bytes.size() < size_t(depth.rows) * depth.cols * 2)
            throw std::invalid_argument("sphere images: BGR u8 x 3 and range u16 of the same size");
        Own* o = nullptr;
        for (auto& x : own_)
            if (x.role == role && x.rows == rgb.rows && x.cols == rgb.cols) o = &x;
        if (!o) {
            own_.push_back(Own{role, rgb.rows, rgb.cols, nullptr, nullptr, ctx_ ? nullptr : default_context_ptr()});
            o = &own_.back();
            check(r360_calib_create_sphere(ctx().get(), rgb.rows, rgb.cols, &o->calib), "sphere calibration");
            check(r360_frame_create(ctx().get(), o->calib, &o->frame), "sphere frame");
        }
        check(r360_frame_set_sphere(o->frame, rgb.data(), reinterpret_cast<const uint16_t*>(depth.data()), rgb.rows,
                                    rgb.cols), "setSourceFrame / setTargetFrame");
        return o->frame;
    }
    struct Own { int role, rows, cols; r360_calib* calib; r360_frame* frame; std::shared_ptr<Context> keep; };
    std::vector<Own> own_;
    Context* ctx_ = nullptr;            // null: the calling thread's default context
    r360_icp_params p_;
    r360_icp_stats st_{};
    r360_frame* src_ = nullptr;
    r360_frame* trg_ = nullptr;
    Matrix4f relPose_;
    Matrix6f hessian_;
    float gradient_[6] = {0, 0, 0, 0, 0, 0};
};

// ------------------------------------------------------------------ RegisterRGBD360
class RegisterRGBD360 {
  public:
    enum registrationType { DEFAULT_6DoF = 0, PLANAR_3DoF = 1, ODOMETRY_6DoF = 2, PLANAR_ODOMETRY_3DoF = 3 };
    // matcher.configLocaliser.load_params(configFile) (:97-100): the [global]/[unary]/[binary] thresholds of
    // the mrpt-pbmap ini; without a file, configLocaliser_sphericalOdometry.ini's values
    // RegisterRGBD360(configFile) (RegisterRGBD360.h:97), on the thread's default context
    // every call on the calling thread's default context
    explicit RegisterRGBD360(const std::string& configFile = "") : config_(configFile) { init(); }
    RegisterRGBD360(Context& ctx, const std::string& configFile = "") : ctx_(&ctx), config_(configFile) { init(); }
    r360_match_params& matchParams() { return match_; }
    void setReference(Frame360* ref, size_t max_match_planes = 0) { ref_ = ref; max_ = max_match_planes; done_ = false; }
    void setTarget(Frame360* trg, size_t max_match_planes = 0) { trg_ = trg; max_ = max_match_planes; done_ = false; }
    bool RegisterPbMap(Frame360* frame1 = nullptr, Frame360* frame2 = nullptr, size_t max_match_planes = 0,
                       registrationType registMode = DEFAULT_6DoF) {
        if (frame1) setReference(frame1, max_match_planes);
        if (frame2) setTarget(frame2, max_match_planes);
        mode_ = registMode;
        done_ = true;
        std::vector<int> pairs(512);
        int n = 0;
        check(r360_ctx_set_match_params(ctx().get(), &match_), "matcher thresholds");
        const int rc = check(r360_register_pbmap(ctx().get(), ref_->get(), trg_->get(), max_, registMode,
                                                 rigidTransf_.data(), informationM_.data(), pairs.data(), 256, &n,
                                                 &areaMatched_, &areaSource, &areaTarget),
                             "RegisterPbMap");
        bestMatch_.clear();
        for (int k = 0; k < n && k < 256; ++k) bestMatch_[unsigned(pairs[2 * k])] = unsigned(pairs[2 * k + 1]);
        return rc == 1;                 // false leaves rigidTransf untouched (RegisterRGBD360.h:306-310)
    }
    Matrix4f getPose() { if (!done_) RegisterPbMap(); return rigidTransf_; }
    Matrix6f& getInfoMat() { if (!done_) RegisterPbMap(); return informationM_; }
    // covarianceM = informationM.inverse() (:208-215)
    Matrix6f getCovMat() {
        if (!done_) RegisterPbMap();
        return inverse6(informationM_);
    }
    // differential entropy of the matched planes' Gaussian, 0.5 (DOF (1 + log 2 pi) + log det cov) (:230-238)
    float calcEntropy() {
        const Matrix6f cov = getCovMat();
        double A[36];
        for (int i = 0; i < 36; ++i) A[i] = cov.data()[i];
        return float(0.5 * (6 * (1 + std::log(2 * 3.14159265359)) + std::log(float(det6(A)))));
    }
    // tracking quality from the matched-area ratio (:526-540): 0 GOOD (>= 0.7), 1 WEAK (>= 0.3), 2 BAD
    int trackingScore(float& score) {
        score = getAreaMatched() / areaSource;
        if (score >= 0.7) return 0;
        if (score >= 0.3) return 1;
        return 2;
    }
    std::map<unsigned, unsigned> getMatchedPlanes() { if (!done_) RegisterPbMap(); return bestMatch_; }
    float getAreaMatched() { if (!done_) RegisterPbMap(); return areaMatched_; }
    // Register(): PbMap -> rotOffset conjugation -> alignFrames360 -> back (OdometryKeyFrame360.cpp:205-254);
    // guess is used when the PbMap stage fails.  Returns true when the PbMap stage succeeded.
    bool Register(Frame360* frame1, Frame360* frame2, const r360_icp_params& icp, Matrix4f& pose,
                  const Matrix4f& guess = Matrix4f::Identity(), size_t max_match_planes = 25,
                  registrationType registMode = PLANAR_3DoF) {
        r360_icp_stats st;
        check(r360_ctx_set_match_params(ctx().get(), &match_), "matcher thresholds");
        const int rc = check(r360_register(ctx().get(), frame1->get(), frame2->get(), guess.data(), &icp,
                                           max_match_planes, registMode, pose.data(), informationM_.data(), &st),
                             "Register");
        return rc == 0;
    }
    // RegisterDensePhotoICP (RegisterRGBD360.h:344-520): frame2's 8 sensor images aligned to frame1's, the
    // Jacobians in the rig frame (calcPhotoICPError_robot / calcHessianGradient_robot).  As in the reference,
    // rigidTransf = pose_estim and informationM = the last level's Hessian; false = ILL-POSED.
    bool RegisterDensePhotoICP(Frame360* frame1, Frame360* frame2, Matrix4f pose_estim = Matrix4f::Identity(),
                               RegisterPhotoICP::costFuncType method = RegisterPhotoICP::PHOTO_CONSISTENCY,
                               registrationType registMode = DEFAULT_6DoF) {
        check(r360_frame_build(frame1->get(), R360_BUILD_SENSOR_PYRAMID), "setTargetFrame (sensor pyramids)");
        check(r360_frame_build(frame2->get(), R360_BUILD_SENSOR_PYRAMID), "setSourceFrame (sensor pyramids)");
        const int rc = check(r360_register_dense(ctx().get(), frame1->get(), frame2->get(), pose_estim.data(), method,
                                                 registMode, nullptr, rigidTransf_.data(), informationM_.data(),
                                                 &dense_st_),
                             "RegisterDensePhotoICP");
        done_ = true;                   // bRegistrationDone (:509)
        return rc == 1;
    }
    const r360_dense_stats& denseStats() const { return dense_st_; }
    float areaSource = 0.f, areaTarget = 0.f;
  private:
    void init() {
        std::memset(informationM_.data(), 0, sizeof(float) * 36);
        r360_match_params_default(&match_);
        if (!config_.empty()) check(r360_match_params_load_ini(config_.c_str(), &match_), "load_params");
    }
    Context& ctx() const { return ctx_ ? *ctx_ : default_context(); }
    r360_dense_stats dense_st_{};
    Context* ctx_ = nullptr;            // null: the calling thread's default context
    std::string config_;
    Frame360* ref_ = nullptr;
    Frame360* trg_ = nullptr;
    size_t max_ = 0;
    int mode_ = DEFAULT_6DoF;
    bool done_ = false;
    Matrix4f rigidTransf_;
    Matrix6f informationM_;
    std::map<unsigned, unsigned> bestMatch_;
    float areaMatched_ = 0.f;
    r360_match_params match_{};
    // 6x6 inverse / determinant by Gaussian elimination with partial pivoting (double)
    static double det6(double A[36]) {
        double d = 1.0;
        for (int k = 0; k < 6; ++k) {
            int p = k;
            for (int r = k + 1; r < 6; ++r) if (std::fabs(A[r * 6 + k]) > std::fabs(A[p * 6 + k])) p = r;
            if (A[p * 6 + k] == 0) return 0.0;
            if (p != k) { for (int c = 0; c < 6; ++c) std::swap(A[k * 6 + c], A[p * 6 + c]); d = -d; }
            d *= A[k * 6 + k];
            for (int r = k + 1; r < 6; ++r) {
                const double f = A[r * 6 + k] / A[k * 6 + k];
                for (int c = k; c < 6; ++c) A[r * 6 + c] -= f * A[k * 6 + c];
            }
        }
        return d;
    }
    static Matrix6f inverse6(const Matrix6f& M) {
        double A[6][12];
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 12; ++c) A[r][c] = c < 6 ? M(r, c) : (c - 6 == r ? 1.0 : 0.0);
        for (int k = 0; k < 6; ++k) {
            int p = k;
            for (int r = k + 1; r < 6; ++r) if (std::fabs(A[r][k]) > std::fabs(A[p][k])) p = r;
            for (int c = 0; c < 12; ++c) std::swap(A[k][c], A[p][c]);
            const double piv = A[k][k];
            for (int c = 0; c < 12; ++c) A[k][c] /= piv;
            for (int r = 0; r < 6; ++r)
                if (r != k) { const double f = A[r][k]; for (int c = 0; c < 12; ++c) A[r][c] -= f * A[k][c]; }
        }
        Matrix6f out;
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) out(r, c) = float(A[r][c + 6]);
        return out;
    }
};

// ------------------------------------------------------------------ batched registrations (§8f-4)
// Worker lanes (own HIP streams and ICP state) run the pairs of one call concurrently; each pair is the
// single-pair code path, so results equal sequential RegisterRGBD360 / RegisterPhotoICP calls.
class BatchRegistration {
  public:
    BatchRegistration(int device = 0, int lanes = 8) { check(r360_batch_create(device, lanes, &h_), "r360_batch_create"); }
    // the matcher thresholds of every lane (e.g. RegisterRGBD360::matchParams() of an ini file)
    void setMatchParams(const r360_match_params& m) { check(r360_batch_set_match_params(h_, &m), "setMatchParams"); }
    ~BatchRegistration() { r360_batch_destroy(h_); }
    BatchRegistration(const BatchRegistration&) = delete;
    BatchRegistration& operator=(const BatchRegistration&) = delete;
    // generic jobs: RegisterPbMap(ref, trg) and the dense stage each job asks for (R360_JOB_*)
    std::vector<r360_pair_result> registerPairs(const std::vector<r360_pair_job>& jobs, size_t max_match_planes,
                                                RegisterRGBD360::registrationType mode, const r360_icp_params* icp,
                                                int min_matches = 0, float min_area = 0.f) {
        std::vector<r360_pair_result> out(jobs.size());
        check(r360_batch_register(h_, jobs.data(), int(jobs.size()), max_match_planes, mode, min_matches, min_area,
                                  icp, out.data()),
              "registerPairs");
        return out;
    }
    // SphereGraphSLAM tracking step: keyframes oldest first; returns the index of the keyframe the sequential
    // loop registers against (-1: "No registration available"), its result in *winner
    int track(const std::vector<Frame360*>& keyframes, Frame360* frame, r360_pair_result* winner = nullptr,
              int numCheckRegistration = 5, int noAssoc_threshold = 40, size_t max_match_planes = 25,
              RegisterRGBD360::registrationType mode = RegisterRGBD360::PLANAR_ODOMETRY_3DoF) {
        std::vector<r360_frame*> kf;
        for (auto f : keyframes) kf.push_back(f->get());
        int chosen = -1;
        check(r360_track_frame(h_, kf.data(), int(kf.size()), frame->get(), numCheckRegistration, noAssoc_threshold,
                               max_match_planes, mode, &chosen, winner, nullptr),
              "track");
        return chosen;
    }
    // LoopClosure360 candidate checks: RegisterPbMap PLANAR_3DoF, gate n_match > minMatchesThreshold and
    // area_matched > areaThreshold (LoopClosure360.h:114-115), then alignFrames360 (keyframe as source,
    // :309-313) of the pairs that pass
    std::vector<r360_pair_result> loopClosures(const std::vector<std::pair<Frame360*, Frame360*> >& pairs,
                                               const r360_icp_params& icp, int minMatchesThreshold = 5,
                                               float areaThreshold = 15.f) {
        std::vector<r360_pair_job> jobs(pairs.size());
        for (size_t i = 0; i < pairs.size(); ++i) {
            std::memset(&jobs[i], 0, sizeof(r360_pair_job));
            jobs[i].ref = pairs[i].first->get();
            jobs[i].trg = pairs[i].second->get();
            jobs[i].dense = R360_JOB_GATED;
            jobs[i].ref_is_source = 1;
        }
        return registerPairs(jobs, 25, RegisterRGBD360::PLANAR_3DoF, &icp, minMatchesThreshold, areaThreshold);
    }
    r360_batch* get() const { return h_; }
  private:
    r360_batch* h_ = nullptr;
};

// ------------------------------------------------------------------ point-cloud filters (FilterPointCloud.h)
// pcl::transformPointCloud(in, out, T): m(k,0)*x + m(k,1)*y + m(k,2)*z + m(k,3) per component in float, left to
// right and never contracted into FMAs; a point with a non-finite coordinate stays as it is (non-dense clouds).
#if defined(__clang__)
#define R360_NO_FP_CONTRACT
#elif defined(__GNUC__)
#define R360_NO_FP_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define R360_NO_FP_CONTRACT
#endif
R360_NO_FP_CONTRACT inline void transformPointCloud(const PointCloud& in, PointCloud& out, const Matrix4f& T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (&in != &out) { out.rgba = in.rgba; out.width = in.width; out.height = in.height; out.xyz.resize(in.xyz.size()); }
    const float* m = T.data();   // column-major
    for (size_t i = 0; i < in.size(); ++i) {
        const float x = in.xyz[3 * i], y = in.xyz[3 * i + 1], z = in.xyz[3 * i + 2];
        float* o = &out.xyz[3 * i];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { o[0] = x; o[1] = y; o[2] = z; continue; }
        for (int k = 0; k < 3; ++k) {
            float a = m[k] * x;
            a = a + m[4 + k] * y;
            a = a + m[8 + k] * z;
            o[k] = a + m[12 + k];
        }
    }
}

// FilterPointCloud (include/FilterPointCloud.h) with the reference's constructor defaults: filterEuclidean works
// on the cloud in place, on the host, and leaves it unorganised; filterVoxel (pcl::VoxelGrid with leaf voxelSize)
// runs on the GPU of the calling thread's default context, or of the Context given to the second constructor, and
// leaves one point per occupied voxel in ascending (k, j, i) voxel order (r360_cloud_filter_voxel).
class FilterPointCloud {
  public:
    FilterPointCloud(const float voxelSize = 0.05f, const float euclideanBox = 4.0f)
        : voxel_(voxelSize), box_(euclideanBox) {}
    FilterPointCloud(Context& ctx, const float voxelSize = 0.05f, const float euclideanBox = 4.0f)
        : ctx_(&ctx), voxel_(voxelSize), box_(euclideanBox) {}
    void filterEuclidean(PointCloud& cloud) {
        size_t n = 0;
        check(r360_cloud_filter_euclidean(cloud.xyz.data(), cloud.rgba.data(), cloud.size(), -2.0f, 1.0f, box_,
                                          cloud.xyz.data(), cloud.rgba.data(), &n),
              "filterEuclidean");
        cloud.resize(n);
    }
    // false: PCL's size guard refused the leaf ("Leaf size is too small for the input dataset"), the cloud is unchanged
    bool filterVoxel(PointCloud& cloud) {
        size_t n = 0;
        Context& c = ctx_ ? *ctx_ : default_context();
        const int rc = check(r360_cloud_filter_voxel(c.get(), cloud.xyz.data(), cloud.rgba.data(), cloud.size(), voxel_,
                                                     cloud.xyz.data(), cloud.rgba.data(), cloud.size(), &n),
                             "filterVoxel");
        if (rc == 0) cloud.resize(n);
        return rc == 0;
    }
    // pcl::StatisticalOutlierRemoval (setMeanK, setStddevMulThresh) on the GPU, in place, order kept; a point with fewer
    // than meanK other points within maxDist is removed and takes no part in the statistics (r360_cloud_filter_outliers)
    void filterStatistical(PointCloud& cloud, int meanK = 20, float stddevMul = 1.f, float maxDist = 0.5f,
                           r360_outlier_stats* stats = nullptr) {
        r360_outlier_params p;
        r360_outlier_default_params(&p);
        p.kind = R360_OUTLIER_STATISTICAL;
        p.mean_k = meanK;
        p.stddev_mul = stddevMul;
        p.max_dist = maxDist;
        filterOutliers(cloud, p, stats, "filterStatistical");
    }
    // pcl::RadiusOutlierRemoval (setRadiusSearch, setMinNeighborsInRadius) on the GPU, in place, order kept
    void filterRadius(PointCloud& cloud, float radius = 0.15f, int minNeighbors = 5, r360_outlier_stats* stats = nullptr) {
        r360_outlier_params p;
        r360_outlier_default_params(&p);
        p.kind = R360_OUTLIER_RADIUS;
        p.radius = radius;
        p.min_neighbors = minNeighbors;
        filterOutliers(cloud, p, stats, "filterRadius");
    }
    float voxelSize() const { return voxel_; }
  private:
    void filterOutliers(PointCloud& cloud, const r360_outlier_params& p, r360_outlier_stats* stats, const char* what) {
        size_t n = 0;
        Context& c = ctx_ ? *ctx_ : default_context();
        check(r360_cloud_filter_outliers(c.get(), cloud.xyz.data(), cloud.rgba.data(), cloud.size(), &p, cloud.xyz.data(),
                                         cloud.rgba.data(), cloud.size(), &n, stats),
              what);
        cloud.resize(n);
    }
    Context* ctx_ = nullptr;
    float voxel_, box_;
};

// A view of a context's global map (r360_ctx_map_*): `globalMap += cloud; filter.filterVoxel(globalMap)` of
// SLAM/SphereGraphSLAM.cpp:136-137, :208-209 with the map resident in HBM.  The map belongs to the context and is
// freed with it; the view owns nothing on the device (its destructor makes no GPU call) and keeps the default
// context alive while it exists.
class GlobalMap360 {
  public:
    explicit GlobalMap360(const float voxelSize = 0.05f, const float euclideanBox = 4.0f)
        : keep_(default_context_ptr()), ctx_(keep_.get()), voxel_(voxelSize), box_(euclideanBox) {}
    explicit GlobalMap360(Context& ctx, const float voxelSize = 0.05f, const float euclideanBox = 4.0f)
        : ctx_(&ctx), voxel_(voxelSize), box_(euclideanBox) {}
    void reset() { check(r360_ctx_map_reset(ctx_->get()), "GlobalMap360::reset"); }
    // the whole map step on the keyframe's cloud in HBM: filterEuclidean, transformPointCloud(pose), +=, filterVoxel
    bool add(Frame360& keyframe, const Matrix4f& pose);
    // globalMap += cloud; filterVoxel(globalMap)
    bool add(const PointCloud& cloud) {
        return check(r360_ctx_map_add_cloud(ctx_->get(), cloud.xyz.data(), cloud.rgba.data(), cloud.size(), voxel_),
                     "GlobalMap360::add") == 0;
    }
    size_t size() const {
        size_t n = 0;
        check(r360_ctx_map_size(ctx_->get(), &n), "GlobalMap360::size");
        return n;
    }
    void download(PointCloud& cloud) const {
        size_t n = size();
        cloud.resize(n);
        check(r360_ctx_map_download(ctx_->get(), cloud.xyz.data(), cloud.rgba.data(), n, &n), "GlobalMap360::download");
    }
    // the statistical or the radius outlier filter on the map where it lies (r360_ctx_map_filter_outliers): the map stays
    // in ascending voxel order and add / size / download go on from the result
    void removeOutliers(const r360_outlier_params& params, r360_outlier_stats* stats = nullptr) {
        check(r360_ctx_map_filter_outliers(ctx_->get(), &params, stats), "GlobalMap360::removeOutliers");
    }
    // normals and curvature of the map where it lies (r360_ctx_map_estimate_normals), each turned towards the nearest
    // of `viewpoints` (xyz triples: the keyframe positions); they stay on the GPU, valid until the map next changes
    void estimateNormals(const r360_normal_params& params, const std::vector<float>& viewpoints,
                         r360_normal_stats* stats = nullptr) {
        check(r360_ctx_map_estimate_normals(ctx_->get(), &params, viewpoints.data(), int(viewpoints.size() / 3), stats),
              "GlobalMap360::estimateNormals");
    }
    // the map's normals in the order of download(); throws when the map changed since estimateNormals
    void getNormals(PointCloudNormal& out) const {
        size_t n = 0;
        check(r360_ctx_map_download_normals(ctx_->get(), nullptr, nullptr, 0, &n), "GlobalMap360::getNormals");
        out.resize(n);
        check(r360_ctx_map_download_normals(ctx_->get(), out.normals.data(), out.curvature.data(), n, &n),
              "GlobalMap360::getNormals");
    }
    // the map with its normals as a PointXYZRGBNormal file (r360_pcd_write_normals; mode as r360_pcd_write)
    void savePCDNormals(const std::string& path, int mode = 0) const {
        PointCloud cloud;
        PointCloudNormal nrm;
        download(cloud);
        getNormals(nrm);
        check(r360_pcd_write_normals(path.c_str(), cloud.xyz.data(), cloud.rgba.data(), nrm.normals.data(),
                                     nrm.curvature.data(), cloud.size(), mode),
              "GlobalMap360::savePCDNormals");
    }
    // Euclidean clusters of the map where it lies (r360_ctx_map_cluster): labels and records stay on the GPU, valid
    // until the map next changes.  use_normals: the normal-aware form on the map's normals (estimateNormals first)
    void cluster(const r360_cluster_params& params, bool use_normals = false, r360_cluster_stats* stats = nullptr) {
        check(r360_ctx_map_cluster(ctx_->get(), &params, use_normals ? 1 : 0, stats), "GlobalMap360::cluster");
    }
    // the map's labels in the order of download() (-1: in no cluster); throws when the map changed since cluster()
    void getLabels(std::vector<int>& labels) const {
        size_t n = 0;
        check(r360_ctx_map_download_labels(ctx_->get(), nullptr, 0, &n), "GlobalMap360::getLabels");
        labels.resize(n);
        check(r360_ctx_map_download_labels(ctx_->get(), labels.data(), n, &n), "GlobalMap360::getLabels");
    }
    // the clusters' records, largest first
    void getClusters(std::vector<r360_cluster_info>& info) const {
        size_t n = 0;
        check(r360_ctx_map_cluster_info(ctx_->get(), nullptr, 0, &n), "GlobalMap360::getClusters");
        info.resize(n);
        check(r360_ctx_map_cluster_info(ctx_->get(), info.data(), n, &n), "GlobalMap360::getClusters");
    }
    // keeps exactly the points of the clusters within the size bounds (r360_ctx_map_filter_clusters), in HBM; the map's
    // normals and labels become invalid, as after removeOutliers
    void removeSmallClusters(const r360_cluster_params& params, bool use_normals = false,
                             r360_cluster_stats* stats = nullptr) {
        check(r360_ctx_map_filter_clusters(ctx_->get(), &params, use_normals ? 1 : 0, stats),
              "GlobalMap360::removeSmallClusters");
    }
    // the map with its labels as a PointXYZRGBL file (r360_pcd_write_labels; mode as r360_pcd_write)
    void savePCDLabels(const std::string& path, int mode = 0) const {
        PointCloud cloud;
        std::vector<int> labels;
        download(cloud);
        getLabels(labels);
        check(r360_pcd_write_labels(path.c_str(), cloud.xyz.data(), cloud.rgba.data(), labels.data(), cloud.size(), mode),
              "GlobalMap360::savePCDLabels");
    }
    // RANSAC planes of the map where it lies (r360_ctx_map_sac_planes): plane labels and records stay on the GPU, valid
    // until the map next changes.  use_normals: the normals gate on the map's normals (estimateNormals first)
    void segmentPlanes(const r360_sac_params& params, bool use_normals = false, r360_sac_stats* stats = nullptr) {
        check(r360_ctx_map_sac_planes(ctx_->get(), &params, use_normals ? 1 : 0, stats), "GlobalMap360::segmentPlanes");
    }
    // the map's plane labels in the order of download() (-1: in no plane); throws when the map changed since segmentPlanes
    void getPlaneLabels(std::vector<int>& labels) const {
        size_t n = 0;
        check(r360_ctx_map_download_plane_labels(ctx_->get(), nullptr, 0, &n), "GlobalMap360::getPlaneLabels");
        labels.resize(n);
        check(r360_ctx_map_download_plane_labels(ctx_->get(), labels.data(), n, &n), "GlobalMap360::getPlaneLabels");
    }
    // the planes' records, in extraction order
    void getPlanes(std::vector<r360_sac_plane>& planes) const {
        size_t n = 0;
        check(r360_ctx_map_plane_info(ctx_->get(), nullptr, 0, &n), "GlobalMap360::getPlanes");
        planes.resize(n);
        check(r360_ctx_map_plane_info(ctx_->get(), planes.data(), n, &n), "GlobalMap360::getPlanes");
    }
    // segments, then drops the plane points / keeps only them (r360_ctx_map_filter_planes), in HBM; the map's normals,
    // cluster labels and plane labels become invalid
    void removePlanes(const r360_sac_params& params, bool use_normals = false, r360_sac_stats* stats = nullptr) {
        check(r360_ctx_map_filter_planes(ctx_->get(), &params, use_normals ? 1 : 0, 0, stats), "GlobalMap360::removePlanes");
    }
    void keepPlanes(const r360_sac_params& params, bool use_normals = false, r360_sac_stats* stats = nullptr) {
        check(r360_ctx_map_filter_planes(ctx_->get(), &params, use_normals ? 1 : 0, 1, stats), "GlobalMap360::keepPlanes");
    }
    // the map with its plane labels as a PointXYZRGBL file (r360_pcd_write_labels; mode as r360_pcd_write)
    void savePCDPlaneLabels(const std::string& path, int mode = 0) const {
        PointCloud cloud;
        std::vector<int> labels;
        download(cloud);
        getPlaneLabels(labels);
        check(r360_pcd_write_labels(path.c_str(), cloud.xyz.data(), cloud.rgba.data(), labels.data(), cloud.size(), mode),
              "GlobalMap360::savePCDPlaneLabels");
    }
  private:
    std::shared_ptr<Context> keep_;
    Context* ctx_;
    float voxel_, box_;
};
inline bool GlobalMap360::add(Frame360& keyframe, const Matrix4f& pose) {
    return check(r360_ctx_map_add_frame(ctx_->get(), keyframe.get(), pose.data(), -2.0f, 1.0f, box_, voxel_),
                 "GlobalMap360::add") == 0;
}

// pcl::NormalEstimation with PCL's names, on the GPU of the calling thread's default context or of the Context given
// (r360_cloud_normals).  The neighbourhood is at most k points within a radius: setKSearch alone
// searches within setSearchBound (0.5 m by default), setRadiusSearch alone takes at most 64 points, and both together
// give the library's rule.  setViewPoint / setViewPoints: the normals turn towards the nearest viewpoint.  The input
// cloud is referenced, not copied: it must outlive compute().
class NormalEstimation {
  public:
    NormalEstimation() {}
    explicit NormalEstimation(Context& ctx) : ctx_(&ctx) {}
    void setInputCloud(const PointCloud& cloud) { cloud_ = &cloud; }
    void setKSearch(int k) { k_ = k; }
    void setRadiusSearch(double radius) { radius_ = float(radius); }
    void setSearchBound(double bound) { bound_ = float(bound); }
    void setViewPoint(float x, float y, float z) { views_.assign({x, y, z}); }
    void setViewPoints(const std::vector<float>& xyz) { views_ = xyz; }
    void getViewPoint(float& x, float& y, float& z) const { x = views_[0]; y = views_[1]; z = views_[2]; }
    const r360_normal_stats& stats() const { return stats_; }
    void compute(PointCloudNormal& out) {
        if (!cloud_) throw std::invalid_argument("NormalEstimation::compute: no input cloud");
        r360_normal_params p;
        r360_normal_default_params(&p);
        if (k_ > 0 || radius_ > 0.f) {
            p.k = k_ > 0 ? k_ : 64;
            p.radius = radius_ > 0.f ? radius_ : bound_;
        }
        Context& c = ctx_ ? *ctx_ : default_context();
        out.resize(cloud_->size());
        check(r360_cloud_normals(c.get(), cloud_->xyz.data(), cloud_->size(), &p, views_.data(), int(views_.size() / 3),
                                 out.normals.data(), out.curvature.data(), &stats_),
              "NormalEstimation::compute");
    }
  private:
    Context* ctx_ = nullptr;
    const PointCloud* cloud_ = nullptr;
    int k_ = 0;
    float radius_ = 0.f, bound_ = 0.5f;
    std::vector<float> views_ = {0.f, 0.f, 0.f};
    r360_normal_stats stats_ = {0, 0, 0, 0};
};

// pcl::EuclideanClusterExtraction with PCL's names, on the GPU of the calling thread's default context or of the Context
// given (r360_cloud_clusters).  extract() returns the clusters largest first (ties by their smallest
// row), each with its rows ascending.  Extension: setInputNormals / setEpsAngle select the normal-aware form, which in
// PCL is the free function pcl::extractEuclideanClusters(cloud, normals, tolerance, tree, clusters, eps_angle, ...).
// The input cloud and normals are referenced, not copied: they must outlive extract().
class EuclideanClusterExtraction {
  public:
    EuclideanClusterExtraction() { r360_cluster_default_params(&prm_); }
    explicit EuclideanClusterExtraction(Context& ctx) : ctx_(&ctx) { r360_cluster_default_params(&prm_); }
    void setClusterTolerance(double tolerance) { prm_.tolerance = float(tolerance); }
    double getClusterTolerance() const { return prm_.tolerance; }
    void setMinClusterSize(int n) { prm_.min_size = n; }
    int getMinClusterSize() const { return prm_.min_size; }
    void setMaxClusterSize(int n) { prm_.max_size = n; }
    int getMaxClusterSize() const { return prm_.max_size; }
    void setInputCloud(const PointCloud& cloud) { cloud_ = &cloud; }
    void setInputNormals(const PointCloudNormal& normals) { normals_ = &normals; }   // extension
    void setEpsAngle(double radians) { prm_.eps_angle = float(radians); }            // extension
    const r360_cluster_stats& stats() const { return stats_; }
    const std::vector<int>& getLabels() const { return labels_; }
    const std::vector<r360_cluster_info>& getClusterInfo() const { return info_; }
    void extract(std::vector<PointIndices>& clusters) {
        if (!cloud_) throw std::invalid_argument("EuclideanClusterExtraction::extract: no input cloud");
        if (normals_ && normals_->size() != cloud_->size())
            throw std::invalid_argument("EuclideanClusterExtraction::extract: normals and cloud differ in size");
        Context& c = ctx_ ? *ctx_ : default_context();
        const size_t n = cloud_->size();
        labels_.assign(n, -1);
        info_.resize(n / size_t(prm_.min_size > 0 ? prm_.min_size : 1) + 1);   // no more clusters than that
        size_t nk = 0;
        check(r360_cloud_clusters(c.get(), cloud_->xyz.data(), normals_ ? normals_->normals.data() : nullptr, n, &prm_,
                                  labels_.data(), info_.data(), info_.size(), &nk, &stats_),
              "EuclideanClusterExtraction::extract");
        info_.resize(nk);
        clusters.assign(nk, PointIndices());
        for (size_t k = 0; k < nk; ++k) clusters[k].indices.reserve(size_t(info_[k].size));
        for (size_t i = 0; i < n; ++i)
            if (labels_[i] >= 0) clusters[size_t(labels_[i])].indices.push_back(int(i));
    }
  private:
    Context* ctx_ = nullptr;
    const PointCloud* cloud_ = nullptr;
    const PointCloudNormal* normals_ = nullptr;
    r360_cluster_params prm_;
    r360_cluster_stats stats_ = {0, 0, 0, 0, 0};
    std::vector<int> labels_;
    std::vector<r360_cluster_info> info_;
};

// pcl::SACSegmentation with PCL's names for the three plane models and RANSAC, on the GPU of the calling thread's
// default context or of the Context given (r360_cloud_sac_planes with max_planes = 1).  segment()
// returns the one largest plane: its inliers ascending and a, b, c, d; both are empty when no plane has
// getMinInliers() points (3 by default; PCL reports an empty model when RANSAC finds none).  Extensions:
// setInputNormals / setNormalAngle select the normals gate (where PCL has SACSegmentationFromNormals), setSeed the
// counter-based sampler's seed, setMinInliers the smallest plane reported.  The input cloud and normals are
// referenced, not copied: they must outlive segment().
class SACSegmentation {
  public:
    SACSegmentation() { init(); }
    explicit SACSegmentation(Context& ctx) : ctx_(&ctx) { init(); }
    void setModelType(int model) {
        if (model == SACMODEL_PLANE) prm_.constraint = R360_SAC_NONE;
        else if (model == SACMODEL_PERPENDICULAR_PLANE) prm_.constraint = R360_SAC_PERPENDICULAR;
        else if (model == SACMODEL_PARALLEL_PLANE) prm_.constraint = R360_SAC_PARALLEL;
        else throw std::invalid_argument("SACSegmentation::setModelType: only the three plane models exist here");
        model_ = model;
    }
    int getModelType() const { return model_; }
    void setMethodType(int method) {
        if (method != SAC_RANSAC) throw std::invalid_argument("SACSegmentation::setMethodType: only SAC_RANSAC exists here");
    }
    int getMethodType() const { return SAC_RANSAC; }
    void setDistanceThreshold(double threshold) { prm_.distance_threshold = float(threshold); }
    double getDistanceThreshold() const { return prm_.distance_threshold; }
    void setMaxIterations(int n) { prm_.max_iterations = n; }
    int getMaxIterations() const { return prm_.max_iterations; }
    void setProbability(double probability) { prm_.probability = float(probability); }
    double getProbability() const { return prm_.probability; }
    void setOptimizeCoefficients(bool optimize) { prm_.optimize = optimize ? 1 : 0; }
    bool getOptimizeCoefficients() const { return prm_.optimize != 0; }
    void setAxis(float x, float y, float z) { prm_.axis[0] = x; prm_.axis[1] = y; prm_.axis[2] = z; }
    void setEpsAngle(double radians) { prm_.eps_angle = float(radians); }
    double getEpsAngle() const { return prm_.eps_angle; }
    void setInputCloud(const PointCloud& cloud) { cloud_ = &cloud; }
    void setInputNormals(const PointCloudNormal& normals) { normals_ = &normals; }   // extension
    void setNormalAngle(double radians) { prm_.normal_angle = float(radians); }      // extension
    void setSeed(unsigned long long seed) { prm_.seed = seed; }                      // extension
    void setMinInliers(int n) { prm_.min_inliers = n; }                              // extension
    int getMinInliers() const { return prm_.min_inliers; }
    const r360_sac_stats& stats() const { return stats_; }
    const r360_sac_plane& getPlaneInfo() const { return plane_; }
    void segment(PointIndices& inliers, ModelCoefficients& coefficients) {
        if (!cloud_) throw std::invalid_argument("SACSegmentation::segment: no input cloud");
        if (normals_ && normals_->size() != cloud_->size())
            throw std::invalid_argument("SACSegmentation::segment: normals and cloud differ in size");
        Context& c = ctx_ ? *ctx_ : default_context();
        const size_t n = cloud_->size();
        std::vector<int> labels(n, -1);
        size_t np = 0;
        check(r360_cloud_sac_planes(c.get(), cloud_->xyz.data(), normals_ ? normals_->normals.data() : nullptr, n, &prm_,
                                    labels.data(), &plane_, 1, &np, &stats_),
              "SACSegmentation::segment");
        inliers.indices.clear();
        coefficients.values.clear();
        if (np == 0) return;
        inliers.indices.reserve(size_t(plane_.size));
        for (size_t i = 0; i < n; ++i)
            if (labels[i] == 0) inliers.indices.push_back(int(i));
        for (int k = 0; k < 4; ++k) coefficients.values.push_back(float(plane_.coef[k]));
    }
  private:
    void init() {
        r360_sac_default_params(&prm_);
        prm_.max_planes = 1;
        prm_.min_inliers = 3;
        std::memset(&plane_, 0, sizeof plane_);
    }
    Context* ctx_ = nullptr;
    const PointCloud* cloud_ = nullptr;
    const PointCloudNormal* normals_ = nullptr;
    int model_ = SACMODEL_PLANE;
    r360_sac_params prm_;
    r360_sac_stats stats_ = {0, 0, 0, 0, 0};
    r360_sac_plane plane_;
};

// ------------------------------------------------------------------ Generalized-ICP
// pcl::GeneralizedIterativeClosestPoint with the call surface of Registration/RegisterPairRGBD360.cpp:109-149, on the
// GPU of the calling thread's default context or of the Context given (r360_gicp_*; the algorithm is restated, with a
// Gauss-Newton inner solve where PCL runs BFGS: DESIGN.md §5c).  The clouds live in the context: one source and one
// target per context at a time.  setRANSACOutlierRejectionThreshold stores its value and nothing reads it, as in
// PCL's GICP, whose computeTransformation never runs the RANSAC rejector.
class GeneralizedIterativeClosestPoint {
  public:
    GeneralizedIterativeClosestPoint() : keep_(default_context_ptr()), ctx_(keep_.get()) { r360_gicp_default_params(&p_); }
    explicit GeneralizedIterativeClosestPoint(Context& ctx) : ctx_(&ctx) { r360_gicp_default_params(&p_); }
    void setMaxCorrespondenceDistance(double d) { p_.max_corr_dist = float(d); }
    void setMaximumIterations(int n) { p_.max_iterations = n; }
    void setTransformationEpsilon(double e) { p_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { p_.rotation_epsilon = e; }
    void setCorrespondenceRandomness(int k) { p_.k_correspondences = k; }
    void setMaximumOptimizerIterations(int n) { p_.max_inner_iterations = n; }
    void setRANSACOutlierRejectionThreshold(double t) { ransac_ = t; }
    double getRANSACOutlierRejectionThreshold() const { return ransac_; }
    // rows with a non-finite coordinate are dropped; fewer than k finite points throws (as PCL does)
    void setInputSource(const PointCloud& cloud) {
        src_ = &cloud;
        check(r360_gicp_set_source(ctx_->get(), cloud.xyz.data(), cloud.size(), &p_), "GICP setInputSource");
    }
    void setInputTarget(const PointCloud& cloud) {
        check(r360_gicp_set_target(ctx_->get(), cloud.xyz.data(), cloud.size(), &p_), "GICP setInputTarget");
    }
    // out: the source cloud under the final transformation (the cloud given to setInputSource must still exist)
    void align(PointCloud& out, const Matrix4f& guess = Matrix4f::Identity()) {
        illposed_ = check(r360_gicp_align(ctx_->get(), guess.data(), &p_, T_.data(), &st_), "GICP align") == 1;
        if (src_) transformPointCloud(*src_, out, T_);
    }
    Matrix4f getFinalTransformation() const { return T_; }
    bool hasConverged() const { return st_.converged != 0; }
    double getFitnessScore() const { return st_.fitness; }
    bool illPosed() const { return illposed_; }   // no pair inside the gate or a singular system: the pose stayed
    const r360_gicp_stats& stats() const { return st_; }
  private:
    std::shared_ptr<Context> keep_;
    Context* ctx_;
    r360_gicp_params p_;
    r360_gicp_stats st_ = r360_gicp_stats();
    const PointCloud* src_ = nullptr;
    Matrix4f T_ = Matrix4f::Identity();
    double ransac_ = 0.05;
    bool illposed_ = false;
};

// ------------------------------------------------------------------ GraphOptimizer
// include/GraphOptimizer.h with its members and signatures, over r360_graph_* (the g2o Levenberg-Marquardt restated,
// its linear solve a block-sparse conjugate gradient on the GPU: DESIGN.md §5d).  The default constructor gives the
// optimiser a context of its own, so an optimiser built on one thread and used on another (LoopClosure360's member,
// LoopClosure360.h:58, 89-91) shares no stream with either.  ThreeDegreesOfFreedom throws: the reference's own 3-DoF
// addVertex and addEdge bodies are commented out.
class GraphOptimizer {
  public:
    enum RigidTransformationType { SixDegreesOfFreedom = 0, ThreeDegreesOfFreedom = 1 } rigidTransformationType;
    int vertex_id = 0;                  // the index of the next vertex (the graph's size)
    r360_graph_params params;           // max_iterations = 10 is the reference's optimize(10)
    GraphOptimizer() : keep_(std::make_shared<Context>(default_device())), ctx_(keep_.get()) { init(); }
    explicit GraphOptimizer(Context& ctx) : ctx_(&ctx) { init(); }
    ~GraphOptimizer() { r360_graph_destroy(h_); }
    GraphOptimizer(const GraphOptimizer&) = delete;
    GraphOptimizer& operator=(const GraphOptimizer&) = delete;
    int addVertex(const Matrix4d vertexPose) {
        int id = -1;
        check(r360_graph_add_vertex(h_, vertexPose.data(), &id), "GraphOptimizer::addVertex");
        vertex_id = id + 1;
        return id;
    }
    void addEdge(const int fromIdx, const int toIdx, const Matrix4d relativePose, const Matrix6d informationMatrix) {
        check(r360_graph_add_edge(h_, fromIdx, toIdx, relativePose.data(), informationMatrix.data()), "GraphOptimizer::addEdge");
    }
    // g2o's setRobustKernel, per edge (kind: R360_GRAPH_KERNEL_NONE / _HUBER / _CAUCHY, delta on sqrt(chi2)): the
    // first call sets the kernel of the edges added from now on, the second that of one edge.  Edges are numbered
    // in the order of the addEdge calls.
    void setRobustKernel(int kind, double delta = 1.0) {
        check(r360_graph_set_default_kernel(h_, kind, delta), "GraphOptimizer::setRobustKernel");
    }
    void setEdgeRobustKernel(int edge, int kind, double delta = 1.0) {
        check(r360_graph_set_edge_kernel(h_, edge, kind, delta), "GraphOptimizer::setEdgeRobustKernel");
    }
    // an inactive edge does not exist for optimizeGraph and saveGraph
    void setEdgeActive(int edge, bool active) {
        check(r360_graph_set_edge_active(h_, edge, active ? 1 : 0), "GraphOptimizer::setEdgeActive");
    }
    // per edge at the current poses: chi2 = e^T info e and the kernel's weight (0 for an inactive edge)
    void getEdgeChi2(std::vector<double>& chi2, std::vector<double>* weight = nullptr) {
        const int m = numEdges();
        int n = 0;
        chi2.assign(size_t(m), 0.0);
        if (weight) weight->assign(size_t(m), 0.0);
        check(r360_graph_edge_stats(h_, chi2.data(), weight ? weight->data() : nullptr, m, &n), "GraphOptimizer::getEdgeChi2");
    }
    int numEdges() const {
        int m = 0;
        check(r360_graph_size(h_, nullptr, &m), "GraphOptimizer::numEdges");
        return m;
    }
    void optimizeGraph() { check(r360_graph_optimize(h_, &params, &stats_), "GraphOptimizer::optimizeGraph"); }
    template <class Alloc>
    void getPoses(std::vector<Matrix4f, Alloc>& poses) {
        int n = 0;
        check(r360_graph_get_poses(h_, nullptr, 0, &n), "GraphOptimizer::getPoses");
        std::vector<double> p(16 * size_t(n));
        check(r360_graph_get_poses(h_, p.data(), n, &n), "GraphOptimizer::getPoses");
        poses.clear();
        poses.resize(n);
        for (int k = 0; k < n; ++k)
            for (int c = 0; c < 4; ++c)
                for (int r = 0; r < 4; ++r) poses[k](r, c) = float(p[16 * size_t(k) + c * 4 + r]);
    }
    void saveGraph(std::string fileName) { check(r360_graph_save(h_, fileName.c_str()), "GraphOptimizer::saveGraph"); }
    void setFixed(int idx, bool fixed) { check(r360_graph_set_fixed(h_, idx, fixed ? 1 : 0), "GraphOptimizer::setFixed"); }
    inline void setRigidTransformationType(RigidTransformationType rttype) {
        if (rttype != SixDegreesOfFreedom)
            throw std::invalid_argument("GraphOptimizer: ThreeDegreesOfFreedom is not supported (the reference's 3-DoF bodies are commented out)");
        rigidTransformationType = rttype;
    }
    const r360_graph_stats& stats() const { return stats_; }
    r360_graph* get() const { return h_; }
  private:
    void init() {
        rigidTransformationType = SixDegreesOfFreedom;
        r360_graph_default_params(&params);
        check(r360_graph_create(ctx_->get(), &h_), "r360_graph_create");
    }
    std::shared_ptr<Context> keep_;     // declared before h_: the graph goes first, then its context
    Context* ctx_;
    r360_graph* h_ = nullptr;
    r360_graph_stats stats_ = r360_graph_stats();
};

// ------------------------------------------------------------------ ControlPlanes / Calibration
// include/Calibration.h with its members, over r360_rigcal_* (restated in fp64: DESIGN.md §5e), so that the calls of
// Calibration/Calibrator.cpp:64-75, 176-192 compile unchanged.  CMatrixDouble is the little of
// mrpt::math::CMatrixDouble those call sites use.
struct CMatrixDouble {
    std::vector<double> v;              // row-major
    size_t rows = 0, cols = 0;
    CMatrixDouble() = default;
    CMatrixDouble(size_t r, size_t c) : v(r * c, 0.0), rows(r), cols(c) {}
    size_t getRowCount() const { return rows; }
    size_t getColCount() const { return cols; }
    void setSize(size_t r, size_t c) { v.assign(r * c, 0.0); rows = r; cols = c; }
    double& operator()(size_t r, size_t c) { return v[r * cols + c]; }
    double operator()(size_t r, size_t c) const { return v[r * cols + c]; }
    void loadFromTextFile(const std::string& path) {
        int nr = 0, nc = 0;
        check(r360_rigcal_read_matrix(path.c_str(), nullptr, 0, &nr, &nc), "CMatrixDouble::loadFromTextFile");
        setSize(size_t(nr), size_t(nc));
        check(r360_rigcal_read_matrix(path.c_str(), v.data(), v.size(), &nr, &nc), "CMatrixDouble::loadFromTextFile");
    }
    void saveToTextFile(const std::string& path) const {
        check(r360_rigcal_write_matrix(path.c_str(), v.data(), int(rows), int(cols)), "CMatrixDouble::saveToTextFile");
    }
};

class ControlPlanes {
  public:
    // mmCorrespondences[i][j], i < j: one row per pair of planes seen by both sensors (Calibration.h:47-52)
    std::map<unsigned, std::map<unsigned, CMatrixDouble> > mmCorrespondences;
    float conditioning[8];              // of the adjacent pairs' normal covariances (the pair (0, 7) under 7)
    ControlPlanes() { std::fill(conditioning, conditioning + 8, 1.f); }
    void loadPlaneCorrespondences(const std::string planeCorrespDirectory) {
        mmCorrespondences.clear();
        for (unsigned i = 0; i < 7; ++i) {
            mmCorrespondences[i] = std::map<unsigned, CMatrixDouble>();
            for (unsigned j = i + 1; j < 8; ++j) {
                const std::string f = format("%s/correspondences_%u_%u.txt", planeCorrespDirectory.c_str(), i, j);
                if (FILE* t = std::fopen(f.c_str(), "r")) {
                    std::fclose(t);
                    mmCorrespondences[i][j].loadFromTextFile(f);
                }
            }
        }
    }
    void savePlaneCorrespondences(const std::string& planeCorrespDirectory) {
        for (auto& a : mmCorrespondences)
            for (auto& b : a.second)
                if (b.second.getRowCount() > 0)
                    b.second.saveToTextFile(format("%s/correspondences_%u_%u.txt", planeCorrespDirectory.c_str(), a.first, b.first));
    }
    // The live form of the pair fit (Calibration/OnlinePairCalibrator.cpp:84-160) with this class's thresholds; the
    // draw is the library's counter-based hash of (seed, trial, redraw).  3 rows or fewer, or no non-degenerate
    // draw, leave the matrix untouched.
    void trimOutliersRANSAC(CMatrixDouble& matched_planes, unsigned seed = 0) {
        if (matched_planes.getRowCount() <= 3) return;
        if (matched_planes.getColCount() != 10) throw std::invalid_argument("trimOutliersRANSAC: a correspondence matrix has 10 columns");
        std::shared_ptr<Context> ctx = default_context_ptr();
        r360_rigcal* h = nullptr;
        check(r360_rigcal_create(ctx->get(), &h), "r360_rigcal_create");
        int n = 0;
        int rc = r360_rigcal_set_pair(h, 0, 1, matched_planes.v.data(), int(matched_planes.rows), 10);
        if (!rc) rc = r360_rigcal_trim(h, 0, 1, nullptr, seed, &trim_stats, nullptr, 0);
        if (!rc) rc = r360_rigcal_get_pair(h, 0, 1, nullptr, 0, &n);
        if (!rc) {
            matched_planes.setSize(size_t(n), 10);
            rc = r360_rigcal_get_pair(h, 0, 1, matched_planes.v.data(), n, &n);
        }
        r360_rigcal_destroy(h);
        check(rc, "ControlPlanes::trimOutliersRANSAC");
    }
    // GetControlPlanes.cpp:358-469 on a frame built with getLocalPlanes(): the pairs of planes seen by two sensors at
    // once are appended to mmCorrespondences and `conditioning` is updated.  Returns the rows added.
    int collect(Frame360& frame, const r360_rigcal_collect_params* params = nullptr) {
        if (!collector_) {
            r360_rigcal* h = nullptr;
            collector_ctx_ = default_context_ptr();
            check(r360_rigcal_create(collector_ctx_->get(), &h), "r360_rigcal_create");
            collector_.reset(h, r360_rigcal_destroy);
        }
        int added[28], total = 0, p = 0;
        check(r360_rigcal_add_frame(collector_.get(), frame.get(), params, added), "ControlPlanes::collect");
        std::vector<double> rows;
        for (unsigned i = 0; i < 7; ++i)
            for (unsigned j = i + 1; j < 8; ++j, ++p) {
                if (!added[p]) continue;
                int n = 0;
                check(r360_rigcal_get_pair(collector_.get(), int(i), int(j), nullptr, 0, &n), "r360_rigcal_get_pair");
                rows.resize(size_t(n) * 10);
                check(r360_rigcal_get_pair(collector_.get(), int(i), int(j), rows.data(), n, &n), "r360_rigcal_get_pair");
                CMatrixDouble& m = mmCorrespondences[i][j];
                if (m.getRowCount() == 0) m.setSize(0, 10);
                m.v.insert(m.v.end(), rows.end() - size_t(added[p]) * 10, rows.end());
                m.rows += size_t(added[p]);
                total += added[p];
            }
        check(r360_rigcal_conditioning(collector_.get(), conditioning), "r360_rigcal_conditioning");
        return total;
    }
    void printConditioning() {
        std::cout << "Conditioning";
        for (unsigned k = 0; k < 7; ++k) std::cout << " " << k << "-" << k + 1 << " " << conditioning[k];
        std::cout << " 0-7 " << conditioning[7] << std::endl;
    }
    r360_rigcal_trim_stats trim_stats = r360_rigcal_trim_stats();
  private:
    std::shared_ptr<Context> collector_ctx_;      // declared before collector_: the handle goes first
    std::shared_ptr<r360_rigcal> collector_;      // holds the collected rows' normal covariances between frames
};

class Calibration {
  public:
    ControlPlanes matchedPlanes;
    Matrix4f Rt_specs[8];               // the construction specifications
    Matrix4f Rt_estimated[8];           // what the calibration estimates
    Calibration() : keep_(default_context_ptr()) { check(r360_rigcal_create(keep_->get(), &h_), "r360_rigcal_create"); }
    ~Calibration() { r360_rigcal_destroy(h_); }
    Calibration(const Calibration&) = delete;
    Calibration& operator=(const Calibration&) = delete;
    void loadConstructionSpecs() {
        double rt[128];
        r360_rigcal_specs(rt);
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 16; ++i) Rt_specs[k].v[i] = float(rt[16 * k + i]);
        specs_loaded_ = true;
    }
    // weightedLS = 1 weights the normal equations only when every matrix has 18 columns, the reference's own
    // condition (Calibration.h:1086), which its 10-column files never meet
    void CalibrateRotation(int weightedLS = 0) {
        const bool weighted = push_rows() && weightedLS == 1;
        double rt[128];
        r360_rigcal_specs(rt);           // the specs in double unless the caller changed Rt_specs
        // Rt_specs is a float member, as in the reference; the solve starts from doubles.  Invariant: an entry that
        // still equals float(spec) is taken to be the untouched spec and gets the spec's double; an entry the
        // caller changed to any other float is used as given.  (A caller's value that happens to equal the float
        // rounding of the spec therefore becomes the spec, which differs from it by less than one float ulp.)
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 16; ++i)
                if (!specs_loaded_ || Rt_specs[k].v[i] != float(rt[16 * k + i])) rt[16 * k + i] = Rt_specs[k].v[i];
        check(r360_rigcal_set_init(h_, rt), "Calibration::CalibrateRotation");
        const int rc = r360_rigcal_rotation(h_, weighted ? 1 : 0, &rotation_stats);
        pull_estimate();
        check(rc, "Calibration::CalibrateRotation");
        const r360_rigcal_stats& s = rotation_stats;
        if (s.iterations > 0)
            std::cout << "ErrorCalibRotation " << (s.status == R360_RIGCAL_BAD_CONDITIONED ? s.error : s.werr0)[s.iterations - 1] / s.rows << " "
                      << s.angle[s.iterations - 1] / s.rows << std::endl;   // accum_error2 as :1157 or :1082 left it
    }
    void CalibrateTranslation(int weightedLS = 0) {
        const bool weighted = push_rows() && weightedLS == 1;
        push_estimate();
        const int rc = r360_rigcal_translation(h_, weighted ? 1 : 0, &translation_stats);
        pull_estimate();
        check(rc, "Calibration::CalibrateTranslation");
        const r360_rigcal_stats& s = translation_stats;
        if (s.status == R360_RIGCAL_CONVERGED) std::cout << "ErrorCalibTranslation " << s.error[0] / s.rows << std::endl;
        else std::cout << "\tTranslation system is bad conditioned " << s.conditioning[0] << " threshold 8000\n";
    }
    void Calibrate() {
        CalibrateRotation();
        CalibrateTranslation();
    }
    // the estimate in double, column-major [8][16], and as the Rt_0k.txt files loadExtrinsicCalibration reads
    void getEstimate(double rt8[128]) const { check(r360_rigcal_get_estimate(h_, rt8), "Calibration::getEstimate"); }
    void saveExtrinsics(const std::string& dir) {
        push_estimate();
        check(r360_rigcal_save_extrinsics(h_, dir.c_str()), "Calibration::saveExtrinsics");
    }
    r360_rigcal* get() const { return h_; }
    r360_rigcal_stats rotation_stats = r360_rigcal_stats(), translation_stats = r360_rigcal_stats();
  private:
    // the matrices' first ten columns into the handle; true when every matrix has 18 columns
    bool push_rows() {
        check(r360_rigcal_clear(h_), "r360_rigcal_clear");
        bool all18 = true;
        std::vector<double> rows;
        for (auto& a : matchedPlanes.mmCorrespondences)
            for (auto& b : a.second) {
                const CMatrixDouble& m = b.second;
                if (m.getRowCount() == 0) continue;
                if (m.getColCount() < 10) throw std::invalid_argument("Calibration: a correspondence matrix has at least 10 columns");
                all18 = all18 && m.getColCount() == 18;
                rows.resize(m.getRowCount() * 10);
                for (size_t r = 0; r < m.getRowCount(); ++r)
                    for (size_t c = 0; c < 10; ++c) rows[r * 10 + c] = m(r, c);
                check(r360_rigcal_set_pair(h_, int(a.first), int(b.first), rows.data(), int(m.getRowCount()), 10), "r360_rigcal_set_pair");
            }
        return all18;
    }
    void pull_estimate() {
        check(r360_rigcal_get_estimate(h_, est_), "r360_rigcal_get_estimate");
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 16; ++i) Rt_estimated[k].v[i] = float(est_[16 * k + i]);
    }
    // Rt_estimated back into the handle where the caller changed it; untouched entries keep their doubles (the same
    // invariant as for Rt_specs above: equal to float(double) means untouched)
    void push_estimate() {
        double rt[128];
        check(r360_rigcal_get_estimate(h_, rt), "r360_rigcal_get_estimate");
        bool changed = false;
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 16; ++i)
                if (Rt_estimated[k].v[i] != float(rt[16 * k + i])) { rt[16 * k + i] = Rt_estimated[k].v[i]; changed = true; }
        if (changed) check(r360_rigcal_set_init(h_, rt), "r360_rigcal_set_init");
    }
    std::shared_ptr<Context> keep_;     // declared before h_: the handle goes first, then its context
    r360_rigcal* h_ = nullptr;
    double est_[128];
    bool specs_loaded_ = false;
};

// ------------------------------------------------------------------ Map360 / TopologicalMap360 / Relocalizer360
// Map360 (include/Map360.h:41-97): the pose graph of keyframes and its arrangement in topological areas.  The
// members are the reference's; TopologicalMap360 keeps vsAreas, vsNeighborAreas, vSelectedKFs, currentArea and every
// frame's node up to date after each of its calls.
class Map360 {
  public:
    std::vector<Frame360*> vpSpheres;
    std::vector<Matrix4f> vTrajectoryPoses;
    std::vector<Matrix4f> vOptimizedPoses;
    std::vector<float> vTrajectoryIncrements;
    std::map<unsigned, std::map<unsigned, std::pair<Matrix4f, Matrix6f> > > mmConnectionKFs;
    unsigned currentArea = 0;
    std::vector<std::set<unsigned> > vsAreas;
    std::vector<std::set<unsigned> > vsNeighborAreas;
    std::vector<unsigned> vSelectedKFs;
    std::mutex mapMutex;
    void addKeyframe(Frame360* sphere, Matrix4f& pose) {
        sphere->pose = pose;
        vpSpheres.push_back(sphere);
        vTrajectoryPoses.push_back(pose);
        vOptimizedPoses.push_back(pose);
    }
};

// TopologicalMap360 (include/TopologicalMap360.h) over r360_topomap_*: the SSO lives in one table keyed by global
// keyframe ids, so the reference's direct writes into vSSO[area](i, j) (KFsphere_SLAM.cpp:613, SphereGraphSLAM.cpp:
// 165-166, 215) become addKeyframe() / addConnection() calls.  addKeyframe() follows Map.addKeyframe() of the same
// keyframe; Partitioner() is RecursiveSpectralPartition(SSO, parts, 0.8, false, true, true, 3) on the GPU.
class TopologicalMap360 {
  public:
    explicit TopologicalMap360(Map360& map) : Map(map), keep_(default_context_ptr()) {
        check(r360_topomap_create(keep_->get(), &h_), "r360_topomap_create");
        sync();
    }
    TopologicalMap360(Map360& map, Context& ctx) : Map(map) {
        check(r360_topomap_create(ctx.get(), &h_), "r360_topomap_create");
        sync();
    }
    ~TopologicalMap360() { r360_topomap_destroy(h_); }
    TopologicalMap360(const TopologicalMap360&) = delete;
    TopologicalMap360& operator=(const TopologicalMap360&) = delete;
    r360_topo_params& params() { return params_; }
    // the newest keyframe of Map.vpSpheres joins the current area (the argument is the reference's, :81)
    void addKeyframe(unsigned /*currentArea*/ = 0) {
        check(r360_topomap_add_keyframe(h_, nullptr), "TopologicalMap360::addKeyframe");
        sync();
    }
    // the not-registered branch (SphereGraphSLAM.cpp:232-242): forget the newest keyframe
    void dropLastKeyframe() {
        check(r360_topomap_drop_last(h_), "TopologicalMap360::dropLastKeyframe");
        sync();
    }
    void addConnection(unsigned kf1_global, unsigned kf2_global, const float& sso) {
        check(r360_topomap_add_connection(h_, int(kf1_global), int(kf2_global), sso), "TopologicalMap360::addConnection");
        sync();
    }
    // the SSO matrix [n][n] (row-major) of the current area's vicinity; vicinityKFs: its keyframes in matrix order
    std::vector<float> getVicinitySSO(std::vector<unsigned>* vicinityKFs = nullptr) {
        int n = 0;
        check(r360_topomap_vicinity(h_, nullptr, nullptr, 0, &n), "getVicinitySSO");
        std::vector<int> ids(std::max(n, 1));
        std::vector<float> sso(size_t(std::max(n, 1)) * std::max(n, 1));
        check(r360_topomap_vicinity(h_, ids.data(), sso.data(), n, &n), "getVicinitySSO");
        sso.resize(size_t(n) * n);
        if (vicinityKFs) vicinityKFs->assign(ids.begin(), ids.begin() + n);
        return sso;
    }
    // returns the number of new areas
    int Partitioner() {
        int k = 0;
        check(r360_topomap_partition(h_, &params_, &k), "TopologicalMap360::Partitioner");
        sync();
        return k;
    }
    r360_topomap* get() const { return h_; }

  private:
    void sync() {
        int n = 0, na = 0, cur = 0;
        check(r360_topomap_areas(h_, nullptr, 0, &n, &na, &cur), "r360_topomap_areas");
        std::vector<int> area(std::max(n, 1));
        check(r360_topomap_areas(h_, area.data(), n, &n, &na, &cur), "r360_topomap_areas");
        Map.currentArea = unsigned(cur);
        Map.vsAreas.assign(na, std::set<unsigned>());
        Map.vsNeighborAreas.assign(na, std::set<unsigned>());
        Map.vSelectedKFs.assign(na, 0u);
        for (int k = 0; k < n; ++k) {
            Map.vsAreas[area[k]].insert(unsigned(k));
            if (size_t(k) < Map.vpSpheres.size() && Map.vpSpheres[k]) Map.vpSpheres[k]->node = unsigned(area[k]);
        }
        std::vector<int> nb(std::max(na, 1));
        for (int a = 0; a < na; ++a) {
            int m = 0, kf = -1;
            check(r360_topomap_neighbors(h_, a, nb.data(), na, &m), "r360_topomap_neighbors");
            Map.vsNeighborAreas[a].insert(nb.begin(), nb.begin() + m);
            check(r360_topomap_selected(h_, a, &kf), "r360_topomap_selected");
            Map.vSelectedKFs[a] = kf < 0 ? 0u : unsigned(kf);
        }
    }
    Map360& Map;
    std::shared_ptr<Context> keep_;     // the default context, when that is the one in use
    r360_topomap* h_ = nullptr;
    r360_topo_params params_ = default_params();
    static r360_topo_params default_params() {
        r360_topo_params p;
        r360_topo_default_params(&p);
        return p;
    }
};

// Relocalizer360 (include/Relocalizer360.h:43-94) over r360_relocalize: the keyframes of Map.vpSpheres, newest first,
// registered with the frame by PbMap under PLANAR_3DoF in chunks of the batch's lanes.
class Relocalizer360 {
  public:
    explicit Relocalizer360(Map360& map, int lanes = 4) : registerer(default_device(), lanes), Map(map) {}
    BatchRegistration registerer;
    unsigned relocKF = 0;
    Matrix4d rigidTransf;
    Matrix6d informationM;
    size_t max_match_planes = 25;
    // the frame with respect to which the system has relocalised, or -1
    int relocalize(Frame360* currentFrame) {
        std::vector<r360_frame*> kfs;
        for (auto f : Map.vpSpheres) kfs.push_back(f->get());
        int kf = -1;
        Matrix4d pose;
        Matrix6d info;
        check(r360_relocalize(registerer.get(), kfs.data(), int(kfs.size()), currentFrame->get(), max_match_planes, 5, 10.f,
                              &kf, pose.data(), info.data()),
              "Relocalizer360::relocalize");
        if (kf < 0) return -1;
        relocKF = unsigned(kf);
        rigidTransf = pose;
        informationM = info;
        return kf;
    }

  private:
    Map360& Map;
};

}  // namespace r360
