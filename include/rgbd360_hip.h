/* rgbd360_hip.h — C-ABI of librgbd360_hip.so, the MI355X-native (gfx950) implementation of
 * rgbd360's frame-to-frame registration hot path.
 *
 * This is the drop-in boundary.  The reference (Dorothy-2016/rgbd360) has no plugin/FFI layer:
 * its applications instantiate header-only classes directly.  Each entry point
 * below replaces one method of those classes; the C++ façade headers in include/rgbd360/ keep
 * the reference class names and signatures on top of this ABI.
 *
 * Conventions
 *   - 4x4 poses are float[16] COLUMN-major (Eigen default, as Eigen::Matrix4f::data()).
 *     6x6 matrices are float[36] column-major (symmetric ones are identical either way).
 *   - Sensor images: 8 sensors stored contiguously, each rows x cols, BGR u8 interleaved
 *     (as cv::Mat CV_8UC3 in the .bin files) and depth u16 millimetres (CV_16UC1).
 *   - Return codes: 0 = OK, 1 = soft failure (the reference returned false / ill-posed),
 *     < 0 = error (message in r360_last_error(), thread-local).  No exceptions cross the ABI.
 *   - One r360_ctx per (GPU, host thread); a ctx is not thread-safe.  All calls are ordered on
 *     the ctx's HIP stream and synchronous at return unless named *_async.
 */
#ifndef RGBD360_HIP_H
#define RGBD360_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R360_NUM_SENSORS 8
#define R360_MAX_PYR 6

typedef struct r360_ctx r360_ctx;
typedef struct r360_calib r360_calib;
typedef struct r360_frame r360_frame;

/* ---------------------------------------------------------------- context */
int         r360_ctx_create(int device, r360_ctx** out);
void        r360_ctx_destroy(r360_ctx* ctx);
int         r360_ctx_sync(r360_ctx* ctx);
void*       r360_ctx_stream(r360_ctx* ctx);        /* hipStream_t of the ctx */
const char* r360_last_error(void);
const char* r360_version(void);
/* The shipped data directory (calib/, config_files/, samples/): $R360_DATA_DIR, else <tree>/data of the tree the
 * library sits in — the files the reference finds under PROJECT_SOURCE_PATH (Calib360.h:107, :125). */
const char* r360_data_dir(void);

/* ---------------------------------------------------------------- Calib360
 * Replaces include/Calib360.h:44-132.  rows/cols = per-sensor image size; the pinhole
 * cameraMatrix is f = 525*cols/640, c = (cols/2-0.5, rows/2-0.5), which reproduces the
 * reference's QVGA constant (Calib360.h:73-77) and its commented VGA one (:83-85). */
int  r360_calib_create(r360_ctx* ctx, int rows, int cols, r360_calib** out);
void r360_calib_destroy(r360_calib* c);
/* Rt_[8] (Calib360.h:53), column-major 8 x float[16]; Rt_inv is derived (Calib360.h:129). */
int  r360_calib_set_extrinsics(r360_calib* c, const float* rt8);
int  r360_calib_get_extrinsics(const r360_calib* c, float* rt8, float* rt_inv8, float K[9]);
/* loadExtrinsicCalibration(dir): reads dir/Rt_0{1..8}.txt (Calib360.h:122-131); dir NULL or "" = the shipped
 * r360_data_dir()/calib/Extrinsics (the reference's "" default, :124-125). */
int  r360_calib_load_extrinsics(r360_calib* c, const char* dir);
/* loadIntrinsicCalibration(dir): CLAMS dir/distortion_model{1..8} + downsampleParams(2)
 * (Calib360.h:104-119); dir NULL or "" = r360_data_dir()/calib/Intrinsics (:106-107).  Without intrinsics
 * undistort() is the identity. */
int  r360_calib_load_intrinsics(r360_calib* c, const char* dir);
/* A calibration without sensors for spheres given as images (setSourceFrame / setTargetFrame(cv::Mat&,
 * cv::Mat&), RegisterPhotoICP.h:480-516): the ICP tables of an sph_rows x sph_cols sphere
 * (sph_cols % 8 == 0).  Its frames only take r360_frame_set_sphere. */
int  r360_calib_create_sphere(r360_ctx* ctx, int sph_rows, int sph_cols, r360_calib** out);

/* ---------------------------------------------------------------- Frame360
 * Replaces include/Frame360.h:93-1150. */
enum {
    R360_BUILD_UNDISTORT = 1u << 0,  /* Frame360::undistort()            Frame360.h:293   */
    R360_BUILD_SPHERE    = 1u << 1,  /* Frame360::stitchSphericalImage() Frame360.h:386   */
    R360_BUILD_PYRAMID   = 1u << 2,  /* RegisterPhotoICP::set{Source,Target}Frame :480-516 */
    R360_BUILD_CLOUD     = 1u << 3,  /* Frame360::buildSphereCloud()     Frame360.h:467   */
    R360_BUILD_PLANES    = 1u << 4,  /* Frame360::getPlanes()            Frame360.h:615   */
    R360_BUILD_SENSOR_PYRAMID = 1u << 5, /* per-sensor setSource/TargetFrame (pinhole alignFrames) */
    R360_BUILD_LOCAL_PLANES = 1u << 6,   /* with R360_BUILD_PLANES: keep each sensor's planes as they were before groupPlanes (r360_frame_get_local_planes) */
    /* Reported by r360_frame_built only (not a stage to ask for): the sphere images and level 0's {gray, depth}
     * image are in HBM.  Clear after the build of a frame that only enters batched alignments
     * (r360_frame_set_compaction(f, 0)) where those passes stream level 0's packed image: such a build writes
     * only that; the first call that reads one of the others (r360_frame_get_sphere, level 0 of
     * r360_frame_get_level / _get_points, a lone or occlusion alignment) stitches again in full and sets it. */
    R360_BUILT_LEVEL0 = 1u << 8,
};
int  r360_frame_create(r360_ctx* ctx, const r360_calib* calib, r360_frame** out);
void r360_frame_destroy(r360_frame* f);
/* Host images -> HBM (8 sensors contiguous).  Replaces loadFrame's decode step. */
int  r360_frame_upload(r360_frame* f, const uint8_t* bgr8, const uint16_t* depth8);
/* Same copy, enqueued on the ctx stream without waiting (OdometryRGBD360's per-frame input upload in
 * the pipelined sequence driver).  The host buffers must stay valid until the stream has consumed
 * them; page-locked buffers (r360_host_register) make the copy asynchronous to the host. */
int  r360_frame_upload_async(r360_frame* f, const uint8_t* bgr8, const uint16_t* depth8);
/* setSourceFrame / setTargetFrame(cv::Mat& imgRGB, cv::Mat& imgDepth) (RegisterPhotoICP.h:480-516): the
 * sphere as images (BGR u8 [sph_rows][sph_cols][3], range u16 mm [sph_rows][sph_cols], as sphereRGB /
 * sphereDepth) replaces the frame's and its pyramid is rebuilt.  The size must be the frame's. */
int  r360_frame_set_sphere(r360_frame* f, const uint8_t* bgr, const uint16_t* range_mm, int sph_rows, int sph_cols);
/* Page-lock / release host memory for asynchronous uploads (hipHostRegister). */
int  r360_host_register(void* p, size_t bytes);
int  r360_host_unregister(void* p);
/* Device-resident images (already in HBM on the ctx's device); copied device-to-device. */
int  r360_frame_upload_device(r360_frame* f, const void* d_bgr8, const void* d_depth8);
/* Frame360::loadFrame(path) (Frame360.h:231-266): Boost binary archive of 8 x {RGB, depth} and
 * the timestamp digit matrix (get_uint64_t_ofMatrixRepresentation, SerializeFrameRGBD.h:77-89). */
int  r360_frame_load_bin(r360_frame* f, const char* path);
/* Frame360::serialize(fileName) (Frame360.h:332-345): writes the raw images as loaded/uploaded. */
int  r360_frame_save_bin(r360_frame* f, const char* path);
/* Frame360::setTimeStamp / timeStamp (Frame360.h:181-184). */
int  r360_frame_set_timestamp(r360_frame* f, uint64_t ts);
int  r360_frame_get_timestamp(const r360_frame* f, uint64_t* ts);
int  r360_frame_build(r360_frame* f, unsigned flags);
int  r360_frame_build_async(r360_frame* f, unsigned flags);
/* r360_frame_build of n distinct frames of one device (Frame360::getPlanes of a keyframe batch, Frame360.h:615-640):
 * the plane stages of frames of one size run batched, up to 8 frames per launch of the plane kernels, on the stream
 * of frames[0]'s context; every other stage on each frame's own stream.  Synchronous; each frame's results equal
 * its r360_frame_build's. */
int  r360_frames_build(r360_frame* const* frames, int n, unsigned flags);
int  r360_frame_dims(const r360_frame* f, int* rows, int* cols, int* sph_rows, int* sph_cols);
/* RegisterPhotoICP::setNumPyr (RegisterPhotoICP.h:224-227) for the frame: its pyramid stops at n levels (default:
 * the calibration's full depth).  Alignments of the frame then take nPyr <= n. */
int  r360_frame_set_levels(r360_frame* f, int n);
/* Source-point compaction of the frame's pyramid builds (no reference counterpart: a layout choice).  all = 1
 * (default): every level's valid source pixels are compacted once per build, which a lone alignment's passes read
 * (PF 5).  all = 0: only the levels a batched pass cannot stream as an image are compacted (two launches per build
 * fewer, for frames that only enter batched alignments, e.g. a dense queue's); a lone alignment then streams the
 * images too.  Poses are equal to rounding either way.  Takes effect at the next build. */
int  r360_frame_set_compaction(r360_frame* f, int all);
/* The R360_BUILD_* stages the frame's current images have been through (an upload or load clears them), and
 * R360_BUILT_LEVEL0. */
int  r360_frame_built(const r360_frame* f, unsigned* flags);
/* sphereRGB (BGR u8) / sphereDepth (u16 range mm) (Frame360.h:104-107). */
int  r360_frame_get_sphere(r360_frame* f, uint8_t* bgr, uint16_t* depth);
/* Undistorted per-sensor depth in metres (CloudRGBD_Ext::m_depthEigUndistort). */
int  r360_frame_get_depth_m(r360_frame* f, float* depth8);
/* Pyramid level of the frame as RegisterPhotoICP sees it (gray /255, depth m, target
 * gradients with the alignFrames360 seam mask applied).  Any pointer may be NULL. */
int  r360_frame_get_level(r360_frame* f, int level, int* rows, int* cols, float* gray, float* depth,
                          float* gx, float* gy, float* dgx, float* dgy);
/* The saliency flags the pyramid build keeps per level-0 pixel for the level-0 ICP pass, which skips the gradient
 * gather and the terms of a target pixel the reference would skip (thresSaliencyIntensity / thresSaliencyDepth):
 * flags[i] bit 0 = !(|gx| < thr_int && |gy| < thr_int), bit 1 the same of the depth gradients with thr_depth, and the
 * thresholds they were built for (the r360_icp_default_params values; NaN: the frame has none).  An alignment with
 * thresholds at or above them uses the flags; one with lower thresholds does not, and is correct but slower.
 * flags: sph_rows x sph_cols bytes, or NULL. */
int  r360_frame_get_saliency(r360_frame* f, uint8_t* flags, float* thr_int, float* thr_depth);
/* The level's compacted ICP source points (valid depth, raster order) as {x, y, z, gray} quadruples:
 * LUT_xyz_sphere (RegisterPhotoICP.h:4553-4587) and the gray value.  *n = their count; copies min(n, cap). */
int  r360_frame_get_points(r360_frame* f, int level, float* xyzg, int cap, int* n);
/* Sensor k's pinhole pyramid level (R360_BUILD_SENSOR_PYRAMID; no seam mask). */
int  r360_frame_get_sensor_level(r360_frame* f, int sensor, int level, int* rows, int* cols, float* gray,
                                 float* depth, float* gx, float* gy, float* dgx, float* dgy);

/* ---------------------------------------------------------------- RegisterPhotoICP
 * Replaces include/RegisterPhotoICP.h:85-4784 (spherical path). */
enum { R360_PHOTO_CONSISTENCY = 0, R360_DEPTH_CONSISTENCY = 1, R360_PHOTO_DEPTH = 2 };

typedef struct {
    int    n_pyr;               /* setNumPyr (default 4; odometry apps use 5)  :224      */
    int    max_iters;           /* maxIters per level = 10                     :4593     */
    float  min_depth;           /* setMinDepth 0.3                             :202,230  */
    float  max_depth;           /* setMaxDepth 6.0                             :203,236  */
    float  std_dev_photo;       /* setGrayVariance: stdDevPhoto (6/255)        :208,242  */
    float  std_dev_depth;       /* setDepthVariance: stdDevDepth (0.2)         :211,248  */
    float  thres_sal_int;       /* thresSaliencyIntensity 0.01                 :218      */
    float  thres_sal_depth;     /* thresSaliencyDepth 0.01                     :219      */
    double tol_residual;        /* 1e-3                                        :4594     */
    double tol_update;          /* 1e-4                                        :4595     */
    double lambda;              /* 1.0, rank test only                         :4589     */
    int    fixed_iters_level0;  /* 0: reference schedule.  K>0: benchmark timing mode, exactly
                                   K candidate evaluations at level 0 (no convergence exit). */
} r360_icp_params;

typedef struct {
    int    iters[8];            /* num_iterations per level (:4772)          */
    int    evals[8];            /* candidate evaluations per level           */
    int    illposed;            /* 1: rank(H + lambda diag H) != 6 (:4682)   */
    float  sso;                 /* SSO (:3226)                               */
    double error;               /* accepted error at level 0                 */
    int    passes;              /* fused residual/Jacobian/JtJ passes run     */
    int    persistent;          /* r360_align360: 1 = each level ran as ONE launch (k_icp_level) instead of
                                   one launch per pass; same results either way */
    /* The public residual members RegisterPhotoICP leaves after the call (RegisterPhotoICP.h:183-189).
     * alignFrames360 with occlusion 1 / 2: avPhotoResidual / avDepthResidual of the last error evaluation
     * (errorPhotoICP_sphereOcc1 :3360-3362, Occ2 :3852-3853); avResidual is set only when ILL-POSED (= 0,
     * :4688).  alignFrames360 with occlusion 0 assigns none of them (errorPhotoICP_sphere does not).
     * alignFrames (pinhole): the values copied at the start of the last loop iteration (:4329-4332,
     * :4507-4509; errorPhotoICP :759-762).  residuals_set: bit 0 = avPhotoResidual / avDepthResidual
     * assigned, bit 1 = avResidual assigned; unassigned members keep their previous value in the façades. */
    double av_photo_residual;
    double av_depth_residual;
    float  av_residual;
    int    residuals_set;
} r360_icp_stats;

void r360_icp_default_params(r360_icp_params* p);

/* alignFrames360(pose_guess, method, occlusion) after setTargetFrame(trg)/setSourceFrame(src)
 * (:4519-4784).  pose_out = getOptimalPose(), H_out = getHessian(), g_out = getGradient().
 * Returns 1 (R360_ILLPOSED) when the reference would print "ILL-POSED" and return early. */
int r360_align360(r360_ctx* ctx, r360_frame* trg, r360_frame* src, const float init[16],
                  int method, int occlusion, const r360_icp_params* p,
                  float pose_out[16], float H_out[36], float g_out[6], r360_icp_stats* st);
int r360_align360_async(r360_ctx* ctx, r360_frame* trg, r360_frame* src, const float init[16],
                        int method, int occlusion, const r360_icp_params* p);
int r360_align360_result(r360_ctx* ctx, float pose_out[16], float H_out[36], float g_out[6],
                         r360_icp_stats* st);

/* Batched alignFrames360 (occlusion 0): n <= R360_MAX_BATCH independent alignments of pairs
 * (trg[j], src[j]) from init[16 j..], each the alignFrames360 of r360_align360 on that pair (same schedule,
 * same per-pair Gauss-Newton state and logic), run as one launch per pass over all pairs.  Batch-invariant:
 * a pair's result is bit-identical in any batch of any size, on any context or rank (the batched grid depends
 * on the level size only).  It equals r360_align360's result to rounding, not bit for bit: a lone alignment
 * sums the same pixels over twice the workgroup records (two per CU) and, on frames with compacted level-0
 * points, with PF 5 instead of PF 6, so a pair whose accept / stop test sits at a rounding edge can stop on
 * another pass (tests/test_gpu_batch_align.py pins the drift).  This is how the reference's callers' many alignFrames360 calls (one per
 * consecutive pair in OdometryRGBD360.cpp:141-257, per keyframe candidate in SphereGraphSLAM /
 * LoopClosure360) fill the GPU.  Frames must share one sphere size and may belong to any ctx of the device:
 * ctx's stream waits for the work already enqueued on their contexts' streams.  _result fills n poses /
 * H / g / stats (NULL skips) and returns the number of ILL-POSED alignments.  One batch per ctx at a time. */
#define R360_MAX_BATCH_ALIGN 16
int r360_align360_batch_async(r360_ctx* ctx, int n, r360_frame* const* trg, r360_frame* const* src,
                              const float* init, int method, const r360_icp_params* p);
int r360_align360_batch_result(r360_ctx* ctx, float* pose_out, float* H_out, float* g_out, r360_icp_stats* st);

/* Dense queue: the alignFrames360 calls of many concurrent registrations (one producer thread per pipeline
 * of frame builds + PbMap stages, e.g. OdometryRGBD360.cpp:141-257 sharded over pipelines) batched on one
 * stream.  A dispatcher thread runs every pending job (up to max_batch of one method / parameter set) as one
 * r360_align360_batch call; the next batch accumulates while one runs.  submit records the frames' build
 * work (their contexts' streams) and returns a ticket at once; collect waits for that job and returns
 * what r360_align360_batch_result returns for the job (0, 1 = ILL-POSED, < 0 error): the batched result,
 * the same in any batch, equal to a lone r360_align360 to rounding (above).  The frames must stay unmodified until
 * their job is collected: a batch waits on each frame's build event, which a rebuild re-records, so a frame
 * rebuilt between submit and dispatch fails the job with an error instead of aligning against the newer build.
 * Every ticket must be collected once.  Thread-safe. */
typedef struct r360_dense_queue r360_dense_queue;
int  r360_dense_queue_create(int device, int max_batch, r360_dense_queue** out);
void r360_dense_queue_destroy(r360_dense_queue* q);
/* the queue's own context (stream, in-kernel span counters, per-launch timing) */
r360_ctx* r360_dense_queue_ctx(r360_dense_queue* q);
int  r360_dense_queue_stats(r360_dense_queue* q, long* batches, long* jobs, int* max_batch_seen);
int  r360_dense_queue_submit(r360_dense_queue* q, r360_frame* trg, r360_frame* src, const float init[16],
                             int method, const r360_icp_params* p, long* ticket);
int  r360_dense_queue_collect(r360_dense_queue* q, long ticket, float pose_out[16], float H_out[36],
                              float g_out[6], r360_icp_stats* st);

/* One fused pass at a fixed pose: errorPhotoICP_sphere (:2545-2739) + calcHessGrad_sphere
 * (:2745-3228) at pyramid level `level`.  H/g in double (sum of the float per-pixel terms). */
int r360_icp_eval(r360_ctx* ctx, r360_frame* trg, r360_frame* src, int level, const float pose[16],
                  int method, const r360_icp_params* p, double H[36], double g[6],
                  double* err2, int* n_valid, int* n_visible);
/* Occlusion-aware pass at `pose` (alignFrames360 occlusion 1 / 2, :4598-4627): H / g of
 * calcHessGrad_sphereOcc{occ} and the value errorPhotoICP_sphereOcc{occ} returns (:3232-3370,
 * :3720-3855); occlusion 0 gives errorPhotoICP_sphere's value.  n_valid = the error's point count
 * (Occ1: photo + depth terms; Occ2: nValidDepthPts), n_visible = the HessGrad's numVisiblePixels. */
int r360_icp_eval_occ(r360_ctx* ctx, r360_frame* trg, r360_frame* src, int level, const float pose[16],
                      int method, int occlusion, const r360_icp_params* p, double H[36], double g[6],
                      double* error, int* n_valid, int* n_visible);

/* ---------------------------------------------------------------- pinhole alignFrames (per sensor)
 * RegisterPhotoICP::alignFrames(pose_guess, method) (:4254-4512) with errorPhotoICP (:560-761) and
 * calcHessGrad (:767-1100), after setTargetFrame / setSourceFrame on sensor k's raw images of two
 * frames (MethodsRegisterRGBD360.cpp:320-345).  Frames need R360_BUILD_SENSOR_PYRAMID.
 * K = {fx, fy, ox, oy} of level 0 (setCameraMatrix); NULL = the calibration's cameraMatrix.
 * Uses p->n_pyr, depth range, std devs and saliency thresholds; the Levenberg-Marquardt constants are
 * alignFrames' own (lambda 0.01, step 10, 10 iterations, tolerances 1e-4).  Returns 1 if ILL-POSED. */
int r360_align_pinhole(r360_ctx* ctx, r360_frame* trg, r360_frame* src, int sensor, const float init[16],
                       int method, const float* K, const r360_icp_params* p, float pose_out[16], float H_out[36],
                       float g_out[6], r360_icp_stats* st);
/* Up to 8 alignments at once (one per listed sensor, init = n x float[16]); _result fills n poses /
 * H / g / stats and returns the number of ILL-POSED jobs. */
int r360_align_pinhole_async(r360_ctx* ctx, r360_frame* trg, r360_frame* src, int n, const int* sensors,
                             const float* init, int method, const float* K, const r360_icp_params* p);
int r360_align_pinhole_result(r360_ctx* ctx, float* poses, float* H, float* g, r360_icp_stats* st);
/* One errorPhotoICP + calcHessGrad pass at `pose` (parity hook): error = avResidual (NaN for
 * PHOTO_CONSISTENCY, as the reference), res = {PhotoResidual, DepthResidual},
 * counts = {nValidPhotoPts, nValidDepthPts, visible}. */
int r360_pinhole_eval(r360_ctx* ctx, r360_frame* trg, r360_frame* src, int sensor, int level, const float pose[16],
                      int method, const float* K, const r360_icp_params* p, double H[36], double g[6],
                      double* error, double res[2], int counts[3]);

/* ---------------------------------------------------------------- RegisterDensePhotoICP (A19)
 * RegisterRGBD360::RegisterDensePhotoICP(frame1, frame2, pose_estim, method, registMode)
 * (RegisterRGBD360.h:344-520): the 8 sensors' pinhole images of frame2 (source) against frame1's
 * (target), Jacobians in the rig frame (calcPhotoICPError_robot, RegisterPhotoICP.h:4905-5076;
 * calcHessianGradient_robot, :5083-5407), sensors summed, LM per level (lambda 1e-3, step 10,
 * tol_residual 0.1).  Frames need R360_BUILD_SENSOR_PYRAMID; p = NULL uses RegisterPhotoICP()'s
 * defaults (4 levels).  As in the reference, the "new" error is evaluated at the unchanged pose, so
 * pose_out = pose_estim and info_out = the Hessian of the last level whose loop ran.
 * Returns 1 (the reference's true) or 0 (ILL-POSED: false, info_out untouched). */
typedef struct {
    double error[8];            /* per level: sum over sensors of calcPhotoICPError_robot   */
    int    ran[8];              /* 1 if the level's LM loop ran (error > tol_residual 0.1)   */
    int    n_visible[8];        /* HessGrad visible pixels per level, 8 sensors             */
    int    n_error[8];          /* error-term visible pixels per level, 8 sensors           */
    int    illposed_level;      /* -1, or the level whose rank test failed                  */
    int    levels;
    int    info_set;            /* 0 if no level ran (the reference's Hessian is then undefined; info = 0) */
    int    pad;
    float  gradient[6];         /* the summed gradient of that level                        */
} r360_dense_stats;
int r360_register_dense(r360_ctx* ctx, r360_frame* frame1, r360_frame* frame2, const float pose_estim[16],
                        int method, int mode, const r360_icp_params* p, float pose_out[16], float info_out[36],
                        r360_dense_stats* st);
/* Parity hook: one level's 8 sensors at `pose`: err[2k] / err[2k+1] = sensor k's photometric / depth
 * part of calcPhotoICPError_robot, H / g = calcHessianGradient_robot's (double sums of the float
 * terms), counts[3k..] = {error visible, error depth terms, HessGrad visible}. */
int r360_dense_robot_eval(r360_ctx* ctx, r360_frame* frame1, r360_frame* frame2, int level, const float pose[16],
                          int method, const r360_icp_params* p, double err[16], double H[8 * 36], double g[8 * 6],
                          int counts[8 * 3]);

/* CPose3D::exp(mu, pseudo) (MRPT; used at RegisterPhotoICP.h:4697). */
void r360_exp_se3(const double mu[6], int pseudo, float T[16]);

/* ---------------------------------------------------------------- PbMap (Frame360 planes)
 * Frame360::getPlanes (Frame360.h:615-640) runs when a frame is built with R360_BUILD_PLANES:
 * cloud + bilateral filter + normals + segmentation on the GPU, per-plane descriptors and the
 * sensor grouping/merging on the host.  One plane = the mrpt::pbmap::Plane fields used on the
 * path, in the rig frame. */
typedef struct {
    float normal[3], center[3], d, area, elongation, curvature, ppal[3], nrgb[3], intensity;
    int   id, sensor, n_inliers, n_hull;
} r360_plane;

int r360_frame_get_planes(r360_frame* f, r360_plane* out, int cap, int* n);
/* The planes of one sensor as getPlanesSensor left them, before groupPlanes / mergePlanes, of a frame built with
 * R360_BUILD_PLANES | R360_BUILD_LOCAL_PLANES (R360_EINVAL without the flag): normal, center, d and ppal taken back
 * to the SENSOR's frame with the build's own Rt_k.  labels: the region labels (r360_frame_get_labels' labf, within
 * the sensor's image) merged into plane `plane`, in merge order. */
int r360_frame_get_local_planes(r360_frame* f, int sensor, r360_plane* out, int cap, int* n);
int r360_frame_get_local_plane_labels(r360_frame* f, int sensor, int plane, int* labels, int cap, int* n);
/* Plane::label of plane i (set by the labelization tools, LabelizeFrame360.cpp).  get returns the
 * label length and copies at most cap-1 bytes plus a terminator. */
int r360_frame_set_plane_label(r360_frame* f, int i, const char* label);
int r360_frame_get_plane_label(r360_frame* f, int i, char* buf, int cap);
/* Closed convex hull polygon (polygonContourPtr) of plane i, xyz triples. */
int r360_frame_get_plane_hull(r360_frame* f, int i, float* xyz, int cap, int* n);

/* ---------------------------------------------------------------- keyframe persistence
 * Frame360::sphereCloud (Frame360.h:120): buildSphereCloud's concatenation of the 8 filtered
 * clouds in the rig frame (width = 8*rows/2, height = cols/2), or the cloud set by loadCloud.
 * xyz [cap][3], rgba [cap] (PointXYZRGBA packing b | g<<8 | r<<16 | a<<24); either may be NULL. */
int r360_frame_get_sphere_cloud(r360_frame* f, float* xyz, uint32_t* rgba, size_t cap, int* width, int* height);
/* pcl::io::savePCDFile / PCDReader::read for PointXYZRGBA (Frame360.h:187-193, 326).
 * mode 0 = DATA ascii (the reference's call), 1 = binary, 2 = binary_compressed (LZF). */
int r360_pcd_write(const char* path, const float* xyz, const uint32_t* rgba, int width, int height, int mode);
int r360_pcd_read(const char* path, float* xyz, uint32_t* rgba, size_t cap, size_t* n, int* width, int* height);
int r360_frame_save_cloud(r360_frame* f, const char* path, int mode);
/* loadCloud (Frame360.h:187-193): sets the frame's sphereCloud. */
int r360_frame_load_cloud(r360_frame* f, const char* path);
/* savePlanes / loadPbMap (Frame360.h:195-210, 312-318): gzip file of the frame's PbMap (format in
 * DESIGN.md; MRPT's CSerializable layout is not restated).  A loaded PbMap replaces the frame's
 * planes and registers (r360_register_pbmap) exactly as the one that was saved. */
int r360_frame_save_planes(r360_frame* f, const char* path);
int r360_frame_load_pbmap(r360_frame* f, const char* path);
/* save(path, frame) (Frame360.h:320-330) and load_PbMap_Cloud(path, index) (:222-228):
 * dir/sphereCloud_<i>.pcd + dir/spherePlanes_<i>.pbmap. */
int r360_frame_save(r360_frame* f, const char* dir, unsigned index);
int r360_frame_load_pbmap_cloud(r360_frame* f, const char* dir, unsigned index);

/* ---------------------------------------------------------------- RegisterRGBD360
 * Replaces include/RegisterRGBD360.h:97-337.  registrationType (:260-266). */
enum { R360_DEFAULT_6DoF = 0, R360_PLANAR_3DoF = 1, R360_ODOMETRY_6DoF = 2, R360_PLANAR_ODOMETRY_3DoF = 3 };

/* SubgraphMatcher thresholds: the [global]/[unary]/[binary] keys of the mrpt-pbmap config file that
 * RegisterRGBD360(configFile) loads (RegisterRGBD360.h:97-100, config_files/configLocaliser_*.ini).  A ctx
 * (and each lane of a batch) holds one set; r360_register_pbmap, r360_register* and the batch use it. */
typedef struct {
    int   min_planes_recognition;   /* [global]; RegisterPbMap itself requires 3 matches (:306)            */
    float dist_d;                   /* [unary] plane offset difference (m)                                  */
    float angle;                    /* [unary] normal angle (deg), odometry modes                           */
    float color_threshold;          /* [unary] normalised-rgb difference                                    */
    float intensity_threshold;      /* [unary]                                                              */
    float elongation_threshold;     /* [unary] ratio                                                        */
    float area_threshold;           /* [unary] ratio                                                        */
    float dist_threshold;           /* [binary] centroid-distance ratio                                     */
    float angle_threshold;          /* [binary] relative-normal-angle difference (deg)                      */
    float height_threshold;         /* [binary] relative height of parallel planes (m)                      */
    float cos_angle_parallel;       /* [binary]                                                             */
    float planar_normal_angle;      /* planar modes: vertical-normal tolerance (deg; not an ini key, 10)    */
    long  max_nodes;                /* interpretation-tree node budget: a guard against pathological inputs  */
} r360_match_params;
/* The configLocaliser_sphericalOdometry.ini values (the odometry apps' file). */
void r360_match_params_default(r360_match_params* m);
/* Reads an mrpt-pbmap ini file into m (keys absent from the file keep m's values).  Returns 0, <0 if the
 * file cannot be read. */
int  r360_match_params_load_ini(const char* path, r360_match_params* m);
int  r360_ctx_set_match_params(r360_ctx* ctx, const r360_match_params* m);
int  r360_ctx_get_match_params(const r360_ctx* ctx, r360_match_params* m);
/* The interpretation-tree searches run on ctx (every RegisterPbMap), how many of them stopped at max_nodes, and the
 * most nodes one search visited.  MRPT's SubgraphMatcher (RegisterRGBD360.h:294) searches exhaustively; this one
 * prunes with forward checking (exhaustive result), so a search that reaches the budget is the only way its result
 * can differ from the exhaustive one — and it is counted here, never silent. */
int  r360_ctx_match_stats(r360_ctx* ctx, long* calls, long* truncated, long* max_nodes);
/* That search alone over given tables (host only; the layout r360_pbmap_match_tables returns, areas of the
 * reference planes): best[i] = matched target of reference i or -1.  Returns 1 if max_nodes stopped it, 0 if not. */
int  r360_match_tree_search(int ns, int nt, const uint8_t* unary, const uint64_t* binary, int words,
                            const double* area, long max_nodes, int* best, long* nodes);

/* RegisterPbMap(ref, trg, max_match_planes, mode) (:276-337): returns 1 (good alignment) or 0
 * (insufficient matching / ill-conditioned; pose and info are then left untouched, :306-310).
 * pose = getPose() (target as seen from the reference), info = getInfoMat(), match_pairs =
 * getMatchedPlanes() as (ref id, trg id) pairs, area_matched = getAreaMatched(),
 * area_src/area_trg = the public areaSource/areaTarget members. */
int r360_register_pbmap(r360_ctx* ctx, r360_frame* ref, r360_frame* trg, size_t max_match_planes, int mode,
                        float pose[16], float info[36], int* match_pairs, int pair_cap, int* n_match,
                        float* area_matched, float* area_src, float* area_trg);
/* Register(): RegisterPbMap, then alignFrames360 initialised with rotOffset * P * rotOffset^-1
 * (OdometryKeyFrame360.cpp:167-171, 205, 244-254; guess replaces P when the PbMap registration
 * fails); pose = rotOffset^-1 * getOptimalPose() * rotOffset.  Returns 0, or 1 when the PbMap stage
 * failed and the dense stage started from guess. */
int r360_register(r360_ctx* ctx, r360_frame* ref, r360_frame* trg, const float guess[16],
                  const r360_icp_params* p, size_t max_match_planes, int mode, float pose[16],
                  float info[36], r360_icp_stats* st);
/* Split form for pipelining several pairs: the PbMap stage runs at the call (it waits for the two
 * frames' plane builds), the dense stage is enqueued on ctx's stream; _result waits for it. */
int r360_register_async(r360_ctx* ctx, r360_frame* ref, r360_frame* trg, const float guess[16],
                        const r360_icp_params* p, size_t max_match_planes, int mode);
int r360_register_result(r360_ctx* ctx, float pose[16], float info[36], r360_icp_stats* st);
/* Register() with the dense stage on a dense queue: the PbMap stage runs at the call on ctx (waiting for the
 * frames' plane builds), the rotOffset-conjugated alignFrames360 is submitted to q; collect waits for it and
 * returns what r360_register_result returns. */
int r360_register_submit(r360_ctx* ctx, r360_dense_queue* q, r360_frame* ref, r360_frame* trg, const float guess[16],
                         const r360_icp_params* p, size_t max_match_planes, int mode, long* ticket);
int r360_register_collect(r360_dense_queue* q, long ticket, float pose[16], float info[36], r360_icp_stats* st);

/* OdometryRGBD360 over a frame sequence, pipelined on one GPU (Registration/OdometryRGBD360.cpp:141-257,
 * BASELINE configs[3]; host/sequence.cpp).  Pairs (i, i+1) of [p0, p1) are split into contiguous runs, one per
 * pipeline (a host thread of the object with its own r360_ctx and ring of Frame360 buffers); per pair the new frame
 * is uploaded and built on the GPU and registered with the Register() alias (RegisterPbMap -> rotOffset conjugation
 * -> alignFrames360, OdometryKeyFrame360.cpp:205-254).  With queue > 0 the alignments of all pipelines are batched on
 * one dense queue, `depth` in flight per pipeline, frames built `lookahead` ahead.  Each pair's record equals the
 * single-pair Register() result. */
enum { R360_SEQ_FULL = 0,     /* configs[3]: Register() per pair                                        */
       R360_SEQ_PLANES = 1,   /* configs[1]: planes + RegisterPbMap only                                  */
       R360_SEQ_DENSE = 2 };  /* configs[2] / [4]: stitch + pyramid + alignFrames360 from identity       */
/* One pair record (floats): pose [0,16) column-major in the rig frame of the pair's first frame, PbMap information
 * [16,52), status [52] (0 PbMap good, 1 PbMap failed and the dense stage started from identity, 2 ill-posed), SSO
 * [53], the accepted level-0 error [54], [55] spare. */
#define R360_SEQ_RECORD 56
typedef struct {
    int rows, cols;                 /* per-sensor image size                                            */
    int pipelines;                  /* host threads + streams                                           */
    int queue;                      /* dense queue batch (pairs per launch); 0 = each pipeline aligns alone */
    int depth;                      /* queued: alignments in flight per pipeline                        */
    int lookahead;                  /* queued: frames built ahead of the pair in hand                   */
    int plane_batch;                /* plane stages of up to this many frames per launch on one stream (0: each
                                       pipeline builds its frames' planes on its own stream)            */
    int workload;                   /* R360_SEQ_*                                                       */
    size_t max_match_planes;        /* RegisterPbMap (25)                                               */
    int mode;                       /* registrationType (PLANAR_3DoF)                                   */
    r360_icp_params icp;            /* alignFrames360 (nPyr 5, stdDevPhoto 3/255, 20 level-0 iterations) */
} r360_sequence_params;
typedef struct r360_sequence r360_sequence;
void r360_sequence_default_params(r360_sequence_params* p);
/* extrinsics_dir: Rt_0{1..8}.txt (NULL / "" = the shipped calibration) */
int  r360_sequence_create(int device, const r360_sequence_params* p, const char* extrinsics_dir, r360_sequence** out);
void r360_sequence_destroy(r360_sequence* s);
/* Registers pairs [p0, p1) `repeats` times.  Frame i's raw images (BGR u8 8 x rows x cols x 3, depth u16 mm
 * 8 x rows x cols) are bgr[i - p0] / depth[i - p0] for i in [p0, p1]: host memory (page-locked for asynchronous
 * uploads) or, with device_inputs, device memory.  The repeats x (p1 - p0) registrations form one stream (repeat-
 * major) cut into P contiguous pieces, one per pipeline; runs (optional): n_runs (first, last + 1) pairs tiling
 * [p0, p1) in order, pipeline k taking run k of every repeat instead.  records: repeats x (p1 - p0) x
 * R360_SEQ_RECORD floats.  Returns 0, or < 0 with the failing pipeline's error. */
int  r360_sequence_run(r360_sequence* s, int p0, int p1, const void* const* bgr, const void* const* depth,
                       int device_inputs, int repeats, const int* runs, int n_runs, float* records);
/* Pipelines and the dense queue (NULL when unqueued). */
int  r360_sequence_info(r360_sequence* s, int* pipelines, r360_dense_queue** queue);
/* The plane queue's batches, frames and largest batch so far, and its context (NULL without one). */
int  r360_sequence_plane_stats(r360_sequence* s, long* batches, long* frames, int* max_batch_seen, r360_ctx** ctx);
/* Pipeline p's context, calibration, frame ring (up to cap handles) and OS thread id. */
int  r360_sequence_pipeline(r360_sequence* s, int p, r360_ctx** ctx, r360_calib** calib, r360_frame** frames, int cap,
                            int* n_frames, long* thread_id);
/* Host seconds per pipeline since the last reset: out[8 p + k], k = 0 load + build enqueue (with the collects that
 * free a buffer), 1 PbMap stage (RegisterPbMap and submit), 2 dense wait, 3 pairs registered; within 0: 4 build
 * enqueue, 5 upload enqueue, 6 (queued) collects before a buffer refill; 7 unused. */
int  r360_sequence_host_times(r360_sequence* s, double* out, int reset);
/* Parity hook: the two raster sweeps of OrganizedMultiPlaneSegmentation::refine as k_refine* run them, on
 * 8 sensors' refinement states (-1 no label, -2 non-planar label, m >= 0 planar model m) and closeness
 * masks (bit m: the pixel is within 0.02 of model m), w x h each; rb = -1: the wavefront sweeps (the
 * default path: 64-row bands pipelined through LDS for h <= 512), -2: the wavefront with a workgroup barrier
 * per diagonal, 0: one wave per sensor walks all rows, rb > 0: rb rows per band.  out = the swept states.
 * Returns the number of sensors whose wavefront second sweep needed corrections of the flat-index wrap push
 * (re-runs or the single-wave fallback; rb < 0), else 0; < 0 on error. */
int r360_refine_eval(const int8_t* state, const uint64_t* mask, int w, int h, int rb, int8_t* out);
/* SubgraphMatcher constraint tables (k_match_tables): unary [ns][nt], binary [(i*nt+j)][words]
 * bitsets over (k*nt+l).  Returns words.  Inspection/parity hook. */
int r360_pbmap_match_tables(r360_ctx* ctx, r360_frame* ref, r360_frame* trg, size_t max_match_planes,
                            int mode, int* ns, int* nt, int* sid, int* tid, uint8_t* unary,
                            uint64_t* binary, int cap);

/* ---------------------------------------------------------------- batched registrations (§8f-4)
 * Many independent pair registrations on one GPU, as SphereGraphSLAM's tracking loop
 * (SLAM/SphereGraphSLAM.cpp:169-231: RegisterPbMap against up to numCheckRegistration = 5 previous
 * keyframes) and LoopClosure360's candidate checks (include/LoopClosure360.h:280-366: RegisterPbMap
 * PLANAR_3DoF, gate on matches/area, alignFrames360 refinement) issue them.  A batch owns `lanes`
 * worker contexts (own HIP stream, ICP state and matcher scratch) and runs the jobs of one call
 * concurrently, one host thread per lane.  Every job is the sequential call itself on its lane's
 * context: the result of a batched job is identical to r360_register_pbmap / r360_align360 on the
 * same frames (lone alignments, not the batched grid of r360_align360_batch).  Frames may belong to any ctx of the same device; each lane's stream waits for
 * the frames' build work before reading them.  The caller must not modify or destroy a frame while a
 * batch call that names it runs.  Calls on one batch are serialised: a call made while another thread's
 * call runs waits for it. */
typedef struct r360_batch r360_batch;
int  r360_batch_create(int device, int lanes, r360_batch** out);
void r360_batch_destroy(r360_batch* b);
int  r360_batch_lanes(const r360_batch* b);
/* The matcher thresholds of every lane (r360_ctx_set_match_params). */
int  r360_batch_set_match_params(r360_batch* b, const r360_match_params* m);

/* dense stage of one job */
enum {
    R360_JOB_PBMAP_ONLY = 0,  /* RegisterPbMap only (SphereGraphSLAM tracking)                          */
    R360_JOB_GATED = 1,       /* alignFrames360 only when RegisterPbMap succeeded with n_match > min_matches
                                 and area_matched > min_area (LoopClosure360.h:298, 342)                */
    R360_JOB_ALWAYS = 2       /* Register(): alignFrames360 from the PbMap pose, or from `guess` when the
                                 PbMap stage failed (OdometryKeyFrame360.cpp:205-254)                   */
};
typedef struct {
    r360_frame* ref;          /* RegisterPbMap(ref, trg, ...): pRef360 (RegisterRGBD360.h:276)           */
    r360_frame* trg;
    int   dense;              /* R360_JOB_*                                                               */
    int   ref_is_source;      /* dense roles. 0: setTargetFrame(ref), setSourceFrame(trg)
                                 (OdometryKeyFrame360.cpp:248-249, LoopClosure360.h:348-349).
                                 1: setSourceFrame(ref), setTargetFrame(trg) (LoopClosure360.h:309-310) */
    float guess[16];          /* R360_JOB_ALWAYS fallback pose (rig frame)                               */
} r360_pair_job;
typedef struct {
    int   good;               /* RegisterPbMap's return value (1 / 0)                                    */
    int   n_match;            /* getMatchedPlanes().size()                                               */
    float area_matched, area_src, area_trg, sso_pbmap;   /* getAreaMatched(), areaSource, areaTarget,
                                 areaMatched / areaSource (SphereGraphSLAM.cpp:214-215; 0 if not good)   */
    float pbmap_pose[16];     /* getPose() (identity if not good)                                        */
    float pbmap_info[36];     /* getInfoMat() (zeros if not good)                                        */
    int   dense_rc;           /* -1: dense stage not run; 0 ok; 1 ill-posed (R360_ILLPOSED)               */
    float pose[16];           /* rotOffset^-1 * getOptimalPose() * rotOffset (LoopClosure360.h:313, 352) */
    float hessian[36];        /* getHessian()                                                            */
    r360_icp_stats stats;     /* SSO, accepted error, iterations                                         */
} r360_pair_result;

/* Runs the n jobs.  max_match_planes/mode apply to every RegisterPbMap; min_matches/min_area gate
 * R360_JOB_GATED jobs; p = the dense stage's RegisterPhotoICP parameters (PHOTO_DEPTH, occlusion 0).
 * Returns 0, or the first job error (< 0, message in r360_last_error()). */
int r360_batch_register(r360_batch* b, const r360_pair_job* jobs, int n, size_t max_match_planes, int mode,
                        int min_matches, float min_area, const r360_icp_params* p, r360_pair_result* out);

/* SphereGraphSLAM tracking step (SphereGraphSLAM.cpp:169-231): RegisterPbMap(kfs[j], frame,
 * max_match_planes, mode) for j = n_kf-1, n_kf-2, ... (newest keyframe first) while fewer than
 * num_check candidates and fewer than no_assoc_threshold failures were tried; the first good one wins.
 * All candidates are registered at once; *chosen = index into kfs of the winner, or -1 ("No
 * registration available").  result (optional) = the winner's r360_pair_result; cand (optional,
 * min(n_kf, num_check, no_assoc_threshold) entries) = every candidate's result in reference order. */
int r360_track_frame(r360_batch* b, r360_frame* const* kfs, int n_kf, r360_frame* frame, int num_check,
                     int no_assoc_threshold, size_t max_match_planes, int mode, int* chosen,
                     r360_pair_result* result, r360_pair_result* cand);

/* Inspection hooks of the per-pixel plane half (parity tests).  Sizes: 8 x (rows/2) x (cols/2). */
typedef struct {
    int   label, count, start_idx, n_contour, n_fit;
    float centroid[3], cov[9], model[4], curvature;
} r360_region;
int r360_frame_get_cloud(r360_frame* f, float* xyz4, uint8_t* rgb4, float* nrm4, float* dist);
int r360_frame_get_labels(r360_frame* f, int* lab, int* labf);
int r360_frame_get_regions(r360_frame* f, int sensor, r360_region* out, int cap, int* n);
/* Parity hook: the frame's segmentation stage on given fields instead of the ones its depth images give.  xyz4
 * [8][h][w][4] (h = rows / 2, w = cols / 2; NaN = no point), nrm [8][h][w][nrm_comps] (nrm_comps 3 or 4: unit
 * normals, NaN = none) and rgb4 [8][h][w][4] {r, g, b, -} go where k_cloud, k_normals and k_rgb write: the points as
 * {x, y, z, 0}, the normals with their fourth component p.n computed on the device as k_normals computes it (a given
 * fourth component is ignored), the colours through the centre pixels of the frame's BGR images, which the stage's
 * k_rgb reads (the frame's uploaded images are overwritten: upload again before an ordinary build).  Then the
 * ordinary launcher of a build (connected components, plane fits, refinement, statistics, contours, voxel fallback,
 * hull prefilter, publication) runs on the frame's buffers on its context's stream.  The host assembly does not
 * run: the frame's PbMap is empty afterwards.  r360_frame_get_labels, r360_frame_get_regions and
 * r360_frame_get_region_detail show the result.  Returns 0, or < 0 with the capacity error of an ordinary build
 * ("plane segmentation capacity exceeded (code ...)"); *err_code (optional) receives the stage's error bits. */
int r360_frame_segment_eval(r360_frame* f, const float* xyz4, const float* nrm, int nrm_comps, const uint8_t* rgb4,
                            int* err_code);
/* The same for n <= 8 frames of one context and size as one batch of the stage's launcher (the batch a plane queue or
 * r360_frames_build forms): xyz4, nrm and rgb4 hold the frames' fields one after the other, err_codes[n] (optional)
 * receives each frame's error bits.  Returns < 0 if any frame's stage failed. */
int r360_frames_segment_eval(r360_frame* const* frames, int n, const float* xyz4, const float* nrm, int nrm_comps,
                             const uint8_t* rgb4, int* err_codes);
/* Parity hook: the refinement's states [8][h][w] after its two sweeps (-1 no label, -2 non-planar label, m >= 0
 * model m of the sensor) as the frame's last build or segment_eval left them, and the wavefront sweeps' flags[24]:
 * [s] != 0: the single-wave fallback redid sensor s's second sweep, [8 + s]: re-runs of its second sweep after wrap
 * pushes, [16 + s] != 0: its pipelined first sweep gave up and the fallback redid both sweeps. */
int r360_frame_get_refine_states(r360_frame* f, int8_t* state, int* flags);
/* Test hook: the frame builds that follow hand the sensors of sensor_mask (bit 8 * frame-in-batch + sensor) to the
 * single-wave fallback kernel after their wavefront sweeps, as if the second sweep's re-runs had run out at the middle
 * row (first_sweep = 0) or the pipelined first sweep had given up (first_sweep != 0); the results must not change.
 * No field makes a build take that path.  0 switches it off.  Process-wide, not for concurrent builds. */
void r360_refine_force_fallback(uint64_t sensor_mask, int first_sweep);
/* Region `region` of `sensor` as the segmentation stage left it, before the hull prefilter and the host assembly:
 * stats[20] = the final inliers' exact moments (PlaneOut::stats: n, s1[3], s2[6] as (low, high) 64-bit words,
 * c[4]), bounds[6] = local-frame min xyz, max xyz, and the traced contour's points in trace order from the device
 * pool (contour4 [cap][4], optional; *n_contour = their number, 0 for a region that takes the voxel fallback). */
int r360_frame_get_region_detail(r360_frame* f, int sensor, int region, int64_t* stats, float* bounds,
                                 float* contour4, int cap, int* n_contour);

/* ---------------------------------------------------------------- multi-GPU sequence driver (§8(e))
 * Pairs of a sequence shard one contiguous run per GPU (one process per GPU); the per-pair records
 * {pose, information, status, ...} are all-gathered to every rank over RCCL (xGMI) and rank 0 composes the
 * trajectory (Registration/OdometryRGBD360.cpp:257).  Rank 0 creates the id; the caller distributes it.
 * Host buffers in and out; each call returns when its result is on the host. */
typedef struct r360_comm r360_comm;
int  r360_comm_unique_id(uint8_t id[128]);
int  r360_comm_init(int device, int nranks, int rank, const uint8_t id[128], r360_comm** out);
void r360_comm_destroy(r360_comm* c);
/* recv[r * bytes .. (r + 1) * bytes) = rank r's send (ncclAllGather). */
int  r360_comm_allgather(r360_comm* c, const void* send, void* recv, size_t bytes);
/* v[i] = max over the ranks of v[i] (ncclAllReduce / ncclMax, f64). */
int  r360_comm_allreduce_max(r360_comm* c, double* v, int n);

/* Plain device buffers (inputs kept resident in HBM, r360_frame_upload_device).  kind: 0 host->device,
 * 1 device->host, 2 device->device; synchronous. */
int  r360_dev_alloc(int device, size_t bytes, void** out);
int  r360_dev_free(void* p);
int  r360_dev_copy(void* dst, const void* src, size_t bytes, int kind);

/* ---------------------------------------------------------------- synthetic scenes
 * Procedural indoor room rendered by the 8 rig cameras.  Deterministic in
 * (seed, frame).  Rig pose of frame `frame` along the generator's planar path; pose_out
 * (column-major) is that rig pose in the room frame. */
int r360_synth_frame(const r360_calib* calib, uint32_t seed, const float rig_pose[16],
                     uint8_t* bgr8, uint16_t* depth8);
/* Host-only variant (no GPU needed): rt8 = the 8 extrinsics Rt_k, column-major, back to back. */
int r360_synth_frame_rt(int rows, int cols, const float* rt8, uint32_t seed, const float rig_pose[16],
                        uint8_t* bgr8, uint16_t* depth8);
int r360_synth_path_pose(uint32_t seed, int frame, float pose_out[16]);

/* ---------------------------------------------------------------- test hooks
 * The float asinf/atan2f program used by the projection (libm_f32.h, bit-identical to x86-64 glibc)
 * evaluated on the host (on_device = 0) or on the GPU (on_device = 1). */
/* The ICP pass's fast-guarded vs the exact spherical projection of points (X, Y, Z) for an
 * nRows x nCols sphere: pixel-decision mismatches (must be 0) and deferred (exact) lanes.  _pose:
 * LUT points (lx, ly, lz) transformed by pose (col-major 4x4) first, fast and exact transforms. */
int r360_proj_check(const float* X, const float* Y, const float* Z, int n, int nRows, int nCols,
                    unsigned long long* mismatches, unsigned long long* fallbacks);
int r360_proj_check_pose(const float* lx, const float* ly, const float* lz, int n, const float pose[16], int nRows,
                         int nCols, unsigned long long* mismatches, unsigned long long* fallbacks);
/* sqrt_rn / div_rn (the pass's correctly rounded f32 sqrt / division) against the compiler's IEEE
 * operations on n hashed operands: out = {sqrt mismatches, division mismatches}, both must be 0. */
int r360_rn_check(unsigned n, unsigned seed, unsigned long long out[2]);
/* The device ILL-POSED test: Eigen FullPivLU<Matrix<float,6,6>>::rank() of n row-major matrices. */
int r360_rank6(const float* M, int n, int* ranks);
/* The device GN solve x = -H^-1 g (RegisterPhotoICP.h:4693; Gaussian elimination with partial pivoting in
 * double) of n systems: H row-major n x 36, g n x 6, x n x 6. */
int r360_solve6(const double* H, const double* g, int n, double* x);
/* What the pass launcher picks for level `level` of src_frame (host only, nothing is launched): the pass form
 * (PF) and the workgroups per job, for a lone pass (batched = 0; occlusion 0 / 1 / 2) or a batched launch
 * (batched = 1; occlusion 0 only). */
int r360_icp_pass_grid(r360_ctx* ctx, const r360_frame* src_frame, int level, int occlusion, int batched, int* pf,
                       int* nb);
/* r360_icp_eval on the batched grid: one eval-only pass of n <= R360_MAX_BATCH_ALIGN jobs at `level`, the jobs
 * prepared and launched as r360_align360_batch_async prepares and launches its passes.  poses: n col-major 4x4;
 * every output holds n entries (H n x 36, g n x 6), job j's raw pass sums.  Refused while a batch is pending. */
int r360_icp_eval_batch(r360_ctx* ctx, int n, r360_frame* const* trg, r360_frame* const* src, int level,
                        const float* poses, int method, const r360_icp_params* p, double* H, double* g,
                        double* err2, int* n_valid, int* n_visible);
int r360_libm_eval(const float* x, const float* y, const float* z, int n, float* asin_out, float* atan2_out,
                   int on_device);

/* s_memrealtime stamps (100 MHz) of the last ICP pass; written only by a -DR360_STAMPS build. */
int r360_ctx_debug_stamps(r360_ctx* ctx, unsigned long long* out12);

/* Lone alignFrames360 (r360_align360*, occlusion 0) as ONE launch per pyramid level (k_icp_level: the level's passes
 * in a persistent grid, the step's workgroup handing each pass over to the others) instead of one launch per pass.
 * Same grid, records and steps: results are bit-identical either way (st->persistent says which ran).  Off by
 * default: measured slower on MI355X.  Used only when every level's grid fits one resident
 * round and no other persistent alignment of the process is in flight. */
int r360_ctx_persistent_levels(r360_ctx* ctx, int enable);

/* Latency mode (no reference counterpart: a scheduling choice; on by default).  On: a thread waiting for the PbMap of
 * a frame built on ctx polls the frame's GPU part itself and runs its assembly tasks; r360_frame_upload_async copies
 * the depth images first and the BGR images on a second stream beside the plane stage's geometric part; a lone
 * frame's plane stage is replayed as two graphs.  Off: waits sleep on the assembly pool, both copies and every
 * launch go in the ctx stream's order (what a context among many pipelines wants: the sequence runner turns it off
 * for more than one pipeline).  Results are the same either way, bit for bit. */
int r360_ctx_latency_mode(r360_ctx* ctx, int enable);

/* ---------------------------------------------------------------- timing hooks (bench) */
/* enable: 0 off, 1 every launch on ctx's stream, 2 the level-0 ICP passes only (HIP events around each) */
int r360_ctx_timing(r360_ctx* ctx, int enable);
/* Per-kernel accumulated device time (ms) and launch counts since the last reset. */
int r360_ctx_timing_read(r360_ctx* ctx, const char* kernel, double* ms, long* launches);
int r360_ctx_timing_reset(r360_ctx* ctx);
/* In-kernel execution spans of the fused ICP passes at one pyramid level (earliest workgroup start to
 * the end of the last workgroup, s_memrealtime), summed in microseconds, and the pass count, since the
 * last reset.  Unlike stream events they exclude queueing behind other streams' kernels. */
int r360_ctx_kernel_time(r360_ctx* ctx, int level, double* us_sum, long* passes);
/* the same, plus the job passes those launches ran (a batched launch runs one per pair; NULL skips) */
int r360_ctx_kernel_stats(r360_ctx* ctx, int level, double* us_sum, long* launches, long* job_passes);
/* Profiling: host time of the ctx's RegisterPbMap calls: out[0] s waiting for the frames' PbMaps (GPU plane
 * stage + host assembly), out[1] s in the match tables, out[2] s in the interpretation tree + ConsistencyTest,
 * out[3] calls; out[4] s of PbMap assembly (the frames' host threads), out[5] frames; reset != 0 zeroes them.
 * (No reference counterpart: instrumentation of r360_register_pbmap and the frames' assembly.) */
int r360_ctx_host_times(r360_ctx* ctx, double out[6], int reset);
int r360_ctx_kernel_time_reset(r360_ctx* ctx);

/* ---------------------------------------------------------------- FilterPointCloud
 * FilterPointCloud::filterEuclidean (include/FilterPointCloud.h; SLAM/SphereGraphSLAM.cpp:116, :193) on the host
 * (no GPU), restated from PCL 1.7's PassThrough: keeps a point iff x, y, z are finite and x_min <= x <= x_max,
 * -box <= y <= box, -box <= z <= box (float compares, closed intervals; the reference uses -2, 1 and 4).  Order is
 * kept and the result is unorganised.  xyz [n][3], rgba [n] PointXYZRGBA packing (NULL: none); the outputs may be
 * the inputs. */
int r360_cloud_filter_euclidean(const float* xyz, const uint32_t* rgba, size_t n, float x_min, float x_max, float box,
                                float* out_xyz, uint32_t* out_rgba, size_t* n_out);

/* FilterPointCloud::filterVoxel (pcl::VoxelGrid with leaf size `leaf` on all axes, restated from PCL 1.7) on ctx's GPU.
 * Non-finite points are dropped; with inv = 1.0f / leaf the voxel of a point is (int)floorf(x * inv) per axis; each
 * occupied voxel gives one point: xyz the mean of its points, r / g / b the integer floor of the channel means,
 * alpha 0; a voxel holding exactly one point gives that point's xyz bits unchanged.  The output is in ascending
 * (k, j, i) voxel order, the same from run to run and for any order of the input.  Means are formed from 64-bit integer
 * sums of llrint(coordinate / R360_VOXEL_QUANTUM): each lies within R360_VOXEL_QUANTUM / 2 + half a float ulp of
 * the exact mean.
 * Returns 1, with the output equal to the input (n points), when PCL's size guard refuses the leaf ("Leaf size is too
 * small for the input dataset"): with min / max the bounds of the finite points and d = (int64)((max - min) * inv) + 1
 * per axis in float, dx * dy * dz > INT32_MAX (or the grid from floor(min * inv) to floor(max * inv) has more cells).
 * Supported domain: ceil(max |coordinate|) * 2^24 * (finite points) < 2^62 (so 1024 m with 2^27 points, 8192 m
 * with 2^24) and |voxel index| < 2^30; outside it the call fails (< 0), as it does for n > 2^30.
 * rgba / out_rgba may be NULL; the outputs may be the inputs; cap = room in the outputs: cap < *n_out is an error
 * (< 0) that still sets *n_out. */
#define R360_VOXEL_QUANTUM (1.0 / 16777216.0)   /* 2^-24 m */
int r360_cloud_filter_voxel(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, float leaf,
                            float* out_xyz, uint32_t* out_rgba, size_t cap, size_t* n_out);

/* The context's global map (globalMap of SLAM/SphereGraphSLAM.cpp): device-resident, one per context, empty at first,
 * owned by the context and freed by r360_ctx_destroy.  add_cloud: map <- voxel grid of (map ++ cloud), bit for bit
 * r360_cloud_filter_voxel of the concatenated arrays.  add_frame: the whole map step on the frame's clouds in HBM
 * (built with R360_BUILD_CLOUD): Rt_[sensor], the Euclidean box (r360_cloud_filter_euclidean), pose (column-major
 * 4x4, m(k,0)*x + m(k,1)*y + m(k,2)*z + m(k,3) in float, left to right), then add_cloud's step; a frame whose
 * sphereCloud was loaded (r360_frame_load_cloud) takes the same steps from that cloud.  The frame may belong to another
 * context of the same device.  A soft failure (1, the size guard) or an error leaves the map as it was.
 * download: cap < the map's size is an error (< 0); *n is set either way; xyz and rgba NULL: only *n. */
int r360_ctx_map_reset(r360_ctx* ctx);
int r360_ctx_map_add_cloud(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n, float leaf);
int r360_ctx_map_add_frame(r360_ctx* ctx, r360_frame* f, const float pose[16], float x_min, float x_max, float box,
                           float leaf);
int r360_ctx_map_size(r360_ctx* ctx, size_t* n);
int r360_ctx_map_download(r360_ctx* ctx, float* xyz, uint32_t* rgba, size_t cap, size_t* n);

/* ---------------------------------------------------------------- outlier removal
 * pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval, restated from PCL 1.7 (unpinned), for a host cloud and
 * for the context's global map where it lies.  The statement is tests/outlier_model.py and DESIGN.md §5b-2.
 * Both: a row with a non-finite coordinate is dropped (PCL keeps it as an inlier); kept points keep their input order and
 * their xyz and rgba bits; the squared distance of two points is dx*dx + dy*dy + dz*dz in double of the float
 * coordinates, left to right, uncontracted.
 * STATISTICAL (mean_k = k, stddev_mul, max_dist): d_i = the mean of the square roots of the k smallest squared
 * distances from point i to other points, summed ascending.  A point whose k-th nearest other point lies farther than
 * max_dist (squared distance > (double)max_dist squared) is short: removed, and no part of the statistics (PCL
 * searches without bound; with max_dist beyond the cloud's diameter the two agree).  Over the m other points
 * mean = sum d / m, stddev = sqrt(sum (d - mean)^2 / (m - 1)) (0 when m < 2), threshold = mean + stddev_mul * stddev;
 * point i is kept iff d_i <= threshold.
 * RADIUS (radius, min_neighbors): c_i = the number of other points with squared distance <= (double)radius squared;
 * point i is kept iff c_i >= min_neighbors (PCL counts the point itself and keeps iff count > min: the same rule).
 * Defaults: STATISTICAL, mean_k 20, stddev_mul 1, max_dist 0.5 m, radius 0.15 m, min_neighbors 5: ten and three leaves
 * of the reference's 5 cm voxel, the application's starting values and no claim about any dataset.
 * Checks (no GPU needed): ctx or params NULL, kind not one of the two, mean_k outside 1..64, max_dist or radius not
 * positive and finite, stddev_mul not finite, min_neighbors < 0: R360_EINVAL (-2).
 * stats: n_in rows given, n_finite of them finite, n_short short points, n_removed = n_in - rows kept; mean, stddev and
 * threshold of the statistical filter (0 for the radius filter, whose n_short is 0 too).
 * r360_cloud_filter_outliers: rgba, out_rgba and stats may be NULL; the outputs may be the inputs; cap = room in the
 * outputs: cap < *n_out is an error (< 0) that still sets *n_out.
 * r360_ctx_map_filter_outliers: the context's map filtered in HBM; only the counts and statistics cross to the host.
 * The map stays in ascending voxel order, and size, download, add_cloud and add_frame go on from the result.  An empty
 * map gives 0 and zero stats; an error leaves the map as it was.
 * r360_cloud_outlier_eval (parity hook): fills the output of the filter named by kind and leaves the other alone:
 * STATISTICAL score[i] = d_i, +inf for a short point, NaN for a dropped row; RADIUS count[i] = c_i (the full count),
 * -1 for a dropped row.  Either pointer may be NULL. */
enum { R360_OUTLIER_STATISTICAL = 0, R360_OUTLIER_RADIUS = 1 };
typedef struct { int kind; int mean_k; float stddev_mul; float max_dist; float radius; int min_neighbors; } r360_outlier_params;
typedef struct { size_t n_in, n_finite, n_short, n_removed; double mean, stddev, threshold; } r360_outlier_stats;
void r360_outlier_default_params(r360_outlier_params* params);
int r360_cloud_filter_outliers(r360_ctx* ctx, const float* xyz, const uint32_t* rgba, size_t n,
                               const r360_outlier_params* params, float* out_xyz, uint32_t* out_rgba, size_t cap,
                               size_t* n_out, r360_outlier_stats* stats);
int r360_ctx_map_filter_outliers(r360_ctx* ctx, const r360_outlier_params* params, r360_outlier_stats* stats);
int r360_cloud_outlier_eval(r360_ctx* ctx, const float* xyz, size_t n, const r360_outlier_params* params, double* score,
                            int* count);

/* ---------------------------------------------------------------- surface normals and curvature
 * pcl::NormalEstimation, restated from PCL 1.7 features/normal_3d.h (unpinned), for a host cloud and for the context's
 * global map where it lies.  The statement is tests/normal_model.py and DESIGN.md §5b-3.
 * A row with a non-finite coordinate is dropped: its normal and curvature are NaN and it is nobody's neighbour.  The
 * neighbourhood of point i is i itself, then its nearest other points with squared distance <= (double)radius squared,
 * at most k points in all (k = 3..64), in ascending (squared distance, input index) order; the squared distance is that
 * of the outlier filters.  One rule covers both PCL modes: a radius beyond the cloud's diameter is setKSearch(k), and
 * k = 64 is setRadiusSearch(radius) for every point with at most 63 others within it.  Unlike PCL the search is always
 * bounded, the neighbourhood is capped at 64, ties go to the lower index, and the moments are fp64 two-pass sums.
 * A point with m < 3 neighbours is short: normal and curvature NaN.  Otherwise mean = (sum p_j) / m and
 * C = sum (p_j - mean)(p_j - mean)^T / m, summed in neighbourhood order in double; l0 <= l1 <= l2 the eigenvalues of C;
 * the normal is the unit eigenvector of l0 and curvature = |l0| / (l0 + l1 + l2), 0 when the trace is 0.
 * Orientation (flipNormalTowardsViewpoint): v = the nearest of the n_view viewpoints ([n_view][3], n_view = 1..4096) by
 * squared distance in double, ties to the lower index; the normal is negated iff (v - p) . n < 0 in double.  One
 * viewpoint is PCL's case; the keyframe positions serve a map fused from many keyframes.
 * Outputs are the float32 of the double values; two runs give the same bytes.
 * Defaults: k 20, radius 0.25 m (five leaves of the reference's 5 cm voxel): starting values, no claim about a dataset.
 * Checks (no GPU needed): ctx or params NULL, k outside 3..64, radius not positive and finite, n_view outside 1..4096,
 * viewpoints NULL, n > 2^30: R360_EINVAL (-2).
 * stats: n_in rows given, n_finite of them finite, n_short short points, sum_neighbors = the sum of m over the finite
 * rows (the point itself counts).
 * r360_cloud_normals: normals [n][3], curvature [n]; either and stats may be NULL.
 * r360_ctx_map_estimate_normals: the normals of the context's map, kept on the device in the map's order until the map
 * next changes (r360_ctx_map_reset, _add_cloud, _add_frame, _filter_outliers).  An empty map gives 0 and zero stats; an
 * error leaves the map and its normals as they were.
 * r360_ctx_map_download_normals: an error (< 0) when the map has no valid normals; *n is the map's size either way;
 * cap < *n is an error (< 0); normals and curvature NULL: only *n.
 * r360_cloud_normals_eval (parity hook): knn [n][k] the neighbourhood's input indices in its order, the point itself
 * first, -1 padded; count [n] m, -1 for a dropped row; normal [n][3], eig [n][3] (ascending) and curvature [n] in
 * double, NaN for dropped and short rows.  Any pointer may be NULL.
 * r360_pcd_write_normals / _read_normals: a PointXYZRGBNormal cloud, FIELDS x y z rgba normal_x normal_y normal_z
 * curvature, WIDTH n HEIGHT 1, in r360_pcd_write's modes (ascii prints the normals with nine digits, which return the
 * bits).  rgba, normals, curvature may be NULL (written as 0 / read and dropped); read fails on a file without the
 * normal fields when it is asked for them; cap < *n reads the first cap points. */
typedef struct { int k; float radius; } r360_normal_params;
typedef struct { size_t n_in, n_finite, n_short; unsigned long long sum_neighbors; } r360_normal_stats;
void r360_normal_default_params(r360_normal_params* params);
int r360_cloud_normals(r360_ctx* ctx, const float* xyz, size_t n, const r360_normal_params* params,
                       const float* viewpoints, int n_view, float* normals, float* curvature, r360_normal_stats* stats);
int r360_ctx_map_estimate_normals(r360_ctx* ctx, const r360_normal_params* params, const float* viewpoints, int n_view,
                                  r360_normal_stats* stats);
int r360_ctx_map_download_normals(r360_ctx* ctx, float* normals, float* curvature, size_t cap, size_t* n);
int r360_cloud_normals_eval(r360_ctx* ctx, const float* xyz, size_t n, const r360_normal_params* params,
                            const float* viewpoints, int n_view, int* knn, int* count, double* normal, double* eig,
                            double* curvature);
int r360_pcd_write_normals(const char* path, const float* xyz, const uint32_t* rgba, const float* normals,
                           const float* curvature, size_t n, int mode);
int r360_pcd_read_normals(const char* path, float* xyz, uint32_t* rgba, float* normals, float* curvature, size_t cap,
                          size_t* n);

/* ---------------------------------------------------------------- Euclidean cluster extraction
 * pcl::EuclideanClusterExtraction and the normal-aware pcl::extractEuclideanClusters overload, restated from PCL 1.7
 * segmentation/extract_clusters.h (unpinned), for a host cloud and for the context's global map where it lies.  The
 * statement is tests/cluster_model.py and DESIGN.md §5b-4.
 * A row with a non-finite coordinate is dropped: label -1, member of nothing.  Two finite rows i != j are joined iff
 * dx*dx + dy*dy + dz*dz <= (double)tolerance^2 (closed; double of the float coordinates, left to right) and, when
 * normals ([n][3]) are given, (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j >= cos((double)eps_angle) in double of the floats:
 * the normals are taken as given, neither normalised nor sign-agnostic, and a row whose normal has a non-finite
 * component is joined to nothing.  A component of that graph is a cluster iff min_size <= size <= max_size.  Clusters
 * are ordered by size descending, ties by their smallest input index (root) ascending; label[i] is the cluster's rank,
 * -1 for a dropped row and for a row of a rejected component.  Two calls give the same bytes.
 * r360_cluster_info: size, root, min / max of the members' coordinates, their centroid, and of their covariance
 * (fp64, two passes, / size) the eigenvalues ascending, the unit eigenvector of eig[0] with its largest-magnitude
 * component positive (ties to the lower axis) and curvature = |eig[0]| / trace (0 when the trace is 0); eig, normal and
 * curvature are NaN for fewer than 3 members.
 * r360_cloud_clusters: normals NULL selects the plain form.  labels [n], info [info_cap], n_clusters and stats may be
 * NULL; info_cap < the number of clusters is an error (< 0) that still sets *n_clusters (and labels and stats).
 * r360_cloud_clusters_eval (parity hook): root [n] the smallest input index of the row's component (-1 dropped),
 * comp_size [n] the component's size before the size bounds (-1 dropped).
 * r360_ctx_map_cluster: labels and records of the context's map, kept on the device in the map's order until the map
 * next changes (r360_ctx_map_reset, _add_cloud, _add_frame, _filter_outliers, _filter_clusters, _filter_planes).
 * use_normals without valid map normals is an error (< 0); an empty map gives 0 and zero stats; an error leaves the map,
 * its normals and its labels as they were.
 * r360_ctx_map_download_labels / r360_ctx_map_cluster_info: an error (< 0) when the map has no valid labels; *n is the
 * map's size / the number of clusters either way; cap < *n is an error (< 0); a NULL array: only *n.
 * r360_ctx_map_filter_clusters: clusters, then keeps exactly the map points with label >= 0, compacted in HBM: the map
 * stays in ascending voxel order and kept points keep their bits.  The map's normals and labels become invalid.
 * r360_pcd_write_labels / _read_labels: a PointXYZRGBL cloud, FIELDS x y z rgba label (label U 4, -1 written as
 * 4294967295), WIDTH n HEIGHT 1, in r360_pcd_write's modes.  rgba and labels may be NULL (written as 0 / read and
 * dropped); read fails on a file without a label field; cap < *n reads the first cap points.
 * Arguments: tolerance positive and finite, 1 <= min_size <= max_size, eps_angle in [0, pi] when normals are used,
 * n <= 2^30 (R360_EINVAL otherwise, before any GPU work). */
typedef struct { float tolerance; int min_size; int max_size; float eps_angle; } r360_cluster_params;
typedef struct { size_t n_in, n_finite, n_components, n_clusters, n_clustered; } r360_cluster_stats;
typedef struct { int size, root; float min[3], max[3]; double centroid[3], eig[3], normal[3], curvature; } r360_cluster_info;
void r360_cluster_default_params(r360_cluster_params* params);
int r360_cloud_clusters(r360_ctx* ctx, const float* xyz, const float* normals, size_t n, const r360_cluster_params* params,
                        int* labels, r360_cluster_info* info, size_t info_cap, size_t* n_clusters,
                        r360_cluster_stats* stats);
int r360_cloud_clusters_eval(r360_ctx* ctx, const float* xyz, const float* normals, size_t n,
                             const r360_cluster_params* params, int* labels, r360_cluster_info* info, size_t info_cap,
                             size_t* n_clusters, r360_cluster_stats* stats, int* root, int* comp_size);
int r360_ctx_map_cluster(r360_ctx* ctx, const r360_cluster_params* params, int use_normals, r360_cluster_stats* stats);
int r360_ctx_map_download_labels(r360_ctx* ctx, int* labels, size_t cap, size_t* n);
int r360_ctx_map_cluster_info(r360_ctx* ctx, r360_cluster_info* info, size_t cap, size_t* n);
int r360_ctx_map_filter_clusters(r360_ctx* ctx, const r360_cluster_params* params, int use_normals,
                                 r360_cluster_stats* stats);
int r360_pcd_write_labels(const char* path, const float* xyz, const uint32_t* rgba, const int* labels, size_t n, int mode);
int r360_pcd_read_labels(const char* path, float* xyz, uint32_t* rgba, int* labels, size_t cap, size_t* n);

/* ---------------------------------------------------------------- RANSAC plane segmentation
 * pcl::SACSegmentation with SACMODEL_PLANE / _PERPENDICULAR_PLANE / _PARALLEL_PLANE and SAC_RANSAC, and the loop of
 * PCL's cluster-extraction recipe that peels planes until a fraction is left, restated (PCL is not pinned) for a host
 * cloud and for the context's global map where it lies.  The statement is tests/sac_model.py and DESIGN.md §5b-5.
 * Everything is double of the float inputs, left to right, uncontracted.
 * A row with a non-finite coordinate is dropped: label -1, never sampled, never an inlier; n_finite counts the others.
 * Plane of three points: u = p1 - p0, v = p2 - p0, n = u x v, s = (nx^2 + ny^2) + nz^2; degenerate (scored 0) iff s is
 * not a finite number > 0; otherwise n /= sqrt(s), d = -((nx p0x + ny p0y) + nz p0z).
 * A point is an inlier iff |((a x + b y) + c z) + d| <= (double)distance_threshold (closed) and, when normals ([n][3])
 * are given, |(nx a + ny b) + nz c| >= cos((double)normal_angle); a row whose normal has a non-finite component is
 * never an inlier but stays in the pool.
 * Constraint on hypotheses, with â the axis normalised in double: PERPENDICULAR |n.â| >= cos(eps_angle) (the plane's
 * normal within eps_angle of the axis), PARALLEL |n.â| <= sin(eps_angle) (the plane parallel to the axis); a
 * hypothesis that fails scores 0.  The refined plane is not re-checked.
 * Sampling is counter-based: mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31.  Draw j of hypothesis h of plane p over a pool of m:
 * (mix(mix(mix(mix(seed) ^ p) ^ h) ^ j) * m) >> 64.  a = draw(0, m), b = draw(1, m-1), c = draw(2, m-2); if b >= a: b++;
 * with lo < hi the two so far: if c >= lo: c++; if c >= hi: c++.  Positions index the pool: the remaining rows in
 * ascending input index.
 * Search for one plane over a pool of m: hypotheses are scored in rounds of R360_SAC_ROUND; after each round best is
 * the highest count so far (ties to the lowest h), w = best / m, q = 1 - w w w clipped to [DBL_EPSILON, 1 - DBL_EPSILON],
 * k = log(1 - probability) / log(q); the search goes on while evaluated < max_iterations and (double)evaluated < k.
 * optimize: when the best hypothesis has >= 3 inliers, the plane through their centroid whose normal is the
 * eigenvector of the smallest eigenvalue of their covariance (fp64, two passes, / size) replaces it and the inliers are
 * selected again from the pool.
 * Peel: for p = 0, 1, ... stop when p = max_planes, the pool is smaller than max(3, min_inliers),
 * (double)pool <= (double)stop_fraction * n_finite, or the plane found has fewer than min_inliers final inliers (it is
 * not recorded, its points stay unlabelled); otherwise the final inliers get label p and leave the pool.
 * r360_sac_plane: coef oriented so that the largest-magnitude component of the normal is positive (ties to the lower
 * axis; all four numbers negated together), size the final inliers, raw_size the best hypothesis' count,
 * best_hypothesis, evaluated, and centroid, eig (ascending) and curvature of the final inliers as in r360_cluster_info.
 * r360_cloud_sac_planes: normals NULL selects the plain form.  labels [n], planes [planes_cap], n_planes and stats may
 * be NULL; planes_cap < the number of planes is an error (< 0) that still sets *n_planes (and labels and stats).
 * r360_cloud_sac_eval (parity hook, plane 0 over the whole finite cloud): with coef_in [n_hyp][4] the coefficients are
 * scored as given; without, hypotheses 0 .. n_hyp - 1 are drawn, and samples [n_hyp][3] gets their input indices (-1
 * with fewer than 3 finite rows).  coef [n_hyp][4] gets what was scored, NaN when degenerate or refused; count
 * [n_hyp].  n_hyp <= 65536; the outputs may be NULL.
 * r360_ctx_map_sac_planes: plane labels and records of the context's map, kept on the device in the map's order until
 * the map next changes.  use_normals without valid map normals is an error (< 0); an empty map gives 0 and zero stats;
 * an error leaves the map, its normals and its labels as they were.  The cluster labels are not touched.
 * r360_ctx_map_download_plane_labels / r360_ctx_map_plane_info: as r360_ctx_map_download_labels / _cluster_info.
 * r360_ctx_map_filter_planes: segments, then drops the plane points (keep_planes 0) or keeps only them (1), compacted
 * in HBM: order and bits are kept.  The map's normals, cluster labels and plane labels become invalid.
 * Arguments: distance_threshold positive and finite, max_iterations 1 .. 65536, probability in (0, 1), max_planes
 * 1 .. 64, min_inliers >= 3, stop_fraction in [0, 1), constraint one of the three, a constrained call's axis finite and
 * non-zero, eps_angle and normal_angle in [0, pi/2], n <= 2^30 (R360_EINVAL otherwise, before any GPU work). */
#define R360_SAC_ROUND 128
#define R360_SAC_NONE 0
#define R360_SAC_PERPENDICULAR 1
#define R360_SAC_PARALLEL 2
typedef struct {
    float distance_threshold; int max_iterations; float probability; int optimize; int constraint; float axis[3];
    float eps_angle, normal_angle; int max_planes, min_inliers; float stop_fraction; int reserved;
    unsigned long long seed;
} r360_sac_params;
typedef struct {
    double coef[4], centroid[3], eig[3], curvature; int size, raw_size, best_hypothesis, evaluated;
} r360_sac_plane;
typedef struct { size_t n_in, n_finite, n_planes, n_in_planes, n_evaluated; } r360_sac_stats;
void r360_sac_default_params(r360_sac_params* params);
int r360_cloud_sac_planes(r360_ctx* ctx, const float* xyz, const float* normals, size_t n, const r360_sac_params* params,
                          int* labels, r360_sac_plane* planes, size_t planes_cap, size_t* n_planes, r360_sac_stats* stats);
int r360_cloud_sac_eval(r360_ctx* ctx, const float* xyz, const float* normals, size_t n, const r360_sac_params* params,
                        const double* coef_in, size_t n_hyp, int* samples, double* coef, int* count);
int r360_ctx_map_sac_planes(r360_ctx* ctx, const r360_sac_params* params, int use_normals, r360_sac_stats* stats);
int r360_ctx_map_download_plane_labels(r360_ctx* ctx, int* labels, size_t cap, size_t* n);
int r360_ctx_map_plane_info(r360_ctx* ctx, r360_sac_plane* planes, size_t cap, size_t* n);
int r360_ctx_map_filter_planes(r360_ctx* ctx, const r360_sac_params* params, int use_normals, int keep_planes,
                               r360_sac_stats* stats);

/* ---------------------------------------------------------------- Generalized-ICP
 * pcl::GeneralizedIterativeClosestPoint as Registration/RegisterPairRGBD360.cpp:109-149 calls it, restated (PCL is
 * not pinned): the statement is tests/gicp_model.py and DESIGN.md §5c.  Per cloud: rows with a non-finite coordinate
 * are dropped (order kept), every point's k nearest points of its own cloud (itself included, ties to the lower
 * index) give C_i = V diag(gicp_epsilon, 1, 1) V^T.  Per outer iteration: the nearest target of every transformed
 * source point (squared distance strictly below max_corr_dist^2), M_i = (Ct_j + R Cs_i R^T)^-1, then a Gauss-Newton
 * inner solve of sum r^T M r with left SE(3) increments (r360_exp_se3, pseudo = 0), where PCL runs BFGS.
 * Poses are column-major 4x4 and map source into target.  The clouds, their indices and every pass buffer belong to
 * the context and are freed by r360_ctx_destroy; a new source or target of any size may be set at any time.
 * set_source / set_target: < 0 with fewer than k_correspondences finite points (PCL throws) or k_correspondences
 * outside 4 .. 32.  align: 0, or 1 (R360_ILLPOSED's value) when no pair passes the gate or the first 6x6 system of
 * an outer iteration is singular: pose_out is then the pose reached so far (init at the first iteration). */
typedef struct {
    int k_correspondences;          /* 20 */
    float gicp_epsilon;             /* 1e-3 */
    float max_corr_dist;            /* 0.4 (the reference program's) */
    int max_iterations;             /* 10 (the reference program's) */
    int max_inner_iterations;       /* 20 */
    double rotation_epsilon;        /* 2e-3 */
    double transformation_epsilon;  /* 1e-9 (the reference program's) */
} r360_gicp_params;
typedef struct {
    int iterations, converged, inner_steps;   /* outer iterations, the epsilon test met, accepted inner steps in all */
    size_t n_corr;                            /* correspondences of the last outer iteration */
    double cost, fitness;                     /* f / n_corr there; mean squared nearest-target distance of all
                                                 source points at the final pose (getFitnessScore, no range limit) */
} r360_gicp_stats;
void r360_gicp_default_params(r360_gicp_params* p);
int r360_gicp_set_source(r360_ctx* ctx, const float* xyz, size_t n, const r360_gicp_params* p);
int r360_gicp_set_target(r360_ctx* ctx, const float* xyz, size_t n, const r360_gicp_params* p);
int r360_gicp_align(r360_ctx* ctx, const float init[16], const r360_gicp_params* p, float pose_out[16],
                    r360_gicp_stats* stats);
/* Parity hooks.  get_cloud: which = 0 source, 1 target; the kept points (3 floats each), the upper triangles
 * xx xy xz yy yz zz of C_i as float and the k neighbour indices per point in ascending (distance, index) order; any
 * output may be NULL; cap = room in points; *n is set either way.  eval: one correspondence pass and one inner pass
 * at `pose`: corr[i] = j(i) or -1 per kept source point (may be NULL), *cost = f (the sum), H row-major, g. */
int r360_gicp_get_cloud(r360_ctx* ctx, int which, float* xyz, float* cov6, int* knn, size_t cap, size_t* n);
int r360_gicp_eval(r360_ctx* ctx, const float pose[16], const r360_gicp_params* p, int* corr, double* cost,
                   double H[36], double g[6], size_t* n_corr);

/* ---------------------------------------------------------------- pose-graph optimisation
 * include/GraphOptimizer.h (g2o VertexSE3 / EdgeSE3, OptimizationAlgorithmLevenberg over LinearSolverDense,
 * optimize(10)) restated (g2o is not pinned): the statement is tests/pgo_model.py and DESIGN.md §5d.  A vertex is a
 * pose, world from keyframe; an edge (from, to, rel, info) says T_to ~ T_from * rel, with info the 6x6 information
 * matrix ordered (translation, rotation), symmetrised on intake and otherwise used as given (getHessian() and
 * getInfoMat() go in unchanged, as in the reference).  Poses and information matrices are COLUMN-major double (the
 * reference casts to double at every call).  Vertex 0 is always fixed (GraphOptimizer.h:105-106).
 * The residual of an edge is e = [t_E ; log(R_E)] of E = rel^-1 T_from^-1 T_to, the cost F = sum e^T info e, the
 * increment T * [Exp(d_w), d_t]; Levenberg-Marquardt after g2o's scheme runs on the host, every sum, the block-sparse
 * H and the block-Jacobi-preconditioned conjugate-gradient solve on the context's GPU, all in a fixed order: two runs
 * give the same bytes.
 * A graph is a handle of its own, as the reference's optimisers are objects (KFsphere_SLAM.cpp:263,
 * LoopClosure360.h:58); it runs on its context's stream and the context must outlive it.
 * R360_EINVAL: an argument or the graph fails a check (message in r360_last_error()); the handle stays usable. */
#define R360_EINVAL (-2)
typedef struct r360_graph r360_graph;
typedef struct {
    int max_iterations;      /* 10: the reference's optimize(10) */
    int max_trials;          /* 10 damping trials per iteration */
    double gain_epsilon;     /* 1e-6: stop when F - F' <= gain_epsilon F */
    double cg_tolerance;     /* 1e-12: the recursive residual against |b| */
    int cg_max_iterations;   /* 0: 12 * the number of free vertices */
    int cg_form;             /* 0 automatic, 1 one workgroup (unknowns and CG vectors in LDS), 2 one launch per step */
} r360_graph_params;
enum { R360_GRAPH_CONVERGED = 0, R360_GRAPH_ITERATION_LIMIT = 1, R360_GRAPH_STALLED = 2, R360_GRAPH_CG_NOT_CONVERGED = 3 };
typedef struct {
    int status;                  /* R360_GRAPH_* */
    int iterations, trials;      /* accepted outer iterations, damped solves in all */
    int cg_form;                 /* the form that ran (1 or 2; 0 if no solve ran) */
    double F_initial, F_final, lambda;
    long long cg_iterations;     /* in all */
    int cg_iterations_max;       /* of one solve */
    int pad;
} r360_graph_stats;
int  r360_graph_create(r360_ctx* ctx, r360_graph** out);
void r360_graph_destroy(r360_graph* g);
/* addVertex (GraphOptimizer.h:96-110; KFsphere_SLAM.cpp:265, 541): *id = the new vertex's index. */
int  r360_graph_add_vertex(r360_graph* g, const double pose[16], int* id);
/* setFixed of a vertex (KFsphere_SLAM.cpp:668-676); vertex 0 cannot be freed. */
int  r360_graph_set_fixed(r360_graph* g, int id, int fixed);
int  r360_graph_set_pose(r360_graph* g, int id, const double pose[16]);
/* addEdge(from, to, relativePose, information) (GraphOptimizer.h:113-133; KFsphere_SLAM.cpp:544, 550, 630;
 * LoopClosure360.h:318).  Either index order; several edges of one pair add up. */
int  r360_graph_add_edge(r360_graph* g, int from, int to, const double rel[16], const double info[36]);
int  r360_graph_size(const r360_graph* g, int* n_vertices, int* n_edges);
/* Robust kernels and the active set (g2o's setRobustKernel, per edge).  Edges are numbered in
 * insertion order, 0 .. n_edges - 1 of r360_graph_size.  With c = e^T info e of an edge and its width delta > 0
 * (delta applies to sqrt(c), as in g2o's RobustKernelHuber / RobustKernelCauchy):
 *   R360_GRAPH_KERNEL_NONE    rho(c) = c                                   w = 1
 *   R360_GRAPH_KERNEL_HUBER   rho(c) = c for c <= delta^2, otherwise
 *                                      2 delta sqrt(c) - delta^2           w = delta / sqrt(c)
 *   R360_GRAPH_KERNEL_CAUCHY  rho(c) = delta^2 log1p(c / delta^2)          w = 1 / (1 + c / delta^2)
 * The cost is F = sum rho(c); an edge adds w J^T info e to b and J^T (w info) J to H (the second-order term is left
 * out, as g2o leaves it out); Levenberg-Marquardt is unchanged, with the robust F in its gain ratio.  A graph whose
 * edges all have NONE computes bit for bit what it computed before kernels existed.
 * An inactive edge does not exist for eval, solve and optimize: it adds nothing, the graph checks do not count it (a
 * free vertex whose only edges are inactive is R360_EINVAL, as is a component anchored only through inactive edges),
 * and a graph with edge k inactive gives the same bytes as the same graph built without edge k.
 * set_default_kernel: the kernel of the edges added (or loaded) from now on; NONE at creation.  R360_EINVAL on an
 * unknown kind, a delta that is not finite and positive (whatever the kind) or a bad edge index; nothing changes then. */
enum { R360_GRAPH_KERNEL_NONE = 0, R360_GRAPH_KERNEL_HUBER = 1, R360_GRAPH_KERNEL_CAUCHY = 2 };
int  r360_graph_set_default_kernel(r360_graph* g, int kind, double delta);
int  r360_graph_set_edge_kernel(r360_graph* g, int edge, int kind, double delta);
int  r360_graph_get_edge_kernel(const r360_graph* g, int edge, int* kind, double* delta);
int  r360_graph_set_edge_active(r360_graph* g, int edge, int active);
int  r360_graph_get_edge_active(const r360_graph* g, int edge, int* active);
/* Per edge at the current poses: chi2 [cap] = c and weight [cap] = w of the edge's kernel, computed on the GPU by the
 * cost-only form of the linearisation.  An inactive edge reports its chi2 with weight 0.  Either output may be NULL;
 * *n = n_edges is set either way; cap < *n with an output given is an error. */
int  r360_graph_edge_stats(r360_graph* g, double* chi2, double* weight, int cap, int* n);
/* getPoses (GraphOptimizer.h:160-175): poses [cap][16]; *n is set either way, cap < *n with poses given is an error. */
int  r360_graph_get_poses(const r360_graph* g, double* poses, int cap, int* n);
void r360_graph_default_params(r360_graph_params* p);
/* optimizeGraph (GraphOptimizer.h:137-157; KFsphere_SLAM.cpp:679-705).  params NULL = the defaults.  Returns 0 with
 * stats->status set, R360_EINVAL when a free vertex has no edge, a connected component has no fixed vertex, or
 * cg_form 1 is asked for a graph too large for it.  With status R360_GRAPH_CG_NOT_CONVERGED or R360_GRAPH_STALLED
 * the poses are those of the last accepted iteration. */
int  r360_graph_optimize(r360_graph* g, const r360_graph_params* params, r360_graph_stats* stats);
/* Parity hooks (at most 1024 vertices).  The unknowns are the free vertices in index order, 6 each (translation,
 * rotation).  eval: F, b [6 n_free] and H densified row-major [6 n_free][6 n_free] on the host from the device's
 * blocks, at the current poses; *n_unknowns is set either way; cap = room in unknowns; b and H may be NULL.
 * solve: one damped solve (H + lambda I) delta = -b with params' CG settings; returns 1 when CG ran out of
 * iterations; *rel_residual = the recursive residual against |b|. */
int  r360_graph_eval(r360_graph* g, double* F, double* b, double* H, int cap, int* n_unknowns);
int  r360_graph_solve(r360_graph* g, const r360_graph_params* params, double lambda, double* delta, int cap,
                      int* n_unknowns, int* iterations, double* rel_residual, int* form);
/* g2o text files as saveGraph writes them (GraphOptimizer.h:178-181; KFsphere_SLAM.cpp:689): host only, no context.
 *   VERTEX_SE3:QUAT id x y z qx qy qz qw  /  FIX id  /  EDGE_SE3:QUAT i j x y z qx qy qz qw + the 21 upper-triangular
 * entries of info, row-major; %.17g; Shepperd's quaternion with qw >= 0, snapped to a 2^-48 lattice of directions so
 * that read-then-write reproduces the file byte for byte (a rotation entry moves by < 1e-14).
 * write: poses [n][16], fixed [n] (may be NULL), ij [m][2], rel [m][16], info [m][36].  read: any output may be NULL;
 * the counts are set either way; all outputs NULL = only count and check.  A malformed file is R360_EINVAL. */
int  r360_g2o_write(const char* path, int n_vertices, const double* poses, const int* fixed, int n_edges, const int* ij,
                    const double* rel, const double* info);
int  r360_g2o_read(const char* path, double* poses, int* fixed, int cap_vertices, int* n_vertices, int* ij, double* rel,
                   double* info, int cap_edges, int* n_edges);
/* saveGraph / the matching load: load replaces the graph's vertices and edges.  save writes the active edges only:
 * the file is the graph that gets optimised.  g2o text has no place for robust kernels, so none is written; load
 * gives every edge it reads the current default kernel and makes it active. */
int  r360_graph_save(const r360_graph* g, const char* path);
int  r360_graph_load(r360_graph* g, const char* path);

/* ---------------------------------------------------------------- rig extrinsic calibration from control planes
 * include/Calibration.h (ControlPlanes, Calibration: loadConstructionSpecs :918-930, CalibrateRotation :1026-1218,
 * CalibrateTranslation :1222-1334, calcConditioning :1346-1352) restated in fp64: the statement is
 * tests/rigcal_model.py and DESIGN.md §5e.  A correspondence row has ten doubles: n_i (3), d_i, n_ii (3), d_ii in the
 * two sensors' own frames, the smaller inlier count and the pixel-centre figure.  Pairs are (i, j), 0 <= i < j < 8, as
 * the reference's mmCorrespondences[i][j]; poses are COLUMN-major double[16], eight of them.
 * The per-row terms and every sum run on the context's GPU in a fixed order (two runs give the same bytes); the
 * 21x21 solve, its conditioning and the Rodrigues update stay on the host.  A handle created with ctx NULL holds rows
 * and files only: every call that needs the GPU returns R360_EINVAL on it.
 * R360_EMISSING_PAIR: an adjacent pair (k, k+1), k = 0..6, has fewer than 3 rows (the reference asserts). */
#define R360_EMISSING_PAIR (-6)
#define R360_RIGCAL_MAX_ITERATIONS 10
typedef struct r360_rigcal r360_rigcal;
enum { R360_RIGCAL_CONVERGED = 0, R360_RIGCAL_ITERATION_LIMIT = 1, R360_RIGCAL_BAD_CONDITIONED = 2, R360_RIGCAL_MISSING_PAIR = 3 };
typedef struct {
    int status;        /* R360_RIGCAL_* */
    int iterations;    /* linearisations made (rotation: up to 10; translation: 1) */
    int rows;          /* correspondence rows in all */
    int pad;
    /* per iteration: sum |r|^2, sum of the angles (rotation only), sigma_max / sigma_min of the 21x21 matrix,
     * |update|^2, the weighted error before and after the step (rotation only), whether the step was applied */
    double error[R360_RIGCAL_MAX_ITERATIONS], angle[R360_RIGCAL_MAX_ITERATIONS], conditioning[R360_RIGCAL_MAX_ITERATIONS];
    double update2[R360_RIGCAL_MAX_ITERATIONS], werr0[R360_RIGCAL_MAX_ITERATIONS], werr1[R360_RIGCAL_MAX_ITERATIONS];
    int accepted[R360_RIGCAL_MAX_ITERATIONS];
} r360_rigcal_stats;
typedef struct {
    double dist;         /* 0.2: |d| threshold; the normals' threshold is dist / 2 (Calibration.h:196) */
    double degenerate;   /* 0.3: a draw with |n1 . (n2 x n3)| below it is redrawn (:221) */
    double prob;         /* 0.99 (:257) */
    int max_iterations;  /* 5000 (:258) */
    int max_redraws;     /* 100 per trial */
    int chunk;           /* trials per launch; 0 = 256.  The outcome does not depend on it. */
    int pad;
} r360_rigcal_trim_params;
typedef struct { int inliers, trials, winner, no_model; } r360_rigcal_trim_stats;
int  r360_rigcal_create(r360_ctx* ctx, r360_rigcal** out);
void r360_rigcal_destroy(r360_rigcal* h);
/* A pair's rows [n][cols] row-major; cols must be 10; n = 0 removes the pair.  get: *n is set either way, cap (in
 * rows) < *n with rows given is an error. */
int  r360_rigcal_set_pair(r360_rigcal* h, int i, int j, const double* rows, int n, int cols);
int  r360_rigcal_get_pair(const r360_rigcal* h, int i, int j, double* rows, int cap, int* n);
int  r360_rigcal_clear(r360_rigcal* h);
/* 0, or R360_EMISSING_PAIR; host only. */
int  r360_rigcal_check(const r360_rigcal* h);
/* loadPlaneCorrespondences / savePlaneCorrespondences (Calibration.h:276-323): dir/correspondences_%u_%u.txt, text
 * matrices, one row per line, %.16e.  Host only.  load replaces every pair; save writes the pairs that have rows. */
int  r360_rigcal_load_dir(r360_rigcal* h, const char* dir);
int  r360_rigcal_save_dir(const r360_rigcal* h, const char* dir);
/* One such text matrix, no handle needed.  read: rows may be NULL (count only); cap in doubles. */
int  r360_rigcal_read_matrix(const char* path, double* rows, size_t cap, int* n_rows, int* n_cols);
int  r360_rigcal_write_matrix(const char* path, const double* rows, int n_rows, int n_cols);
/* loadConstructionSpecs. */
void r360_rigcal_specs(double rt8[8 * 16]);
/* The starting extrinsics of CalibrateRotation (a new handle holds the specs) and the current estimate. */
int  r360_rigcal_set_init(r360_rigcal* h, const double rt8[8 * 16]);
int  r360_rigcal_get_estimate(const r360_rigcal* h, double rt8[8 * 16]);
/* The estimate as dir/Rt_0{1..8}.txt, the files r360_calib_load_extrinsics reads.  Host only. */
int  r360_rigcal_save_extrinsics(const r360_rigcal* h, const char* dir);
/* CalibrateRotation(weighted): starts from the init extrinsics.  CalibrateTranslation(weighted): on the current
 * estimate's rotations; applied only when the conditioning is below 8000.  weighted is a plain flag (the reference
 * also asks for 18 columns).  Return 0 with stats->status set, or R360_EMISSING_PAIR (stats->status says so too). */
int  r360_rigcal_rotation(r360_rigcal* h, int weighted, r360_rigcal_stats* stats);
int  r360_rigcal_translation(r360_rigcal* h, int weighted, r360_rigcal_stats* stats);
void r360_rigcal_default_trim_params(r360_rigcal_trim_params* p);
/* trimOutliersRANSAC on one pair's rows, the live form of the fit (Calibration/OnlinePairCalibrator.cpp:84-160), a
 * counter-based hash of (seed, trial, redraw) for the draw.  The pair keeps its inliers, in order; mask [cap] (may be
 * NULL) gets one byte per former row.  3 rows or fewer, or no non-degenerate trial (no_model), leave it untouched. */
int  r360_rigcal_trim(r360_rigcal* h, int i, int j, const r360_rigcal_trim_params* params, unsigned seed,
                      r360_rigcal_trim_stats* stats, unsigned char* mask, int cap);
/* The collector, GetControlPlanes.cpp:358-469, on a frame built with R360_BUILD_PLANES | R360_BUILD_LOCAL_PLANES (on
 * the handle's device; R360_EINVAL without the flag): for sensors s1 < s2 and their local planes i, j, a row is added
 * when both have more than min_inliers pixels and an elongation below max_elongation, their rig-frame normals have a
 * dot product above min_dot and their rig-frame distances differ by less than max_dist.  Columns: the planes'
 * sensor-frame normal and d (r360_frame_get_local_planes), the smaller pixel count, and the larger of the two means of
 * (row + col) over a plane's pixels in its sensor's organised cloud, counted on the GPU over the final label image.
 * added[28] (may be NULL): rows added per pair.  conditioning: sigma_max / sigma_min of the adjacent pairs' sums of
 * n_i n_j^T (rig frame) over the rows collected so far, the pair (0, 7) under index 7 (:446-462); 1 before any row. */
typedef struct {
    int min_inliers;        /* 1000 */
    int pad;
    double max_elongation;  /* 5 */
    double min_dot;         /* 0.99 */
    double max_dist;        /* 0.2 */
} r360_rigcal_collect_params;
void r360_rigcal_default_collect_params(r360_rigcal_collect_params* p);
int  r360_rigcal_add_frame(r360_rigcal* h, r360_frame* frame, const r360_rigcal_collect_params* params, int* added);
int  r360_rigcal_conditioning(const r360_rigcal* h, float conditioning[8]);
/* Parity hooks.  eval: mode 0 rotation, 1 translation, at the current estimate: H [21][21] row-major, g [21],
 * scalars [4] = sum of squared residuals, sum of angles, rows, weighted error.  ransac_eval: trials [trial0, trial0 +
 * n) of a pair: the inlier count and the no-draw flag of each. */
int  r360_rigcal_eval(r360_rigcal* h, int mode, int weighted, double* H, double* g, double* scalars);
int  r360_rigcal_ransac_eval(r360_rigcal* h, int i, int j, const r360_rigcal_trim_params* params, unsigned seed,
                             int trial0, int n, int* counts, int* flags);

/* ---- Topological submaps: the SSO graph and its spectral partition (include/Map360.h, TopologicalMap360.h,
 * Relocalizer360.h; statement: tests/topo_model.py).
 *
 * A graph is a symmetric n x n matrix A of fp32 sensed-space-overlap values, row-major, >= 0, zero diagonal,
 * 1 <= n <= R360_TOPO_MAX_NODES.  bisect: the Fiedler vector v of the plain Laplacian diag(row sums) - A (cyclic Jacobi
 * in fp64, sweeps until off(L) <= 1e-14 ||L||_F), side 1 = {i : v_i >= mean(v)}, side 2 the rest ({i <= n/2} and
 * the rest when one would be empty), cut = the normalised cut of the two sides.  partition
 * (mrpt::graphs::CGraphPartitioner::RecursiveSpectralPartition, TopologicalMap360.h:411): a cluster whose cut is above
 * threshold_ncut, or one of whose sides has fewer than min_cluster nodes, stays one part; otherwise its sides are
 * partitioned in turn (recursive) or are the two parts; parts are numbered by their first node (RearrangePartition,
 * :372-387).  One workgroup per cluster, one launch per recursion level for all graphs of a call; results are
 * identical bit for bit between runs and between a lone and a batched call.
 * Return values: 0; R360_TOPO_NOT_CONVERGED (results written) when a cluster's Jacobi sweeps ran out; R360_EINVAL for
 * n < 1, n > R360_TOPO_MAX_NODES, a non-finite, negative or asymmetric entry, a non-zero diagonal or bad parameters
 * (nothing is launched; the context stays usable). */
#define R360_TOPO_MAX_NODES 256
#define R360_TOPO_NOT_CONVERGED 1
typedef struct {
    double threshold_ncut;   /* 0.8 */
    int min_cluster;         /* 3; at least 1 */
    int recursive;           /* 1 */
} r360_topo_params;
void r360_topo_default_params(r360_topo_params* p);
/* Parity hook: one bisection.  side [n]: 1 or 2; eigenvalues [n] ascending and fiedler [n] may be NULL; sweeps: the
 * Jacobi sweeps done. */
int  r360_topo_bisect(r360_ctx* ctx, const float* A, int n, int* side, double* cut, double* eigenvalues, double* fiedler,
                      int* sweeps);
/* part_of [n]; cuts (may be NULL, 2 n - 1 entries at most): the cut of every bisection made, ordered by the bisected
 * cluster's lowest node, of nested clusters the larger first (an order that does not depend on the eigenvectors'
 * signs); n_bisections (may be NULL) their number. */
int  r360_topo_partition(r360_ctx* ctx, const float* A, int n, const r360_topo_params* params, int* part_of, int* n_parts,
                         double* cuts, int* n_bisections);
int  r360_topo_partition_batch(r360_ctx* ctx, int count, const float* const* A, const int* n,
                               const r360_topo_params* params, int* const* part_of, int* n_parts);

/* The bookkeeping of Map360 + TopologicalMap360 on the host: keyframes (global ids 0, 1, ...) with an area each, one
 * symmetric SSO table over keyframe ids, the current area.  Two areas are neighbours exactly when a positive SSO joins
 * two of their keyframes; an area neighbours itself.  An area's representative keyframe (vSelectedKFs) has the
 * largest sum of SSO to the area's other keyframes, the lowest id among equals.
 *   add_keyframe    the new keyframe joins the current area; *kf (may be NULL) = its id
 *   drop_last       undoes the last add_keyframe and that keyframe's connections (SphereGraphSLAM.cpp:232-242)
 *   add_connection  sets SSO(kf1, kf2) = SSO(kf2, kf1) = sso, within one area or across two (TopologicalMap360.h:107-131)
 *   vicinity        the keyframes of the current area's neighbours (itself included), areas ascending, ids ascending
 *                   inside an area, and their SSO matrix [n][n]; kf_ids / sso may be NULL (count only); -4 when cap < n
 *   partition       Partitioner(): cuts the vicinity's matrix.  Nothing happens with fewer than 3 keyframes or when the
 *                   parts are no more than the vicinity's areas; otherwise those areas, ascending, take the first
 *                   parts, *n_new_areas new areas the others, and the current area is the one of the newest keyframe
 *   areas           area_of [cap] (may be NULL), the counts and the current area
 *   neighbors       the area's neighbours ascending; out may be NULL
 *   selected        the area's representative keyframe, -1 for an empty area
 * Only partition uses the context, which must live until the last partition call; destroy never reads it. */
typedef struct r360_topomap r360_topomap;
int  r360_topomap_create(r360_ctx* ctx, r360_topomap** out);
void r360_topomap_destroy(r360_topomap* m);
int  r360_topomap_add_keyframe(r360_topomap* m, int* kf);
int  r360_topomap_drop_last(r360_topomap* m);
int  r360_topomap_add_connection(r360_topomap* m, int kf1, int kf2, float sso);
int  r360_topomap_vicinity(r360_topomap* m, int* kf_ids, float* sso, int cap, int* n);
int  r360_topomap_partition(r360_topomap* m, const r360_topo_params* params, int* n_new_areas);
int  r360_topomap_areas(const r360_topomap* m, int* area_of, int cap, int* n_kf, int* n_areas, int* current_area);
int  r360_topomap_neighbors(const r360_topomap* m, int area, int* out, int cap, int* n);
int  r360_topomap_selected(const r360_topomap* m, int area, int* kf);

/* Relocalizer360::relocalize (include/Relocalizer360.h:78-93): RegisterPbMap(kfs[i], frame, max_match_planes,
 * PLANAR_3DoF) for i = n_kf - 1, ..., 0; the first keyframe in that order registered with at least min_matches (5)
 * matched planes and more than min_area (10) m2 of matched area wins: *kf = its index, pose [16] and info [36] (may be
 * NULL) = getPose() / getInfoMat() as doubles, layouts as r360_pair_result's.  *kf = -1 when there is none.  Candidates run in
 * chunks of the batch's lanes through r360_batch_register, newest first; later chunks are not run once one wins. */
int  r360_relocalize(r360_batch* b, r360_frame* const* kfs, int n_kf, r360_frame* frame, size_t max_match_planes,
                     int min_matches, float min_area, int* kf, double* pose, double* info);

#ifdef __cplusplus
}
#endif
#endif
