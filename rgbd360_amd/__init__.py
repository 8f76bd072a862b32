"""rgbd360_amd — MI355X-native (gfx950) registration hot path of rgbd360.

Python mirror of the reference's C++ class surface for the hot path, written over the C-ABI of
``rgbd360_amd/lib/librgbd360_hip.so`` (declared in ``include/rgbd360_hip.h``):

    Calib360          include/Calib360.h:44-132
    Frame360          include/Frame360.h:93-1150   (loadFrame / undistort / stitchSphericalImage /
                      buildSphereCloud / getPlanes)
    RegisterRGBD360   include/RegisterRGBD360.h:47-340 (RegisterPbMap / getPose / getInfoMat /
                      getMatchedPlanes / getAreaMatched / areaSource / areaTarget, Register alias)
    RegisterPhotoICP  include/RegisterPhotoICP.h:85-4784 (setSourceFrame / setTargetFrame /
                      alignFrames360 / getOptimalPose / getHessian / getGradient)

The HIP library is the only compute path: there is no CPU fallback.  Importing works without a
GPU (so the CPU test-suite can check that the library loads and exports its ABI); creating a
``Context`` on a machine without a GPU raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

C = C  # re-exported for callers that drive the C-ABI directly (bench.py)

__all__ = [
    "lib", "Context", "Calib360", "Frame360", "RegisterPhotoICP", "RegisterRGBD360", "IcpParams", "IcpStats",
    "GicpParams", "GicpStats", "GeneralizedICP", "GraphParams", "GraphStats", "PoseGraph", "g2o_write", "g2o_read",
    "PHOTO_CONSISTENCY", "DEPTH_CONSISTENCY", "PHOTO_DEPTH", "synth_path_pose", "exp_se3",
    "LIB_PATH", "ABI_SYMBOLS", "Batch", "PairJob", "PairResult", "JOB_PBMAP_ONLY", "JOB_GATED", "JOB_ALWAYS",
    "TopoParams", "TopologicalMap", "Relocalizer", "topo_bisect", "topo_partition", "topo_partition_batch",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R360_LIB") or os.path.join(_HERE, "lib", "librgbd360_hip.so")
REPO_ROOT = os.path.dirname(_HERE)

PHOTO_CONSISTENCY, DEPTH_CONSISTENCY, PHOTO_DEPTH = 0, 1, 2
BUILD_UNDISTORT, BUILD_SPHERE, BUILD_PYRAMID, BUILD_CLOUD, BUILD_PLANES = 1, 2, 4, 8, 16
BUILD_SENSOR_PYRAMID = 32
BUILD_LOCAL_PLANES = 64
BUILT_LEVEL0 = 256   # reported by Frame360.built() only: the sphere images and level 0's {gray, depth} are in HBM
PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED = 0, 1, 2


class IcpParams(C.Structure):
    """r360_icp_params — RegisterPhotoICP settings (see include/rgbd360_hip.h)."""
    _fields_ = [
        ("n_pyr", C.c_int), ("max_iters", C.c_int), ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("std_dev_photo", C.c_float), ("std_dev_depth", C.c_float), ("thres_sal_int", C.c_float),
        ("thres_sal_depth", C.c_float), ("tol_residual", C.c_double), ("tol_update", C.c_double),
        ("lambda_", C.c_double), ("fixed_iters_level0", C.c_int),
    ]

    @classmethod
    def default(cls) -> "IcpParams":
        p = cls()
        lib().r360_icp_default_params(C.byref(p))
        return p


class GicpParams(C.Structure):
    """r360_gicp_params — Generalized-ICP settings under PCL's names (see include/rgbd360_hip.h)."""
    _fields_ = [
        ("k_correspondences", C.c_int), ("gicp_epsilon", C.c_float), ("max_corr_dist", C.c_float),
        ("max_iterations", C.c_int), ("max_inner_iterations", C.c_int), ("rotation_epsilon", C.c_double),
        ("transformation_epsilon", C.c_double),
    ]

    @classmethod
    def default(cls) -> "GicpParams":
        p = cls()
        lib().r360_gicp_default_params(C.byref(p))
        return p


class GicpStats(C.Structure):
    """r360_gicp_stats — what one r360_gicp_align did."""
    _fields_ = [
        ("iterations", C.c_int), ("converged", C.c_int), ("inner_steps", C.c_int), ("n_corr", C.c_size_t),
        ("cost", C.c_double), ("fitness", C.c_double),
    ]


OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1


class OutlierParams(C.Structure):
    """r360_outlier_params — pcl::StatisticalOutlierRemoval (mean_k, stddev_mul, max_dist) or
    pcl::RadiusOutlierRemoval (radius, min_neighbors), chosen by kind (see include/rgbd360_hip.h)."""
    _fields_ = [
        ("kind", C.c_int), ("mean_k", C.c_int), ("stddev_mul", C.c_float), ("max_dist", C.c_float),
        ("radius", C.c_float), ("min_neighbors", C.c_int),
    ]

    @classmethod
    def default(cls) -> "OutlierParams":
        p = cls()
        lib().r360_outlier_default_params(C.byref(p))
        return p

    @classmethod
    def statistical(cls, mean_k: int = 20, stddev_mul: float = 1.0, max_dist: float = 0.5) -> "OutlierParams":
        p = cls.default()
        p.kind, p.mean_k, p.stddev_mul, p.max_dist = OUTLIER_STATISTICAL, mean_k, stddev_mul, max_dist
        return p

    @classmethod
    def radius_filter(cls, radius: float = 0.15, min_neighbors: int = 5) -> "OutlierParams":
        p = cls.default()
        p.kind, p.radius, p.min_neighbors = OUTLIER_RADIUS, radius, min_neighbors
        return p


class OutlierStats(C.Structure):
    """r360_outlier_stats — what one outlier filter call saw and did."""
    _fields_ = [
        ("n_in", C.c_size_t), ("n_finite", C.c_size_t), ("n_short", C.c_size_t), ("n_removed", C.c_size_t),
        ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double),
    ]


class NormalParams(C.Structure):
    """r360_normal_params — pcl::NormalEstimation's neighbourhood: at most k points, the point itself included, within
    radius (see include/rgbd360_hip.h)."""
    _fields_ = [("k", C.c_int), ("radius", C.c_float)]

    @classmethod
    def default(cls) -> "NormalParams":
        p = cls()
        lib().r360_normal_default_params(C.byref(p))
        return p

    @classmethod
    def make(cls, k: int = 20, radius: float = 0.25) -> "NormalParams":
        p = cls.default()
        p.k, p.radius = k, radius
        return p


class NormalStats(C.Structure):
    """r360_normal_stats — what one normal estimation saw."""
    _fields_ = [("n_in", C.c_size_t), ("n_finite", C.c_size_t), ("n_short", C.c_size_t),
                ("sum_neighbors", C.c_ulonglong)]


class ClusterParams(C.Structure):
    """r360_cluster_params — pcl::EuclideanClusterExtraction's tolerance and size bounds, and the angle of the
    normal-aware form in radians (see include/rgbd360_hip.h)."""
    _fields_ = [("tolerance", C.c_float), ("min_size", C.c_int), ("max_size", C.c_int), ("eps_angle", C.c_float)]

    @classmethod
    def default(cls) -> "ClusterParams":
        p = cls()
        lib().r360_cluster_default_params(C.byref(p))
        return p

    @classmethod
    def make(cls, tolerance: float = 0.10, min_size: int = 100, max_size: int = 1 << 30,
             eps_angle: "float | None" = None) -> "ClusterParams":
        p = cls.default()
        p.tolerance, p.min_size, p.max_size = tolerance, min_size, max_size
        if eps_angle is not None:
            p.eps_angle = eps_angle
        return p


class ClusterStats(C.Structure):
    """r360_cluster_stats — what one cluster extraction saw."""
    _fields_ = [("n_in", C.c_size_t), ("n_finite", C.c_size_t), ("n_components", C.c_size_t), ("n_clusters", C.c_size_t),
                ("n_clustered", C.c_size_t)]


class ClusterInfo(C.Structure):
    """r360_cluster_info — one cluster's record."""
    _fields_ = [("size", C.c_int), ("root", C.c_int), ("min", C.c_float * 3), ("max", C.c_float * 3),
                ("centroid", C.c_double * 3), ("eig", C.c_double * 3), ("normal", C.c_double * 3), ("curvature", C.c_double)]


# the records as a numpy structured array, field for field
CLUSTER_INFO_DTYPE = np.dtype([("size", np.int32), ("root", np.int32), ("min", np.float32, 3), ("max", np.float32, 3),
                               ("centroid", np.float64, 3), ("eig", np.float64, 3), ("normal", np.float64, 3),
                               ("curvature", np.float64)])
assert CLUSTER_INFO_DTYPE.itemsize == C.sizeof(ClusterInfo)

SAC_ROUND = 128           # R360_SAC_ROUND: hypotheses per round of the plane search
SAC_NONE, SAC_PERPENDICULAR, SAC_PARALLEL = 0, 1, 2


class SacParams(C.Structure):
    """r360_sac_params — pcl::SACSegmentation's settings for the three plane models with SAC_RANSAC, and the peel loop's
    (see include/rgbd360_hip.h); angles in radians."""
    _fields_ = [("distance_threshold", C.c_float), ("max_iterations", C.c_int), ("probability", C.c_float),
                ("optimize", C.c_int), ("constraint", C.c_int), ("axis", C.c_float * 3), ("eps_angle", C.c_float),
                ("normal_angle", C.c_float), ("max_planes", C.c_int), ("min_inliers", C.c_int),
                ("stop_fraction", C.c_float), ("reserved", C.c_int), ("seed", C.c_ulonglong)]

    @classmethod
    def default(cls) -> "SacParams":
        p = cls()
        lib().r360_sac_default_params(C.byref(p))
        return p

    @classmethod
    def make(cls, **kw) -> "SacParams":
        """The defaults with the given fields replaced (axis: three floats)."""
        p = cls.default()
        for k, v in kw.items():
            if k == "axis":
                p.axis[0], p.axis[1], p.axis[2] = (float(a) for a in v)
            elif k in ("reserved",) or k not in dict(cls._fields_):
                raise TypeError(f"SacParams has no field {k!r}")
            else:
                setattr(p, k, v)
        return p


class SacStats(C.Structure):
    """r360_sac_stats — what one plane segmentation saw."""
    _fields_ = [("n_in", C.c_size_t), ("n_finite", C.c_size_t), ("n_planes", C.c_size_t), ("n_in_planes", C.c_size_t),
                ("n_evaluated", C.c_size_t)]


class SacPlane(C.Structure):
    """r360_sac_plane — one plane's record."""
    _fields_ = [("coef", C.c_double * 4), ("centroid", C.c_double * 3), ("eig", C.c_double * 3), ("curvature", C.c_double),
                ("size", C.c_int), ("raw_size", C.c_int), ("best_hypothesis", C.c_int), ("evaluated", C.c_int)]


SAC_PLANE_DTYPE = np.dtype([("coef", np.float64, 4), ("centroid", np.float64, 3), ("eig", np.float64, 3),
                            ("curvature", np.float64), ("size", np.int32), ("raw_size", np.int32),
                            ("best_hypothesis", np.int32), ("evaluated", np.int32)])
assert SAC_PLANE_DTYPE.itemsize == C.sizeof(SacPlane)
SAC_MAX_PLANES = 64


class GraphParams(C.Structure):
    """r360_graph_params — pose-graph optimisation settings (see include/rgbd360_hip.h)."""
    _fields_ = [
        ("max_iterations", C.c_int), ("max_trials", C.c_int), ("gain_epsilon", C.c_double), ("cg_tolerance", C.c_double),
        ("cg_max_iterations", C.c_int), ("cg_form", C.c_int),
    ]

    @classmethod
    def default(cls, **kw) -> "GraphParams":
        p = cls()
        lib().r360_graph_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class GraphStats(C.Structure):
    """r360_graph_stats — what one r360_graph_optimize did."""
    _fields_ = [
        ("status", C.c_int), ("iterations", C.c_int), ("trials", C.c_int), ("cg_form", C.c_int),
        ("F_initial", C.c_double), ("F_final", C.c_double), ("lambda_", C.c_double), ("cg_iterations", C.c_longlong),
        ("cg_iterations_max", C.c_int), ("pad", C.c_int),
    ]


GRAPH_CONVERGED, GRAPH_ITERATION_LIMIT, GRAPH_STALLED, GRAPH_CG_NOT_CONVERGED = 0, 1, 2, 3
GRAPH_KERNEL_NONE, GRAPH_KERNEL_HUBER, GRAPH_KERNEL_CAUCHY = 0, 1, 2   # R360_GRAPH_KERNEL_*


class TopoParams(C.Structure):
    """r360_topo_params — the spectral partition's settings (see include/rgbd360_hip.h)."""
    _fields_ = [("threshold_ncut", C.c_double), ("min_cluster", C.c_int), ("recursive", C.c_int)]

    @classmethod
    def default(cls, **kw) -> "TopoParams":
        p = cls()
        lib().r360_topo_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


TOPO_MAX_NODES = 256
TOPO_LDS_MAX_NODES = 96   # up to here a cluster's matrices live in LDS, above in the context's scratch


class RigcalStats(C.Structure):
    """r360_rigcal_stats — what one r360_rigcal_rotation / _translation did (per-iteration arrays of 10)."""
    _fields_ = [
        ("status", C.c_int), ("iterations", C.c_int), ("rows", C.c_int), ("pad", C.c_int),
        ("error", C.c_double * 10), ("angle", C.c_double * 10), ("conditioning", C.c_double * 10),
        ("update2", C.c_double * 10), ("werr0", C.c_double * 10), ("werr1", C.c_double * 10), ("accepted", C.c_int * 10),
    ]


class RigcalTrimParams(C.Structure):
    """r360_rigcal_trim_params — the outlier trimmer's settings (see include/rgbd360_hip.h)."""
    _fields_ = [
        ("dist", C.c_double), ("degenerate", C.c_double), ("prob", C.c_double), ("max_iterations", C.c_int),
        ("max_redraws", C.c_int), ("chunk", C.c_int), ("pad", C.c_int),
    ]

    @classmethod
    def default(cls, **kw) -> "RigcalTrimParams":
        p = cls()
        lib().r360_rigcal_default_trim_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class RigcalCollectParams(C.Structure):
    """r360_rigcal_collect_params — the collector's thresholds (GetControlPlanes.cpp:386-389)."""
    _fields_ = [("min_inliers", C.c_int), ("pad", C.c_int), ("max_elongation", C.c_double), ("min_dot", C.c_double),
                ("max_dist", C.c_double)]

    @classmethod
    def default(cls, **kw) -> "RigcalCollectParams":
        p = cls()
        lib().r360_rigcal_default_collect_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class RigcalTrimStats(C.Structure):
    """r360_rigcal_trim_stats — what one r360_rigcal_trim did."""
    _fields_ = [("inliers", C.c_int), ("trials", C.c_int), ("winner", C.c_int), ("no_model", C.c_int)]


RIGCAL_CONVERGED, RIGCAL_ITERATION_LIMIT, RIGCAL_BAD_CONDITIONED, RIGCAL_MISSING_PAIR = 0, 1, 2, 3
EMISSING_PAIR = -6


class MatchParams(C.Structure):
    """r360_match_params — SubgraphMatcher thresholds, the keys of config_files/configLocaliser_*.ini that
    RegisterRGBD360(configFile) loads (RegisterRGBD360.h:97-100); angles in degrees."""
    _fields_ = [("min_planes_recognition", C.c_int), ("dist_d", C.c_float), ("angle", C.c_float),
                ("color_threshold", C.c_float), ("intensity_threshold", C.c_float),
                ("elongation_threshold", C.c_float), ("area_threshold", C.c_float), ("dist_threshold", C.c_float),
                ("angle_threshold", C.c_float), ("height_threshold", C.c_float), ("cos_angle_parallel", C.c_float),
                ("planar_normal_angle", C.c_float), ("max_nodes", C.c_long)]

    @classmethod
    def default(cls) -> "MatchParams":
        """configLocaliser_sphericalOdometry.ini (the odometry apps' file)."""
        m = cls()
        lib().r360_match_params_default(C.byref(m))
        return m

    @classmethod
    def load_ini(cls, path: str, base: "MatchParams | None" = None) -> "MatchParams":
        m = cls.default() if base is None else base
        _check(lib().r360_match_params_load_ini(path.encode(), C.byref(m)), "match_params_load_ini")
        return m


class IcpStats(C.Structure):
    _fields_ = [
        ("iters", C.c_int * 8), ("evals", C.c_int * 8), ("illposed", C.c_int), ("sso", C.c_float),
        ("error", C.c_double), ("passes", C.c_int), ("persistent", C.c_int),
        ("av_photo_residual", C.c_double), ("av_depth_residual", C.c_double), ("av_residual", C.c_float),
        ("residuals_set", C.c_int),
    ]


class PairJob(C.Structure):
    """r360_pair_job — one pair of a batched registration call (include/rgbd360_hip.h, §8f-4)."""
    _fields_ = [("ref", C.c_void_p), ("trg", C.c_void_p), ("dense", C.c_int), ("ref_is_source", C.c_int),
                ("guess", C.c_float * 16)]


class PairResult(C.Structure):
    """r360_pair_result — RegisterPbMap outputs and the dense refinement of one batched pair."""
    _fields_ = [("good", C.c_int), ("n_match", C.c_int), ("area_matched", C.c_float), ("area_src", C.c_float),
                ("area_trg", C.c_float), ("sso_pbmap", C.c_float), ("pbmap_pose", C.c_float * 16),
                ("pbmap_info", C.c_float * 36), ("dense_rc", C.c_int), ("pose", C.c_float * 16),
                ("hessian", C.c_float * 36), ("stats", IcpStats)]

    def as_dict(self) -> dict:
        return {"good": self.good, "n_match": self.n_match, "area_matched": self.area_matched,
                "area_src": self.area_src, "area_trg": self.area_trg, "sso_pbmap": self.sso_pbmap,
                "pbmap_pose": _from16(np.array(self.pbmap_pose, np.float32)),
                "pbmap_info": np.array(self.pbmap_info, np.float32).reshape(6, 6).T.copy(),
                "dense_rc": self.dense_rc, "pose": _from16(np.array(self.pose, np.float32)),
                "hessian": np.array(self.hessian, np.float32).reshape(6, 6).T.copy(),
                "sso": self.stats.sso, "error": self.stats.error}


JOB_PBMAP_ONLY, JOB_GATED, JOB_ALWAYS = 0, 1, 2


class DenseStats(C.Structure):
    """r360_dense_stats — RegisterDensePhotoICP per-level diagnostics."""
    _fields_ = [("error", C.c_double * 8), ("ran", C.c_int * 8), ("n_visible", C.c_int * 8), ("n_error", C.c_int * 8),
                ("illposed_level", C.c_int), ("levels", C.c_int), ("info_set", C.c_int), ("pad", C.c_int),
                ("gradient", C.c_float * 6)]


class Plane(C.Structure):
    """r360_plane — the mrpt::pbmap::Plane fields used on the path (rig frame)."""
    _fields_ = [("normal", C.c_float * 3), ("center", C.c_float * 3), ("d", C.c_float), ("area", C.c_float),
                ("elongation", C.c_float), ("curvature", C.c_float), ("ppal", C.c_float * 3), ("nrgb", C.c_float * 3),
                ("intensity", C.c_float), ("id", C.c_int), ("sensor", C.c_int), ("n_inliers", C.c_int),
                ("n_hull", C.c_int)]


class Region(C.Structure):
    _fields_ = [("label", C.c_int), ("count", C.c_int), ("start_idx", C.c_int), ("n_contour", C.c_int),
                ("n_fit", C.c_int), ("centroid", C.c_float * 3), ("cov", C.c_float * 9), ("model", C.c_float * 4),
                ("curvature", C.c_float)]


DEFAULT_6DoF, PLANAR_3DoF, ODOMETRY_6DoF, PLANAR_ODOMETRY_3DoF = 0, 1, 2, 3


# (name, restype, argtypes) of every exported entry point of include/rgbd360_hip.h
_P = C.c_void_p
_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int)
_SIGS = [
    ("r360_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("r360_ctx_destroy", None, [_P]),
    ("r360_ctx_sync", C.c_int, [_P]),
    ("r360_ctx_stream", _P, [_P]),
    ("r360_last_error", C.c_char_p, []),
    ("r360_version", C.c_char_p, []),
    ("r360_calib_create", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    ("r360_calib_destroy", None, [_P]),
    ("r360_calib_set_extrinsics", C.c_int, [_P, _FP]),
    ("r360_calib_get_extrinsics", C.c_int, [_P, _FP, _FP, _FP]),
    ("r360_calib_load_extrinsics", C.c_int, [_P, C.c_char_p]),
    ("r360_calib_load_intrinsics", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_create", C.c_int, [_P, _P, C.POINTER(_P)]),
    ("r360_frame_destroy", None, [_P]),
    ("r360_frame_upload", C.c_int, [_P, _P, _P]),
    ("r360_frame_upload_device", C.c_int, [_P, _P, _P]),
    ("r360_frame_upload_async", C.c_int, [_P, _P, _P]),
    ("r360_frame_set_sphere", C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    ("r360_calib_create_sphere", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    ("r360_host_register", C.c_int, [_P, C.c_size_t]),
    ("r360_host_unregister", C.c_int, [_P]),
    ("r360_frame_load_bin", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_save_bin", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_set_timestamp", C.c_int, [_P, C.c_uint64]),
    ("r360_frame_get_timestamp", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("r360_frame_get_sphere_cloud", C.c_int, [_P, _FP, _P, C.c_size_t, _IP, _IP]),
    ("r360_pcd_write", C.c_int, [C.c_char_p, _FP, _P, C.c_int, C.c_int, C.c_int]),
    ("r360_pcd_read", C.c_int, [C.c_char_p, _FP, _P, C.c_size_t, C.POINTER(C.c_size_t), _IP, _IP]),
    ("r360_frame_save_cloud", C.c_int, [_P, C.c_char_p, C.c_int]),
    ("r360_frame_load_cloud", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_save_planes", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_load_pbmap", C.c_int, [_P, C.c_char_p]),
    ("r360_frame_save", C.c_int, [_P, C.c_char_p, C.c_uint]),
    ("r360_frame_load_pbmap_cloud", C.c_int, [_P, C.c_char_p, C.c_uint]),
    ("r360_frame_set_plane_label", C.c_int, [_P, C.c_int, C.c_char_p]),
    ("r360_frame_get_plane_label", C.c_int, [_P, C.c_int, C.c_char_p, C.c_int]),
    ("r360_frame_build", C.c_int, [_P, C.c_uint]),
    ("r360_frame_build_async", C.c_int, [_P, C.c_uint]),
    ("r360_frames_build", C.c_int, [_P, C.c_int, C.c_uint]),
    ("r360_frame_dims", C.c_int, [_P, _IP, _IP, _IP, _IP]),
    ("r360_frame_set_levels", C.c_int, [_P, C.c_int]),
    ("r360_frame_set_compaction", C.c_int, [_P, C.c_int]),
    ("r360_frame_built", C.c_int, [_P, C.POINTER(C.c_uint)]),
    ("r360_frame_get_sphere", C.c_int, [_P, _P, _P]),
    ("r360_frame_get_depth_m", C.c_int, [_P, _P]),
    ("r360_frame_get_level", C.c_int, [_P, C.c_int, _IP, _IP, _P, _P, _P, _P, _P, _P]),
    ("r360_frame_get_saliency", C.c_int, [_P, _P, _FP, _FP]),
    ("r360_frame_get_points", C.c_int, [_P, C.c_int, _FP, C.c_int, _IP]),
    ("r360_frame_get_sensor_level", C.c_int, [_P, C.c_int, C.c_int, _IP, _IP, _P, _P, _P, _P, _P, _P]),
    ("r360_icp_default_params", None, [C.POINTER(IcpParams)]),
    ("r360_align360", C.c_int, [_P, _P, _P, _FP, C.c_int, C.c_int, C.POINTER(IcpParams), _FP, _FP, _FP,
                                C.POINTER(IcpStats)]),
    ("r360_align360_async", C.c_int, [_P, _P, _P, _FP, C.c_int, C.c_int, C.POINTER(IcpParams)]),
    ("r360_align360_result", C.c_int, [_P, _FP, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_align360_batch_async", C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _FP, C.c_int,
                                            C.POINTER(IcpParams)]),
    ("r360_align360_batch_result", C.c_int, [_P, _FP, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_refine_eval", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("r360_dense_queue_create", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("r360_dense_queue_destroy", None, [_P]),
    ("r360_dense_queue_ctx", C.c_void_p, [_P]),
    ("r360_dense_queue_stats", C.c_int, [_P, C.POINTER(C.c_long), C.POINTER(C.c_long), _IP]),
    ("r360_dense_queue_submit", C.c_int, [_P, _P, _P, _FP, C.c_int, C.POINTER(IcpParams), C.POINTER(C.c_long)]),
    ("r360_dense_queue_collect", C.c_int, [_P, C.c_long, _FP, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_register_submit", C.c_int, [_P, _P, _P, _P, _FP, C.POINTER(IcpParams), C.c_size_t, C.c_int,
                                       C.POINTER(C.c_long)]),
    ("r360_register_collect", C.c_int, [_P, C.c_long, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_sequence_default_params", None, [_P]),
    ("r360_sequence_create", C.c_int, [C.c_int, _P, C.c_char_p, C.POINTER(_P)]),
    ("r360_sequence_destroy", None, [_P]),
    ("r360_sequence_run", C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P]),
    ("r360_sequence_info", C.c_int, [_P, _IP, C.POINTER(_P)]),
    ("r360_sequence_pipeline", C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), _P, C.c_int, _IP,
                                         C.POINTER(C.c_long)]),
    ("r360_sequence_host_times", C.c_int, [_P, _P, C.c_int]),
    ("r360_sequence_plane_stats", C.c_int, [_P, C.POINTER(C.c_long), C.POINTER(C.c_long), _IP, C.POINTER(_P)]),
    ("r360_icp_eval", C.c_int, [_P, _P, _P, C.c_int, _FP, C.c_int, C.POINTER(IcpParams), _DP, _DP, _DP, _IP,
                                _IP]),
    ("r360_icp_eval_occ", C.c_int, [_P, _P, _P, C.c_int, _FP, C.c_int, C.c_int, C.POINTER(IcpParams), _DP, _DP,
                                    _DP, _IP, _IP]),
    ("r360_icp_pass_grid", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _IP, _IP]),
    ("r360_icp_eval_batch", C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, _FP, C.c_int,
                                      C.POINTER(IcpParams), _DP, _DP, _DP, _IP, _IP]),
    ("r360_exp_se3", None, [_DP, C.c_int, _FP]),
    ("r360_align_pinhole", C.c_int, [_P, _P, _P, C.c_int, _FP, C.c_int, _FP, C.POINTER(IcpParams), _FP, _FP, _FP,
                                     C.POINTER(IcpStats)]),
    ("r360_align_pinhole_async", C.c_int, [_P, _P, _P, C.c_int, _IP, _FP, C.c_int, _FP, C.POINTER(IcpParams)]),
    ("r360_align_pinhole_result", C.c_int, [_P, _FP, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_pinhole_eval", C.c_int, [_P, _P, _P, C.c_int, C.c_int, _FP, C.c_int, _FP, C.POINTER(IcpParams), _DP, _DP,
                                    _DP, _DP, _IP]),
    ("r360_register_dense", C.c_int, [_P, _P, _P, _FP, C.c_int, C.c_int, C.POINTER(IcpParams), _FP, _FP,
                                      C.POINTER(DenseStats)]),
    ("r360_dense_robot_eval", C.c_int, [_P, _P, _P, C.c_int, _FP, C.c_int, C.POINTER(IcpParams), _DP, _DP, _DP,
                                        _IP]),
    ("r360_frame_get_planes", C.c_int, [_P, C.POINTER(Plane), C.c_int, _IP]),
    ("r360_frame_get_plane_hull", C.c_int, [_P, C.c_int, _FP, C.c_int, _IP]),
    ("r360_match_params_default", None, [C.POINTER(MatchParams)]),
    ("r360_match_params_load_ini", C.c_int, [C.c_char_p, C.POINTER(MatchParams)]),
    ("r360_ctx_set_match_params", C.c_int, [_P, C.POINTER(MatchParams)]),
    ("r360_ctx_get_match_params", C.c_int, [_P, C.POINTER(MatchParams)]),
    ("r360_ctx_match_stats", C.c_int, [_P, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    ("r360_match_tree_search", C.c_int, [C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_long, _P, C.POINTER(C.c_long)]),
    ("r360_batch_set_match_params", C.c_int, [_P, C.POINTER(MatchParams)]),
    ("r360_register_pbmap", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _FP, _FP, _IP, C.c_int, _IP, _FP, _FP, _FP]),
    ("r360_register", C.c_int, [_P, _P, _P, _FP, C.POINTER(IcpParams), C.c_size_t, C.c_int, _FP, _FP,
                                C.POINTER(IcpStats)]),
    ("r360_register_async", C.c_int, [_P, _P, _P, _FP, C.POINTER(IcpParams), C.c_size_t, C.c_int]),
    ("r360_register_result", C.c_int, [_P, _FP, _FP, C.POINTER(IcpStats)]),
    ("r360_pbmap_match_tables", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _IP, _IP, _IP, _IP, _P, _P, C.c_int]),
    ("r360_batch_create", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("r360_batch_destroy", None, [_P]),
    ("r360_batch_lanes", C.c_int, [_P]),
    ("r360_batch_register", C.c_int, [_P, C.POINTER(PairJob), C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_float,
                                      C.POINTER(IcpParams), C.POINTER(PairResult)]),
    ("r360_track_frame", C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, _P, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                   _IP, C.POINTER(PairResult), C.POINTER(PairResult)]),
    ("r360_frame_get_cloud", C.c_int, [_P, _FP, _P, _FP, _FP]),
    ("r360_frame_get_labels", C.c_int, [_P, _IP, _IP]),
    ("r360_frame_get_regions", C.c_int, [_P, C.c_int, C.POINTER(Region), C.c_int, _IP]),
    ("r360_frame_segment_eval", C.c_int, [_P, _FP, _FP, C.c_int, _P, _IP]),
    ("r360_frames_segment_eval", C.c_int, [C.POINTER(C.c_void_p), C.c_int, _FP, _FP, C.c_int, _P, _IP]),
    ("r360_frame_get_refine_states", C.c_int, [_P, _P, _IP]),
    ("r360_refine_force_fallback", None, [C.c_uint64, C.c_int]),
    ("r360_frame_get_region_detail", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), _FP, _FP, C.c_int, _IP]),
    ("r360_comm_unique_id", C.c_int, [_P]),
    ("r360_comm_init", C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    ("r360_comm_destroy", None, [_P]),
    ("r360_comm_allgather", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("r360_comm_allreduce_max", C.c_int, [_P, _DP, C.c_int]),
    ("r360_dev_alloc", C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    ("r360_dev_free", C.c_int, [_P]),
    ("r360_dev_copy", C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    ("r360_synth_frame", C.c_int, [_P, C.c_uint32, _FP, _P, _P]),
    ("r360_synth_frame_rt", C.c_int, [C.c_int, C.c_int, _FP, C.c_uint32, _FP, _P, _P]),
    ("r360_synth_path_pose", C.c_int, [C.c_uint32, C.c_int, _FP]),
    ("r360_libm_eval", C.c_int, [_FP, _FP, _FP, C.c_int, _FP, _FP, C.c_int]),
    ("r360_rn_check", C.c_int, [C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong)]),
    ("r360_rank6", C.c_int, [_FP, C.c_int, _IP]),
    ("r360_data_dir", C.c_char_p, []),
    ("r360_solve6", C.c_int, [_DP, _DP, C.c_int, _DP]),
    ("r360_proj_check_pose", C.c_int, [_FP, _FP, _FP, C.c_int, _FP, C.c_int, C.c_int, C.POINTER(C.c_ulonglong),
                                       C.POINTER(C.c_ulonglong)]),
    ("r360_proj_check", C.c_int, [_FP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong),
                                  C.POINTER(C.c_ulonglong)]),
    ("r360_ctx_debug_stamps", C.c_int, [_P, C.POINTER(C.c_ulonglong)]),
    ("r360_ctx_kernel_time", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    ("r360_ctx_kernel_time_reset", C.c_int, [_P]),
    ("r360_ctx_host_times", C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
    ("r360_ctx_kernel_stats", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long),
                                        C.POINTER(C.c_long)]),
    ("r360_ctx_timing", C.c_int, [_P, C.c_int]),
    ("r360_ctx_persistent_levels", C.c_int, [_P, C.c_int]),
    ("r360_ctx_latency_mode", C.c_int, [_P, C.c_int]),
    ("r360_ctx_timing_read", C.c_int, [_P, C.c_char_p, _DP, C.POINTER(C.c_long)]),
    ("r360_ctx_timing_reset", C.c_int, [_P]),
    ("r360_cloud_filter_euclidean", C.c_int, [_FP, _P, C.c_size_t, C.c_float, C.c_float, C.c_float, _FP, _P,
                                              C.POINTER(C.c_size_t)]),
    ("r360_cloud_filter_voxel", C.c_int, [_P, _FP, _P, C.c_size_t, C.c_float, _FP, _P, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_reset", C.c_int, [_P]),
    ("r360_ctx_map_add_cloud", C.c_int, [_P, _FP, _P, C.c_size_t, C.c_float]),
    ("r360_ctx_map_add_frame", C.c_int, [_P, _P, _FP, C.c_float, C.c_float, C.c_float, C.c_float]),
    ("r360_ctx_map_size", C.c_int, [_P, C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_download", C.c_int, [_P, _FP, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_outlier_default_params", None, [C.POINTER(OutlierParams)]),
    ("r360_cloud_filter_outliers", C.c_int, [_P, _FP, _P, C.c_size_t, C.POINTER(OutlierParams), _FP, _P, C.c_size_t,
                                             C.POINTER(C.c_size_t), C.POINTER(OutlierStats)]),
    ("r360_ctx_map_filter_outliers", C.c_int, [_P, C.POINTER(OutlierParams), C.POINTER(OutlierStats)]),
    ("r360_cloud_outlier_eval", C.c_int, [_P, _FP, C.c_size_t, C.POINTER(OutlierParams), _DP, _IP]),
    ("r360_normal_default_params", None, [C.POINTER(NormalParams)]),
    ("r360_cloud_normals", C.c_int, [_P, _FP, C.c_size_t, C.POINTER(NormalParams), _FP, C.c_int, _FP, _FP,
                                     C.POINTER(NormalStats)]),
    ("r360_ctx_map_estimate_normals", C.c_int, [_P, C.POINTER(NormalParams), _FP, C.c_int, C.POINTER(NormalStats)]),
    ("r360_ctx_map_download_normals", C.c_int, [_P, _FP, _FP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_cloud_normals_eval", C.c_int, [_P, _FP, C.c_size_t, C.POINTER(NormalParams), _FP, C.c_int, _IP, _IP, _DP, _DP,
                                          _DP]),
    ("r360_pcd_write_normals", C.c_int, [C.c_char_p, _FP, _P, _FP, _FP, C.c_size_t, C.c_int]),
    ("r360_pcd_read_normals", C.c_int, [C.c_char_p, _FP, _P, _FP, _FP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_cluster_default_params", None, [C.POINTER(ClusterParams)]),
    ("r360_cloud_clusters", C.c_int, [_P, _FP, _FP, C.c_size_t, C.POINTER(ClusterParams), _IP, _P, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(ClusterStats)]),
    ("r360_cloud_clusters_eval", C.c_int, [_P, _FP, _FP, C.c_size_t, C.POINTER(ClusterParams), _IP, _P, C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(ClusterStats), _IP, _IP]),
    ("r360_ctx_map_cluster", C.c_int, [_P, C.POINTER(ClusterParams), C.c_int, C.POINTER(ClusterStats)]),
    ("r360_ctx_map_download_labels", C.c_int, [_P, _IP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_cluster_info", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_filter_clusters", C.c_int, [_P, C.POINTER(ClusterParams), C.c_int, C.POINTER(ClusterStats)]),
    ("r360_sac_default_params", None, [C.POINTER(SacParams)]),
    ("r360_cloud_sac_planes", C.c_int, [_P, _FP, _FP, C.c_size_t, C.POINTER(SacParams), _IP, _P, C.c_size_t,
                                        C.POINTER(C.c_size_t), C.POINTER(SacStats)]),
    ("r360_cloud_sac_eval", C.c_int, [_P, _FP, _FP, C.c_size_t, C.POINTER(SacParams), _DP, C.c_size_t, _IP, _DP, _IP]),
    ("r360_ctx_map_sac_planes", C.c_int, [_P, C.POINTER(SacParams), C.c_int, C.POINTER(SacStats)]),
    ("r360_ctx_map_download_plane_labels", C.c_int, [_P, _IP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_plane_info", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_ctx_map_filter_planes", C.c_int, [_P, C.POINTER(SacParams), C.c_int, C.c_int, C.POINTER(SacStats)]),
    ("r360_pcd_write_labels", C.c_int, [C.c_char_p, _FP, _P, _IP, C.c_size_t, C.c_int]),
    ("r360_pcd_read_labels", C.c_int, [C.c_char_p, _FP, _P, _IP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_gicp_default_params", None, [C.POINTER(GicpParams)]),
    ("r360_gicp_set_source", C.c_int, [_P, _FP, C.c_size_t, C.POINTER(GicpParams)]),
    ("r360_gicp_set_target", C.c_int, [_P, _FP, C.c_size_t, C.POINTER(GicpParams)]),
    ("r360_gicp_align", C.c_int, [_P, _FP, C.POINTER(GicpParams), _FP, C.POINTER(GicpStats)]),
    ("r360_gicp_get_cloud", C.c_int, [_P, C.c_int, _FP, _FP, _IP, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r360_gicp_eval", C.c_int, [_P, _FP, C.POINTER(GicpParams), _IP, _DP, _DP, _DP, C.POINTER(C.c_size_t)]),
    ("r360_graph_create", C.c_int, [_P, C.POINTER(_P)]),
    ("r360_graph_destroy", None, [_P]),
    ("r360_graph_add_vertex", C.c_int, [_P, _DP, _IP]),
    ("r360_graph_set_fixed", C.c_int, [_P, C.c_int, C.c_int]),
    ("r360_graph_set_pose", C.c_int, [_P, C.c_int, _DP]),
    ("r360_graph_add_edge", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("r360_graph_size", C.c_int, [_P, _IP, _IP]),
    ("r360_graph_set_default_kernel", C.c_int, [_P, C.c_int, C.c_double]),
    ("r360_graph_set_edge_kernel", C.c_int, [_P, C.c_int, C.c_int, C.c_double]),
    ("r360_graph_get_edge_kernel", C.c_int, [_P, C.c_int, _IP, _DP]),
    ("r360_graph_set_edge_active", C.c_int, [_P, C.c_int, C.c_int]),
    ("r360_graph_get_edge_active", C.c_int, [_P, C.c_int, _IP]),
    ("r360_graph_edge_stats", C.c_int, [_P, _DP, _DP, C.c_int, _IP]),
    ("r360_graph_get_poses", C.c_int, [_P, _DP, C.c_int, _IP]),
    ("r360_graph_default_params", None, [C.POINTER(GraphParams)]),
    ("r360_graph_optimize", C.c_int, [_P, C.POINTER(GraphParams), C.POINTER(GraphStats)]),
    ("r360_graph_eval", C.c_int, [_P, _DP, _DP, _DP, C.c_int, _IP]),
    ("r360_graph_solve", C.c_int, [_P, C.POINTER(GraphParams), C.c_double, _DP, C.c_int, _IP, _IP, _DP, _IP]),
    ("r360_g2o_write", C.c_int, [C.c_char_p, C.c_int, _DP, _IP, C.c_int, _IP, _DP, _DP]),
    ("r360_g2o_read", C.c_int, [C.c_char_p, _DP, _IP, C.c_int, _IP, _IP, _DP, _DP, C.c_int, _IP]),
    ("r360_graph_save", C.c_int, [_P, C.c_char_p]),
    ("r360_graph_load", C.c_int, [_P, C.c_char_p]),
    ("r360_rigcal_create", C.c_int, [_P, C.POINTER(_P)]),
    ("r360_rigcal_destroy", None, [_P]),
    ("r360_rigcal_set_pair", C.c_int, [_P, C.c_int, C.c_int, _DP, C.c_int, C.c_int]),
    ("r360_rigcal_get_pair", C.c_int, [_P, C.c_int, C.c_int, _DP, C.c_int, _IP]),
    ("r360_rigcal_clear", C.c_int, [_P]),
    ("r360_rigcal_check", C.c_int, [_P]),
    ("r360_rigcal_load_dir", C.c_int, [_P, C.c_char_p]),
    ("r360_rigcal_save_dir", C.c_int, [_P, C.c_char_p]),
    ("r360_rigcal_read_matrix", C.c_int, [C.c_char_p, _DP, C.c_size_t, _IP, _IP]),
    ("r360_rigcal_write_matrix", C.c_int, [C.c_char_p, _DP, C.c_int, C.c_int]),
    ("r360_rigcal_specs", None, [_DP]),
    ("r360_rigcal_set_init", C.c_int, [_P, _DP]),
    ("r360_rigcal_get_estimate", C.c_int, [_P, _DP]),
    ("r360_rigcal_save_extrinsics", C.c_int, [_P, C.c_char_p]),
    ("r360_rigcal_rotation", C.c_int, [_P, C.c_int, C.POINTER(RigcalStats)]),
    ("r360_rigcal_translation", C.c_int, [_P, C.c_int, C.POINTER(RigcalStats)]),
    ("r360_rigcal_default_trim_params", None, [C.POINTER(RigcalTrimParams)]),
    ("r360_rigcal_trim", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(RigcalTrimParams), C.c_uint,
                                   C.POINTER(RigcalTrimStats), C.c_void_p, C.c_int]),
    ("r360_rigcal_eval", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP, _DP]),
    ("r360_rigcal_default_collect_params", None, [C.POINTER(RigcalCollectParams)]),
    ("r360_rigcal_add_frame", C.c_int, [_P, _P, C.POINTER(RigcalCollectParams), _IP]),
    ("r360_rigcal_conditioning", C.c_int, [_P, _FP]),
    ("r360_frame_get_local_planes", C.c_int, [_P, C.c_int, C.POINTER(Plane), C.c_int, _IP]),
    ("r360_frame_get_local_plane_labels", C.c_int, [_P, C.c_int, C.c_int, _IP, C.c_int, _IP]),
    ("r360_rigcal_ransac_eval", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(RigcalTrimParams), C.c_uint, C.c_int, C.c_int,
                                          _IP, _IP]),
    ("r360_topo_default_params", None, [C.POINTER(TopoParams)]),
    ("r360_topo_bisect", C.c_int, [_P, _FP, C.c_int, _IP, _DP, _DP, _DP, _IP]),
    ("r360_topo_partition", C.c_int, [_P, _FP, C.c_int, C.POINTER(TopoParams), _IP, _IP, _DP, _IP]),
    ("r360_topo_partition_batch", C.c_int, [_P, C.c_int, C.POINTER(_FP), _IP, C.POINTER(TopoParams), C.POINTER(_IP),
                                            _IP]),
    ("r360_topomap_create", C.c_int, [_P, C.POINTER(_P)]),
    ("r360_topomap_destroy", None, [_P]),
    ("r360_topomap_add_keyframe", C.c_int, [_P, _IP]),
    ("r360_topomap_drop_last", C.c_int, [_P]),
    ("r360_topomap_add_connection", C.c_int, [_P, C.c_int, C.c_int, C.c_float]),
    ("r360_topomap_vicinity", C.c_int, [_P, _IP, _FP, C.c_int, _IP]),
    ("r360_topomap_partition", C.c_int, [_P, C.POINTER(TopoParams), _IP]),
    ("r360_topomap_areas", C.c_int, [_P, _IP, C.c_int, _IP, _IP, _IP]),
    ("r360_topomap_neighbors", C.c_int, [_P, C.c_int, _IP, C.c_int, _IP]),
    ("r360_topomap_selected", C.c_int, [_P, C.c_int, _IP]),
    ("r360_relocalize", C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, _P, C.c_size_t, C.c_int, C.c_float, _IP, _DP,
                                  _DP]),
]
ABI_SYMBOLS = [s[0] for s in _SIGS]

_lib = None


def lib() -> C.CDLL:
    """Load librgbd360_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SIGS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().r360_last_error().decode()}")
    return rc


def pcd_write(path: str, xyz: np.ndarray, rgba: np.ndarray | None, width: int, height: int, mode: int = PCD_ASCII):
    """pcl::io::savePCDFile of a PointXYZRGBA cloud (host-only codec)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    assert xyz.shape[0] == width * height
    if rgba is not None:
        rgba = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
        assert rgba.shape[0] == xyz.shape[0]
    _check(lib().r360_pcd_write(path.encode(), _fptr(xyz), None if rgba is None else _vptr(rgba), width, height, mode),
           "pcd_write")


def pcd_read(path: str):
    """PCDReader::read into (xyz [n,3] f32, rgba [n] u32, width, height)."""
    n, w, h = C.c_size_t(), C.c_int(), C.c_int()
    _check(lib().r360_pcd_read(path.encode(), None, None, 0, C.byref(n), C.byref(w), C.byref(h)), "pcd_read")
    xyz = np.zeros((n.value, 3), np.float32)
    rgba = np.zeros(n.value, np.uint32)
    _check(lib().r360_pcd_read(path.encode(), _fptr(xyz), _vptr(rgba), n.value, C.byref(n), C.byref(w), C.byref(h)),
           "pcd_read")
    return xyz, rgba, w.value, h.value


def pcd_write_normals(path: str, xyz, rgba, normals, curvature, mode: int = PCD_ASCII):
    """A PointXYZRGBNormal cloud (x y z rgba normal_x normal_y normal_z curvature), unorganised, in pcd_write's modes."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint32).reshape(-1)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    curvature = np.ascontiguousarray(curvature, np.float32).reshape(-1)
    assert normals.shape[0] == n and curvature.shape[0] == n and (rgba is None or rgba.shape[0] == n)
    _check(lib().r360_pcd_write_normals(path.encode(), _fptr(xyz), None if rgba is None else _vptr(rgba), _fptr(normals),
                                        _fptr(curvature), n, mode), "pcd_write_normals")


def pcd_read_normals(path: str):
    """(xyz [n,3] f32, rgba [n] u32, normals [n,3] f32, curvature [n] f32) of a PCD file that holds the normal fields."""
    n = C.c_size_t()
    _check(lib().r360_pcd_read_normals(path.encode(), None, None, None, None, 0, C.byref(n)), "pcd_read_normals")
    xyz, rgba = np.zeros((n.value, 3), np.float32), np.zeros(n.value, np.uint32)
    nrm, curv = np.zeros((n.value, 3), np.float32), np.zeros(n.value, np.float32)
    _check(lib().r360_pcd_read_normals(path.encode(), _fptr(xyz), _vptr(rgba), _fptr(nrm), _fptr(curv), n.value, C.byref(n)),
           "pcd_read_normals")
    return xyz, rgba, nrm, curv


def write_pcd_labels(path: str, xyz, rgba, labels, mode: int = PCD_ASCII):
    """A PointXYZRGBL cloud (x y z rgba label; -1 is written as 4294967295), unorganised, in pcd_write's modes."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint32).reshape(-1)
    labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
    assert labels.shape[0] == n and (rgba is None or rgba.shape[0] == n)
    _check(lib().r360_pcd_write_labels(path.encode(), _fptr(xyz), None if rgba is None else _vptr(rgba),
                                       labels.ctypes.data_as(_IP), n, mode), "write_pcd_labels")


def read_pcd_labels(path: str):
    """(xyz [n,3] f32, rgba [n] u32, labels [n] i32) of a PCD file that holds a label field."""
    n = C.c_size_t()
    _check(lib().r360_pcd_read_labels(path.encode(), None, None, None, 0, C.byref(n)), "read_pcd_labels")
    xyz, rgba, labels = np.zeros((n.value, 3), np.float32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.int32)
    _check(lib().r360_pcd_read_labels(path.encode(), _fptr(xyz), _vptr(rgba), labels.ctypes.data_as(_IP), n.value,
                                      C.byref(n)), "read_pcd_labels")
    return xyz, rgba, labels


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(_FP)


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_DP)


def _vptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data)


def _mat16(m) -> np.ndarray:
    """4x4 numpy (row-major semantic) -> column-major float[16] (Eigen::Matrix4f::data())."""
    return np.ascontiguousarray(np.asarray(m, dtype=np.float32).T).reshape(16).copy()


def _from16(a: np.ndarray) -> np.ndarray:
    return a.reshape(4, 4).T.copy()


class Context:
    """One HIP device + stream (r360_ctx).  Not thread-safe; use one per host thread."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib().r360_ctx_create(device, C.byref(h)), "r360_ctx_create")
        self.h = h
        self.device = device

    @classmethod
    def _view(cls, h, device: int) -> "Context":
        """A non-owning view of a context the library owns (a sequence runner's pipeline, a dense queue)."""
        c = cls.__new__(cls)
        c.h, c.device = h, device
        c.close = lambda: None
        return c

    def sync(self):
        _check(lib().r360_ctx_sync(self.h), "r360_ctx_sync")

    def persistent_levels(self, enable=True):
        """Lone alignFrames360 as one persistent launch per pyramid level (bit-identical; off by default)."""
        _check(lib().r360_ctx_persistent_levels(self.h, int(enable)), "persistent_levels")

    def latency_mode(self, enable=True):
        """On (the default): PbMap waits assemble the frame themselves, split uploads, graph-replayed lone plane
        stages; off for a context among many pipelines.  Results are identical either way."""
        _check(lib().r360_ctx_latency_mode(self.h, int(enable)), "latency_mode")

    def timing(self, enable):
        """0/False off, 1/True HIP events around every launch, 2 around the level-0 ICP passes only."""
        _check(lib().r360_ctx_timing(self.h, int(enable)), "timing")

    def timing_read(self, kernel: str):
        ms, n = C.c_double(), C.c_long()
        _check(lib().r360_ctx_timing_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)), "timing_read")
        return ms.value, n.value

    def timing_reset(self):
        _check(lib().r360_ctx_timing_reset(self.h), "timing_reset")

    def kernel_time(self, level: int):
        """(summed in-kernel execution span in us, pass count) of the ICP passes at `level`."""
        us, n = C.c_double(), C.c_long()
        _check(lib().r360_ctx_kernel_time(self.h, level, C.byref(us), C.byref(n)), "kernel_time")
        return us.value, n.value

    def kernel_stats(self, level: int):
        """(summed in-kernel span in us, launches, job passes) of the ICP passes at `level`."""
        us, n, j = C.c_double(), C.c_long(), C.c_long()
        _check(lib().r360_ctx_kernel_stats(self.h, level, C.byref(us), C.byref(n), C.byref(j)), "kernel_stats")
        return us.value, n.value, j.value

    def host_times(self, reset: bool = False):
        """Host seconds of this ctx's RegisterPbMap calls: (waiting for the frames' PbMaps, match tables, tree search +
        ConsistencyTest, calls, PbMap assembly of its frames, frames)."""
        out = (C.c_double * 6)()
        _check(lib().r360_ctx_host_times(self.h, out, 1 if reset else 0), "host_times")
        return tuple(out)

    def kernel_time_reset(self):
        _check(lib().r360_ctx_kernel_time_reset(self.h), "kernel_time_reset")

    def match_stats(self):
        """(interpretation-tree searches, searches stopped by the node budget, most nodes of one search) on this ctx."""
        a, b, c = C.c_long(), C.c_long(), C.c_long()
        _check(lib().r360_ctx_match_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "match_stats")
        return a.value, b.value, c.value

    def filter_voxel(self, xyz, rgba=None, leaf: float = 0.05):
        """FilterPointCloud::filterVoxel on this context's GPU (r360_cloud_filter_voxel): one point per occupied voxel
        of size `leaf`, in ascending (k, j, i) voxel order.  Returns (xyz [m,3], rgba [m] or None, ok); ok is False
        when PCL's size guard refuses the leaf, and the cloud then comes back unchanged."""
        xyz, rgba = _cloud_arrays(xyz, rgba)
        n = xyz.shape[0]
        oxyz = np.zeros((n, 3), np.float32)
        orgba = None if rgba is None else np.zeros(n, np.uint32)
        m = C.c_size_t()
        rc = _check(lib().r360_cloud_filter_voxel(self.h, _fptr(xyz), None if rgba is None else _vptr(rgba), n, leaf,
                                                  _fptr(oxyz), None if rgba is None else _vptr(orgba), n, C.byref(m)),
                    "filter_voxel")
        return oxyz[:m.value].copy(), None if rgba is None else orgba[:m.value].copy(), rc == 0

    def map_reset(self):
        """Empties the context's global map."""
        _check(lib().r360_ctx_map_reset(self.h), "map_reset")

    def map_add_cloud(self, xyz, rgba=None, leaf: float = 0.05) -> bool:
        """globalMap += cloud; filterVoxel(globalMap) on the device-resident map.  False: the size guard refused the
        leaf and the map is as it was."""
        xyz, rgba = _cloud_arrays(xyz, rgba)
        return _check(lib().r360_ctx_map_add_cloud(self.h, _fptr(xyz), None if rgba is None else _vptr(rgba),
                                                   xyz.shape[0], leaf), "map_add_cloud") == 0

    def map_add_frame(self, frame, pose, leaf: float = 0.05, box: float = 4.0, x_min: float = -2.0,
                      x_max: float = 1.0) -> bool:
        """The map step on a frame's cloud in HBM (built with BUILD_CLOUD): Euclidean box in the rig frame, `pose`
        (4x4), append, voxel grid."""
        return _check(lib().r360_ctx_map_add_frame(self.h, frame.h, _fptr(_mat16(pose)), x_min, x_max, box, leaf),
                      "map_add_frame") == 0

    def map_size(self) -> int:
        n = C.c_size_t()
        _check(lib().r360_ctx_map_size(self.h, C.byref(n)), "map_size")
        return n.value

    def map_download(self):
        """The map as (xyz [n,3] f32, rgba [n] u32), in ascending voxel order."""
        n = C.c_size_t(self.map_size())
        xyz = np.zeros((n.value, 3), np.float32)
        rgba = np.zeros(n.value, np.uint32)
        _check(lib().r360_ctx_map_download(self.h, _fptr(xyz), _vptr(rgba), n.value, C.byref(n)), "map_download")
        return xyz, rgba

    def filter_outliers(self, xyz, rgba=None, params: "OutlierParams | None" = None):
        """pcl::StatisticalOutlierRemoval / RadiusOutlierRemoval on this context's GPU (r360_cloud_filter_outliers): the
        kept points in input order with their bits.  Returns (xyz [m,3], rgba [m] or None, OutlierStats)."""
        xyz, rgba = _cloud_arrays(xyz, rgba)
        p = params if params is not None else OutlierParams.default()
        n = xyz.shape[0]
        oxyz = np.zeros((n, 3), np.float32)
        orgba = None if rgba is None else np.zeros(n, np.uint32)
        m, st = C.c_size_t(), OutlierStats()
        _check(lib().r360_cloud_filter_outliers(self.h, _fptr(xyz), None if rgba is None else _vptr(rgba), n, C.byref(p),
                                                _fptr(oxyz), None if rgba is None else _vptr(orgba), n, C.byref(m),
                                                C.byref(st)), "filter_outliers")
        return oxyz[:m.value].copy(), None if rgba is None else orgba[:m.value].copy(), st

    def map_filter_outliers(self, params: "OutlierParams | None" = None) -> "OutlierStats":
        """The same filter on the context's global map where it lies in HBM; only the statistics come back."""
        p = params if params is not None else OutlierParams.default()
        st = OutlierStats()
        _check(lib().r360_ctx_map_filter_outliers(self.h, C.byref(p), C.byref(st)), "map_filter_outliers")
        return st

    def outlier_eval(self, xyz, params: "OutlierParams"):
        """Parity hook (r360_cloud_outlier_eval): for a statistical `params` the scores d_i [n] f64 (+inf short, NaN
        dropped row), for a radius one the full neighbour counts c_i [n] i32 (-1 dropped row)."""
        xyz, _ = _cloud_arrays(xyz, None)
        n = xyz.shape[0]
        if params.kind == OUTLIER_STATISTICAL:
            out = np.zeros(n, np.float64)
            _check(lib().r360_cloud_outlier_eval(self.h, _fptr(xyz), n, C.byref(params), _dptr(out), None), "outlier_eval")
        else:
            out = np.zeros(n, np.int32)
            _check(lib().r360_cloud_outlier_eval(self.h, _fptr(xyz), n, C.byref(params), None, out.ctypes.data_as(_IP)),
                   "outlier_eval")
        return out

    @staticmethod
    def _viewpoints(viewpoints) -> np.ndarray:
        return np.ascontiguousarray(viewpoints, np.float32).reshape(-1, 3)

    def estimate_normals(self, xyz, viewpoints=(0.0, 0.0, 0.0), params: "NormalParams | None" = None):
        """pcl::NormalEstimation on this context's GPU (r360_cloud_normals): per point the unit normal of its at most k
        nearest points within the radius, turned towards the nearest of `viewpoints` ([v,3] or one point), and the
        curvature; NaN for dropped and short rows.  Returns (normals [n,3] f32, curvature [n] f32, NormalStats)."""
        xyz, _ = _cloud_arrays(xyz, None)
        p = params if params is not None else NormalParams.default()
        v = self._viewpoints(viewpoints)
        n = xyz.shape[0]
        nrm, curv, st = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), NormalStats()
        _check(lib().r360_cloud_normals(self.h, _fptr(xyz), n, C.byref(p), _fptr(v), v.shape[0], _fptr(nrm), _fptr(curv),
                                        C.byref(st)), "estimate_normals")
        return nrm, curv, st

    def map_estimate_normals(self, viewpoints=(0.0, 0.0, 0.0), params: "NormalParams | None" = None) -> "NormalStats":
        """The same on the context's global map where it lies; the normals stay in HBM, valid until the map changes."""
        p = params if params is not None else NormalParams.default()
        v = self._viewpoints(viewpoints)
        st = NormalStats()
        _check(lib().r360_ctx_map_estimate_normals(self.h, C.byref(p), _fptr(v), v.shape[0], C.byref(st)),
               "map_estimate_normals")
        return st

    def map_normals(self):
        """The map's normals and curvature (normals [n,3] f32, curvature [n] f32) in the map's order; raises when the
        map changed since they were estimated."""
        n = C.c_size_t()
        _check(lib().r360_ctx_map_download_normals(self.h, None, None, 0, C.byref(n)), "map_normals")
        nrm, curv = np.zeros((n.value, 3), np.float32), np.zeros(n.value, np.float32)
        _check(lib().r360_ctx_map_download_normals(self.h, _fptr(nrm), _fptr(curv), n.value, C.byref(n)), "map_normals")
        return nrm, curv

    def normals_eval(self, xyz, viewpoints, params: "NormalParams"):
        """Parity hook (r360_cloud_normals_eval): (knn [n,k] i32, count [n] i32, normal [n,3] f64, eig [n,3] f64,
        curvature [n] f64)."""
        xyz, _ = _cloud_arrays(xyz, None)
        v = self._viewpoints(viewpoints)
        n = xyz.shape[0]
        knn, count = np.full((n, params.k), -1, np.int32), np.full(n, -1, np.int32)
        nrm, eig, curv = np.full((n, 3), np.nan), np.full((n, 3), np.nan), np.full(n, np.nan)
        _check(lib().r360_cloud_normals_eval(self.h, _fptr(xyz), n, C.byref(params), _fptr(v), v.shape[0],
                                             knn.ctypes.data_as(_IP), count.ctypes.data_as(_IP), _dptr(nrm), _dptr(eig),
                                             _dptr(curv)), "normals_eval")
        return knn, count, nrm, eig, curv

    def _clusters(self, xyz, prm, normals, hook):
        xyz, _ = _cloud_arrays(xyz, None)
        p = prm if prm is not None else ClusterParams.default()
        n = xyz.shape[0]
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert nrm is None or nrm.shape[0] == n
        labels, st, nk = np.full(n, -1, np.int32), ClusterStats(), C.c_size_t()
        root, comp = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        cap = n // max(int(p.min_size), 1) + 1     # no more clusters than that
        info = np.zeros(cap, CLUSTER_INFO_DTYPE)
        args = [self.h, _fptr(xyz), None if nrm is None else _fptr(nrm), n, C.byref(p), labels.ctypes.data_as(_IP),
                _vptr(info), cap, C.byref(nk), C.byref(st)]
        if hook:
            _check(lib().r360_cloud_clusters_eval(*args, root.ctypes.data_as(_IP), comp.ctypes.data_as(_IP)), "clusters_eval")
            return labels, info[:nk.value].copy(), st, root, comp
        _check(lib().r360_cloud_clusters(*args), "clusters")
        return labels, info[:nk.value].copy(), st

    def clusters(self, xyz, prm: "ClusterParams | None" = None, normals=None):
        """pcl::EuclideanClusterExtraction on this context's GPU (r360_cloud_clusters): the connected components of
        "closer than the tolerance" within the size bounds, largest first; with `normals` [n,3] the normal-aware form
        (an edge also needs an angle of at most eps_angle between the two normals).  Returns (labels [n] i32, -1 = in no
        cluster; info, a CLUSTER_INFO_DTYPE array with one record per cluster; ClusterStats)."""
        return self._clusters(xyz, prm, normals, False)

    def clusters_eval(self, xyz, prm: "ClusterParams | None" = None, normals=None):
        """Parity hook (r360_cloud_clusters_eval): clusters()'s three, then root [n] i32 (the smallest index of the row's
        component, -1 dropped) and comp_size [n] i32 (its size before the size bounds)."""
        return self._clusters(xyz, prm, normals, True)

    def map_cluster(self, prm: "ClusterParams | None" = None, use_normals: bool = False) -> "ClusterStats":
        """The same on the context's global map where it lies; labels and records stay in HBM, valid until the map
        changes.  use_normals: the normal-aware form on the map's normals (map_estimate_normals first)."""
        p = prm if prm is not None else ClusterParams.default()
        st = ClusterStats()
        _check(lib().r360_ctx_map_cluster(self.h, C.byref(p), int(use_normals), C.byref(st)), "map_cluster")
        return st

    def map_labels(self) -> np.ndarray:
        """The map's labels [n] i32 in the map's order; raises when the map changed since map_cluster."""
        n = C.c_size_t()
        _check(lib().r360_ctx_map_download_labels(self.h, None, 0, C.byref(n)), "map_labels")
        labels = np.full(n.value, -1, np.int32)
        _check(lib().r360_ctx_map_download_labels(self.h, labels.ctypes.data_as(_IP), n.value, C.byref(n)), "map_labels")
        return labels

    def map_clusters(self) -> np.ndarray:
        """The map's cluster records (CLUSTER_INFO_DTYPE); raises when the map changed since map_cluster."""
        n = C.c_size_t()
        _check(lib().r360_ctx_map_cluster_info(self.h, None, 0, C.byref(n)), "map_clusters")
        info = np.zeros(n.value, CLUSTER_INFO_DTYPE)
        _check(lib().r360_ctx_map_cluster_info(self.h, _vptr(info), n.value, C.byref(n)), "map_clusters")
        return info

    def map_filter_clusters(self, prm: "ClusterParams | None" = None, use_normals: bool = False) -> "ClusterStats":
        """Clusters the map and keeps exactly the points of the kept clusters, where the map lies in HBM."""
        p = prm if prm is not None else ClusterParams.default()
        st = ClusterStats()
        _check(lib().r360_ctx_map_filter_clusters(self.h, C.byref(p), int(use_normals), C.byref(st)), "map_filter_clusters")
        return st

    def sac_planes(self, xyz, prm: "SacParams | None" = None, normals=None):
        """pcl::SACSegmentation's RANSAC plane search on this context's GPU, peeled plane after plane
        (r360_cloud_sac_planes); with `normals` [n,3] an inlier's normal must also lie within normal_angle of the
        plane's.  Returns (labels [n] i32, the plane's extraction order or -1; planes, a SAC_PLANE_DTYPE array;
        SacStats)."""
        xyz, _ = _cloud_arrays(xyz, None)
        p = prm if prm is not None else SacParams.default()
        n = xyz.shape[0]
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert nrm is None or nrm.shape[0] == n
        labels, st, np_ = np.full(n, -1, np.int32), SacStats(), C.c_size_t()
        info = np.zeros(SAC_MAX_PLANES, SAC_PLANE_DTYPE)
        _check(lib().r360_cloud_sac_planes(self.h, _fptr(xyz), None if nrm is None else _fptr(nrm), n, C.byref(p),
                                           labels.ctypes.data_as(_IP), _vptr(info), SAC_MAX_PLANES, C.byref(np_),
                                           C.byref(st)), "sac_planes")
        return labels, info[:np_.value].copy(), st

    def sac_eval(self, xyz, prm: "SacParams | None" = None, normals=None, n_hyp: int = SAC_ROUND, coef_in=None):
        """Parity hook (r360_cloud_sac_eval) of plane 0 over the whole finite cloud: (samples [n_hyp,3] i32, coef
        [n_hyp,4] f64, count [n_hyp] i32).  With coef_in [n_hyp,4] those coefficients are scored as they are."""
        xyz, _ = _cloud_arrays(xyz, None)
        p = prm if prm is not None else SacParams.default()
        n = xyz.shape[0]
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert nrm is None or nrm.shape[0] == n
        cin = None
        if coef_in is not None:
            cin = np.ascontiguousarray(coef_in, np.float64).reshape(-1, 4)
            n_hyp = cin.shape[0]
        samples = np.full((n_hyp, 3), -1, np.int32)
        coef, count = np.full((n_hyp, 4), np.nan), np.zeros(n_hyp, np.int32)
        _check(lib().r360_cloud_sac_eval(self.h, _fptr(xyz), None if nrm is None else _fptr(nrm), n, C.byref(p),
                                         None if cin is None else _dptr(cin), n_hyp, samples.ctypes.data_as(_IP),
                                         _dptr(coef), count.ctypes.data_as(_IP)), "sac_eval")
        return samples, coef, count

    def map_sac_planes(self, prm: "SacParams | None" = None, use_normals: bool = False) -> "SacStats":
        """The same on the context's global map where it lies; plane labels and records stay in HBM, valid until the
        map changes.  use_normals: the gate on the map's normals (map_estimate_normals first)."""
        p = prm if prm is not None else SacParams.default()
        st = SacStats()
        _check(lib().r360_ctx_map_sac_planes(self.h, C.byref(p), int(use_normals), C.byref(st)), "map_sac_planes")
        return st

    def map_plane_labels(self) -> np.ndarray:
        """The map's plane labels [n] i32 in the map's order; raises when the map changed since map_sac_planes."""
        n = C.c_size_t()
        _check(lib().r360_ctx_map_download_plane_labels(self.h, None, 0, C.byref(n)), "map_plane_labels")
        labels = np.full(n.value, -1, np.int32)
        _check(lib().r360_ctx_map_download_plane_labels(self.h, labels.ctypes.data_as(_IP), n.value, C.byref(n)),
               "map_plane_labels")
        return labels

    def map_planes(self) -> np.ndarray:
        """The map's plane records (SAC_PLANE_DTYPE); raises when the map changed since map_sac_planes."""
        n = C.c_size_t()
        _check(lib().r360_ctx_map_plane_info(self.h, None, 0, C.byref(n)), "map_planes")
        info = np.zeros(n.value, SAC_PLANE_DTYPE)
        _check(lib().r360_ctx_map_plane_info(self.h, _vptr(info), n.value, C.byref(n)), "map_planes")
        return info

    def map_filter_planes(self, prm: "SacParams | None" = None, use_normals: bool = False,
                          keep_planes: bool = False) -> "SacStats":
        """Segments the map and drops the plane points (keep_planes: keeps only them), where the map lies in HBM."""
        p = prm if prm is not None else SacParams.default()
        st = SacStats()
        _check(lib().r360_ctx_map_filter_planes(self.h, C.byref(p), int(use_normals), int(keep_planes), C.byref(st)),
               "map_filter_planes")
        return st

    def _gicp_set(self, fn, xyz, params, what):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        p = params if params is not None else GicpParams.default()
        _check(fn(self.h, _fptr(xyz), xyz.shape[0], C.byref(p)), what)

    def gicp_set_source(self, xyz, params: "GicpParams | None" = None):
        """The Generalized-ICP source cloud ([n,3] float32): non-finite rows dropped, grid index, kNN covariances."""
        self._gicp_set(lib().r360_gicp_set_source, xyz, params, "gicp_set_source")

    def gicp_set_target(self, xyz, params: "GicpParams | None" = None):
        """The Generalized-ICP target cloud (as gicp_set_source)."""
        self._gicp_set(lib().r360_gicp_set_target, xyz, params, "gicp_set_target")

    def gicp_align(self, init=None, params: "GicpParams | None" = None):
        """r360_gicp_align from `init` (4x4, source into target).  Returns (pose 4x4 float32, GicpStats, status);
        status 1: ill-posed (no pair inside the gate or a singular system), the pose is the one reached so far."""
        p = params if params is not None else GicpParams.default()
        out = np.zeros(16, np.float32)
        st = GicpStats()
        rc = _check(lib().r360_gicp_align(self.h, _fptr(_mat16(np.eye(4) if init is None else init)), C.byref(p),
                                          _fptr(out), C.byref(st)), "gicp_align")
        return _from16(out), st, rc

    def gicp_eval(self, pose, params: "GicpParams | None" = None):
        """One correspondence pass and one inner pass at `pose` (r360_gicp_eval): (corr [n] int32 with -1 for none,
        cost f, H [6,6], g [6], n_corr), the sums in double."""
        p = params if params is not None else GicpParams.default()
        n = C.c_size_t()
        _check(lib().r360_gicp_get_cloud(self.h, 0, None, None, None, 0, C.byref(n)), "gicp_get_cloud")
        corr = np.zeros(n.value, np.int32)
        cost, nc = C.c_double(), C.c_size_t()
        H, g = np.zeros(36, np.float64), np.zeros(6, np.float64)
        _check(lib().r360_gicp_eval(self.h, _fptr(_mat16(pose)), C.byref(p), corr.ctypes.data_as(_IP), C.byref(cost),
                                    _dptr(H), _dptr(g), C.byref(nc)), "gicp_eval")
        return corr, cost.value, H.reshape(6, 6), g, nc.value

    def gicp_cloud(self, which: int, k: int = 20):
        """The kept points of the source (0) or target (1) cloud, their covariances' upper triangles [n,6] float32
        and the kNN index lists [n,k] (k: the k_correspondences the cloud was set with)."""
        n = C.c_size_t()
        _check(lib().r360_gicp_get_cloud(self.h, which, None, None, None, 0, C.byref(n)), "gicp_get_cloud")
        xyz = np.zeros((n.value, 3), np.float32)
        cov = np.zeros((n.value, 6), np.float32)
        knn = np.zeros((n.value, k), np.int32)
        _check(lib().r360_gicp_get_cloud(self.h, which, _fptr(xyz), _fptr(cov), knn.ctypes.data_as(_IP), n.value,
                                         C.byref(n)), "gicp_get_cloud")
        return xyz, cov, knn

    def close(self):
        if self.h:
            lib().r360_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Calib360:
    """Calib360 (include/Calib360.h:44-132): Rt_[8], Rt_inv[8], cameraMatrix, CLAMS models."""

    def __init__(self, ctx: Context, rows: int = 240, cols: int = 320, _sphere: tuple | None = None):
        h = C.c_void_p()
        if _sphere is None:
            _check(lib().r360_calib_create(ctx.h, rows, cols, C.byref(h)), "r360_calib_create")
        else:
            _check(lib().r360_calib_create_sphere(ctx.h, _sphere[0], _sphere[1], C.byref(h)), "r360_calib_create_sphere")
            rows = cols = 0
        self.h, self.ctx, self.rows, self.cols = h, ctx, rows, cols

    @classmethod
    def _view(cls, h, ctx: Context, rows: int, cols: int) -> "Calib360":
        """A non-owning view of a calibration the library owns."""
        c = cls.__new__(cls)
        c.h, c.ctx, c.rows, c.cols = h, ctx, rows, cols
        c.close = lambda: None
        return c

    @classmethod
    def for_sphere(cls, ctx: Context, sph_rows: int, sph_cols: int) -> "Calib360":
        """A calibration without sensors for spheres given as images (setSourceFrame / setTargetFrame(cv::Mat&,
        cv::Mat&), RegisterPhotoICP.h:480-516)."""
        return cls(ctx, _sphere=(sph_rows, sph_cols))

    def loadExtrinsicCalibration(self, path: str):
        _check(lib().r360_calib_load_extrinsics(self.h, path.encode()), "loadExtrinsicCalibration")

    def loadIntrinsicCalibration(self, path: str):
        _check(lib().r360_calib_load_intrinsics(self.h, path.encode()), "loadIntrinsicCalibration")

    def setRt(self, rt8: np.ndarray):
        """rt8: (8,4,4) rig extrinsics (row-major numpy)."""
        a = np.concatenate([_mat16(m) for m in rt8]).astype(np.float32)
        _check(lib().r360_calib_set_extrinsics(self.h, _fptr(a)), "setRt")

    def extrinsics(self):
        rt = np.zeros(128, np.float32)
        rti = np.zeros(128, np.float32)
        K = np.zeros(9, np.float32)
        _check(lib().r360_calib_get_extrinsics(self.h, _fptr(rt), _fptr(rti), _fptr(K)), "get_extrinsics")
        return rt, rti, K  # column-major blocks, as the C-ABI stores them

    def synth_frame(self, seed: int, rig_pose: np.ndarray):
        """Render a synthetic 8-camera frame of the procedural room (seed) at rig_pose (4x4)."""
        bgr = np.zeros((8, self.rows, self.cols, 3), np.uint8)
        dep = np.zeros((8, self.rows, self.cols), np.uint16)
        p = _mat16(rig_pose)
        _check(lib().r360_synth_frame(self.h, seed, _fptr(p), _vptr(bgr), _vptr(dep)), "synth_frame")
        return bgr, dep

    def close(self):
        if self.h:
            lib().r360_calib_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame360:
    """Frame360 (include/Frame360.h:93-1150) with device-resident images and sphere pyramid."""

    def __init__(self, calib: Calib360):
        h = C.c_void_p()
        _check(lib().r360_frame_create(calib.ctx.h, calib.h, C.byref(h)), "r360_frame_create")
        self.h, self.calib = h, calib
        r, c, sr, sc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib().r360_frame_dims(h, C.byref(r), C.byref(c), C.byref(sr), C.byref(sc))
        self.rows, self.cols, self.sph_rows, self.sph_cols = r.value, c.value, sr.value, sc.value

    @classmethod
    def _view(cls, h, calib: Calib360) -> "Frame360":
        """A non-owning view of a frame the library owns (a sequence runner's ring buffer)."""
        f = cls.__new__(cls)
        f.h, f.calib = h, calib
        r, c, sr, sc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib().r360_frame_dims(h, C.byref(r), C.byref(c), C.byref(sr), C.byref(sc))
        f.rows, f.cols, f.sph_rows, f.sph_cols = r.value, c.value, sr.value, sc.value
        f.close = lambda: None
        return f

    def setNumPyr(self, n: int):
        """r360_frame_set_levels: the frame's pyramid stops at n levels (RegisterPhotoICP::setNumPyr)."""
        _check(lib().r360_frame_set_levels(self.h, int(n)), "r360_frame_set_levels")

    def setCompaction(self, all_levels: bool):
        """r360_frame_set_compaction: compact every level's source points at the next build (default), or only the
        levels a batched pass cannot stream as an image."""
        _check(lib().r360_frame_set_compaction(self.h, int(bool(all_levels))), "r360_frame_set_compaction")

    def loadFrame(self, path: str):
        _check(lib().r360_frame_load_bin(self.h, path.encode()), "loadFrame")

    def serialize(self, fileName: str):
        """Frame360::serialize (Frame360.h:332-345): the raw images + timestamp as a .bin archive."""
        _check(lib().r360_frame_save_bin(self.h, fileName.encode()), "serialize")

    def setTimeStamp(self, timestamp: int):
        _check(lib().r360_frame_set_timestamp(self.h, int(timestamp)), "setTimeStamp")

    @property
    def timeStamp(self) -> int:
        t = C.c_uint64()
        _check(lib().r360_frame_get_timestamp(self.h, C.byref(t)), "timeStamp")
        return t.value

    def sphereCloud(self):
        """Frame360::sphereCloud: (xyz [n,3] f32, rgba [n] u32, width, height)."""
        w, h = C.c_int(), C.c_int()
        _check(lib().r360_frame_get_sphere_cloud(self.h, None, None, 0, C.byref(w), C.byref(h)), "sphereCloud")
        n = w.value * h.value
        xyz = np.zeros((n, 3), np.float32)
        rgba = np.zeros(n, np.uint32)
        _check(lib().r360_frame_get_sphere_cloud(self.h, _fptr(xyz), _vptr(rgba), n, C.byref(w), C.byref(h)),
               "sphereCloud")
        return xyz, rgba, w.value, h.value

    def loadCloud(self, pointCloudPath: str):
        _check(lib().r360_frame_load_cloud(self.h, pointCloudPath.encode()), "loadCloud")

    def loadPbMap(self, pbmapPath: str):
        _check(lib().r360_frame_load_pbmap(self.h, pbmapPath.encode()), "loadPbMap")

    def load_PbMap_Cloud(self, path: str, index_or_pbmap):
        """load_PbMap_Cloud(cloudPath, pbmapPath) or load_PbMap_Cloud(dir, index) (Frame360.h:212-228)."""
        if isinstance(index_or_pbmap, str):
            self.loadCloud(path)
            self.loadPbMap(index_or_pbmap)
        else:
            _check(lib().r360_frame_load_pbmap_cloud(self.h, path.encode(), int(index_or_pbmap)), "load_PbMap_Cloud")

    def savePlanes(self, pathPbMap: str):
        _check(lib().r360_frame_save_planes(self.h, pathPbMap.encode()), "savePlanes")

    def saveCloud(self, path: str, mode: int = PCD_ASCII):
        _check(lib().r360_frame_save_cloud(self.h, path.encode(), mode), "saveCloud")

    def save(self, path: str, frame: int):
        """Frame360::save (Frame360.h:320-330): path/sphereCloud_<frame>.pcd + path/spherePlanes_<frame>.pbmap."""
        _check(lib().r360_frame_save(self.h, path.encode(), int(frame)), "save")

    def setPlaneLabel(self, i: int, label: str):
        _check(lib().r360_frame_set_plane_label(self.h, i, label.encode()), "setPlaneLabel")

    def planeLabel(self, i: int) -> str:
        n = lib().r360_frame_get_plane_label(self.h, i, None, 0)
        _check(min(n, 0), "planeLabel")
        buf = C.create_string_buffer(n + 1)
        lib().r360_frame_get_plane_label(self.h, i, buf, n + 1)
        return buf.value.decode()

    def upload(self, bgr8: np.ndarray, depth8: np.ndarray):
        bgr8 = np.ascontiguousarray(bgr8, np.uint8)
        depth8 = np.ascontiguousarray(depth8, np.uint16)
        assert bgr8.shape == (8, self.rows, self.cols, 3) and depth8.shape == (8, self.rows, self.cols)
        _check(lib().r360_frame_upload(self.h, _vptr(bgr8), _vptr(depth8)), "upload")

    def set_sphere(self, bgr: np.ndarray, range_mm: np.ndarray):
        """The sphere as images (BGR u8 [H, W, 3], range u16 mm [H, W]; sphereRGB / sphereDepth) replaces the
        frame's; its ICP pyramid is rebuilt (setSourceFrame / setTargetFrame(cv::Mat&, cv::Mat&))."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        range_mm = np.ascontiguousarray(range_mm, np.uint16)
        H, W = range_mm.shape
        assert bgr.shape == (H, W, 3)
        _check(lib().r360_frame_set_sphere(self.h, _vptr(bgr), _vptr(range_mm), H, W), "set_sphere")

    def upload_async(self, bgr8: np.ndarray, depth8: np.ndarray):
        """Enqueue the upload on the frame's stream; the arrays must stay alive (and should be page-locked,
        see HostPinned) until the stream has consumed them."""
        assert bgr8.dtype == np.uint8 and depth8.dtype == np.uint16
        assert bgr8.flags.c_contiguous and depth8.flags.c_contiguous
        assert bgr8.shape == (8, self.rows, self.cols, 3) and depth8.shape == (8, self.rows, self.cols)
        _check(lib().r360_frame_upload_async(self.h, _vptr(bgr8), _vptr(depth8)), "upload_async")

    def upload_device(self, d_bgr: int, d_depth: int):
        _check(lib().r360_frame_upload_device(self.h, C.c_void_p(d_bgr), C.c_void_p(d_depth)), "upload_device")

    def build(self, flags: int = BUILD_UNDISTORT | BUILD_SPHERE | BUILD_PYRAMID, sync: bool = True):
        fn = lib().r360_frame_build if sync else lib().r360_frame_build_async
        _check(fn(self.h, flags), "r360_frame_build")

    def built(self) -> int:
        """r360_frame_built: the BUILD_* stages done, and BUILT_LEVEL0."""
        u = C.c_uint()
        _check(lib().r360_frame_built(self.h, C.byref(u)), "r360_frame_built")
        return u.value

    def undistort(self):
        self.build(BUILD_UNDISTORT)

    def stitchSphericalImage(self):
        self.build(BUILD_SPHERE | BUILD_PYRAMID)

    def buildSphereCloud(self):
        self.build(BUILD_UNDISTORT | BUILD_CLOUD)

    def getPlanes(self):
        """Frame360::getPlanes (Frame360.h:615-640): builds the PbMap; returns the plane list."""
        self.build(BUILD_UNDISTORT | BUILD_PLANES)
        return self.planes()

    def planes(self) -> list[dict]:
        n = C.c_int()
        _check(lib().r360_frame_get_planes(self.h, None, 0, C.byref(n)), "get_planes")
        arr = (Plane * max(n.value, 1))()
        _check(lib().r360_frame_get_planes(self.h, arr, n.value, C.byref(n)), "get_planes")
        out = []
        for i, p in enumerate(arr[:n.value]):
            hull = np.zeros((max(p.n_hull, 1), 3), np.float32)
            m = C.c_int()
            _check(lib().r360_frame_get_plane_hull(self.h, i, _fptr(hull), p.n_hull, C.byref(m)), "get_plane_hull")
            out.append(dict(normal=np.array(p.normal[:]), center=np.array(p.center[:]), d=p.d, area=p.area,
                            elongation=p.elongation, curvature=p.curvature, ppal=np.array(p.ppal[:]),
                            nrgb=np.array(p.nrgb[:]), intensity=p.intensity, id=p.id, sensor=p.sensor,
                            n_inliers=p.n_inliers, hull=hull[:p.n_hull].copy()))
        return out

    def cloud(self):
        """Per-sensor organized clouds after downsample + bilateral filter, normals and distance map."""
        h, w = self.rows // 2, self.cols // 2
        xyz = np.zeros((8, h, w, 4), np.float32)
        rgb = np.zeros((8, h, w, 4), np.uint8)
        nrm = np.zeros((8, h, w, 4), np.float32)
        dist = np.zeros((8, h, w), np.float32)
        _check(lib().r360_frame_get_cloud(self.h, _fptr(xyz), _vptr(rgb), _fptr(nrm), _fptr(dist)), "get_cloud")
        return xyz, rgb, nrm, dist

    def localPlanes(self, sensor: int) -> list[dict]:
        """r360_frame_get_local_planes (a build with BUILD_PLANES | BUILD_LOCAL_PLANES): the sensor's planes before
        groupPlanes, in the sensor's frame, each with the region labels merged into it."""
        n = C.c_int()
        _check(lib().r360_frame_get_local_planes(self.h, sensor, None, 0, C.byref(n)), "get_local_planes")
        arr = (Plane * max(n.value, 1))()
        _check(lib().r360_frame_get_local_planes(self.h, sensor, arr, n.value, C.byref(n)), "get_local_planes")
        out = []
        for i, p in enumerate(arr[:n.value]):
            m = C.c_int()
            _check(lib().r360_frame_get_local_plane_labels(self.h, sensor, i, None, 0, C.byref(m)), "get_local_plane_labels")
            lab = np.zeros(max(m.value, 1), np.int32)
            _check(lib().r360_frame_get_local_plane_labels(self.h, sensor, i, lab.ctypes.data_as(_IP), m.value, C.byref(m)),
                   "get_local_plane_labels")
            out.append(dict(normal=np.array(p.normal[:], np.float32), center=np.array(p.center[:], np.float32), d=np.float32(p.d),
                            elongation=p.elongation, n_inliers=p.n_inliers, labels=lab[:m.value].copy()))
        return out

    def labels(self):
        h, w = self.rows // 2, self.cols // 2
        lab = np.zeros((8, h, w), np.int32)
        labf = np.zeros((8, h, w), np.int32)
        _check(lib().r360_frame_get_labels(self.h, lab.ctypes.data_as(_IP), labf.ctypes.data_as(_IP)), "get_labels")
        return lab, labf

    def regions(self, sensor: int) -> list[dict]:
        n = C.c_int()
        arr = (Region * 64)()
        _check(lib().r360_frame_get_regions(self.h, sensor, arr, 64, C.byref(n)), "get_regions")
        return [dict(label=r.label, count=r.count, start_idx=r.start_idx, n_contour=r.n_contour, n_fit=r.n_fit,
                     centroid=np.array(r.centroid[:]), cov=np.array(r.cov[:]).reshape(3, 3),
                     model=np.array(r.model[:]), curvature=r.curvature) for r in arr[:n.value]]

    def segment_eval(self, xyz4: np.ndarray, nrm: np.ndarray, rgb4: np.ndarray) -> int:
        """Parity hook (r360_frame_segment_eval): the frame's segmentation stage on given points [8, h, w, 4], unit
        normals [8, h, w, 3 or 4] and colours [8, h, w, 4] (h = rows / 2, w = cols / 2).  Returns 0; a capacity
        error raises RuntimeError with the stage's error bits in its `code` attribute.  labels(), regions(k) and
        region_detail(k, m) show the result; the frame's images are overwritten and its PbMap is empty."""
        h, w = self.rows // 2, self.cols // 2
        xyz4 = np.ascontiguousarray(xyz4, np.float32)
        nrm = np.ascontiguousarray(nrm, np.float32)
        rgb4 = np.ascontiguousarray(rgb4, np.uint8)
        if xyz4.shape != (8, h, w, 4) or nrm.shape[:3] != (8, h, w) or nrm.shape[3] not in (3, 4) or \
                rgb4.shape != (8, h, w, 4):
            raise ValueError(f"segment_eval: fields of 8 x {h} x {w} expected")
        code = C.c_int(0)
        rc = lib().r360_frame_segment_eval(self.h, _fptr(xyz4), _fptr(nrm), nrm.shape[3], _vptr(rgb4), C.byref(code))
        if rc < 0:
            e = RuntimeError(f"segment_eval failed ({rc}): {lib().r360_last_error().decode()}")
            e.code = code.value
            raise e
        return rc

    def refine_states(self):
        """Parity hook (r360_frame_get_refine_states): the refinement's states int8 [8, h, w] after its sweeps (-1 no
        label, -2 non-planar label, m >= 0 model m) and the wavefront sweeps' 24 flag words ([s]: the single-wave
        fallback redid sensor s, [8 + s]: re-runs of its second sweep, [16 + s]: its first sweep gave up)."""
        state = np.zeros((8, self.rows // 2, self.cols // 2), np.int8)
        flags = np.zeros(24, np.int32)
        _check(lib().r360_frame_get_refine_states(self.h, state.ctypes.data, flags.ctypes.data_as(_IP)),
               "get_refine_states")
        return state, flags

    def region_detail(self, sensor: int, region: int) -> dict:
        """Region `region` of `sensor` before the hull prefilter and the host assembly: the exact moments of its final
        inliers (Python integers: n, s1[3], s2[6] = xx xy xz yy yz zz, c[4]), its local-frame bounds and its traced
        contour's points [n_contour, 4] in trace order (none for a region that takes the voxel fallback)."""
        st = (C.c_int64 * 20)()
        bounds = np.zeros(6, np.float32)
        n = C.c_int()
        _check(lib().r360_frame_get_region_detail(self.h, sensor, region, st, _fptr(bounds), None, 0, C.byref(n)),
               "get_region_detail")
        contour = np.zeros((max(n.value, 1), 4), np.float32)
        if n.value:
            _check(lib().r360_frame_get_region_detail(self.h, sensor, region, None, None, _fptr(contour), n.value,
                                                      C.byref(n)), "get_region_detail")
        s2 = []
        for k in range(6):
            v = (int(st[4 + 2 * k]) & 0xFFFFFFFFFFFFFFFF) | ((int(st[5 + 2 * k]) & 0xFFFFFFFFFFFFFFFF) << 64)
            s2.append(v - (1 << 128) if v >> 127 else v)
        return dict(n=int(st[0]), s1=[int(st[1 + k]) for k in range(3)], s2=s2, c=[int(st[16 + k]) for k in range(4)],
                    bmin=bounds[:3].copy(), bmax=bounds[3:].copy(), contour=contour[:n.value].copy())

    def sphere(self):
        bgr = np.zeros((self.sph_rows, self.sph_cols, 3), np.uint8)
        dep = np.zeros((self.sph_rows, self.sph_cols), np.uint16)
        _check(lib().r360_frame_get_sphere(self.h, _vptr(bgr), _vptr(dep)), "get_sphere")
        return bgr, dep

    def depth_m(self):
        d = np.zeros((8, self.rows, self.cols), np.float32)
        _check(lib().r360_frame_get_depth_m(self.h, _vptr(d)), "get_depth_m")
        return d

    def level(self, level: int):
        r, c = C.c_int(), C.c_int()
        _check(lib().r360_frame_get_level(self.h, level, C.byref(r), C.byref(c), None, None, None, None, None,
                                          None), "get_level")
        arrs = [np.zeros((r.value, c.value), np.float32) for _ in range(6)]
        _check(lib().r360_frame_get_level(self.h, level, C.byref(r), C.byref(c), *[_vptr(a) for a in arrs]),
               "get_level")
        return dict(zip(["gray", "depth", "gx", "gy", "dgx", "dgy"], arrs))

    def saliency(self):
        """Level 0's saliency flags (bit 0: intensity gradient, bit 1: depth gradient) as a (sph_rows, sph_cols) uint8
        array, and the (intensity, depth) thresholds they were built for (NaN: the frame has none)."""
        fl = np.zeros((self.sph_rows, self.sph_cols), np.uint8)
        ti, td = C.c_float(), C.c_float()
        _check(lib().r360_frame_get_saliency(self.h, _vptr(fl), C.byref(ti), C.byref(td)), "get_saliency")
        return fl, (ti.value, td.value)

    def points(self, level: int) -> np.ndarray:
        """The level's compacted ICP source points: (n, 4) {x, y, z, gray} (valid depth, raster order)."""
        n = C.c_int()
        _check(lib().r360_frame_get_points(self.h, level, None, 0, C.byref(n)), "get_points")
        out = np.zeros((max(n.value, 1), 4), np.float32)
        _check(lib().r360_frame_get_points(self.h, level, _fptr(out), n.value, C.byref(n)), "get_points")
        return out[:n.value]

    def sensor_level(self, sensor: int, level: int):
        """Sensor k's pinhole pyramid level (BUILD_SENSOR_PYRAMID)."""
        r, c = C.c_int(), C.c_int()
        _check(lib().r360_frame_get_sensor_level(self.h, sensor, level, C.byref(r), C.byref(c), None, None, None,
                                                 None, None, None), "get_sensor_level")
        arrs = [np.zeros((r.value, c.value), np.float32) for _ in range(6)]
        _check(lib().r360_frame_get_sensor_level(self.h, sensor, level, C.byref(r), C.byref(c),
                                                 *[_vptr(a) for a in arrs]), "get_sensor_level")
        return dict(zip(["gray", "depth", "gx", "gy", "dgx", "dgy"], arrs))

    def close(self):
        if self.h:
            lib().r360_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegisterRGBD360:
    """RegisterRGBD360 (include/RegisterRGBD360.h:47-340): PbMap registration of two Frame360."""

    def __init__(self, ctx: "Context", config_file: str | None = None):
        # RegisterRGBD360(configFile): matcher.configLocaliser.load_params(configFile) (:97-100); without a
        # file, the configLocaliser_sphericalOdometry.ini values
        self.ctx = ctx
        self.config_file = config_file
        self.match = MatchParams.load_ini(config_file) if config_file else MatchParams.default()
        self.rigidTransf = np.eye(4, dtype=np.float32)
        self.informationM = np.zeros((6, 6), np.float32)
        self.bestMatch: dict[int, int] = {}
        self.areaMatched = self.areaSource = self.areaTarget = 0.0
        self.ref = self.trg = None
        self.max_match_planes = 0

    def setReference(self, ref: "Frame360", max_match_planes: int = 0):
        self.ref, self.max_match_planes = ref, max_match_planes

    def setTarget(self, trg: "Frame360", max_match_planes: int = 0):
        self.trg, self.max_match_planes = trg, max_match_planes

    def RegisterPbMap(self, frame1=None, frame2=None, max_match_planes: int = 0, registMode: int = DEFAULT_6DoF) -> bool:
        if frame1 is not None:
            self.setReference(frame1, max_match_planes)
        if frame2 is not None:
            self.setTarget(frame2, max_match_planes)
        pose = _mat16(self.rigidTransf)
        info = np.ascontiguousarray(self.informationM.T).reshape(36).copy()
        pairs = np.zeros(512, np.int32)
        n = C.c_int()
        am, as_, at = C.c_float(), C.c_float(self.areaSource), C.c_float(self.areaTarget)
        _check(lib().r360_ctx_set_match_params(self.ctx.h, C.byref(self.match)), "set_match_params")
        rc = _check(lib().r360_register_pbmap(self.ctx.h, self.ref.h, self.trg.h, self.max_match_planes, registMode,
                                              _fptr(pose), _fptr(info), pairs.ctypes.data_as(_IP), 256, C.byref(n),
                                              C.byref(am), C.byref(as_), C.byref(at)), "RegisterPbMap")
        self.bestMatch = {int(pairs[2 * k]): int(pairs[2 * k + 1]) for k in range(min(n.value, 256))}
        self.areaMatched = am.value
        if rc == 1:
            self.rigidTransf = _from16(pose)
            self.informationM = info.reshape(6, 6).T.copy()
            self.areaSource, self.areaTarget = as_.value, at.value
        return rc == 1

    def RegisterDensePhotoICP(self, frame1, frame2, pose_estim=None, method: int = PHOTO_CONSISTENCY,
                              registMode: int = DEFAULT_6DoF, params: "IcpParams | None" = None) -> bool:
        """RegisterDensePhotoICP (RegisterRGBD360.h:344-520): frame2's 8 sensor images aligned to frame1's in
        the rig frame.  Frames need BUILD_SENSOR_PYRAMID.  params None = RegisterPhotoICP()'s defaults."""
        init = _mat16(np.eye(4) if pose_estim is None else pose_estim)
        po = np.zeros(16, np.float32)
        info = np.ascontiguousarray(self.informationM.T).reshape(36).copy()
        self.dense_stats = DenseStats()
        rc = _check(lib().r360_register_dense(self.ctx.h, frame1.h, frame2.h, _fptr(init), method, registMode,
                                              None if params is None else C.byref(params), _fptr(po), _fptr(info),
                                              C.byref(self.dense_stats)), "RegisterDensePhotoICP")
        self.rigidTransf = _from16(po)
        if rc == 1:
            self.informationM = info.reshape(6, 6).T.copy()
        return rc == 1

    def eval_dense_robot(self, frame1, frame2, level: int, pose, method: int = PHOTO_CONSISTENCY,
                         params: "IcpParams | None" = None):
        """Per-sensor calcPhotoICPError_robot / calcHessianGradient_robot at `pose` on one level ->
        dict(err_photo[8], err_depth[8], H[8,6,6], g[8,6], n_error[8], n_depth[8], n_vis[8])."""
        err, H, g = np.zeros(16), np.zeros(8 * 36), np.zeros(8 * 6)
        cnt = np.zeros(24, np.int32)
        _check(lib().r360_dense_robot_eval(self.ctx.h, frame1.h, frame2.h, level, _fptr(_mat16(pose)), method,
                                           None if params is None else C.byref(params), err.ctypes.data_as(_DP),
                                           H.ctypes.data_as(_DP), g.ctypes.data_as(_DP), cnt.ctypes.data_as(_IP)),
               "eval_dense_robot")
        c = cnt.reshape(8, 3)
        return dict(err_photo=err[0::2].copy(), err_depth=err[1::2].copy(), H=H.reshape(8, 6, 6), g=g.reshape(8, 6),
                    n_error=c[:, 0].copy(), n_depth=c[:, 1].copy(), n_vis=c[:, 2].copy())

    def getPose(self): return self.rigidTransf
    def getInfoMat(self): return self.informationM
    def getCovMat(self):
        """covarianceM = informationM.inverse() (:208-215)."""
        return np.linalg.inv(self.informationM.astype(np.float64)).astype(np.float32)

    def calcEntropy(self) -> float:
        """0.5 (DOF (1 + log 2 pi) + log det(covariance)) (:230-238), DOF = 6, PI = 3.14159265359."""
        det = np.float32(np.linalg.det(self.getCovMat().astype(np.float64)))
        return float(np.float32(0.5 * (6 * (1 + np.log(2 * 3.14159265359)) + np.log(det))))

    def trackingScore(self):
        """(quality, score) of trackingScore(float& score) (:526-540): score = areaMatched / areaSource;
        0 GOOD (>= 0.7), 1 WEAK (>= 0.3), 2 BAD."""
        score = float(np.float32(np.float32(self.getAreaMatched()) / np.float32(self.areaSource))) \
            if self.areaSource else float("nan")
        return (0 if score >= 0.7 else 1 if score >= 0.3 else 2), score

    def getMatchedPlanes(self): return dict(self.bestMatch)
    def getAreaMatched(self): return self.areaMatched

    def match_tables(self, mode: int = PLANAR_3DoF, cap: int = 128):
        """k_match_tables output for the current reference/target subgraphs (inspection)."""
        ns, nt = C.c_int(), C.c_int()
        sid, tid = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        un = np.zeros(cap * cap, np.uint8)
        words = (cap * cap + 63) // 64
        bi = np.zeros(cap * cap * words, np.uint64)
        _check(lib().r360_ctx_set_match_params(self.ctx.h, C.byref(self.match)), "set_match_params")
        w = _check(lib().r360_pbmap_match_tables(self.ctx.h, self.ref.h, self.trg.h, self.max_match_planes, mode,
                                                 C.byref(ns), C.byref(nt), sid.ctypes.data_as(_IP),
                                                 tid.ctypes.data_as(_IP), _vptr(un), _vptr(bi), cap), "match_tables")
        n, m = ns.value, nt.value
        return dict(sid=sid[:n].copy(), tid=tid[:m].copy(), unary=un[:n * m].reshape(n, m).copy(),
                    binary=bi[:n * m * w].reshape(n * m, w).copy(), words=w)


def frames_build(frames, flags: int = None):
    """r360_frames_build: Frame360::getPlanes (Frame360.h:615-640) of several frames with their plane stages batched
    (up to 8 frames of one size per launch, on frames[0]'s context stream).  Same results as building each alone."""
    if flags is None:
        flags = BUILD_UNDISTORT | BUILD_CLOUD | BUILD_PLANES | BUILD_SPHERE | BUILD_PYRAMID
    arr = (C.c_void_p * len(frames))(*[f.h for f in frames])
    _check(lib().r360_frames_build(arr, len(frames), flags), "r360_frames_build")


def refine_force_fallback(sensor_mask: int = 0, first_sweep: bool = False):
    """Test hook (r360_refine_force_fallback): the builds that follow hand the sensors of sensor_mask (bit 8 * frame in
    batch + sensor) to the single-wave fallback kernel after their wavefront sweeps; 0 switches it off."""
    lib().r360_refine_force_fallback(sensor_mask, int(first_sweep))


def frames_segment_eval(frames, xyz4: np.ndarray, nrm: np.ndarray, rgb4: np.ndarray):
    """Parity hook (r360_frames_segment_eval): Frame360.segment_eval of up to 8 frames of one context and size as one
    batch of the stage's launcher.  xyz4 [n, 8, h, w, 4], nrm [n, 8, h, w, 3 or 4], rgb4 [n, 8, h, w, 4].  Returns the
    frames' error bits; a capacity error of any frame raises RuntimeError with them in its `codes` attribute."""
    n = len(frames)
    h, w = frames[0].rows // 2, frames[0].cols // 2
    xyz4 = np.ascontiguousarray(xyz4, np.float32)
    nrm = np.ascontiguousarray(nrm, np.float32)
    rgb4 = np.ascontiguousarray(rgb4, np.uint8)
    if xyz4.shape != (n, 8, h, w, 4) or nrm.shape[:4] != (n, 8, h, w) or nrm.shape[4] not in (3, 4) or \
            rgb4.shape != (n, 8, h, w, 4):
        raise ValueError(f"frames_segment_eval: fields of {n} x 8 x {h} x {w} expected")
    arr = (C.c_void_p * n)(*[f.h for f in frames])
    codes = np.zeros(n, np.int32)
    rc = lib().r360_frames_segment_eval(arr, n, _fptr(xyz4), _fptr(nrm), nrm.shape[4], _vptr(rgb4),
                                        codes.ctypes.data_as(_IP))
    if rc < 0:
        e = RuntimeError(f"frames_segment_eval failed ({rc}): {lib().r360_last_error().decode()}")
        e.codes = codes
        raise e
    return codes


def register(ctx: "Context", ref: "Frame360", trg: "Frame360", guess=None, params: "IcpParams | None" = None,
             max_match_planes: int = 25, mode: int = PLANAR_3DoF):
    """Register() alias: PbMap -> rotOffset conjugation -> alignFrames360 (OdometryKeyFrame360.cpp:248-254).
    Returns (pose, info, stats, pbmap_ok)."""
    g = _mat16(np.eye(4) if guess is None else guess)
    pose, info = np.zeros(16, np.float32), np.zeros(36, np.float32)
    st = IcpStats()
    p = params if params is not None else IcpParams.default()
    rc = _check(lib().r360_register(ctx.h, ref.h, trg.h, _fptr(g), C.byref(p), max_match_planes, mode, _fptr(pose),
                                    _fptr(info), C.byref(st)), "register")
    return _from16(pose), info.reshape(6, 6).T.copy(), st, rc == 0


class Batch:
    """Batched pair registrations (r360_batch, §8f-4): `lanes` worker contexts on one GPU run the jobs of a
    call concurrently.  Each job is the single-pair code path, so results equal the sequential calls.

    * ``register_pairs`` — generic jobs (RegisterPbMap, optionally gated / always refined by alignFrames360).
    * ``track`` — SphereGraphSLAM's tracking step (SLAM/SphereGraphSLAM.cpp:169-231).
    * ``loop_closures`` — LoopClosure360's candidate checks (include/LoopClosure360.h:280-366).
    """

    def __init__(self, device: int = 0, lanes: int = 8):
        h = C.c_void_p()
        _check(lib().r360_batch_create(device, lanes, C.byref(h)), "r360_batch_create")
        self.h = h
        self.lanes = lib().r360_batch_lanes(h)

    def register_pairs(self, jobs, max_match_planes: int = 25, mode: int = PLANAR_3DoF, min_matches: int = 0,
                       min_area: float = 0.0, params: "IcpParams | None" = None) -> list[dict]:
        """jobs: iterable of dicts {ref, trg, dense=JOB_PBMAP_ONLY, ref_is_source=False, guess=None}."""
        jobs = list(jobs)
        arr = (PairJob * max(1, len(jobs)))()
        for a, j in zip(arr, jobs):
            a.ref, a.trg = j["ref"].h.value, j["trg"].h.value
            a.dense = int(j.get("dense", JOB_PBMAP_ONLY))
            a.ref_is_source = int(bool(j.get("ref_is_source", False)))
            g = j.get("guess")
            a.guess[:] = [float(v) for v in _mat16(np.eye(4) if g is None else g)]
        out = (PairResult * max(1, len(jobs)))()
        p = params if params is not None else IcpParams.default()
        _check(lib().r360_batch_register(self.h, arr, len(jobs), max_match_planes, mode, min_matches, min_area,
                                         C.byref(p), out), "r360_batch_register")
        return [out[i].as_dict() for i in range(len(jobs))]

    def track(self, keyframes, frame, num_check: int = 5, no_assoc_threshold: int = 40, max_match_planes: int = 25,
              mode: int = PLANAR_ODOMETRY_3DoF):
        """Register `frame` against the newest keyframes (list, oldest first) -> (index into keyframes or -1,
        winner's result dict or None, every candidate's result in the reference's order)."""
        kfs = list(keyframes)
        ptrs = (C.c_void_p * max(1, len(kfs)))(*[k.h.value for k in kfs])
        m = min(len(kfs), num_check, no_assoc_threshold)
        res, cand = PairResult(), (PairResult * max(1, m))()
        chosen = C.c_int()
        _check(lib().r360_track_frame(self.h, ptrs, len(kfs), frame.h, num_check, no_assoc_threshold,
                                      max_match_planes, mode, C.byref(chosen), C.byref(res), cand), "r360_track_frame")
        return chosen.value, (res.as_dict() if chosen.value >= 0 else None), [cand[i].as_dict() for i in range(m)]

    def loop_closures(self, pairs, min_matches: int = 5, min_area: float = 15.0, ref_is_source: bool = True,
                      params: "IcpParams | None" = None, max_match_planes: int = 25) -> list[dict]:
        """pairs: [(keyframe, new_keyframe)].  RegisterPbMap PLANAR_3DoF, the matches/area gate
        (LoopClosure360.h:114-115, 298) and the alignFrames360 refinement of the pairs that pass."""
        jobs = [{"ref": a, "trg": b, "dense": JOB_GATED, "ref_is_source": ref_is_source} for a, b in pairs]
        return self.register_pairs(jobs, max_match_planes, PLANAR_3DoF, min_matches, min_area, params)

    def close(self):
        if self.h:
            lib().r360_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MAX_BATCH_ALIGN = 16


def align360_batch(ctx: "Context", pairs, inits=None, method: int = PHOTO_CONSISTENCY, params: "IcpParams" = None):
    """Batched alignFrames360 (r360_align360_batch_*): pairs = [(target Frame360, source Frame360), ...] (at most
    MAX_BATCH_ALIGN), inits = per-pair 4x4 guesses (identity if None).  Every pair's result equals
    RegisterPhotoICP.alignFrames360 on that pair alone.  Returns (poses [n,4,4], H [n,6,6], g [n,6], stats list,
    illposed count)."""
    n = len(pairs)
    p = params or IcpParams.default()
    trg = (C.c_void_p * n)(*[t.h for t, _ in pairs])
    src = (C.c_void_p * n)(*[s.h for _, s in pairs])
    init = np.concatenate([_mat16(np.eye(4) if inits is None or inits[j] is None else inits[j]) for j in range(n)])
    init = np.ascontiguousarray(init, np.float32)
    _check(lib().r360_align360_batch_async(ctx.h, n, trg, src, _fptr(init), method, C.byref(p)),
           "r360_align360_batch_async")
    po, Ho, go = np.zeros(16 * n, np.float32), np.zeros(36 * n, np.float32), np.zeros(6 * n, np.float32)
    st = (IcpStats * n)()
    ill = _check(lib().r360_align360_batch_result(ctx.h, _fptr(po), _fptr(Ho), _fptr(go), st),
                 "r360_align360_batch_result")
    poses = np.stack([_from16(po[16 * j:16 * j + 16]) for j in range(n)])
    H = np.stack([Ho[36 * j:36 * j + 36].reshape(6, 6).T.copy() for j in range(n)])
    return poses, H, go.reshape(n, 6).copy(), list(st), ill


def align_eval_batch(ctx: "Context", pairs, level: int, poses, method: int = PHOTO_DEPTH, params: "IcpParams" = None):
    """RegisterPhotoICP.eval on the batched grid (r360_icp_eval_batch, a test hook): one eval-only pass of
    pairs = [(target Frame360, source Frame360), ...] at `level`, job j at poses[j].  Returns (H [n,6,6], g [n,6],
    err2 [n], n_valid [n], n_visible [n])."""
    n = len(pairs)
    p = params or IcpParams.default()
    trg = (C.c_void_p * n)(*[t.h for t, _ in pairs])
    src = (C.c_void_p * n)(*[s.h for _, s in pairs])
    assert len(poses) == n
    ps = np.ascontiguousarray(np.concatenate([_mat16(P) for P in poses]), np.float32)
    H, g, e2 = np.zeros(36 * n), np.zeros(6 * n), np.zeros(n)
    nv, nvis = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(lib().r360_icp_eval_batch(ctx.h, n, trg, src, level, _fptr(ps), method, C.byref(p), H.ctypes.data_as(_DP),
                                     g.ctypes.data_as(_DP), e2.ctypes.data_as(_DP), nv.ctypes.data_as(_IP),
                                     nvis.ctypes.data_as(_IP)), "r360_icp_eval_batch")
    return H.reshape(n, 6, 6), g.reshape(n, 6), e2, nv, nvis


class DenseQueue:
    """The alignFrames360 stage of many concurrent registrations batched on one stream (r360_dense_queue):
    submit from any thread, collect by ticket; a job's result equals the single-pair alignment."""

    def __init__(self, device: int = 0, max_batch: int = MAX_BATCH_ALIGN):
        h = C.c_void_p()
        _check(lib().r360_dense_queue_create(device, max_batch, C.byref(h)), "r360_dense_queue_create")
        self.h, self.device = h, device
        ctx = Context.__new__(Context)      # non-owning view of the queue's own context (timing reads)
        ctx.h, ctx.device = C.c_void_p(lib().r360_dense_queue_ctx(h)), device
        ctx.close = lambda: None
        self.ctx = ctx

    @classmethod
    def _view(cls, h, device: int) -> "DenseQueue":
        """A non-owning view of a dense queue the library owns (a sequence runner's)."""
        q = cls.__new__(cls)
        q.h, q.device = h, device
        q.ctx = Context._view(C.c_void_p(lib().r360_dense_queue_ctx(h)), device)
        q.close = lambda: None
        return q

    def submit(self, trg: "Frame360", src: "Frame360", init=None, method: int = PHOTO_DEPTH,
               params: "IcpParams" = None) -> int:
        t = C.c_long()
        i16 = _mat16(np.eye(4) if init is None else init)
        _check(lib().r360_dense_queue_submit(self.h, trg.h, src.h, _fptr(i16), method,
                                             C.byref(params or IcpParams.default()), C.byref(t)), "dense submit")
        return t.value

    def collect(self, ticket: int):
        po, Ho, go = np.zeros(16, np.float32), np.zeros(36, np.float32), np.zeros(6, np.float32)
        st = IcpStats()
        rc = _check(lib().r360_dense_queue_collect(self.h, ticket, _fptr(po), _fptr(Ho), _fptr(go), C.byref(st)),
                    "dense collect")
        return _from16(po), Ho.reshape(6, 6).T.copy(), go, st, rc

    def stats(self):
        b, j, m = C.c_long(), C.c_long(), C.c_int()
        _check(lib().r360_dense_queue_stats(self.h, C.byref(b), C.byref(j), C.byref(m)), "dense stats")
        return {"batches": b.value, "jobs": j.value, "max_batch": m.value}

    def close(self):
        if self.h:
            lib().r360_dense_queue_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegisterPhotoICP:
    """RegisterPhotoICP spherical path (include/RegisterPhotoICP.h), frames stay in HBM."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.params = IcpParams.default()
        self.src = self.trg = None
        self.relPose = np.eye(4, dtype=np.float32)
        self.hessian = np.zeros((6, 6), np.float32)
        self.gradient = np.zeros(6, np.float32)
        self.stats = IcpStats()
        # public members (:180-192); the reference leaves the residuals uninitialised until an error function
        # that assigns them runs (NaN here)
        self.avResidual = self.avPhotoResidual = self.avDepthResidual = float("nan")
        self.SSO = 0.0
        self._own = {}         # sphere-only frames for spheres given as images, per (role, size)

    def _residuals(self):
        if self.stats.residuals_set & 1:
            self.avPhotoResidual = self.stats.av_photo_residual
            self.avDepthResidual = self.stats.av_depth_residual
        if self.stats.residuals_set & 2:
            self.avResidual = self.stats.av_residual
        self.SSO = self.stats.sso

    def setVisualization(self, b: bool):
        """visualizeIterations (OpenCV windows): no display here."""
        self.visualize = bool(b)

    # setters (:224-269)
    def setNumPyr(self, n: int): self.params.n_pyr = n
    def setMinDepth(self, d: float): self.params.min_depth = d
    def setMaxDepth(self, d: float): self.params.max_depth = d
    def setGrayVariance(self, s: float): self.params.std_dev_photo = s
    def setDepthVariance(self, s: float): self.params.std_dev_depth = s

    def useSaliency(self, b: bool):
        if b:
            raise NotImplementedError("saliency subsampling is commented out in the reference's sphere path")

    def _sphere_frame(self, role: str, bgr, range_mm) -> Frame360:
        H, W = np.asarray(range_mm).shape
        key = (role, H, W)
        if key not in self._own:
            cal = Calib360.for_sphere(self.ctx, H, W)
            self._own[key] = (cal, Frame360(cal))
        f = self._own[key][1]
        f.set_sphere(bgr, range_mm)
        return f

    def setSourceFrame(self, f, imgDepth=None):
        """setSourceFrame(Frame360) — the frame's sphere and pyramid in HBM — or setSourceFrame(imgRGB,
        imgDepth) with the sphere as images (BGR u8 [H, W, 3], range u16 mm [H, W]; :496-516)."""
        self.src = f if imgDepth is None else self._sphere_frame("src", f, imgDepth)

    def setTargetFrame(self, f, imgDepth=None):
        """setTargetFrame(Frame360) or setTargetFrame(imgRGB, imgDepth) (:480-494)."""
        self.trg = f if imgDepth is None else self._sphere_frame("trg", f, imgDepth)

    def alignFrames360(self, pose_guess=None, method: int = PHOTO_CONSISTENCY, occlusion: int = 0) -> int:
        init = _mat16(np.eye(4) if pose_guess is None else pose_guess)
        po, Ho, go = np.zeros(16, np.float32), np.zeros(36, np.float32), np.zeros(6, np.float32)
        rc = _check(lib().r360_align360(self.ctx.h, self.trg.h, self.src.h, _fptr(init), method, occlusion,
                                        C.byref(self.params), _fptr(po), _fptr(Ho), _fptr(go),
                                        C.byref(self.stats)), "alignFrames360")
        self._residuals()
        self.relPose = _from16(po)
        self.hessian = Ho.reshape(6, 6).T.copy()
        self.gradient = go.copy()
        return rc

    def getOptimalPose(self): return self.relPose
    def getHessian(self): return self.hessian
    def getGradient(self): return self.gradient

    # ---- pinhole per-sensor path (§8(f) rank 3): alignFrames (:4254-4512) on sensor images
    def setCameraMatrix(self, K):
        """cameraMatrix (3x3); None = the calibration's (f = 525*cols/640, c = (cols/2-0.5, rows/2-0.5))."""
        self.K = None if K is None else np.array([K[0][0], K[1][1], K[0][2], K[1][2]], np.float32)

    def setSourceSensor(self, f: Frame360, sensor: int):
        """setSourceFrame(frameRGBD_[sensor].getRGBImage(), getDepthImage()) (:496-516)."""
        self.src, self.src_sensor = f, sensor

    def setTargetSensor(self, f: Frame360, sensor: int):
        """setTargetFrame(frameRGBD_[sensor].getRGBImage(), getDepthImage()) (:480-494)."""
        self.trg, self.trg_sensor = f, sensor

    def _K(self):
        k = getattr(self, "K", None)
        return None if k is None else _fptr(k)

    def alignFrames(self, pose_guess=None, method: int = PHOTO_CONSISTENCY, occlusion: int = 0) -> int:
        if occlusion:
            raise NotImplementedError("pinhole alignFrames: occlusion variants 1/2 are not built")
        if self.src_sensor != self.trg_sensor:
            raise ValueError("source and target sensors differ")
        init = _mat16(np.eye(4) if pose_guess is None else pose_guess)
        po, Ho, go = np.zeros(16, np.float32), np.zeros(36, np.float32), np.zeros(6, np.float32)
        rc = _check(lib().r360_align_pinhole(self.ctx.h, self.trg.h, self.src.h, self.src_sensor, _fptr(init), method,
                                             self._K(), C.byref(self.params), _fptr(po), _fptr(Ho), _fptr(go),
                                             C.byref(self.stats)), "alignFrames")
        self._residuals()
        self.relPose = _from16(po)
        self.hessian = Ho.reshape(6, 6).T.copy()
        self.gradient = go.copy()
        return rc

    def alignSensors(self, trg: Frame360, src: Frame360, sensors, pose_guesses, method: int = PHOTO_DEPTH):
        """alignFrames on several sensors of one pair at once (one batched pass sequence).
        Returns (poses [n,4,4], hessians [n,6,6], stats list, n_illposed)."""
        sensors = np.ascontiguousarray(sensors, np.int32)
        n = len(sensors)
        init = np.concatenate([_mat16(P) for P in pose_guesses]).astype(np.float32)
        _check(lib().r360_align_pinhole_async(self.ctx.h, trg.h, src.h, n, sensors.ctypes.data_as(_IP), _fptr(init),
                                              method, self._K(), C.byref(self.params)), "alignSensors")
        po, Ho, go = np.zeros(16 * n, np.float32), np.zeros(36 * n, np.float32), np.zeros(6 * n, np.float32)
        st = (IcpStats * n)()
        ill = _check(lib().r360_align_pinhole_result(self.ctx.h, _fptr(po), _fptr(Ho), _fptr(go), st),
                     "alignSensors")
        poses = np.stack([_from16(po[16 * j:16 * j + 16]) for j in range(n)])
        Hs = np.stack([Ho[36 * j:36 * j + 36].reshape(6, 6).T for j in range(n)])
        return poses, Hs, list(st), ill

    def eval_pinhole(self, level: int, pose, method: int = PHOTO_DEPTH):
        """One errorPhotoICP + calcHessGrad pass -> dict(H, g, error, res_photo, res_depth, n_photo, n_depth, n_vis)."""
        H, g = np.zeros(36), np.zeros(6)
        err, res = C.c_double(), np.zeros(2)
        cnt = np.zeros(3, np.int32)
        _check(lib().r360_pinhole_eval(self.ctx.h, self.trg.h, self.src.h, self.src_sensor, level, _fptr(_mat16(pose)),
                                       method, self._K(), C.byref(self.params), H.ctypes.data_as(_DP),
                                       g.ctypes.data_as(_DP), C.byref(err), res.ctypes.data_as(_DP),
                                       cnt.ctypes.data_as(_IP)), "eval_pinhole")
        return dict(H=H.reshape(6, 6), g=g, error=err.value, res_photo=res[0], res_depth=res[1], n_photo=int(cnt[0]),
                    n_depth=int(cnt[1]), n_vis=int(cnt[2]))

    def eval(self, level: int, pose, method: int = PHOTO_DEPTH):
        """One fused errorPhotoICP_sphere + calcHessGrad_sphere pass at a fixed pose."""
        p = _mat16(pose)
        H, g = np.zeros(36), np.zeros(6)
        e2, nv, nvis = C.c_double(), C.c_int(), C.c_int()
        _check(lib().r360_icp_eval(self.ctx.h, self.trg.h, self.src.h, level, _fptr(p), method,
                                   C.byref(self.params), H.ctypes.data_as(_DP), g.ctypes.data_as(_DP),
                                   C.byref(e2), C.byref(nv), C.byref(nvis)), "icp_eval")
        return H.reshape(6, 6), g, e2.value, nv.value, nvis.value

    def pass_grid(self, level: int, occlusion: int = 0, batched: bool = False):
        """(pass form PF, workgroups per job) the launcher picks for `level` of the source frame (r360_icp_pass_grid,
        a test hook; host only)."""
        pf, nb = C.c_int(), C.c_int()
        _check(lib().r360_icp_pass_grid(self.ctx.h, self.src.h, level, occlusion, int(bool(batched)), C.byref(pf),
                                        C.byref(nb)), "icp_pass_grid")
        return pf.value, nb.value

    def eval_occ(self, level: int, pose, method: int = PHOTO_DEPTH, occlusion: int = 1):
        """One occlusion-aware pass at a fixed pose: H, g of calcHessGrad_sphereOcc{occlusion}, the value
        of errorPhotoICP_sphereOcc{occlusion}, its point count and numVisiblePixels."""
        p = _mat16(pose)
        H, g = np.zeros(36), np.zeros(6)
        e, nv, nvis = C.c_double(), C.c_int(), C.c_int()
        _check(lib().r360_icp_eval_occ(self.ctx.h, self.trg.h, self.src.h, level, _fptr(p), method, occlusion,
                                       C.byref(self.params), H.ctypes.data_as(_DP), g.ctypes.data_as(_DP),
                                       C.byref(e), C.byref(nv), C.byref(nvis)), "icp_eval_occ")
        return H.reshape(6, 6), g, e.value, nv.value, nvis.value


def match_tree_search(unary: np.ndarray, binary: np.ndarray, area, max_nodes: int = 4000000):
    """The interpretation-tree search alone (host only): unary [ns, nt] bool, binary [ns * nt, words] uint64 (bit k * nt
    + l of row i * nt + j: references i, k matched to targets j, l are consistent), area [ns].  Returns (best [ns]
    target or -1, nodes, truncated)."""
    unary = np.ascontiguousarray(unary, np.uint8)
    ns, nt = unary.shape
    words = (ns * nt + 63) // 64
    binary = np.ascontiguousarray(binary, np.uint64).reshape(ns * nt, words) if ns * nt else np.zeros((0, 0), np.uint64)
    area = np.ascontiguousarray(area, np.float64)
    best = np.zeros(max(ns, 1), np.int32)
    nodes = C.c_long()
    rc = _check(lib().r360_match_tree_search(ns, nt, _vptr(unary), _vptr(binary), words, _vptr(area), max_nodes,
                                             _vptr(best), C.byref(nodes)), "match_tree_search")
    return best[:ns], nodes.value, bool(rc)


def refine_eval(state: np.ndarray, mask: np.ndarray, rb: int = 0, return_fallbacks: bool = False):
    """refine()'s two sweeps on the device (parity hook): state int8 (8, h, w), mask uint64 (8, h, w); rb = -1 the
    wavefront sweeps (the default path; LDS-pipelined 64-row bands for h <= 512), -2 the barrier-per-diagonal
    wavefront, 0 the single-wave sweeps, rb > 0 banded.  With return_fallbacks, also the
    number of sensors whose wavefront second sweep needed wrap-push corrections (re-runs or the fallback)."""
    state = np.ascontiguousarray(state, np.int8)
    mask = np.ascontiguousarray(mask, np.uint64)
    _, h, w = state.shape
    out = np.zeros_like(state)
    nfb = _check(lib().r360_refine_eval(state.ctypes.data, mask.ctypes.data, w, h, rb, out.ctypes.data),
                 "r360_refine_eval")
    return (out, nfb) if return_fallbacks else out


def libm_eval(x, y, z, on_device: bool = False):
    """Evaluate the projection's asinf / atan2f port (libm_f32.h) on the host or the GPU."""
    x, y, z = (np.ascontiguousarray(a, np.float32) for a in (x, y, z))
    a, t = np.zeros_like(x), np.zeros_like(x)
    _check(lib().r360_libm_eval(_fptr(x), _fptr(y), _fptr(z), x.size, _fptr(a), _fptr(t), int(on_device)),
           "libm_eval")
    return a, t


class Comm:
    """RCCL communicator of one rank (r360_comm): the sequence driver's record all_gather over xGMI.
    Rank 0 calls unique_id() and hands the bytes to the other ranks (e.g. over a gloo process group)."""

    @staticmethod
    def unique_id() -> bytes:
        b = (C.c_uint8 * 128)()
        _check(lib().r360_comm_unique_id(b), "comm_unique_id")
        return bytes(b)

    def __init__(self, device: int, nranks: int, rank: int, uid: bytes):
        assert len(uid) == 128
        self.nranks = nranks
        self.h = C.c_void_p()
        b = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().r360_comm_init(device, nranks, rank, b, C.byref(self.h)), "comm_init")

    def allgather(self, a: np.ndarray) -> np.ndarray:
        """(nranks,) + a.shape: every rank's array, in rank order."""
        a = np.ascontiguousarray(a)
        out = np.zeros((self.nranks,) + a.shape, a.dtype)
        _check(lib().r360_comm_allgather(self.h, _vptr(a), _vptr(out), a.nbytes), "comm_allgather")
        return out

    def allreduce_max(self, v: float) -> float:
        x = np.array([v], np.float64)
        _check(lib().r360_comm_allreduce_max(self.h, x.ctypes.data_as(_DP), 1), "comm_allreduce_max")
        return float(x[0])

    def close(self):
        if self.h:
            lib().r360_comm_destroy(self.h)
            self.h = None


class DeviceArray:
    """A host array's copy resident in HBM (r360_dev_alloc); ptr(i) = device address of element i along
    the first axis."""

    def __init__(self, device: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        self.nbytes, self.row = a.nbytes, a[0].nbytes if a.ndim else a.nbytes
        self.p = C.c_void_p()
        _check(lib().r360_dev_alloc(device, self.nbytes, C.byref(self.p)), "dev_alloc")
        _check(lib().r360_dev_copy(self.p, _vptr(a), self.nbytes, 0), "dev_copy")

    def ptr(self, i: int = 0) -> int:
        return self.p.value + i * self.row

    def close(self):
        if self.p:
            lib().r360_dev_free(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostPinned:
    """Page-locks numpy arrays for asynchronous uploads (hipHostRegister); released by close()."""

    def __init__(self, *arrays):
        self.arrays = []
        for a in arrays:
            assert a.flags.c_contiguous
            _check(lib().r360_host_register(_vptr(a), a.nbytes), "host_register")
            self.arrays.append(a)

    def close(self):
        for a in self.arrays:
            lib().r360_host_unregister(_vptr(a))
        self.arrays = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_frame_rt(rows: int, cols: int, rt8: np.ndarray, seed: int, rig_pose: np.ndarray):
    """Host-only synthetic frame (no GPU): rt8 = (8, 4, 4) extrinsics."""
    bgr = np.zeros((8, rows, cols, 3), np.uint8)
    dep = np.zeros((8, rows, cols), np.uint16)
    rt = np.ascontiguousarray(np.stack([_mat16(m) for m in rt8]), np.float32)
    p = _mat16(rig_pose)
    _check(lib().r360_synth_frame_rt(rows, cols, _fptr(rt), seed, _fptr(p), _vptr(bgr), _vptr(dep)), "synth_frame_rt")
    return bgr, dep


def synth_path_pose(seed: int, frame: int) -> np.ndarray:
    a = np.zeros(16, np.float32)
    lib().r360_synth_path_pose(seed, frame, _fptr(a))
    return _from16(a)


def exp_se3(mu, pseudo: bool = True) -> np.ndarray:
    m = np.asarray(mu, np.float64)
    T = np.zeros(16, np.float32)
    lib().r360_exp_se3(m.ctypes.data_as(_DP), int(pseudo), _fptr(T))
    return _from16(T)


def _cloud_arrays(xyz, rgba):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if rgba is not None:
        rgba = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
        assert rgba.shape[0] == xyz.shape[0]
    return xyz, rgba


def filter_euclidean(xyz, rgba=None, x_min: float = -2.0, x_max: float = 1.0, box: float = 4.0):
    """FilterPointCloud::filterEuclidean on the host (r360_cloud_filter_euclidean, no GPU): the points with finite
    coordinates inside [x_min, x_max] x [-box, box]^2, in order.  Returns (xyz [m,3], rgba [m] or None)."""
    xyz, rgba = _cloud_arrays(xyz, rgba)
    n = xyz.shape[0]
    oxyz = np.zeros((n, 3), np.float32)
    orgba = None if rgba is None else np.zeros(n, np.uint32)
    m = C.c_size_t()
    _check(lib().r360_cloud_filter_euclidean(_fptr(xyz), None if rgba is None else _vptr(rgba), n, x_min, x_max, box,
                                             _fptr(oxyz), None if rgba is None else _vptr(orgba), C.byref(m)),
           "filter_euclidean")
    return oxyz[:m.value].copy(), None if rgba is None else orgba[:m.value].copy()


class FilterPointCloud:
    """FilterPointCloud (include/FilterPointCloud.h) with the reference's constructor defaults: filterEuclidean on
    the host, returning (xyz, rgba); filterVoxel on the GPU of `ctx`, returning (xyz, rgba) one point per voxel of
    voxelSize (the cloud unchanged when PCL's size guard refuses the leaf)."""

    def __init__(self, voxelSize: float = 0.05, euclideanBox: float = 4.0, ctx: "Context | None" = None):
        self.voxelSize, self.euclideanBox, self.ctx = voxelSize, euclideanBox, ctx

    def filterEuclidean(self, xyz, rgba=None):
        return filter_euclidean(xyz, rgba, -2.0, 1.0, self.euclideanBox)

    def filterVoxel(self, xyz, rgba=None):
        if self.ctx is None:
            raise RuntimeError("FilterPointCloud.filterVoxel runs on a GPU: construct the filter with ctx=Context(...)")
        oxyz, orgba, _ = self.ctx.filter_voxel(xyz, rgba, self.voxelSize)
        return oxyz, orgba


VOXEL_QUANTUM = 2.0 ** -24   # R360_VOXEL_QUANTUM: the fixed-point unit (m) of the voxel grid's coordinate sums


DATA_DIR = os.path.join(REPO_ROOT, "data")
EXTRINSICS_DIR = os.path.join(DATA_DIR, "calib", "Extrinsics")   # Rt_0{1..8}.txt (reference rig)
INTRINSICS_DIR = os.path.join(DATA_DIR, "calib", "Intrinsics")   # CLAMS tables (compact form)
SAMPLES_DIR = os.path.join(DATA_DIR, "samples")                  # sphere_images_{1,10}.bin


class GeneralizedICP:
    """r360::GeneralizedIterativeClosestPoint's Python mirror: pcl::GeneralizedIterativeClosestPoint's call surface
    as Registration/RegisterPairRGBD360.cpp:109-149 uses it, over Context.gicp_*.  Clouds are [n,3] float32."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.params = GicpParams.default()
        self.ransac_threshold = 0.05   # stored and never read, as in PCL's GICP
        self.stats = GicpStats()
        self._pose = np.eye(4, dtype=np.float32)
        self._src = None
        self._status = 0

    def setMaxCorrespondenceDistance(self, d: float): self.params.max_corr_dist = d
    def setMaximumIterations(self, n: int): self.params.max_iterations = n
    def setTransformationEpsilon(self, e: float): self.params.transformation_epsilon = e
    def setRotationEpsilon(self, e: float): self.params.rotation_epsilon = e
    def setCorrespondenceRandomness(self, k: int): self.params.k_correspondences = k
    def setMaximumOptimizerIterations(self, n: int): self.params.max_inner_iterations = n
    def setRANSACOutlierRejectionThreshold(self, t: float): self.ransac_threshold = t

    def setInputSource(self, xyz):
        self._src = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.ctx.gicp_set_source(self._src, self.params)

    def setInputTarget(self, xyz):
        self.ctx.gicp_set_target(xyz, self.params)

    def align(self, guess=None) -> np.ndarray:
        """Runs the registration and returns the source cloud under the final transformation (float, left to right,
        as transformPointCloud)."""
        self._pose, self.stats, self._status = self.ctx.gicp_align(guess, self.params)
        m = self._pose
        s = self._src
        out = np.empty_like(s)
        for k in range(3):
            out[:, k] = ((m[k, 0] * s[:, 0] + m[k, 1] * s[:, 1]) + m[k, 2] * s[:, 2]) + m[k, 3]
        return out

    def getFinalTransformation(self) -> np.ndarray: return self._pose.copy()
    def hasConverged(self) -> bool: return bool(self.stats.converged)
    def getFitnessScore(self) -> float: return self.stats.fitness


def _mat16d(m) -> np.ndarray:
    """4x4 -> column-major double[16] (Eigen::Matrix4d::data())."""
    return np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(4, 4).T).reshape(16).copy()


def _mat36d(m) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(6, 6).T).reshape(36).copy()


def g2o_write(path: str, poses, fixed, edges):
    """r360_g2o_write: poses [n] 4x4, fixed [n] flags (or None), edges [(i, j, rel 4x4, info 6x6)]."""
    P = np.concatenate([_mat16d(T) for T in poses]) if len(poses) else np.zeros(0)
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=np.int32))
    ij = np.ascontiguousarray(np.array([[e[0], e[1]] for e in edges], dtype=np.int32).reshape(-1))
    Z = np.concatenate([_mat16d(e[2]) for e in edges]) if len(edges) else np.zeros(0)
    Om = np.concatenate([_mat36d(e[3]) for e in edges]) if len(edges) else np.zeros(0)
    _check(lib().r360_g2o_write(path.encode(), len(poses), _dptr(P), None if fx is None else fx.ctypes.data_as(_IP),
                                len(edges), ij.ctypes.data_as(_IP), _dptr(Z), _dptr(Om)), "g2o_write")


def g2o_read(path: str):
    """r360_g2o_read: (poses [n,4,4], fixed [n] int32, edges [(i, j, rel 4x4, info 6x6)])."""
    nv, ne = C.c_int(), C.c_int()
    _check(lib().r360_g2o_read(path.encode(), None, None, 0, C.byref(nv), None, None, None, 0, C.byref(ne)), "g2o_read")
    P = np.zeros(16 * nv.value)
    fx = np.zeros(nv.value, np.int32)
    ij = np.zeros(2 * ne.value, np.int32)
    Z = np.zeros(16 * ne.value)
    Om = np.zeros(36 * ne.value)
    _check(lib().r360_g2o_read(path.encode(), _dptr(P), fx.ctypes.data_as(_IP), nv.value, C.byref(nv),
                               ij.ctypes.data_as(_IP), _dptr(Z), _dptr(Om), ne.value, C.byref(ne)), "g2o_read")
    poses = P.reshape(-1, 4, 4).transpose(0, 2, 1).copy()
    edges = [(int(ij[2 * e]), int(ij[2 * e + 1]), Z[16 * e:16 * e + 16].reshape(4, 4).T.copy(),
              Om[36 * e:36 * e + 36].reshape(6, 6).T.copy()) for e in range(ne.value)]
    return poses, fx, edges


class PoseGraph:
    """The reference's GraphOptimizer (include/GraphOptimizer.h) over r360_graph_*: addVertex / addEdge / optimizeGraph /
    getPoses / saveGraph, on the context's GPU.  Poses are 4x4 float64, world from keyframe; an edge says
    T_to ~ T_from @ rel with a 6x6 information matrix ordered (translation, rotation).  The context must stay open
    while the graph is used; closing the graph after its context is safe."""

    def __init__(self, ctx: "Context"):
        h = C.c_void_p()
        _check(lib().r360_graph_create(ctx.h, C.byref(h)), "r360_graph_create")
        self.h, self.ctx = h, ctx
        self.params = GraphParams.default()
        self.stats = GraphStats()

    def close(self):
        if self.h:
            lib().r360_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def addVertex(self, pose) -> int:
        i = C.c_int()
        _check(lib().r360_graph_add_vertex(self.h, _dptr(_mat16d(pose)), C.byref(i)), "graph_add_vertex")
        return i.value

    def addEdge(self, i: int, j: int, rel, info):
        _check(lib().r360_graph_add_edge(self.h, i, j, _dptr(_mat16d(rel)), _dptr(_mat36d(info))), "graph_add_edge")

    def setFixed(self, i: int, fixed: bool = True):
        _check(lib().r360_graph_set_fixed(self.h, i, int(fixed)), "graph_set_fixed")

    def setPose(self, i: int, pose):
        _check(lib().r360_graph_set_pose(self.h, i, _dptr(_mat16d(pose))), "graph_set_pose")

    def size(self):
        nv, ne = C.c_int(), C.c_int()
        _check(lib().r360_graph_size(self.h, C.byref(nv), C.byref(ne)), "graph_size")
        return nv.value, ne.value

    def numEdges(self) -> int:
        return self.size()[1]

    def setRobustKernel(self, kind: int, delta: float = 1.0):
        """The kernel (GRAPH_KERNEL_*) of the edges added from now on; delta applies to sqrt(chi2)."""
        _check(lib().r360_graph_set_default_kernel(self.h, kind, delta), "graph_set_default_kernel")

    def setEdgeRobustKernel(self, edge: int, kind: int, delta: float = 1.0):
        _check(lib().r360_graph_set_edge_kernel(self.h, edge, kind, delta), "graph_set_edge_kernel")

    def getEdgeRobustKernel(self, edge: int):
        kind, delta = C.c_int(), C.c_double()
        _check(lib().r360_graph_get_edge_kernel(self.h, edge, C.byref(kind), C.byref(delta)), "graph_get_edge_kernel")
        return kind.value, delta.value

    def setEdgeActive(self, edge: int, active: bool = True):
        """An inactive edge does not exist for eval, solve, optimizeGraph and saveGraph."""
        _check(lib().r360_graph_set_edge_active(self.h, edge, int(active)), "graph_set_edge_active")

    def getEdgeActive(self, edge: int) -> bool:
        a = C.c_int()
        _check(lib().r360_graph_get_edge_active(self.h, edge, C.byref(a)), "graph_get_edge_active")
        return bool(a.value)

    def getEdgeChi2(self):
        """r360_graph_edge_stats: (chi2 [n_edges], weight [n_edges]) at the current poses; an inactive edge has weight 0."""
        m = self.numEdges()
        chi2, w = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        n = C.c_int()
        _check(lib().r360_graph_edge_stats(self.h, _dptr(chi2), _dptr(w), m, C.byref(n)), "graph_edge_stats")
        return chi2[:m].copy(), w[:m].copy()

    def getPoses(self) -> np.ndarray:
        n = self.size()[0]
        P = np.zeros(16 * n)
        m = C.c_int()
        _check(lib().r360_graph_get_poses(self.h, _dptr(P), n, C.byref(m)), "graph_get_poses")
        return P.reshape(n, 4, 4).transpose(0, 2, 1).copy()

    def optimizeGraph(self, params: "GraphParams | None" = None) -> "GraphStats":
        st = GraphStats()
        p = params if params is not None else self.params
        _check(lib().r360_graph_optimize(self.h, C.byref(p), C.byref(st)), "graph_optimize")
        self.stats = st
        return st

    def eval(self):
        """r360_graph_eval: (F, b [N], H [N, N]) over the free vertices in index order."""
        n = C.c_int()
        _check(lib().r360_graph_eval(self.h, None, None, None, 0, C.byref(n)), "graph_eval")
        N = n.value
        F = C.c_double()
        b = np.zeros(max(N, 1))
        H = np.zeros((max(N, 1), max(N, 1)))
        _check(lib().r360_graph_eval(self.h, C.byref(F), _dptr(b), _dptr(H), N, C.byref(n)), "graph_eval")
        return F.value, b[:N].copy(), H[:N, :N].copy() if N else np.zeros((0, 0))

    def solve(self, lam: float, params: "GraphParams | None" = None):
        """r360_graph_solve: (delta [N], iterations, relative residual, form, converged)."""
        n = C.c_int()
        p = params if params is not None else self.params
        _check(lib().r360_graph_solve(self.h, C.byref(p), lam, None, 0, C.byref(n), None, None, None), "graph_solve")
        d = np.zeros(n.value)
        it, form, rel = C.c_int(), C.c_int(), C.c_double()
        rc = _check(lib().r360_graph_solve(self.h, C.byref(p), lam, _dptr(d), n.value, C.byref(n), C.byref(it),
                                           C.byref(rel), C.byref(form)), "graph_solve")
        return d, it.value, rel.value, form.value, rc == 0

    def saveGraph(self, path: str):
        _check(lib().r360_graph_save(self.h, path.encode()), "graph_save")

    def loadGraph(self, path: str):
        _check(lib().r360_graph_load(self.h, path.encode()), "graph_load")


def rigcal_read_matrix(path: str) -> np.ndarray:
    """One of the reference's text matrices (correspondences_i_j.txt) through the library's reader; no GPU."""
    nr, nc = C.c_int(), C.c_int()
    _check(lib().r360_rigcal_read_matrix(path.encode(), None, 0, C.byref(nr), C.byref(nc)), "rigcal_read_matrix")
    a = np.zeros((nr.value, nc.value))
    _check(lib().r360_rigcal_read_matrix(path.encode(), _dptr(a), a.size, C.byref(nr), C.byref(nc)), "rigcal_read_matrix")
    return a


def rigcal_write_matrix(path: str, rows: np.ndarray):
    a = np.ascontiguousarray(rows, np.float64)
    assert a.ndim == 2
    _check(lib().r360_rigcal_write_matrix(path.encode(), _dptr(a), a.shape[0], a.shape[1]), "rigcal_write_matrix")


def rigcal_specs() -> np.ndarray:
    """loadConstructionSpecs (Calibration.h:918-930): (8, 4, 4) float64."""
    a = np.zeros(128)
    lib().r360_rigcal_specs(_dptr(a))
    return a.reshape(8, 4, 4).transpose(0, 2, 1).copy()


class RigCalibration:
    """The reference's ControlPlanes + Calibration (include/Calibration.h) over r360_rigcal_*: correspondence rows per
    sensor pair (i, j), i < j, the rotation and translation solves and the outlier trimmer on the context's GPU.
    ctx None gives a handle for rows and files only.  Extrinsics are (8, 4, 4) float64."""

    def __init__(self, ctx: "Context | None" = None):
        h = C.c_void_p()
        _check(lib().r360_rigcal_create(ctx.h if ctx is not None else None, C.byref(h)), "r360_rigcal_create")
        self.h, self.ctx = h, ctx

    def close(self):
        if self.h:
            lib().r360_rigcal_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setPair(self, i: int, j: int, rows):
        a = np.ascontiguousarray(rows, np.float64).reshape(-1, 10) if len(rows) else np.zeros((0, 10))
        _check(lib().r360_rigcal_set_pair(self.h, i, j, _dptr(a), a.shape[0], 10), "rigcal_set_pair")

    def getPair(self, i: int, j: int) -> np.ndarray:
        n = C.c_int()
        _check(lib().r360_rigcal_get_pair(self.h, i, j, None, 0, C.byref(n)), "rigcal_get_pair")
        a = np.zeros((n.value, 10))
        _check(lib().r360_rigcal_get_pair(self.h, i, j, _dptr(a), n.value, C.byref(n)), "rigcal_get_pair")
        return a

    def setPairs(self, rows: dict):
        self.clear()
        for (i, j), r in rows.items():
            self.setPair(i, j, r)

    def pairs(self) -> dict:
        out = {}
        for i in range(8):
            for j in range(i + 1, 8):
                r = self.getPair(i, j)
                if len(r):
                    out[(i, j)] = r
        return out

    def clear(self):
        _check(lib().r360_rigcal_clear(self.h), "rigcal_clear")

    def check(self) -> int:
        """0, or EMISSING_PAIR when an adjacent pair has fewer than 3 rows."""
        rc = lib().r360_rigcal_check(self.h)
        return rc if rc == EMISSING_PAIR else _check(rc, "rigcal_check")

    def loadPlaneCorrespondences(self, path: str):
        _check(lib().r360_rigcal_load_dir(self.h, path.encode()), "rigcal_load_dir")

    def savePlaneCorrespondences(self, path: str):
        _check(lib().r360_rigcal_save_dir(self.h, path.encode()), "rigcal_save_dir")

    def setInit(self, rt8):
        a = np.ascontiguousarray(np.asarray(rt8, np.float64).reshape(8, 4, 4).transpose(0, 2, 1)).reshape(128)
        _check(lib().r360_rigcal_set_init(self.h, _dptr(a)), "rigcal_set_init")

    def estimate(self) -> np.ndarray:
        a = np.zeros(128)
        _check(lib().r360_rigcal_get_estimate(self.h, _dptr(a)), "rigcal_get_estimate")
        return a.reshape(8, 4, 4).transpose(0, 2, 1).copy()

    def saveExtrinsics(self, path: str):
        _check(lib().r360_rigcal_save_extrinsics(self.h, path.encode()), "rigcal_save_extrinsics")

    def _solve(self, fn, what, weighted) -> "RigcalStats":
        st = RigcalStats()
        rc = fn(self.h, int(weighted), C.byref(st))
        if rc != EMISSING_PAIR:
            _check(rc, what)
        return st

    def CalibrateRotation(self, weighted: bool = False) -> "RigcalStats":
        return self._solve(lib().r360_rigcal_rotation, "rigcal_rotation", weighted)

    def CalibrateTranslation(self, weighted: bool = False) -> "RigcalStats":
        return self._solve(lib().r360_rigcal_translation, "rigcal_translation", weighted)

    def Calibrate(self):
        return self.CalibrateRotation(), self.CalibrateTranslation()

    def trimOutliersRANSAC(self, i: int, j: int, seed: int = 0, params: "RigcalTrimParams | None" = None):
        """r360_rigcal_trim: (stats, mask over the pair's former rows)."""
        p = params if params is not None else RigcalTrimParams.default()
        n = len(self.getPair(i, j))
        mask = np.ones(max(n, 1), np.uint8)
        st = RigcalTrimStats()
        _check(lib().r360_rigcal_trim(self.h, i, j, C.byref(p), seed, C.byref(st), _vptr(mask), n), "rigcal_trim")
        return st, mask[:n].astype(bool)

    def addFrame(self, frame: "Frame360", params: "RigcalCollectParams | None" = None) -> np.ndarray:
        """r360_rigcal_add_frame: the collector on a frame built with BUILD_LOCAL_PLANES; rows added per pair [28]."""
        p = params if params is not None else RigcalCollectParams.default()
        added = np.zeros(28, np.int32)
        _check(lib().r360_rigcal_add_frame(self.h, frame.h, C.byref(p), added.ctypes.data_as(_IP)), "rigcal_add_frame")
        return added

    def conditioning(self) -> np.ndarray:
        c = np.zeros(8, np.float32)
        _check(lib().r360_rigcal_conditioning(self.h, _fptr(c)), "rigcal_conditioning")
        return c

    def eval(self, mode: int, weighted: bool = False):
        """r360_rigcal_eval at the current estimate: (H [21, 21], g [21], scalars [4]); EMISSING_PAIR when it applies."""
        H, g, sc = np.zeros((21, 21)), np.zeros(21), np.zeros(4)
        rc = lib().r360_rigcal_eval(self.h, mode, int(weighted), _dptr(H), _dptr(g), _dptr(sc))
        if rc == EMISSING_PAIR:
            return rc
        _check(rc, "rigcal_eval")
        return H, g, sc

    def ransacEval(self, i: int, j: int, seed: int, trial0: int, n: int, params: "RigcalTrimParams | None" = None):
        """r360_rigcal_ransac_eval: (inlier counts [n], no-draw flags [n]) of trials trial0 .. trial0 + n - 1."""
        p = params if params is not None else RigcalTrimParams.default()
        counts, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().r360_rigcal_ransac_eval(self.h, i, j, C.byref(p), seed, trial0, n, counts.ctypes.data_as(_IP),
                                             flags.ctypes.data_as(_IP)), "rigcal_ransac_eval")
        return counts, flags


def _topo_matrix(A) -> np.ndarray:
    A = np.ascontiguousarray(A, np.float32)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("a square matrix is expected")
    return A


def topo_bisect(ctx: "Context", A):
    """r360_topo_bisect: one spectral bisection of the SSO graph A [n, n] ->
    dict(side [n] (1 / 2), cut, eigenvalues [n] ascending, fiedler [n], sweeps, converged)."""
    A = _topo_matrix(A)
    n = A.shape[0]
    side = np.zeros(max(n, 1), np.int32)
    ev, fv = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    cut, sweeps = C.c_double(), C.c_int()
    rc = _check(lib().r360_topo_bisect(ctx.h, _fptr(A), n, side.ctypes.data_as(_IP), C.byref(cut), _dptr(ev), _dptr(fv),
                                       C.byref(sweeps)), "topo_bisect")
    return dict(side=side[:n], cut=cut.value, eigenvalues=ev[:n], fiedler=fv[:n], sweeps=sweeps.value, converged=rc == 0)


def topo_partition(ctx: "Context", A, params: "TopoParams | None" = None, return_cuts: bool = False):
    """r360_topo_partition (RecursiveSpectralPartition, TopologicalMap360.h:411) -> part_of [n], the parts numbered by
    their first node; with return_cuts also the cut of every bisection (by the cluster's lowest node, larger first)."""
    A = _topo_matrix(A)
    n = A.shape[0]
    part = np.zeros(max(n, 1), np.int32)
    cuts = np.zeros(2 * max(n, 1))
    n_parts, n_bis = C.c_int(), C.c_int()
    _check(lib().r360_topo_partition(ctx.h, _fptr(A), n, None if params is None else C.byref(params),
                                     part.ctypes.data_as(_IP), C.byref(n_parts), _dptr(cuts), C.byref(n_bis)),
           "topo_partition")
    return (part[:n], cuts[:n_bis.value].copy()) if return_cuts else part[:n]


def topo_partition_batch(ctx: "Context", graphs, params: "TopoParams | None" = None):
    """r360_topo_partition_batch: every graph's part_of, all graphs' clusters of one recursion level in one launch."""
    mats = [_topo_matrix(A) for A in graphs]
    count = len(mats)
    ns = np.array([A.shape[0] for A in mats] or [0], np.int32)
    parts = [np.zeros(max(A.shape[0], 1), np.int32) for A in mats]
    ap = (_FP * max(count, 1))(*[_fptr(A) for A in mats])
    pp = (_IP * max(count, 1))(*[p.ctypes.data_as(_IP) for p in parts])
    n_parts = np.zeros(max(count, 1), np.int32)
    _check(lib().r360_topo_partition_batch(ctx.h, count, ap, ns.ctypes.data_as(_IP),
                                           None if params is None else C.byref(params), pp,
                                           n_parts.ctypes.data_as(_IP)), "topo_partition_batch")
    return [p[:A.shape[0]] for p, A in zip(parts, mats)]


class TopologicalMap:
    """The bookkeeping of Map360 + TopologicalMap360 (r360_topomap_*): keyframes with an area each, one SSO table, the
    current area; Partitioner() cuts the current area's vicinity on the GPU."""

    def __init__(self, ctx: "Context"):
        h = C.c_void_p()
        _check(lib().r360_topomap_create(ctx.h, C.byref(h)), "r360_topomap_create")
        self.h = h
        self.ctx = ctx

    def close(self):
        if self.h:
            lib().r360_topomap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def addKeyframe(self) -> int:
        kf = C.c_int()
        _check(lib().r360_topomap_add_keyframe(self.h, C.byref(kf)), "topomap_add_keyframe")
        return kf.value

    def dropLast(self):
        _check(lib().r360_topomap_drop_last(self.h), "topomap_drop_last")

    def addConnection(self, kf1: int, kf2: int, sso: float):
        _check(lib().r360_topomap_add_connection(self.h, kf1, kf2, sso), "topomap_add_connection")

    def getVicinitySSO(self):
        """(keyframe ids [n], SSO [n, n]) of the current area and its neighbours."""
        n = C.c_int()
        _check(lib().r360_topomap_vicinity(self.h, None, None, 0, C.byref(n)), "topomap_vicinity")
        ids, A = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1) ** 2, np.float32)
        _check(lib().r360_topomap_vicinity(self.h, ids.ctypes.data_as(_IP), _fptr(A), n.value, C.byref(n)),
               "topomap_vicinity")
        return ids[:n.value], A[:n.value * n.value].reshape(n.value, n.value)

    def Partitioner(self, params: "TopoParams | None" = None) -> int:
        """Returns the number of new areas."""
        k = C.c_int()
        _check(lib().r360_topomap_partition(self.h, None if params is None else C.byref(params), C.byref(k)),
               "topomap_partition")
        return k.value

    def areas(self):
        """(area_of [n_kf], n_areas, current_area)."""
        n, na, cur = C.c_int(), C.c_int(), C.c_int()
        _check(lib().r360_topomap_areas(self.h, None, 0, C.byref(n), C.byref(na), C.byref(cur)), "topomap_areas")
        a = np.zeros(max(n.value, 1), np.int32)
        _check(lib().r360_topomap_areas(self.h, a.ctypes.data_as(_IP), n.value, C.byref(n), C.byref(na), C.byref(cur)),
               "topomap_areas")
        return a[:n.value], na.value, cur.value

    def neighbors(self, area: int) -> list:
        n = C.c_int()
        _check(lib().r360_topomap_neighbors(self.h, area, None, 0, C.byref(n)), "topomap_neighbors")
        out = np.zeros(max(n.value, 1), np.int32)
        _check(lib().r360_topomap_neighbors(self.h, area, out.ctypes.data_as(_IP), n.value, C.byref(n)),
               "topomap_neighbors")
        return [int(v) for v in out[:n.value]]

    def selected(self, area: int) -> int:
        kf = C.c_int()
        _check(lib().r360_topomap_selected(self.h, area, C.byref(kf)), "topomap_selected")
        return kf.value


class Relocalizer:
    """Relocalizer360 (include/Relocalizer360.h:43-94) over r360_relocalize: the newest keyframe that registers with
    the frame by PbMap under PLANAR_3DoF with enough matched planes and area."""

    def __init__(self, batch: "Batch", max_match_planes: int = 25, min_matches: int = 5, min_area: float = 10.0):
        self.batch = batch
        self.max_match_planes, self.min_matches, self.min_area = max_match_planes, min_matches, min_area
        self.relocKF = -1
        self.rigidTransf = np.eye(4)
        self.informationM = np.zeros((6, 6))

    def relocalize(self, keyframes, frame) -> int:
        kfs = list(keyframes)
        ptrs = (C.c_void_p * max(1, len(kfs)))(*[k.h.value for k in kfs])
        pose, info = np.zeros(16), np.zeros(36)
        kf = C.c_int()
        _check(lib().r360_relocalize(self.batch.h, ptrs, len(kfs), frame.h, self.max_match_planes, self.min_matches,
                                     self.min_area, C.byref(kf), _dptr(pose), _dptr(info)), "r360_relocalize")
        if kf.value >= 0:
            self.relocKF = kf.value
            self.rigidTransf = _from16(pose)
            self.informationM = info.reshape(6, 6).T.copy()
        return kf.value
