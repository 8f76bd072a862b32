"""ctypes wrapper of oracle/liboracle360.so — the CPU ORACLE.

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg, as the checker / CPU baseline.  The product (rgbd360_amd) never imports this module.

Parity status: the reference cannot be compiled or imported here.  The parts
restating vendored reference code (.bin reader, CLAMS, stitching, RegisterPhotoICP arithmetic) follow
the cited file:line expression by expression; OpenCV's cvtColor/pyrDown rounding and all PCL/MRPT
pieces are restated from their published algorithms — **parity unpinned** at those boundaries.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "liboracle360.so")

PHOTO, DEPTH, PHOTO_DEPTH = 0, 1, 2


class IcpParams(C.Structure):
    _fields_ = [
        ("n_pyr", C.c_int), ("max_iters", C.c_int), ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("std_dev_photo", C.c_float), ("std_dev_depth", C.c_float), ("thres_sal_int", C.c_float),
        ("thres_sal_depth", C.c_float), ("tol_residual", C.c_double), ("tol_update", C.c_double),
        ("lambda_", C.c_double), ("fixed_iters_level0", C.c_int),
    ]

    @classmethod
    def default(cls, n_pyr=4, std_dev_photo=6.0 / 255, fixed_iters_level0=0):
        return cls(n_pyr, 10, 0.3, 6.0, np.float32(std_dev_photo), 0.2, 0.01, 0.01, 1e-3, 1e-4, 1.0,
                   fixed_iters_level0)


class IcpStats(C.Structure):
    _fields_ = [("iters", C.c_int * 8), ("evals", C.c_int * 8), ("illposed", C.c_int), ("sso", C.c_float),
                ("error", C.c_double), ("av_photo_residual", C.c_double), ("av_depth_residual", C.c_double),
                ("av_residual", C.c_float), ("residuals_set", C.c_int)]


class DenseStats(C.Structure):
    _fields_ = [("error", C.c_double * 8), ("ran", C.c_int * 8), ("iters", C.c_int * 8), ("illposed_level", C.c_int),
                ("info_set", C.c_int), ("gradient", C.c_float * 6)]


class Level(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int)] + [
        (n, C.POINTER(C.c_float)) for n in ("gray_src", "depth_src", "gray_trg", "depth_trg", "gx", "gy", "dgx", "dgy")]


class Pinhole(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("ox", C.c_float), ("oy", C.c_float)]

    @classmethod
    def rgbd360(cls, rows: int, cols: int):
        """MethodsRegisterRGBD360.cpp:323-330: f = 525*w/640, c = (w/2 - 0.5, h/2 - 0.5), float."""
        f = np.float32(525) * (np.float32(cols) / np.float32(640.0))
        return cls(f, f, np.float32(cols) / 2 - np.float32(0.5), np.float32(rows) / 2 - np.float32(0.5))


class Region(C.Structure):
    _fields_ = [("label", C.c_int), ("count", C.c_int), ("start_idx", C.c_int), ("n_contour", C.c_int),
                ("contour_off", C.c_int), ("centroid", C.c_float * 3), ("cov", C.c_float * 9),
                ("model", C.c_float * 4), ("curvature", C.c_float)]


class Plane(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("center", C.c_float * 3), ("d", C.c_float), ("area", C.c_float),
                ("elongation", C.c_float), ("curvature", C.c_float), ("ppal", C.c_float * 3), ("nrgb", C.c_float * 3),
                ("intensity", C.c_float), ("id", C.c_int), ("sensor", C.c_int), ("n_inliers", C.c_int),
                ("n_hull", C.c_int)]


_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        L = C.CDLL(LIB)
        fp, dp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
        sig = {
            "orc_bin_dims": (C.c_int, [C.c_char_p, ip, ip]),
            "orc_bin_load": (C.c_int, [C.c_char_p, vp, vp]),
            "orc_bin_write": (C.c_int, [C.c_char_p, vp, vp, C.c_int, C.c_int]),
            "orc_clams_load": (vp, [C.c_char_p]),
            "orc_clams_free": (None, [vp]),
            "orc_clams_undistort": (None, [vp, vp, C.c_int, C.c_int]),
            "orc_clams_export": (C.c_int, [vp, ip, fp, fp]),
            "orc_stitch": (None, [vp, vp, C.c_int, C.c_int, fp, fp, vp, vp]),
            "orc_rgb2gray": (None, [vp, C.c_int, fp]),
            "orc_depth_to_m": (None, [vp, C.c_int, fp]),
            "orc_pyrdown": (None, [fp, C.c_int, C.c_int, fp]),
            "orc_pyr_range": (None, [fp, C.c_int, C.c_int, C.c_float, C.c_float, fp]),
            "orc_gradient": (None, [fp, C.c_int, C.c_int, fp, fp]),
            "orc_error_sphere": (C.c_double, [C.POINTER(Level), fp, C.c_int, C.POINTER(IcpParams), ip, dp]),
            "orc_hessgrad_sphere": (None, [C.POINTER(Level), fp, C.c_int, C.POINTER(IcpParams), dp, dp, ip]),
            "orc_align360": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, fp, C.c_int, C.POINTER(IcpParams), fp,
                                       fp, fp, C.POINTER(IcpStats)]),
            "orc_align360_occ": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, fp, C.c_int, C.c_int,
                                           C.POINTER(IcpParams), fp, fp, fp, C.POINTER(IcpStats)]),
            "orc_error_sphere_occ": (C.c_double, [C.POINTER(Level), fp, C.c_int, C.c_int, C.POINTER(IcpParams), ip]),
            "orc_hessgrad_sphere_occ": (None, [C.POINTER(Level), fp, C.c_int, C.c_int, C.POINTER(IcpParams), dp, dp,
                                               ip]),
            "orc_error_pinhole": (C.c_double, [C.POINTER(Level), C.POINTER(Pinhole), C.c_int, fp, C.c_int,
                                               C.POINTER(IcpParams), ip, ip, dp, dp]),
            "orc_hessgrad_pinhole": (None, [C.POINTER(Level), C.POINTER(Pinhole), C.c_int, fp, C.c_int,
                                            C.POINTER(IcpParams), dp, dp, ip]),
            "orc_align_pinhole": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(Pinhole), fp, C.c_int,
                                            C.POINTER(IcpParams), fp, fp, fp, C.POINTER(IcpStats)]),
            "orc_error_robot": (C.c_double, [C.POINTER(Level), C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_int,
                                             C.POINTER(IcpParams), dp, dp, ip]),
            "orc_hessgrad_robot": (None, [C.POINTER(Level), C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_int,
                                          C.POINTER(IcpParams), fp, fp, dp, dp, ip]),
            "orc_register_dense_robot": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, fp, fp, fp, C.c_int,
                                                   C.POINTER(IcpParams), fp, fp, C.POINTER(DenseStats)]),
            "orc_exp_se3": (None, [dp, C.c_int, fp]),
            "orc_rank6f": (C.c_int, [fp]),
            "orc_solve6": (C.c_int, [dp, dp, dp]),
            "orc_huber": (C.c_float, [C.c_float, C.c_float]),
            "orc_libm": (None, [fp, fp, fp, C.c_int, fp, fp]),
            "orc_cloud_downsample": (None, [fp, vp, C.c_int, C.c_int, fp, vp]),
            "orc_bilateral": (None, [fp, C.c_int, C.c_int]),
            "orc_normals": (None, [fp, C.c_int, C.c_int, fp, fp]),
            "orc_segment": (C.c_int, [fp, fp, C.c_int, C.c_int, ip, ip, C.POINTER(Region), C.c_int, ip, C.c_int]),
            "orc_pbmap_build": (vp, [fp, vp, C.c_int, C.c_int, fp]),
            "orc_pbmap_from_planes": (vp, [C.POINTER(Plane), C.c_int]),
            "orc_pbmap_free": (None, [vp]),
            "orc_pbmap_count": (C.c_int, [vp]),
            "orc_pbmap_get": (C.c_int, [vp, C.c_int, C.POINTER(Plane), fp, C.c_int]),
            "orc_match_tables": (C.c_int, [vp, vp, C.c_size_t, C.c_int, ip, ip, ip, ip, vp, vp, C.c_int, vp]),
            "orc_register_pbmap": (C.c_int, [vp, vp, C.c_size_t, C.c_int, fp, fp, ip, C.c_int, ip, fp, fp, fp, vp]),
            "orc_last_match_stats": (None, [C.POINTER(C.c_long), ip]),
            "orc_tree_search": (C.c_int, [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_long, ip, C.POINTER(C.c_long)]),
        }
        for k, (r, a) in sig.items():
            f = getattr(L, k)
            f.restype, f.argtypes = r, a
        _lib = L
    return _lib


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _v(a):
    return C.c_void_p(a.ctypes.data)


def mat16(m) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(m, np.float32).T).reshape(16).copy()


def from16(a) -> np.ndarray:
    return np.asarray(a, np.float32).reshape(4, 4).T.copy()


# ---------------------------------------------------------------- A1 / A2 / A10
def load_bin(path: str):
    r, c = C.c_int(), C.c_int()
    if lib().orc_bin_dims(path.encode(), C.byref(r), C.byref(c)):
        raise IOError(path)
    bgr = np.zeros((8, r.value, c.value, 3), np.uint8)
    dep = np.zeros((8, r.value, c.value), np.uint16)
    rc = lib().orc_bin_load(path.encode(), _v(bgr), _v(dep))
    if rc:
        raise IOError(f"{path}: {rc}")
    return bgr, dep


def write_bin(path: str, bgr, dep):
    bgr = np.ascontiguousarray(bgr, np.uint8)
    dep = np.ascontiguousarray(dep, np.uint16)
    assert lib().orc_bin_write(path.encode(), _v(bgr), _v(dep), dep.shape[1], dep.shape[2]) == 0


def read_extrinsics(dirpath: str) -> np.ndarray:
    """Rt_0{1..8}.txt (Calib360.h:122-131) as (8,4,4) float32; Rt_inv via float64 inverse."""
    return np.stack([np.loadtxt(os.path.join(dirpath, f"Rt_0{k + 1}.txt")).reshape(4, 4) for k in range(8)]
                    ).astype(np.float32)


def camera_matrix(rows: int, cols: int) -> np.ndarray:
    f = np.float32(525 * np.float32(cols / 640.0))
    return np.array([[f, 0, cols // 2 - 0.5], [0, f, rows // 2 - 0.5], [0, 0, 1]], np.float32)


class Clams:
    def __init__(self, path: str):
        self.h = lib().orc_clams_load(path.encode())
        if not self.h:
            raise IOError(path)

    def undistort(self, depth_m: np.ndarray) -> np.ndarray:
        d = np.ascontiguousarray(depth_m, np.float32).copy()
        lib().orc_clams_undistort(self.h, _v(d), d.shape[0], d.shape[1])
        return d

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_clams_free(self.h)


def depth_to_m(d: np.ndarray) -> np.ndarray:
    d = np.ascontiguousarray(d, np.uint16)
    out = np.zeros(d.shape, np.float32)
    lib().orc_depth_to_m(_v(d), d.size, _f(out))
    return out


def stitch(bgr8, dep8, rt_inv8: np.ndarray, K: np.ndarray):
    """rt_inv8: column-major (8*16,) float32 as the product stores it; K: 3x3."""
    bgr8 = np.ascontiguousarray(bgr8, np.uint8)
    dep8 = np.ascontiguousarray(dep8, np.uint16)
    rows, cols = dep8.shape[1], dep8.shape[2]
    W = rows * 8
    H = int(W * 0.5 * 60.0 / 180)
    sb = np.zeros((H, W, 3), np.uint8)
    sd = np.zeros((H, W), np.uint16)
    Kc = np.ascontiguousarray(np.asarray(K, np.float32).T).reshape(9).copy()
    rti = np.ascontiguousarray(rt_inv8, np.float32)
    lib().orc_stitch(_v(bgr8), _v(dep8), rows, cols, _f(rti), _f(Kc), _v(sb), _v(sd))
    return sb, sd


# ---------------------------------------------------------------- A14
def rgb2gray(bgr: np.ndarray) -> np.ndarray:
    bgr = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros(bgr.shape[:-1], np.float32)
    lib().orc_rgb2gray(_v(bgr), out.size, _f(out))
    return out


def pyrdown(img: np.ndarray) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    out = np.zeros((img.shape[0] // 2, img.shape[1] // 2), np.float32)
    lib().orc_pyrdown(_f(img), img.shape[0], img.shape[1], _f(out))
    return out


def pyr_range(img: np.ndarray, min_d=0.3, max_d=6.0) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    out = np.zeros((img.shape[0] // 2, img.shape[1] // 2), np.float32)
    lib().orc_pyr_range(_f(img), img.shape[0], img.shape[1], min_d, max_d, _f(out))
    return out


def gradient(img: np.ndarray):
    img = np.ascontiguousarray(img, np.float32)
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    lib().orc_gradient(_f(img), img.shape[0], img.shape[1], _f(gx), _f(gy))
    return gx, gy


def seam_mask(g: np.ndarray) -> np.ndarray:
    """alignFrames360 seam masking (RegisterPhotoICP.h:4538-4549)."""
    g = g.copy()
    ws = g.shape[1] // 8
    for s in range(1, 8):
        g[:, s * ws - 1:s * ws + 1] = 0
    return g


def sphere_pyramid(sph_bgr, sph_depth, n_levels: int, mask: bool = True):
    """setSourceFrame/setTargetFrame pyramids (:480-516) + seam masks, per level dicts."""
    gray = rgb2gray(sph_bgr)
    dep = depth_to_m(sph_depth)
    levels = []
    for l in range(n_levels):
        if l:
            gray, dep = pyrdown(gray), pyr_range(dep)
        gx, gy = gradient(gray)
        dgx, dgy = gradient(dep)
        if mask:
            gx, gy, dgx, dgy = map(seam_mask, (gx, gy, dgx, dgy))
        levels.append(dict(gray=gray, depth=dep, gx=gx, gy=gy, dgx=dgx, dgy=dgy))
    return levels


def _level_struct(src: dict, trg: dict):
    arrs = [np.ascontiguousarray(a, np.float32) for a in
            (src["gray"], src["depth"], trg["gray"], trg["depth"], trg["gx"], trg["gy"], trg["dgx"], trg["dgy"])]
    L = Level(arrs[0].shape[0], arrs[0].shape[1], *[_f(a) for a in arrs])
    return L, arrs


def error_sphere(src: dict, trg: dict, pose, method=PHOTO_DEPTH, params: IcpParams | None = None):
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    nv, e2 = C.c_int(), C.c_double()
    e = lib().orc_error_sphere(C.byref(L), _f(mat16(pose)), method, C.byref(p), C.byref(nv), C.byref(e2))
    return e, e2.value, nv.value


def hessgrad_sphere(src: dict, trg: dict, pose, method=PHOTO_DEPTH, params: IcpParams | None = None):
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    H, g, nvis = np.zeros(36), np.zeros(6), C.c_int()
    lib().orc_hessgrad_sphere(C.byref(L), _f(mat16(pose)), method, C.byref(p),
                              H.ctypes.data_as(C.POINTER(C.c_double)), g.ctypes.data_as(C.POINTER(C.c_double)),
                              C.byref(nvis))
    return H.reshape(6, 6), g, nvis.value


def error_sphere_occ(src: dict, trg: dict, pose, method=PHOTO_DEPTH, occlusion=1,
                     params: IcpParams | None = None):
    """errorPhotoICP_sphereOcc{1,2} (occlusion 0 = errorPhotoICP_sphere): (error, n_valid)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    nv = C.c_int()
    e = lib().orc_error_sphere_occ(C.byref(L), _f(mat16(pose)), method, occlusion, C.byref(p), C.byref(nv))
    return e, nv.value


def hessgrad_sphere_occ(src: dict, trg: dict, pose, method=PHOTO_DEPTH, occlusion=2,
                        params: IcpParams | None = None):
    """calcHessGrad_sphereOcc2 (occlusion 0 / 1 = calcHessGrad_sphere): (H, g, n_visible)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    H, g, nvis = np.zeros(36), np.zeros(6), C.c_int()
    lib().orc_hessgrad_sphere_occ(C.byref(L), _f(mat16(pose)), method, occlusion, C.byref(p),
                                  H.ctypes.data_as(C.POINTER(C.c_double)), g.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.byref(nvis))
    return H.reshape(6, 6), g, nvis.value


def align360(trg_bgr, trg_dep, src_bgr, src_dep, init=None, method=PHOTO_DEPTH, params: IcpParams | None = None,
             occlusion=0):
    trg_bgr, trg_dep, src_bgr, src_dep = [np.ascontiguousarray(a) for a in (trg_bgr, trg_dep, src_bgr, src_dep)]
    p = params or IcpParams.default()
    init16 = mat16(np.eye(4) if init is None else init)
    po, Ho, go = np.zeros(16, np.float32), np.zeros(36, np.float32), np.zeros(6, np.float32)
    st = IcpStats()
    rc = lib().orc_align360_occ(_v(trg_bgr), _v(trg_dep), _v(src_bgr), _v(src_dep), src_dep.shape[0],
                                src_dep.shape[1], _f(init16), method, occlusion, C.byref(p), _f(po), _f(Ho), _f(go),
                                C.byref(st))
    return rc, from16(po), Ho.reshape(6, 6).T.copy(), go, st


# ---------------------------------------------------------------- §8(f)3 pinhole per-sensor path
def sensor_pyramid(bgr, dep, n_levels: int):
    """setTargetFrame / setSourceFrame (:480-516) on one sensor's raw images: no seam mask."""
    return sphere_pyramid(bgr, dep, n_levels, mask=False)


def error_pinhole(src: dict, trg: dict, K: Pinhole, level: int, pose, method=PHOTO_DEPTH,
                  params: IcpParams | None = None):
    """errorPhotoICP (:560-761) -> (avResidual, n_photo, n_depth, photo_sum, depth_sum)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    nP, nD, rP, rD = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    e = lib().orc_error_pinhole(C.byref(L), C.byref(K), level, _f(mat16(pose)), method, C.byref(p), C.byref(nP),
                                C.byref(nD), C.byref(rP), C.byref(rD))
    return e, nP.value, nD.value, rP.value, rD.value


def hessgrad_pinhole(src: dict, trg: dict, K: Pinhole, level: int, pose, method=PHOTO_DEPTH,
                     params: IcpParams | None = None):
    """calcHessGrad (:767-1100) -> (H, g, n_visible)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    H, g, nvis = np.zeros(36), np.zeros(6), C.c_int()
    lib().orc_hessgrad_pinhole(C.byref(L), C.byref(K), level, _f(mat16(pose)), method, C.byref(p),
                               H.ctypes.data_as(C.POINTER(C.c_double)), g.ctypes.data_as(C.POINTER(C.c_double)),
                               C.byref(nvis))
    return H.reshape(6, 6), g, nvis.value


def align_pinhole(trg_bgr, trg_dep, src_bgr, src_dep, K: Pinhole | None = None, init=None, method=PHOTO_DEPTH,
                  params: IcpParams | None = None):
    """alignFrames (:4254-4512) on one sensor -> (rc, pose, H, g, stats)."""
    trg_bgr, trg_dep, src_bgr, src_dep = [np.ascontiguousarray(a) for a in (trg_bgr, trg_dep, src_bgr, src_dep)]
    rows, cols = src_dep.shape
    K = K or Pinhole.rgbd360(rows, cols)
    p = params or IcpParams.default()
    init16 = mat16(np.eye(4) if init is None else init)
    po, Ho, go = np.zeros(16, np.float32), np.zeros(36, np.float32), np.zeros(6, np.float32)
    st = IcpStats()
    rc = lib().orc_align_pinhole(_v(trg_bgr), _v(trg_dep), _v(src_bgr), _v(src_dep), rows, cols, C.byref(K),
                                 _f(init16), method, C.byref(p), _f(po), _f(Ho), _f(go), C.byref(st))
    return rc, from16(po), Ho.reshape(6, 6).T.copy(), go, st


# ---------------------------------------------------------------- A19 RegisterDensePhotoICP (robot frame)
def error_robot(src: dict, trg: dict, rows0: int, cols0: int, level: int, pose, rt, rt_inv, method=PHOTO,
                params: IcpParams | None = None):
    """calcPhotoICPError_robot (:4905-5076) of one sensor -> (error2, photo_sum, depth_sum, n_visible, n_depth)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    eP, eD, cnt = C.c_double(), C.c_double(), np.zeros(2, np.int32)
    e = lib().orc_error_robot(C.byref(L), rows0, cols0, level, _f(mat16(pose)), _f(mat16(rt)), _f(mat16(rt_inv)),
                              method, C.byref(p), C.byref(eP), C.byref(eD), cnt.ctypes.data_as(C.POINTER(C.c_int)))
    return e, eP.value, eD.value, int(cnt[0]), int(cnt[1])


def hessgrad_robot(src: dict, trg: dict, rows0: int, cols0: int, level: int, pose, rt, rt_inv,
                   method=PHOTO, params: IcpParams | None = None):
    """calcHessianGradient_robot (:5083-5407) of one sensor -> (Hf, gf (float, raster order, the reference's),
    Hd, gd (the same terms summed in double), n_visible)."""
    L, keep = _level_struct(src, trg)
    p = params or IcpParams.default()
    Hf, gf, Hd, gd, nv = np.zeros(36, np.float32), np.zeros(6, np.float32), np.zeros(36), np.zeros(6), C.c_int()
    dp = C.POINTER(C.c_double)
    lib().orc_hessgrad_robot(C.byref(L), rows0, cols0, level, _f(mat16(pose)), _f(mat16(rt)), _f(mat16(rt_inv)),
                             method, C.byref(p), _f(Hf), _f(gf), Hd.ctypes.data_as(dp), gd.ctypes.data_as(dp),
                             C.byref(nv))
    return Hf.reshape(6, 6), gf, Hd.reshape(6, 6), gd, nv.value


def register_dense_robot(bgr1, dep1, bgr2, dep2, rt8, rt_inv8, init=None, method=PHOTO,
                         params: IcpParams | None = None):
    """RegisterDensePhotoICP(frame1, frame2, pose_estim, method) (RegisterRGBD360.h:344-520).
    rt8 / rt_inv8: [8,4,4].  Returns (ok, pose, informationM, DenseStats)."""
    bgr1, dep1, bgr2, dep2 = [np.ascontiguousarray(a) for a in (bgr1, dep1, bgr2, dep2)]
    rows, cols = dep1.shape[1], dep1.shape[2]
    p = params or IcpParams.default()
    r8 = np.concatenate([mat16(m) for m in rt8]).astype(np.float32)
    ri8 = np.concatenate([mat16(m) for m in rt_inv8]).astype(np.float32)
    init16 = mat16(np.eye(4) if init is None else init)
    po, info = np.zeros(16, np.float32), np.zeros(36, np.float32)
    st = DenseStats()
    ok = lib().orc_register_dense_robot(_v(bgr1), _v(dep1), _v(bgr2), _v(dep2), rows, cols, _f(r8), _f(ri8),
                                        _f(init16), method, C.byref(p), _f(po), _f(info), C.byref(st))
    return ok == 1, from16(po), info.reshape(6, 6).T.copy(), st


def exp_se3(mu, pseudo=True) -> np.ndarray:
    m = np.asarray(mu, np.float64)
    T = np.zeros(16, np.float32)
    lib().orc_exp_se3(m.ctypes.data_as(C.POINTER(C.c_double)), int(pseudo), _f(T))
    return from16(T)


def rank6f(M) -> int:
    """Eigen FullPivLU<Matrix<float,6,6>>::rank() of M (the alignFrames360 ILL-POSED test, :4682)."""
    m = np.ascontiguousarray(np.asarray(M, np.float32).reshape(6, 6))
    return int(lib().orc_rank6f(_f(m)))


def solve6(H, g):
    """x = -H^-1 g by the GN step's Gaussian elimination with partial pivoting (double, :4693); None where a pivot is
    exactly 0 (unreachable in alignFrames360: the rank test returns ILL-POSED first)."""
    h = np.ascontiguousarray(np.asarray(H, np.float64).reshape(36))
    gg = np.ascontiguousarray(np.asarray(g, np.float64).reshape(6))
    x = np.zeros(6, np.float64)
    dp_ = C.POINTER(C.c_double)
    ok = lib().orc_solve6(h.ctypes.data_as(dp_), gg.ctypes.data_as(dp_), x.ctypes.data_as(dp_))
    return x if ok else None


def libm(x, y, z):
    x, y, z = (np.ascontiguousarray(a, np.float32) for a in (x, y, z))
    a, t = np.zeros_like(x), np.zeros_like(x)
    lib().orc_libm(_f(x), _f(y), _f(z), x.size, _f(a), _f(t))
    return a, t


def huber(e: float, reg: float) -> float:
    return lib().orc_huber(e, reg)


def rot_angle(Ra, Rb) -> float:
    """Angle (rad) of Ra Rb^T — the angularDistance of diffRotation (Miscellaneous.h:127-139)."""
    R = np.asarray(Ra, np.float64)[:3, :3] @ np.asarray(Rb, np.float64)[:3, :3].T
    c = (np.trace(R) - 1) / 2
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(s, c))  # well conditioned near 0, unlike arccos


# ---------------------------------------------------------------- plane half: per-pixel stages
def cloud_downsample(depth_m: np.ndarray, bgr: np.ndarray):
    """A3 for one sensor: (rows, cols) metres + (rows, cols, 3) BGR -> xyz4 (h, w, 4) f32, rgb4 u8."""
    rows, cols = depth_m.shape
    d = np.ascontiguousarray(depth_m, np.float32)
    b = np.ascontiguousarray(bgr, np.uint8)
    xyz = np.zeros((rows // 2, cols // 2, 4), np.float32)
    rgb = np.zeros((rows // 2, cols // 2, 4), np.uint8)
    lib().orc_cloud_downsample(_f(d), _v(b), rows, cols, _f(xyz), _v(rgb))
    return xyz, rgb


def bilateral(xyz4: np.ndarray) -> np.ndarray:
    """A4: returns a filtered copy (only z changes)."""
    out = np.ascontiguousarray(xyz4, np.float32).copy()
    h, w = out.shape[:2]
    lib().orc_bilateral(_f(out), w, h)
    return out


def normals(xyz4: np.ndarray):
    """A6: -> (nrm4 (h, w, 4), distance map (h, w))."""
    x = np.ascontiguousarray(xyz4, np.float32)
    h, w = x.shape[:2]
    n = np.zeros((h, w, 4), np.float32)
    dm = np.zeros((h, w), np.float32)
    lib().orc_normals(_f(x), w, h, _f(n), _f(dm))
    return n, dm


def segment(xyz4: np.ndarray, nrm4: np.ndarray, max_regions: int = 512):
    """A7: -> (labels_ccl, labels_final, [region dicts with 'contour' index arrays])."""
    x = np.ascontiguousarray(xyz4, np.float32)
    n = np.ascontiguousarray(nrm4, np.float32)
    h, w = x.shape[:2]
    lc = np.zeros((h, w), np.int32)
    lf = np.zeros((h, w), np.int32)
    regs = (Region * max_regions)()
    cap = 64 * w * h
    cont = np.zeros(cap, np.int32)
    ip = C.POINTER(C.c_int)
    nr = lib().orc_segment(_f(x), _f(n), w, h, lc.ctypes.data_as(ip), lf.ctypes.data_as(ip), regs, max_regions,
                           cont.ctypes.data_as(ip), cap)
    if nr < 0:
        raise RuntimeError("orc_segment: capacity exceeded")
    out = []
    for r in regs[:nr]:
        out.append(dict(label=r.label, count=r.count, start_idx=r.start_idx, centroid=np.array(r.centroid[:]),
                        cov=np.array(r.cov[:]).reshape(3, 3), model=np.array(r.model[:]), curvature=r.curvature,
                        contour=cont[r.contour_off:r.contour_off + r.n_contour].copy()))
    return lc, lf, out


# ---------------------------------------------------------------- plane half: PbMap + registration
DEFAULT_6DoF, PLANAR_3DoF, ODOMETRY_6DoF, PLANAR_ODOMETRY_3DoF = 0, 1, 2, 3


def plane_dict(p: Plane, hull: np.ndarray) -> dict:
    return dict(normal=np.array(p.normal[:]), center=np.array(p.center[:]), d=p.d, area=p.area,
                elongation=p.elongation, curvature=p.curvature, ppal=np.array(p.ppal[:]), nrgb=np.array(p.nrgb[:]),
                intensity=p.intensity, id=p.id, sensor=p.sensor, n_inliers=p.n_inliers, hull=hull)


class PbMap:
    """Plane half of one frame (A3-A9): depth_m8 (8, rows, cols) undistorted metres, bgr8 (8, rows, cols, 3),
    rt8 (8, 4, 4) extrinsics."""

    def __init__(self, depth_m8, bgr8, rt8):
        d = np.ascontiguousarray(depth_m8, np.float32)
        b = np.ascontiguousarray(bgr8, np.uint8)
        rt = np.ascontiguousarray(np.stack([mat16(m) for m in rt8]), np.float32)
        self.h = lib().orc_pbmap_build(_f(d), _v(b), d.shape[1], d.shape[2], _f(rt))
        if not self.h:
            raise RuntimeError("orc_pbmap_build failed")

    @classmethod
    def from_planes(cls, planes) -> "PbMap":
        """A crafted map: dicts with normal, center, d, area, elongation, curvature, nrgb, intensity and optionally
        ppal, id (default: the position), sensor, n_inliers.  No hull, no moments: for the matcher and the pose."""
        arr = (Plane * max(1, len(planes)))()
        for i, (a, p) in enumerate(zip(arr, planes)):
            a.normal[:] = [float(v) for v in p["normal"]]
            a.center[:] = [float(v) for v in p["center"]]
            a.ppal[:] = [float(v) for v in p.get("ppal", (0, 0, 0))]
            a.nrgb[:] = [float(v) for v in p["nrgb"]]
            a.d, a.area, a.elongation, a.curvature = p["d"], p["area"], p["elongation"], p["curvature"]
            a.intensity = p["intensity"]
            a.id, a.sensor, a.n_inliers = int(p.get("id", i)), int(p.get("sensor", 0)), int(p.get("n_inliers", 1))
        self = cls.__new__(cls)
        self.h = lib().orc_pbmap_from_planes(arr, len(planes))
        if not self.h:
            raise ValueError("plane ids are not 0..n-1")
        return self

    def __len__(self):
        return lib().orc_pbmap_count(self.h)

    def planes(self) -> list[dict]:
        out = []
        for i in range(len(self)):
            p = Plane()
            hull = np.zeros((4096, 3), np.float32)
            lib().orc_pbmap_get(self.h, i, C.byref(p), _f(hull), 4096)
            out.append(plane_dict(p, hull[:p.n_hull].copy()))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_pbmap_free(self.h)
            self.h = None


class MatchParams(C.Structure):
    """orc_match_params: SubgraphMatcher thresholds (the mrpt-pbmap ini keys, angles in degrees)."""
    _fields_ = [("min_planes_recognition", C.c_int), ("dist_d", C.c_float), ("angle", C.c_float),
                ("color_threshold", C.c_float), ("intensity_threshold", C.c_float),
                ("elongation_threshold", C.c_float), ("area_threshold", C.c_float), ("dist_threshold", C.c_float),
                ("angle_threshold", C.c_float), ("height_threshold", C.c_float), ("cos_angle_parallel", C.c_float),
                ("planar_normal_angle", C.c_float), ("max_nodes", C.c_long)]

    @classmethod
    def odometry_default(cls) -> "MatchParams":
        """config_files/configLocaliser_sphericalOdometry.ini"""
        return cls(3, 0.5, 50.0, 0.07, 100.0, 2.5, 3.0, 3.0, 10.0, 0.33, 0.985, 10.0, 4000000)


def load_match_ini(path, base: "MatchParams | None" = None) -> MatchParams:
    """mrpt-pbmap config_heuristics::load_params: the [global]/[unary]/[binary] keys the matcher uses
    (INI 'key=value', '//' and '%' comments); keys absent from the file keep base's values."""
    m = MatchParams.odometry_default() if base is None else base
    keys = {("global", "min_planes_recognition"): int, ("unary", "dist_d"): float, ("unary", "angle"): float,
            ("unary", "color_threshold"): float, ("unary", "intensity_threshold"): float,
            ("unary", "elongation_threshold"): float, ("unary", "area_threshold"): float,
            ("binary", "dist_threshold"): float, ("binary", "angle_threshold"): float,
            ("binary", "height_threshold"): float, ("binary", "cos_angle_parallel"): float}
    sec = ""
    for raw in open(path):
        line = raw.split("//")[0].split("%")[0].strip()
        if not line:
            continue
        if line.startswith("["):
            sec = line[1:line.index("]")].strip()
            continue
        if "=" not in line:
            continue
        k, v = (x.strip() for x in line.split("=", 1))
        if (sec, k) in keys:
            setattr(m, k, keys[(sec, k)](float(v)))
    return m


def match_tables(ref: PbMap, trg: PbMap, max_match_planes=25, mode=PLANAR_3DoF, cap=128, params=None):
    ns, nt = C.c_int(), C.c_int()
    sid = np.zeros(cap, np.int32)
    tid = np.zeros(cap, np.int32)
    un = np.zeros(cap * cap, np.uint8)
    words = (cap * cap + 63) // 64
    bi = np.zeros(cap * cap * words, np.uint64)
    ip = C.POINTER(C.c_int)
    w = lib().orc_match_tables(ref.h, trg.h, max_match_planes, mode, C.byref(ns), C.byref(nt), sid.ctypes.data_as(ip),
                               tid.ctypes.data_as(ip), _v(un), _v(bi), cap,
                               C.byref(params) if params is not None else None)
    n, m = ns.value, nt.value
    return dict(sid=sid[:n].copy(), tid=tid[:m].copy(), unary=un[:n * m].reshape(n, m).copy(),
                binary=bi[:n * m * w].reshape(n * m, w).copy(), words=w)


def tree_search(unary: np.ndarray, binary: np.ndarray, area, max_nodes: int = 4000000):
    """The oracle's interpretation tree alone: (best [ns], nodes, truncated)."""
    unary = np.ascontiguousarray(unary, np.uint8)
    ns, nt = unary.shape
    words = (ns * nt + 63) // 64
    binary = np.ascontiguousarray(binary, np.uint64).reshape(-1)
    area = np.ascontiguousarray(area, np.float64)
    best = np.zeros(max(ns, 1), np.int32)
    nodes = C.c_long()
    rc = lib().orc_tree_search(ns, nt, unary.ctypes.data, binary.ctypes.data, words, area.ctypes.data, max_nodes,
                               best.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nodes))
    return best[:ns], nodes.value, bool(rc)


def register_pbmap(ref: PbMap, trg: PbMap, max_match_planes=25, mode=PLANAR_3DoF, params=None):
    pose = np.zeros(16, np.float32)
    info = np.zeros(36, np.float32)
    pairs = np.zeros(2 * 256, np.int32)
    n, am, as_, at = C.c_int(), C.c_float(), C.c_float(), C.c_float()
    ip = C.POINTER(C.c_int)
    rc = lib().orc_register_pbmap(ref.h, trg.h, max_match_planes, mode, _f(pose), _f(info), pairs.ctypes.data_as(ip),
                                  256, C.byref(n), C.byref(am), C.byref(as_), C.byref(at),
                                  C.byref(params) if params is not None else None)
    nodes, trunc = C.c_long(), C.c_int()
    lib().orc_last_match_stats(C.byref(nodes), C.byref(trunc))
    return dict(good=rc, pose=from16(pose), info=info.reshape(6, 6).T.copy(),
                matches={int(pairs[2 * k]): int(pairs[2 * k + 1]) for k in range(min(n.value, 256))},
                area_matched=am.value, area_src=as_.value, area_trg=at.value, nodes=nodes.value,
                truncated=bool(trunc.value))
