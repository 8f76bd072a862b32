"""tests/outlier_model.py against answers worked by hand, and the outlier filters' C-ABI checks that need no GPU
(include/rgbd360_hip.h, "outlier removal"): the documented defaults and every R360_EINVAL case, which return before
anything touches a device."""
import ctypes as C
import math
import subprocess

import numpy as np

import outlier_model as OM
import rgbd360_amd as R

EINVAL = -2


# ------------------------------------------------------------------ the model, by hand
def test_five_collinear_points_k2():
    """x = 0 .. 4 at unit spacing, k = 2: d = (1 + 2) / 2 at the ends, (1 + 1) / 2 inside.  mean = 6 / 5, the squared
    deviations are 0.09, 0.04, 0.04, 0.04, 0.09, stddev = sqrt(0.30 / 4): with mul = 1 the threshold 1.4739 removes the
    two ends, with mul = 2 (1.7477) everything stays.  With max_dist 1.5 the ends' second neighbour (at 2) is out of
    reach: they are short, and the three others (d = 1, stddev 0, threshold 1) stay."""
    p = np.array([[x, 0, 0] for x in range(5)], np.float32)
    r = OM.statistical(p, 2, 1.0, 10.0)
    assert r.d.tolist() == [1.5, 1.0, 1.0, 1.0, 1.5]
    assert not r.short.any()
    assert abs(r.mean - 1.2) < 1e-15 and abs(r.stddev - math.sqrt(0.075)) < 1e-15
    assert abs(r.threshold - (1.2 + math.sqrt(0.075))) < 1e-15
    assert r.keep.tolist() == [False, True, True, True, False] and len(r.band) == 0
    assert OM.statistical(p, 2, 2.0, 10.0).keep.all()
    s = OM.statistical(p, 2, 1.0, 1.5)
    assert s.short.tolist() == [True, False, False, False, True] and np.isinf(s.d[[0, 4]]).all()
    assert (s.mean, s.stddev, s.threshold) == (1.0, 0.0, 1.0)
    assert s.keep.tolist() == [False, True, True, True, False]
    assert s.band.tolist() == [1, 2, 3]          # d equals the threshold: the band names them, the rule keeps them


def test_lattice_radius_is_closed():
    """3 x 3 x 3 points at spacing 0.25 and radius exactly 0.25f: the neighbours at distance 0.25 count (closed
    interval), the diagonal ones (0.3536) do not: 3 at a corner, 4 on an edge, 5 on a face, 6 in the centre."""
    g = np.array([[i, j, k] for k in range(3) for j in range(3) for i in range(3)])
    p = (g * 0.25).astype(np.float32)
    r = OM.radius(p, np.float32(0.25), 5)
    inner = (g == 1).sum(axis=1)                 # how many coordinates are the middle one
    assert np.array_equal(r.c, 3 + inner)
    assert np.array_equal(r.keep, inner >= 2) and r.keep.sum() == 7
    assert OM.radius(p, np.float32(0.2499), 1).c.max() == 0


def test_duplicate_pair():
    """Two copies of a point and one point 1 m away: each copy's nearest other point is the other copy, at 0."""
    p = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    r = OM.statistical(p, 1, 1.0, 2.0)
    assert r.d.tolist() == [0.0, 0.0, 1.0]
    assert r.keep.tolist() == [True, True, False]            # mean 1/3, stddev 0.5774: threshold 0.9107
    assert OM.radius(p, 1e-3, 1).c.tolist() == [1, 1, 0]
    assert OM.radius(p, 1e-3, 1).keep.tolist() == [True, True, False]


def test_n_equals_k_every_point_is_short():
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (4, 3)).astype(np.float32)
    r = OM.statistical(p, 4, 1.0, 10.0)
    assert r.short.all() and np.isinf(r.d).all() and not r.keep.any()
    assert (r.mean, r.stddev, r.threshold) == (0.0, 0.0, 0.0)
    assert not OM.statistical(p, 3, 1.0, 10.0).short.any()


def test_non_finite_rows_are_dropped():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [0, np.inf, 0], [0, 0.1, 0]], np.float32)
    r = OM.radius(p, 0.2, 1)
    assert r.c.tolist() == [2, -1, 2, -1, 2] and r.keep.tolist() == [True, False, True, False, True]
    s = OM.statistical(p, 2, 1.0, 1.0)
    assert np.isnan(s.d[[1, 3]]).all() and np.isfinite(s.d[[0, 2, 4]]).all() and not s.keep[[1, 3]].any()


# ------------------------------------------------------------------ the C-ABI without a GPU
def test_default_params_are_the_documented_ones():
    p = R.OutlierParams.default()
    assert (p.kind, p.mean_k, p.stddev_mul, p.max_dist, p.min_neighbors) == (R.OUTLIER_STATISTICAL, 20, 1.0, 0.5, 5)
    assert p.radius == float(np.float32(0.15))
    for s in ("r360_outlier_default_params", "r360_cloud_filter_outliers", "r360_ctx_map_filter_outliers",
              "r360_cloud_outlier_eval"):
        assert s in R.ABI_SYMBOLS and hasattr(R.lib(), s), s
    for name in ("filter_outliers", "map_filter_outliers", "outlier_eval"):
        assert callable(getattr(R.Context, name)), name


def _calls(L, ctx, prm):
    xyz = np.zeros((4, 3), np.float32)
    n, st = C.c_size_t(77), R.OutlierStats()
    score, count = np.zeros(4), np.zeros(4, np.int32)
    fx = R._fptr(xyz)
    return (L.r360_cloud_filter_outliers(ctx, fx, None, 4, prm, fx, None, 4, C.byref(n), C.byref(st)),
            L.r360_ctx_map_filter_outliers(ctx, prm, C.byref(st)),
            L.r360_cloud_outlier_eval(ctx, fx, 4, prm, R._dptr(score), count.ctypes.data_as(R._IP)))


def test_invalid_arguments_are_einval_without_a_device():
    """A null context, null parameters and every parameter outside its domain return R360_EINVAL from the argument
    check, which runs before anything touches a device.  `fake` stands in for a context: the checks that fail here
    never read it."""
    L = R.lib()
    good = R.OutlierParams.default()
    assert _calls(L, None, C.byref(good)) == (EINVAL, EINVAL, EINVAL)
    assert b"null ctx" in L.r360_last_error()
    buf = C.create_string_buffer(1 << 16)
    fake = C.c_void_p(C.addressof(buf))
    assert _calls(L, fake, None) == (EINVAL, EINVAL, EINVAL)
    assert b"null params" in L.r360_last_error()
    bad = [("kind", 2), ("kind", -1), ("mean_k", 0), ("mean_k", 65), ("mean_k", -3), ("max_dist", 0.0), ("max_dist", -0.5),
           ("max_dist", float("nan")), ("max_dist", float("inf")), ("radius", 0.0), ("radius", -1.0),
           ("radius", float("nan")), ("radius", float("inf")), ("min_neighbors", -1), ("stddev_mul", float("nan"))]
    for name, value in bad:
        for kind in (R.OUTLIER_STATISTICAL, R.OUTLIER_RADIUS):
            p = R.OutlierParams.default()
            p.kind = kind
            setattr(p, name, value)
            assert _calls(L, fake, C.byref(p)) == (EINVAL, EINVAL, EINVAL), (name, value, kind)


def test_outlier_call_sequence_compiles(root):
    """tests/dropin/outlier_dropin.cpp — voxel grid, then filterStatistical / filterRadius on the cloud and
    removeOutliers on the device-resident map — compiles with g++ alone, warning-free."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/outlier_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    src = open(f"{root}/tests/dropin/outlier_dropin.cpp").read()
    for call in ("filter.filterVoxel(globalMap)", "filter.filterStatistical(", "filter.filterRadius(", "removeOutliers("):
        assert call in src, call
