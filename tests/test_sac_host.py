"""The plane search's host side (no GPU): tests/host/sac_host_check.cpp, a stand-alone program with its own main that
includes rgbd360_amd/csrc/host/sac_sample.h (the sampler and the plane of three points the hypothesis kernel runs) and
is built with g++ -ffp-contract=off under the address and undefined-behaviour sanitizers; its samples and hex-float
coefficients equal tests/sac_model.py exactly.  Then the defaults and the argument checks, which answer R360_EINVAL
before any device is touched: a NULL context shows them."""
import ctypes as C
import math
import subprocess

import numpy as np

import rgbd360_amd as R
import sac_model as M

NEW_SYMBOLS = ["r360_sac_default_params", "r360_cloud_sac_planes", "r360_cloud_sac_eval", "r360_ctx_map_sac_planes",
               "r360_ctx_map_download_plane_labels", "r360_ctx_map_plane_info", "r360_ctx_map_filter_planes"]


def test_new_symbols_are_bound():
    for s in NEW_SYMBOLS:
        assert s in R.ABI_SYMBOLS and hasattr(R.lib(), s), s


def test_sampler_and_plane_under_sanitizers(root, tmp_path):
    exe = tmp_path / "sac_host_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", f"-I{root}/rgbd360_amd/csrc",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-o", str(exe),
                        f"{root}/tests/host/sac_host_check.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rng = np.random.default_rng(7)
    keys = [(0, 0, 0, 3), (0, 0, 1, 4), (2016, 3, 129, 5), (2 ** 64 - 1, 63, 65535, 2 ** 30), (12345678901234567, 7, 128, 1000003)]
    keys += [(int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 64)), int(rng.integers(0, 65536)),
              int(rng.integers(3, 2 ** 30))) for _ in range(200)]
    tri = rng.uniform(-4, 4, (200, 3, 3)).astype(np.float32)
    tri[0, 1] = tri[0, 0]                                     # a duplicate
    tri[1, 2] = tri[1, 0] + 2 * (tri[1, 1] - tri[1, 0])        # nearly collinear: whatever float32 leaves
    tri[2] = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)      # exactly collinear
    tri[3] = np.array([[3e38, 0, 0], [-3e38, 1, 0], [0, -3e38, 3e38]], np.float32)   # huge, yet s stays finite in double
    tri[4] = np.array([[0, 0, 0.25], [1, 0, 0.25], [0, 1, 0.25]], np.float32)
    lines = [f"s {s} {p_} {h} {m}" for s, p_, h, m in keys]
    lines += ["t " + " ".join(f"{b:08x}" for b in t.reshape(-1).view(np.uint32)) for t in tri]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    for (s, p_, h, m), line in zip(keys, out):
        assert tuple(int(v) for v in line.split()) == M.sample3(s, p_, h, m), (s, p_, h, m)
    coef = M.planes3(tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.isnan(coef[[0, 2]]).all() and np.isfinite(coef[3]).all() and np.array_equal(coef[4], [0.0, 0.0, 1.0, -0.25])
    for c, line in zip(coef, out[len(keys):]):
        if np.isnan(c).any():
            assert line == "degenerate"
        else:
            got = np.array([float.fromhex(v) for v in line.split()])
            assert np.array_equal(got.view(np.uint64), c.view(np.uint64)), (line, c)


def test_default_params():
    p = R.SacParams.default()
    assert p.distance_threshold == np.float32(0.05) and p.max_iterations == 1024 and p.probability == np.float32(0.99)
    assert p.optimize == 1 and p.constraint == R.SAC_NONE and tuple(p.axis) == (0.0, 0.0, 1.0)
    assert p.eps_angle == np.float32(math.radians(10)) and p.normal_angle == np.float32(math.radians(10))
    assert p.max_planes == 8 and p.min_inliers == 100 and p.stop_fraction == 0.0 and p.seed == 0
    assert R.SAC_ROUND == M.ROUND == 128
    assert (R.SAC_NONE, R.SAC_PERPENDICULAR, R.SAC_PARALLEL) == (M.NONE, M.PERPENDICULAR, M.PARALLEL)


def _rc(prm, n=4, normals=False, ctx=None):
    xyz = np.zeros((4, 3), np.float32)
    nrm = np.zeros((4, 3), np.float32)
    npl = C.c_size_t(99)
    rc = R.lib().r360_cloud_sac_planes(ctx, xyz.ctypes.data_as(R._FP), nrm.ctypes.data_as(R._FP) if normals else None, n,
                                       None if prm is None else C.byref(prm), None, None, 0, C.byref(npl), None)
    return rc, R.lib().r360_last_error().decode()


def test_argument_checks_need_no_context():
    mk = R.SacParams.make
    rc, msg = _rc(mk())
    assert rc == -2 and "null ctx" in msg                     # the parameters passed: only the context is missing
    assert _rc(None)[0] == -2 and "null params" in _rc(None)[1]
    bad = [("distance_threshold", (0.0, -0.1, math.inf, math.nan)), ("max_iterations", (0, -1, 65537)),
           ("probability", (0.0, 1.0, -0.5, 1.5, math.nan)), ("max_planes", (0, 65)), ("min_inliers", (2, 0, -1)),
           ("stop_fraction", (-0.1, 1.0, math.nan)), ("constraint", (-1, 3))]
    for name, values in bad:
        for v in values:
            rc, msg = _rc(mk(**{name: v}))
            assert rc == -2 and name in msg, (name, v, msg)
    good = [("max_iterations", (1, 65536)), ("max_planes", (1, 64)), ("min_inliers", (3,)), ("stop_fraction", (0.0, 0.999)),
            ("constraint", (0, 1, 2))]
    for name, values in good:
        for v in values:
            assert "null ctx" in _rc(mk(**{name: v}))[1], (name, v)
    for con in (R.SAC_PERPENDICULAR, R.SAC_PARALLEL):
        for axis in ((0, 0, 0), (math.nan, 0, 1), (math.inf, 0, 0)):
            rc, msg = _rc(mk(constraint=con, axis=axis))
            assert rc == -2 and "axis" in msg
        for eps in (-0.01, 1.6, math.nan):
            rc, msg = _rc(mk(constraint=con, eps_angle=eps))
            assert rc == -2 and "eps_angle" in msg
        for eps in (0.0, math.pi / 2):
            assert "null ctx" in _rc(mk(constraint=con, eps_angle=eps))[1]
    assert "null ctx" in _rc(mk(axis=(0, 0, 0), eps_angle=9.0))[1]          # unconstrained: unused, unchecked
    for ang in (-0.01, 1.6, math.nan):
        rc, msg = _rc(mk(normal_angle=ang), normals=True)
        assert rc == -2 and "normal_angle" in msg
        assert "null ctx" in _rc(mk(normal_angle=ang), normals=False)[1]
    rc, msg = _rc(mk(), n=2 ** 30 + 1)
    assert rc == -2 and "2^30" in msg
    st = R.SacStats()
    L = R.lib()
    assert L.r360_ctx_map_sac_planes(None, C.byref(mk()), 0, C.byref(st)) == -2
    assert L.r360_ctx_map_sac_planes(None, C.byref(mk(probability=1.0)), 0, C.byref(st)) == -2
    assert "probability" in L.r360_last_error().decode()
    assert L.r360_ctx_map_filter_planes(None, C.byref(mk()), 0, 0, C.byref(st)) == -2
    assert L.r360_ctx_map_filter_planes(None, C.byref(mk(min_inliers=1)), 0, 1, C.byref(st)) == -2
    assert "min_inliers" in L.r360_last_error().decode()
    cnt = np.zeros(4, np.int32)
    assert L.r360_cloud_sac_eval(None, None, None, 0, C.byref(mk()), None, 4, None, None, cnt.ctypes.data_as(R._IP)) == -2
    n = C.c_size_t()
    assert L.r360_ctx_map_download_plane_labels(None, None, 0, C.byref(n)) == -2
    assert L.r360_ctx_map_plane_info(None, None, 0, C.byref(n)) == -2
