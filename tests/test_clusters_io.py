"""The cluster extraction's host side (no GPU): the labelled PCD codec (r360_pcd_write_labels / r360_pcd_read_labels),
the defaults, the argument checks that return before any device is touched, and tests/host/cluster_host_check.cpp, a
stand-alone program that runs the codec and the ranking tables (rgbd360_amd/csrc/host/cluster_rank.h) under the address
and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

NEW_SYMBOLS = ["r360_cluster_default_params", "r360_cloud_clusters", "r360_cloud_clusters_eval", "r360_ctx_map_cluster",
               "r360_ctx_map_download_labels", "r360_ctx_map_cluster_info", "r360_ctx_map_filter_clusters",
               "r360_pcd_write_labels", "r360_pcd_read_labels"]


def _cloud(n=300, seed=3):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    xyz[5] = np.nan
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    labels = rng.integers(-1, 7, n).astype(np.int32)
    labels[:3] = [-1, 0, 2 ** 31 - 1]
    return xyz, rgba, labels


def test_new_symbols_are_bound():
    for s in NEW_SYMBOLS:
        assert s in R.ABI_SYMBOLS, s
        assert hasattr(R.lib(), s), s
    for name in ("clusters", "clusters_eval", "map_cluster", "map_labels", "map_clusters", "map_filter_clusters"):
        assert callable(getattr(R.Context, name)), name
    assert C.sizeof(R.ClusterInfo) == 112 and R.CLUSTER_INFO_DTYPE.itemsize == 112


@pytest.mark.parametrize("mode", [R.PCD_ASCII, R.PCD_BINARY, R.PCD_BINARY_COMPRESSED])
def test_labels_pcd_round_trip(tmp_path, mode):
    xyz, rgba, labels = _cloud()
    path = str(tmp_path / "labels.pcd")
    R.write_pcd_labels(path, xyz, rgba, labels, mode)
    head = open(path, "rb").read(400).decode("latin1")
    assert "FIELDS x y z rgba label\n" in head and "SIZE 4 4 4 4 4\n" in head and "TYPE F F F U U\n" in head
    assert f"WIDTH {len(xyz)}\nHEIGHT 1\n" in head
    if mode == R.PCD_ASCII:
        first = open(path).read().split("DATA ascii\n")[1].splitlines()[0].split()
        assert first[4] == "4294967295"                       # -1 as PointXYZRGBL's unsigned label
    x2, c2, l2 = R.read_pcd_labels(path)
    assert np.array_equal(l2, labels) and l2.dtype == np.int32 and np.array_equal(c2, rgba)
    if mode == R.PCD_ASCII:                                   # eight digits, as savePCDFile prints
        assert np.allclose(x2, xyz, rtol=1e-7, atol=0, equal_nan=True)
    else:
        assert x2.tobytes() == xyz.tobytes()
    # the plain reader reads the same file's points and colours
    x3, c3, w, h = R.pcd_read(path)
    assert (w, h) == (len(xyz), 1) and np.array_equal(c3, rgba) and x3.tobytes() == x2.tobytes()


def test_reading_labels_from_a_file_without_them_fails(tmp_path):
    xyz, rgba, _ = _cloud(20)
    path = str(tmp_path / "plain.pcd")
    R.pcd_write(path, xyz, rgba, 20, 1, R.PCD_BINARY)
    with pytest.raises(RuntimeError, match="no label field"):
        R.read_pcd_labels(path)
    nrm = str(tmp_path / "normals.pcd")
    R.pcd_write_normals(nrm, xyz, rgba, np.zeros((20, 3), np.float32), np.zeros(20, np.float32), R.PCD_BINARY)
    with pytest.raises(RuntimeError, match="no label field"):
        R.read_pcd_labels(nrm)
    with pytest.raises(RuntimeError):
        R.read_pcd_labels(str(tmp_path / "missing.pcd"))


def test_default_params():
    p = R.ClusterParams.default()
    assert p.tolerance == np.float32(0.10) and p.min_size == 100 and p.max_size == 2 ** 30
    assert p.eps_angle == np.float32(math.radians(10.0))
    q = R.ClusterParams.make(0.2, 5, 50)
    assert (q.tolerance, q.min_size, q.max_size, q.eps_angle) == (np.float32(0.2), 5, 50, p.eps_angle)
    assert R.ClusterParams.make(eps_angle=0.5).eps_angle == 0.5
    R.lib().r360_cluster_default_params(None)                 # tolerated


def _rc(prm, normals=False, n=4, ctx=None):
    xyz = np.zeros((4, 3), np.float32)
    nrm = np.zeros((4, 3), np.float32)
    nk = C.c_size_t(99)
    rc = R.lib().r360_cloud_clusters(ctx, xyz.ctypes.data_as(R._FP), nrm.ctypes.data_as(R._FP) if normals else None, n,
                                     None if prm is None else C.byref(prm), None, None, 0, C.byref(nk), None)
    return rc, R.lib().r360_last_error().decode()


def test_argument_checks_need_no_context():
    """Every parameter check answers R360_EINVAL (-2) before the context is looked at, so a NULL context shows them."""
    ok = R.ClusterParams.make(0.1, 1, 10)
    rc, msg = _rc(ok)
    assert rc == -2 and "null ctx" in msg                     # the parameters passed: only the context is missing
    assert _rc(None)[0] == -2 and "null params" in _rc(None)[1]
    for tol in (0.0, -0.1, math.inf, math.nan):
        rc, msg = _rc(R.ClusterParams.make(tol, 1, 10))
        assert rc == -2 and "tolerance" in msg, tol
    rc, msg = _rc(R.ClusterParams.make(0.1, 0, 10))
    assert rc == -2 and "min_size" in msg
    rc, msg = _rc(R.ClusterParams.make(0.1, 5, 4))
    assert rc == -2 and "max_size" in msg
    assert "null ctx" in _rc(R.ClusterParams.make(0.1, 5, 5))[1]
    for eps in (-0.01, 3.2, math.nan):
        rc, msg = _rc(R.ClusterParams.make(0.1, 1, 10, eps_angle=eps), normals=True)
        assert rc == -2 and "eps_angle" in msg, eps
        assert "null ctx" in _rc(R.ClusterParams.make(0.1, 1, 10, eps_angle=eps), normals=False)[1]   # unused: unchecked
    for eps in (0.0, math.pi):                                # float32(pi) is the closed end
        assert "null ctx" in _rc(R.ClusterParams.make(0.1, 1, 10, eps_angle=eps), normals=True)[1]
    rc, msg = _rc(ok, n=2 ** 30 + 1)
    assert rc == -2 and "2^30" in msg
    st = R.ClusterStats()
    for fn in (R.lib().r360_ctx_map_cluster, R.lib().r360_ctx_map_filter_clusters):
        assert fn(None, C.byref(ok), 0, C.byref(st)) == -2
        assert fn(None, C.byref(R.ClusterParams.make(-1.0, 1, 10)), 0, C.byref(st)) == -2
        assert "tolerance" in R.lib().r360_last_error().decode()
    n = C.c_size_t()
    assert R.lib().r360_ctx_map_download_labels(None, None, 0, C.byref(n)) == -2
    assert R.lib().r360_ctx_map_cluster_info(None, None, 0, C.byref(n)) == -2


def test_host_side_under_sanitizers(root, tmp_path):
    rocm = os.environ.get("ROCM") or os.environ.get("ROCM_PATH") or "/opt/rocm"   # the Makefile's ROCM
    exe = tmp_path / "cluster_host_check"
    p = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{root}/rgbd360_amd/csrc",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-w", "-o", str(exe),
                        f"{root}/tests/host/cluster_host_check.cpp", f"{root}/rgbd360_amd/csrc/host/io.cpp"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "cluster host ok", (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
