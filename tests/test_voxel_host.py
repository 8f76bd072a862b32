"""The voxel grid's host side (no GPU): the new C-ABI symbols, their argument checks (which return before any device
is touched), the numpy statement of PCL's size guard with a known answer, and the drop-in call sequence of the whole
map step (tests/dropin/global_map_voxel_dropin.cpp) compiled with g++ alone.

The voxel semantics themselves are tests/test_map.py::voxel_model; the guard below completes it:
  with inv = float32(1 / leaf) and min_p / max_p the bounds of the finite points, d = int64((max_p - min_p) * inv) + 1
  per axis (float32 subtract and multiply); dx * dy * dz > INT32_MAX -> the filter does not bin (soft failure 1, the
  output is the input).  Otherwise min_b = floor(min_p * inv), max_b = floor(max_p * inv), the grid's extents are
  max_b - min_b + 1 (each can be one more than d), and a voxel's linear index
  (i - min_b.x) + (j - min_b.y) * ex + (k - min_b.z) * ex * ey must fit 31 bits: a grid of more than INT32_MAX cells
  is refused in the same way.  Ascending linear index is ascending (k, j, i)."""
import ctypes as C
import subprocess

import numpy as np

import rgbd360_amd as R

INT32_MAX = 2 ** 31 - 1
NEW_SYMBOLS = ["r360_cloud_filter_voxel", "r360_ctx_map_reset", "r360_ctx_map_add_cloud", "r360_ctx_map_add_frame",
               "r360_ctx_map_size", "r360_ctx_map_download"]


# ------------------------------------------------------------------ the guard's model
def guard_model(xyz, leaf):
    """(bins, min_b [3], extents [3]): bins is False when the size guard refuses the leaf; min_b and extents are
    python ints (None without finite points or when refused by the first condition)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    if len(p) == 0:
        return True, None, None
    inv = np.float32(1.0) / np.float32(leaf)
    mn, mx = p.min(0), p.max(0)
    with np.errstate(over="ignore"):
        d = (mx - mn) * inv                                   # float32
    if not np.isfinite(d).all() or (d >= np.float32(4.0e18)).any():
        return False, None, None
    dx, dy, dz = (int(v) + 1 for v in d)                      # truncation of a non-negative float
    if dx * dy * dz > INT32_MAX:
        return False, None, None
    lo = [int(v) for v in np.floor(mn * inv)]
    hi = [int(v) for v in np.floor(mx * inv)]
    ext = [h - l + 1 for l, h in zip(lo, hi)]
    if ext[0] * ext[1] * ext[2] > INT32_MAX:
        return False, lo, ext
    return True, lo, ext


def linear_index(ijk, min_b, ext):
    ijk = np.asarray(ijk, np.int64)
    return (ijk[:, 0] - min_b[0]) + (ijk[:, 1] - min_b[1]) * ext[0] + (ijk[:, 2] - min_b[2]) * ext[0] * ext[1]


# ------------------------------------------------------------------ tests
def test_new_symbols_are_bound():
    for s in NEW_SYMBOLS:
        assert s in R.ABI_SYMBOLS, s
        assert hasattr(R.lib(), s), s
    for name in ("filter_voxel", "map_reset", "map_add_cloud", "map_add_frame", "map_size", "map_download"):
        assert callable(getattr(R.Context, name)), name
    assert callable(R.FilterPointCloud.filterVoxel)
    assert R.FilterPointCloud(0.1, 3.0).voxelSize == 0.1
    assert R.VOXEL_QUANTUM == 2.0 ** -24


def test_invalid_arguments_fail_without_a_device():
    """Null handles, null arrays and leaves without a usable 1 / leaf return rc < 0 from the argument checks, which run
    before anything touches a device (this machine has none).  `fake` stands in for a context: the checks that fail
    here never read it."""
    L = R.lib()
    xyz = np.zeros((4, 3), np.float32)
    rgba = np.zeros(4, np.uint32)
    n = C.c_size_t(77)
    fx, vc = R._fptr(xyz), R._vptr(rgba)
    pose = R._fptr(np.eye(4, dtype=np.float32).reshape(16).copy())
    assert L.r360_cloud_filter_voxel(None, fx, vc, 4, 0.05, fx, vc, 4, C.byref(n)) < 0
    assert b"null ctx" in L.r360_last_error()
    assert L.r360_ctx_map_reset(None) < 0
    assert L.r360_ctx_map_add_cloud(None, fx, vc, 4, 0.05) < 0
    assert L.r360_ctx_map_add_frame(None, None, pose, -2.0, 1.0, 4.0, 0.05) < 0
    assert L.r360_ctx_map_size(None, C.byref(n)) < 0
    assert L.r360_ctx_map_download(None, fx, vc, 4, C.byref(n)) < 0
    buf = C.create_string_buffer(1 << 16)
    fake = C.c_void_p(C.addressof(buf))
    assert L.r360_cloud_filter_voxel(fake, None, vc, 4, 0.05, fx, vc, 4, C.byref(n)) < 0          # null xyz
    for leaf in (0.0, -0.05, float("nan"), float("inf"), 1e-45):                                 # 1 / 1e-45f overflows
        assert L.r360_cloud_filter_voxel(fake, fx, vc, 4, leaf, fx, vc, 4, C.byref(n)) < 0, leaf
        assert L.r360_ctx_map_add_cloud(fake, fx, vc, 4, leaf) < 0, leaf
    assert b"leaf" in L.r360_last_error()
    assert L.r360_cloud_filter_voxel(fake, fx, vc, 4, 0.05, fx, vc, 4, None) < 0                  # null n_out
    assert L.r360_cloud_filter_voxel(fake, fx, vc, 4, 0.05, None, vc, 4, C.byref(n)) < 0          # null output
    assert L.r360_ctx_map_add_frame(fake, None, pose, -2.0, 1.0, 4.0, 0.05) < 0                   # null frame
    assert L.r360_ctx_map_add_frame(fake, fake, None, -2.0, 1.0, 4.0, 0.05) < 0                   # null pose
    assert L.r360_ctx_map_size(fake, None) < 0
    assert L.r360_ctx_map_download(fake, fx, vc, 4, None) < 0
    f = R.FilterPointCloud()
    try:
        f.filterVoxel(xyz, rgba)
    except RuntimeError as e:
        assert "ctx" in str(e)
    else:
        raise AssertionError("filterVoxel without a context must fail loudly")


def test_guard_model_known_answer():
    """Two finite points 10,000 m apart, (0, 0, 0) and (6000, 8000, 0) (a 3-4-5 triangle), plus a NaN row the bounds
    ignore.  At leaf 0.001 (inv = 1000): dx = 6,000,001, dy = 8,000,001, dz = 1, product 4.8e13 > INT32_MAX: refused.
    At leaf 1: 6001 * 8001 * 1 = 48,014,001 cells: bins, and the two voxels' linear indices are 0 and
    6000 + 8000 * 6001 = 48,014,000."""
    xyz = np.array([[0, 0, 0], [np.nan, 1e9, 0], [6000, 8000, 0]], np.float32)
    assert np.linalg.norm(xyz[2].astype(np.float64)) == 10000.0
    bins, lo, ext = guard_model(xyz, 0.001)
    assert not bins
    bins, lo, ext = guard_model(xyz, 1.0)
    assert bins and lo == [0, 0, 0] and ext == [6001, 8001, 1]
    from test_map import voxel_keys
    idx = linear_index(voxel_keys(xyz[[0, 2]], 1.0), lo, ext)
    assert idx.tolist() == [0, 48014000] and idx.max() <= INT32_MAX
    # the estimate from (max - min) * inv can be one short of the real extent: 0.9 .. 1.1 at leaf 1 spans two voxels
    bins, lo, ext = guard_model(np.array([[0.9, 0, 0], [1.1, 0, 0]], np.float32), 1.0)
    assert bins and lo == [0, 0, 0] and ext == [2, 1, 1]
    assert guard_model(np.zeros((0, 3), np.float32), 0.05) == (True, None, None)


def test_linear_index_order_is_kji_order():
    from test_map import voxel_keys
    rng = np.random.default_rng(3)
    p = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    bins, lo, ext = guard_model(p, 0.05)
    assert bins
    ijk = voxel_keys(p, 0.05)
    lin = linear_index(ijk, lo, ext)
    assert lin.min() >= 0 and lin.max() < ext[0] * ext[1] * ext[2] <= INT32_MAX
    assert np.array_equal(np.argsort(lin, kind="stable"), np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2])))


def test_global_map_voxel_call_sequence_compiles(root):
    """tests/dropin/global_map_voxel_dropin.cpp — the full map step with filter.filterVoxel(globalMap), and the
    device-resident r360::GlobalMap360 beside it — compiles with g++ alone, warning-free, at -O0 and -O2."""
    for opt in ("-O0", "-O2"):
        p = subprocess.run(["g++", "-std=c++17", opt, "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                            f"{root}/tests/dropin/global_map_voxel_dropin.cpp"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
    src = open(f"{root}/tests/dropin/global_map_voxel_dropin.cpp").read()
    for call in ("FilterPointCloud filter", "filterEuclidean(", "transformPointCloud(", "+=", "filter.filterVoxel(globalMap)",
                 "GlobalMap360"):
        assert call in src, call
