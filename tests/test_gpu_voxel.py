"""FilterPointCloud::filterVoxel on the GPU (r360_cloud_filter_voxel) and the context's device-resident global map
(r360_ctx_map_*) against the numpy statement of tests/test_map.py (voxel_model, transform_model, euclid_model) and
the size guard of tests/test_voxel_host.py.

The xyz bound of a voxel with more than one point is derived, not measured: every point moves at most q / 2 when it
is quantised to q = R360_VOXEL_QUANTUM, so the mean moves at most q / 2; the integer sums are exact; the mean is
rounded to float32 once: |got - mean64| <= q / 2 + ulp_float32(|mean64|) / 2.  A voxel with one point returns that
point's bits.  The C ABI returns no per-voxel counts; they are checked through what they determine: the number of
voxels, the truncated colour means and the coordinate means."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R
from test_map import euclid_model, transform_model, voxel_keys, voxel_model
from test_voxel_host import guard_model, linear_index

pytestmark = pytest.mark.gpu

Q = R.VOXEL_QUANTUM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 360 << 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pack(r, g, b, a=255):
    return a << 24 | r << 16 | g << 8 | b


def _ulp32(v):
    """ulp of the float32 binade that holds |v| (v float64)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 23)


def _check_against_model(xyz, rgba, leaf, got_xyz, got_rgba):
    ijk, mean64, xyz32, c, counts = voxel_model(xyz, rgba, leaf)
    assert got_xyz.shape == (len(ijk), 3) and got_rgba.shape == (len(ijk),)     # as many voxels as the model has
    if len(ijk) == 0:
        return
    bins, lo, ext = guard_model(xyz, leaf)
    assert bins
    assert (np.diff(linear_index(ijk, lo, ext)) > 0).all()                     # the model's order is the linear order
    assert np.array_equal(got_rgba, c)                                         # colours exactly, alpha 0
    one = counts == 1
    assert np.array_equal(_bits(got_xyz)[one], _bits(xyz32)[one])              # singletons bit for bit
    bound = Q / 2 + _ulp32(mean64) / 2
    err = np.abs(got_xyz.astype(np.float64) - mean64)
    print(f"n={len(xyz)} leaf={leaf}: {len(ijk)} voxels, {int(one.sum())} singletons, max err/bound "
          f"{(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()
    # row t is voxel ijk[t]: the output's own voxel, except where the exact mean lies within the bound of a face
    inv = np.float32(1.0) / np.float32(leaf)
    same = (voxel_keys(got_xyz, leaf) == ijk)
    s = mean64 * float(inv)
    near_face = np.abs(s - np.rint(s)) * leaf <= 2 * bound
    assert (same | near_face).all()
    assert same[one].all()


@functools.lru_cache(maxsize=None)
def _cloud():
    """40,000 points: 25,000 uniform in a 1 m cube, 5,000 inside one voxel, 4,000 with coordinates k / 16 exactly on
    voxel faces (signs mixed), 3,000 uniform in +-30 m, 2,950 exact duplicates of earlier rows, 50 non-finite rows;
    shuffled, so every prefix mixes the kinds."""
    rng = np.random.default_rng(360)
    cube = rng.uniform(0, 1, (25000, 3))
    one = np.array([0.4, -0.3, 0.2]) + rng.uniform(0.001, 0.049, (5000, 3))          # voxel (8, -6, 4) at 0.05
    face = rng.integers(-32, 33, (4000, 3)) / 16.0
    far = rng.uniform(-30, 30, (3000, 3))
    xyz = np.vstack([cube, one, face, far]).astype(np.float32)
    xyz = np.vstack([xyz, xyz[rng.integers(0, len(xyz), 2950)]])
    bad = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    bad[np.arange(50), rng.integers(0, 3, 50)] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), 50)
    xyz = np.vstack([xyz, bad]).astype(np.float32)
    rgba = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    p = rng.permutation(len(xyz))
    xyz, rgba = xyz[p], rgba[p]
    xyz.setflags(write=False)
    rgba.setflags(write=False)
    assert len(xyz) == 40000
    return xyz, rgba


def test_known_answer():
    """The six points of test_map.test_model_known_answer plus a NaN row and an Inf row: three voxels in the order
    B, A, C with the hand-computed colours."""
    xyz = np.array([[0.12, -0.07, 0.26], [0.01, 0.01, 0.01], [-0.01, 0.01, 0.01], [0.03, 0.02, 0.04],
                    [0.14, -0.06, 0.27], [-0.03, 0.03, 0.02], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    rgba = np.array([_pack(100, 100, 100), _pack(10, 20, 30), _pack(255, 0, 1), _pack(11, 21, 33), _pack(101, 103, 100),
                     _pack(0, 255, 2), 1, 2], np.uint32)
    ctx = R.Context(0)
    try:
        gx, gc, ok = ctx.filter_voxel(xyz, rgba, 0.05)
    finally:
        ctx.close()
    assert ok and gx.shape == (3, 3)
    assert voxel_keys(gx, 0.05).tolist() == [[-1, 0, 0], [0, 0, 0], [2, -2, 5]]
    assert gc.tolist() == [127 << 16 | 127 << 8 | 1, 10 << 16 | 20 << 8 | 31, 100 << 16 | 101 << 8 | 100]
    want = np.array([[-0.02, 0.02, 0.015], [0.02, 0.015, 0.025], [0.13, -0.065, 0.265]])
    # the float32 inputs' means lie within 1e-8 of the decimals (test_model_known_answer); ulp / 2 below 0.5 is 2^-26
    assert np.abs(gx - want).max() < 1e-8 + Q / 2 + 2.0 ** -26
    _check_against_model(xyz, rgba, 0.05, gx, gc)


@pytest.mark.parametrize("leaf", [0.05, 0.0625, 0.2])
def test_model_parity(leaf):
    xyz, rgba = _cloud()
    ctx = R.Context(0)
    try:
        for n in (0, 1, 63, 64, 65, 257, 40000):
            gx, gc, ok = ctx.filter_voxel(xyz[:n], rgba[:n], leaf)
            assert ok
            _check_against_model(xyz[:n], rgba[:n], leaf, gx, gc)
        # without colours
        gx2, none, ok = ctx.filter_voxel(xyz[:257], None, leaf)
        assert ok and none is None
        assert np.array_equal(_bits(gx2), _bits(ctx.filter_voxel(xyz[:257], rgba[:257], leaf)[0]))
    finally:
        ctx.close()


def test_reproducible_and_order_independent():
    xyz, rgba = _cloud()
    p = np.random.default_rng(1).permutation(len(xyz))
    ctx = R.Context(0)
    try:
        a = ctx.filter_voxel(xyz, rgba, 0.05)
        b = ctx.filter_voxel(xyz[p], rgba[p], 0.05)
        c = ctx.filter_voxel(xyz, rgba, 0.05)
    finally:
        ctx.close()
    for o in (b, c):
        assert _bits(o[0]).tobytes() == _bits(a[0]).tobytes() and o[1].tobytes() == a[1].tobytes()


def test_aliasing_capacity_and_guard():
    import ctypes as C
    xyz, rgba = _cloud()
    L = R.lib()
    ctx = R.Context(0)
    try:
        wx, wc, ok = ctx.filter_voxel(xyz, rgba, 0.05)
        m = len(wx)
        # outputs aliasing the inputs
        ax, ac, n = xyz.copy(), rgba.copy(), C.c_size_t()
        assert L.r360_cloud_filter_voxel(ctx.h, R._fptr(ax), R._vptr(ac), len(ax), 0.05, R._fptr(ax), R._vptr(ac), len(ax),
                                         C.byref(n)) == 0
        assert n.value == m and _bits(ax[:m]).tobytes() == _bits(wx).tobytes() and ac[:m].tobytes() == wc.tobytes()
        # one slot short
        ox, oc = np.zeros((m, 3), np.float32), np.zeros(m, np.uint32)
        ix, ic = xyz.copy(), rgba.copy()
        rc = L.r360_cloud_filter_voxel(ctx.h, R._fptr(ix), R._vptr(ic), len(ix), 0.05, R._fptr(ox), R._vptr(oc), m - 1,
                                       C.byref(n))
        assert rc < 0 and n.value == m
        # the size guard: rc 1, the output is the input byte for byte (non-finite rows and alpha included)
        gx = np.array([[0, 0, 0], [np.nan, 1, 2], [6000, 8000, 0], [1, -np.inf, 3]], np.float32)
        gc = np.array([0xff010203, 0x80000001, 0x7f0a0b0c, 5], np.uint32)
        assert not guard_model(gx, 0.001)[0] and guard_model(gx, 1.0)[0]
        ox, oc = np.full((4, 3), 7, np.float32), np.full(4, 7, np.uint32)
        rc = L.r360_cloud_filter_voxel(ctx.h, R._fptr(gx), R._vptr(gc), 4, 0.001, R._fptr(ox), R._vptr(oc), 4, C.byref(n))
        assert rc == 1 and n.value == 4
        assert _bits(ox).tobytes() == _bits(gx).tobytes() and oc.tobytes() == gc.tobytes()
        bx, bc, ok = ctx.filter_voxel(gx, gc, 0.001)
        assert not ok and _bits(bx).tobytes() == _bits(gx).tobytes() and bc.tobytes() == gc.tobytes()
        bx, bc, ok = ctx.filter_voxel(gx, gc, 1.0)          # the same pair at leaf 1 bins
        assert ok
        _check_against_model(gx, gc, 1.0, bx, bc)
        # outside the supported domain: an error, never a wrong map
        with pytest.raises(RuntimeError, match="domain|overflow"):
            ctx.filter_voxel(np.array([[3e9, 0, 0], [3e9 + 1024, 0, 0]], np.float32), None, 1.0)
        # the table is clean after all of this
        cx, cc, ok = ctx.filter_voxel(xyz, rgba, 0.05)
        assert ok and _bits(cx).tobytes() == _bits(wx).tobytes() and cc.tobytes() == wc.tobytes()
    finally:
        ctx.close()


def test_context_map(tmp_path):
    leaf = 0.05
    ctx, ctx2, ctx3 = R.Context(0), R.Context(0), None
    cal = frames = None
    try:
        cal = R.Calib360(ctx, 240, 320)
        cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
        frames, poses, chains = [], [], []
        for k in range(3):
            pose = R.synth_path_pose(SEED, 2 * k)
            bgr, dep = cal.synth_frame(SEED, pose)
            f = R.Frame360(cal)
            frames.append(f)
            f.upload(bgr, dep)
            f.build(R.BUILD_UNDISTORT | R.BUILD_CLOUD)
            sx, sc, w, h = f.sphereCloud()
            assert len(sx) == 153600
            ex, ec = euclid_model(sx, sc)
            assert 0 < len(ex) < len(sx)
            poses.append(pose)
            chains.append((transform_model(ex, pose), ec))
        assert ctx.map_size() == 0
        mx, mc = np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
        for f, pose, (hx, hc) in zip(frames, poses, chains):
            assert ctx.map_add_frame(f, pose, leaf)
            gx, gc = ctx.map_download()
            cat_x, cat_c = np.vstack([mx, hx]), np.concatenate([mc, hc])
            wx, wc, ok = ctx2.filter_voxel(cat_x, cat_c, leaf)
            assert ok and len(gx) == ctx.map_size() == len(wx)
            assert _bits(gx).tobytes() == _bits(wx).tobytes() and gc.tobytes() == wc.tobytes()
            _check_against_model(cat_x, cat_c, leaf, gx, gc)
            assert ctx2.map_add_frame(f, pose, leaf)        # a frame of another context of the same device
            mx, mc = gx, gc
        final_x, final_c = mx, mc
        ctx.map_reset()
        assert ctx.map_size() == 0 and len(ctx.map_download()[0]) == 0
        assert ctx2.map_size() == len(final_x)                        # the second context's map is its own
        for hx, hc in chains:                                         # the host chain through add_cloud: the same bytes
            assert ctx.map_add_cloud(hx, hc, leaf)
        for c in (ctx, ctx2):
            gx, gc = c.map_download()
            assert _bits(gx).tobytes() == _bits(final_x).tobytes() and gc.tobytes() == final_c.tobytes()
        # the guard's soft failure leaves the map as it was
        assert not ctx.map_add_cloud(np.array([[6000, 8000, 0]], np.float32), None, 0.001)
        assert ctx.map_size() == len(final_x)
        assert _bits(ctx.map_download()[0]).tobytes() == _bits(final_x).tobytes()
        # a context destroyed with a non-empty map; a new one starts empty and works
        ctx2.close()
        ctx3 = R.Context(0)
        assert ctx3.map_size() == 0
        assert ctx3.map_add_cloud(chains[0][0], chains[0][1], leaf)
        wx, wc, ok = ctx.filter_voxel(chains[0][0], chains[0][1], leaf)
        gx, gc = ctx3.map_download()
        assert _bits(gx).tobytes() == _bits(wx).tobytes() and gc.tobytes() == wc.tobytes()
        # a frame whose sphereCloud was loaded goes through the host cloud: the same map
        pcd = str(tmp_path / "cloud0.pcd")
        frames[0].saveCloud(pcd, R.PCD_BINARY)
        g = R.Frame360(cal)
        frames.append(g)
        g.loadCloud(pcd)
        ctx3.map_reset()
        assert ctx3.map_add_frame(g, poses[0], leaf)
        gx, gc = ctx3.map_download()
        assert _bits(gx).tobytes() == _bits(wx).tobytes() and gc.tobytes() == wc.tobytes()
    finally:
        for f in frames or []:
            f.close()
        if cal is not None:
            cal.close()
        for c in (ctx3, ctx2, ctx):
            if c is not None:
                c.close()


def test_app_writes_the_map(tmp_path):
    exe = os.path.join(ROOT, "build", "bin", "SphereGraphTracking")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    out = str(tmp_path / "map.pcd")
    p = subprocess.run([exe, "--synthetic", "6", "--map", out], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    m = re.search(r"global map: (\d+) points", p.stdout)
    assert m and "6 keyframes" in p.stdout, p.stdout
    xyz, rgba, w, h = R.pcd_read(out)
    assert len(xyz) == int(m.group(1)) == w * h > 1000
    assert np.isfinite(xyz).all() and (rgba >> 24 == 0).all()
    keys = voxel_keys(xyz, 0.05)
    assert len(np.unique(keys, axis=0)) >= 0.999 * len(keys)          # one point per voxel, up to means on a face
