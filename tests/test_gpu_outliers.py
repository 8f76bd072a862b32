"""The outlier filters on the GPU (r360_cloud_filter_outliers, r360_ctx_map_filter_outliers, r360_cloud_outlier_eval)
against the brute-force numpy statement tests/outlier_model.py.

Bounds, derived and not measured:
  * count (radius): exact.  The squared distances are the same float64 operations on both sides.
  * score (statistical): relative (k + 2) * 2^-52.  The k smallest squared distances are the same numbers on both sides
    and their square roots are correctly rounded on both; the device adds them ascending (k additions, half an ulp each)
    and divides once (half an ulp), the model adds them with fsum (one rounding) and divides once.
  * mean, stddev, threshold: relative 1e-9.  A fixed-order float64 sum of n positive terms differs from fsum by at
    most n * 2^-53 of the sum; the variance's cancellation multiplies the mean's share of that by (mean / stddev)^2.
    The worst cases here are the walls (n = 3030, mean / stddev 6.7: 1.5e-11) and the lattice (n = 125, 23.9: 8e-12).
  * kept set (statistical): identical outside the model's band |d - threshold| <= 1e-9 threshold, and every case first
    asserts that the band is empty (the seeds were chosen on the CPU so that it is), so the comparison is exact."""
import ctypes as C
import functools
import os
import re
import subprocess
import time

import numpy as np
import pytest

import outlier_model as OM
import rgbd360_amd as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
SEED = 360 << 16
SIZES_SEED = 12


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sor(k, mul, d):
    return R.OutlierParams.statistical(k, mul, d)


def _rad(r, m):
    return R.OutlierParams.radius_filter(r, m)


def _rel(a, b):
    return abs(a - b) <= 1e-9 * abs(b)


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def _colours(n, seed=5):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _check_statistical(ctx, xyz, k, mul, d, rgba=None, model=None):
    """Hook and filter parity of one statistical case; returns (model, kept xyz, kept rgba, stats)."""
    m = model if model is not None else OM.statistical(xyz, k, mul, d)
    assert len(m.band) == 0, ("the model's band is not empty: choose another seed", m.band, m.threshold)
    prm = _sor(k, mul, d)
    score = ctx.outlier_eval(xyz, prm)
    assert np.array_equal(np.isnan(score), ~m.finite)                           # dropped rows
    assert np.array_equal(np.isinf(score), m.short) and (score[m.short] > 0).all()
    ok = np.isfinite(m.d)
    err = np.abs(score[ok] - m.d[ok])
    bound = (k + 2) * 2.0 ** -52 * m.d[ok]
    print(f"statistical n={len(xyz)} k={k} mul={mul} D={d}: {int(m.short.sum())} short, {int(m.keep.sum())} kept, "
          f"max score err/bound {(err / np.maximum(bound, 1e-300)).max() if ok.any() else 0:.3f}, threshold {m.threshold:.9g}")
    assert (err <= bound).all()
    gx, gc, st = ctx.filter_outliers(xyz, rgba, prm)
    print(f"  mean {st.mean!r} / {m.mean!r}  stddev {st.stddev!r} / {m.stddev!r}  threshold {st.threshold!r} / {m.threshold!r}")
    assert _rel(st.mean, m.mean) and _rel(st.stddev, m.stddev) and _rel(st.threshold, m.threshold)
    assert (st.n_in, st.n_finite, st.n_short) == (len(xyz), int(m.finite.sum()), int(m.short.sum()))
    assert st.n_removed == len(xyz) - int(m.keep.sum())
    assert _bits(gx).tobytes() == _bits(np.asarray(xyz, np.float32)[m.keep]).tobytes()
    if rgba is not None:
        assert gc.tobytes() == rgba[m.keep].tobytes()
    return m, gx, gc, st


def _check_radius(ctx, xyz, r, mn, rgba=None, model=None):
    m = model if model is not None else OM.radius(xyz, r, mn)
    prm = _rad(r, mn)
    count = ctx.outlier_eval(xyz, prm)
    assert np.array_equal(count, m.c), np.flatnonzero(count != m.c)[:10]
    gx, gc, st = ctx.filter_outliers(xyz, rgba, prm)
    print(f"radius n={len(xyz)} r={r} min={mn}: {int(m.keep.sum())} kept")
    assert (st.n_in, st.n_finite, st.n_short, st.n_removed) == (len(xyz), int(m.finite.sum()), 0, len(xyz) - int(m.keep.sum()))
    assert (st.mean, st.stddev, st.threshold) == (0.0, 0.0, 0.0)
    assert _bits(gx).tobytes() == _bits(np.asarray(xyz, np.float32)[m.keep]).tobytes()
    if rgba is not None:
        assert gc.tobytes() == rgba[m.keep].tobytes()
    return m, gx, gc, st


# ------------------------------------------------------------------ clouds
@functools.lru_cache(maxsize=None)
def box_cloud():
    """257 random points in a 1 m box; the sizes take its prefixes."""
    return np.random.default_rng(SIZES_SEED).uniform(0, 1, (257, 3)).astype(np.float32)


def sizes_for(k):
    return sorted({1, 2, k, k + 1, 63, 64, 65, 257})


@functools.lru_cache(maxsize=None)
def walls_scene(per=1000, planted=30, seed=7):
    """Two walls (x = 0 and y = 0) and a floor (z = 0) of 4 m x 4 m with 5 mm noise, `per` points each, plus `planted`
    points in free space, at least 0.6 m from every surface; shuffled."""
    rng = np.random.default_rng(seed)
    parts = []
    for axis in range(3):
        p = rng.uniform(0, 4, (per, 3))
        p[:, axis] = rng.normal(0, 0.005, per)
        parts.append(p)
    free = rng.uniform(0.6, 3.8, (planted, 3))
    xyz = np.vstack(parts + [free]).astype(np.float32)
    is_planted = np.arange(len(xyz)) >= 3 * per
    p = rng.permutation(len(xyz))
    return xyz[p], is_planted[p]


def lattice(e, side=4):
    """side^3 points whose coordinates are multiples of e (float32 products of small integers), around the origin."""
    g = np.arange(side) - side // 2
    i, j, k = np.meshgrid(g, g, g, indexing="ij")
    return (np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float32) * np.float32(e)).astype(np.float32)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("k", [1, 4, 20, 64])
def test_sizes_statistical(ctx, k):
    xyz = box_cloud()
    for n in sizes_for(k):
        m, gx, _, st = _check_statistical(ctx, xyz[:n], k, 1.0, 0.5)
        if n <= k:
            assert m.short.all() and len(gx) == 0 and st.n_short == n


@pytest.mark.parametrize("r,mn", [(0.15, 5), (0.3, 1), (0.15, 0)])
def test_sizes_radius(ctx, r, mn):
    xyz = box_cloud()
    for n in (1, 2, 20, 21, 63, 64, 65, 257):
        _check_radius(ctx, xyz[:n], r, mn)


def test_points_on_cell_faces(ctx):
    """Coordinates that are multiples of the search bound: every point lies on a face of the cell grid, and its
    axis neighbours are at exactly the bound (inside: the interval is closed)."""
    for e in (0.25, 0.15, 0.3):
        p = lattice(e)
        m, *_ = _check_radius(ctx, p, e, 4)
        if e == 0.25:                                # exact in float32: the axis neighbours are at exactly the radius
            assert m.c.max() == 6 and m.c.min() == 3
        _check_radius(ctx, p, e, 6)
        _check_radius(ctx, lattice(e / 2, 5), e, 12)
    for e in (0.5, 0.3):
        # spacing e / 2, 5^3 points.  A corner has 3 + 3 + 1 others at s, s sqrt 2, s sqrt 3 and 3 at 2 s = max_dist
        # exactly: with k = 10 its k-th is at the bound (not short, the comparison is strict), with k = 11 it is short
        p = lattice(e / 2, 5)
        m, *_ = _check_statistical(ctx, p, 10, 1.5, e)
        if e == 0.5:
            assert not m.short.any()
        m, *_ = _check_statistical(ctx, p, 11, 1.5, e)
        if e == 0.5:
            assert m.short.sum() == 8


def test_one_cell_and_duplicates(ctx):
    rng = np.random.default_rng(21)
    one = (np.array([10.26, -3.26, 0.26]) + rng.uniform(0, 0.04, (200, 3))).astype(np.float32)   # inside one 0.075 m cell
    _check_statistical(ctx, one, 20, 1.0, 0.5)
    _check_statistical(ctx, one, 8, 2.0, 0.15)
    _check_radius(ctx, one, 0.15, 5)
    _check_radius(ctx, one, 0.01, 2)
    dup = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (300, 1))
    rg = _colours(300)
    # every d is 0 = the threshold: the band is the whole cloud by construction, so compare the kept set directly
    prm = _sor(20, 1.0, 0.5)
    score = ctx.outlier_eval(dup, prm)
    assert (score == 0.0).all()
    gx, gc, st = ctx.filter_outliers(dup, rg, prm)
    assert len(gx) == 300 and gc.tobytes() == rg.tobytes() and (st.mean, st.stddev, st.threshold, st.n_short) == (0, 0, 0, 0)
    m, gx, *_ = _check_radius(ctx, dup, 0.15, 5, rg)
    assert (m.c == 299).all() and len(gx) == 300


def test_extent(ctx):
    """A 1,000-point cluster plus single points at 50 m and at 4,000 m: the far points are short / have no neighbour,
    and the call does not take longer for them (a walk over the rings between would take 10^4 .. 10^12 cell visits)."""
    rng = np.random.default_rng(33)
    cluster = rng.uniform(0, 1, (1000, 3)).astype(np.float32)
    far = np.vstack([cluster, [[50.0, 0.2, 0.3]], [[-4000.0, 4000.0, 3999.5]]]).astype(np.float32)
    ms = OM.statistical(far, 20, 1.0, 0.5)
    assert ms.short[1000] and ms.short[1001]
    _check_statistical(ctx, far, 20, 1.0, 0.5, model=ms)
    mr, *_ = _check_radius(ctx, far, 0.15, 5)
    assert mr.c[1000] == 0 and mr.c[1001] == 0

    def timed(p, prm):
        ctx.filter_outliers(p, None, prm)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.filter_outliers(p, None, prm)
            t.append(time.perf_counter() - t0)
        return min(t)
    for prm in (_sor(20, 1.0, 0.5), _rad(0.15, 5)):
        near_t, far_t = timed(cluster, prm), timed(far, prm)
        print(f"kind {prm.kind}: cluster {near_t * 1e3:.2f} ms, with the far points {far_t * 1e3:.2f} ms")
        assert far_t < 3 * near_t + 0.02


def test_non_finite_rows_aliasing_and_capacity(ctx):
    xyz, _ = walls_scene(per=85, planted=2, seed=9)           # 257 points
    xyz = xyz.copy()
    rgba = _colours(len(xyz))
    bad = np.arange(3, len(xyz), 7)
    xyz[bad[0::3], 0] = np.nan
    xyz[bad[1::3], 1] = np.inf
    xyz[bad[2::3], 2] = -np.inf
    ms, *_ = _check_statistical(ctx, xyz, 4, 1.0, 0.5, rgba)
    mr, wx, wc, _ = _check_radius(ctx, xyz, 0.3, 1, rgba)
    assert not ms.keep[bad].any() and not mr.keep[bad].any()
    L = R.lib()
    for prm, model in ((_sor(4, 1.0, 0.5), ms), (_rad(0.3, 1), mr)):
        want_x, want_c = xyz[model.keep], rgba[model.keep]
        ax, ac = xyz.copy(), rgba.copy()                      # the outputs are the inputs
        n = C.c_size_t()
        rc = L.r360_cloud_filter_outliers(ctx.h, R._fptr(ax), R._vptr(ac), len(ax), C.byref(prm), R._fptr(ax), R._vptr(ac),
                                          len(ax), C.byref(n), None)
        assert rc == 0 and n.value == len(want_x)
        assert _bits(ax[:n.value]).tobytes() == _bits(want_x).tobytes() and ac[:n.value].tobytes() == want_c.tobytes()
        ox, oc = np.zeros((len(xyz), 3), np.float32), np.zeros(len(xyz), np.uint32)
        n = C.c_size_t()
        rc = L.r360_cloud_filter_outliers(ctx.h, R._fptr(xyz), R._vptr(rgba), len(xyz), C.byref(prm), R._fptr(ox), R._vptr(oc),
                                          len(want_x) - 1, C.byref(n), None)
        assert rc < 0 and n.value == len(want_x) and b"capacity" in L.r360_last_error()
        assert not ox.any() and not oc.any()
        # no colours
        gx, gc, _ = ctx.filter_outliers(xyz, None, prm)
        assert gc is None and _bits(gx).tobytes() == _bits(want_x).tobytes()
    # nothing finite, and nothing at all
    nothing = np.full((5, 3), np.nan, np.float32)
    for prm in (_sor(4, 1.0, 0.5), _rad(0.3, 0)):
        gx, _, st = ctx.filter_outliers(nothing, None, prm)
        assert len(gx) == 0 and (st.n_in, st.n_finite, st.n_removed) == (5, 0, 5)
        gx, _, st = ctx.filter_outliers(np.zeros((0, 3), np.float32), None, prm)
        assert len(gx) == 0 and st.n_in == 0
    assert np.isnan(ctx.outlier_eval(nothing, _sor(4, 1.0, 0.5))).all()
    assert (ctx.outlier_eval(nothing, _rad(0.3, 0)) == -1).all()


@pytest.mark.parametrize("k,mul,d", [(20, 1.0, 0.5), (8, 2.0, 0.5)])
def test_walls_statistical(ctx, k, mul, d):
    xyz, planted = walls_scene()
    rgba = _colours(len(xyz))
    m, *_ = _check_statistical(ctx, xyz, k, mul, d, rgba)
    assert planted.sum() == 30 and not m.keep[planted].any()          # every planted point goes
    assert m.keep[~planted].mean() > 0.8
    gap = np.abs(m.d[np.isfinite(m.d)] - m.threshold).min() / m.threshold
    print(f"closest non-short point to the threshold: {gap:.3g} (relative)")


@pytest.mark.parametrize("r,mn", [(0.15, 5), (0.3, 1)])
def test_walls_radius(ctx, r, mn):
    xyz, planted = walls_scene()
    m, *_ = _check_radius(ctx, xyz, r, mn, _colours(len(xyz)))
    assert not m.keep[planted].any()


def test_walls_small(ctx):
    xyz, _ = walls_scene(per=85, planted=2, seed=9)
    assert len(xyz) == 257
    _check_statistical(ctx, xyz, 4, 1.0, 0.5)


def test_deterministic_and_order_independent(ctx):
    xyz, _ = walls_scene()
    rgba = _colours(len(xyz))
    p = np.random.default_rng(2).permutation(len(xyz))
    for prm, model in ((_sor(20, 1.0, 0.5), OM.statistical(xyz, 20, 1.0, 0.5)), (_rad(0.15, 5), None)):
        ax, ac, ast = ctx.filter_outliers(xyz, rgba, prm)
        ea = ctx.outlier_eval(xyz, prm)
        bx, bc, bst = ctx.filter_outliers(xyz, rgba, prm)
        eb = ctx.outlier_eval(xyz, prm)
        assert _bits(ax).tobytes() == _bits(bx).tobytes() and ac.tobytes() == bc.tobytes()
        assert ea.tobytes() == eb.tobytes() and bytes(ast) == bytes(bst)
        if model is not None:
            assert len(model.band) == 0
            keep = model.keep
        else:
            keep = OM.radius(xyz, 0.15, 5).keep
        px, pc, _ = ctx.filter_outliers(xyz[p], rgba[p], prm)
        assert _bits(px).tobytes() == _bits(xyz[p][keep[p]]).tobytes() and pc.tobytes() == rgba[p][keep[p]].tobytes()
        ep = ctx.outlier_eval(xyz[p], prm)
        assert ep.tobytes() == ea[p].tobytes()                 # a point's score / count does not depend on the order


def _voxel_index(xyz, leaf=0.05):
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(xyz.astype(np.float32) * inv).astype(np.int64)


def test_context_map():
    leaf = 0.05
    ctx, ctx2 = R.Context(0), R.Context(0)
    cal = frames = None
    try:
        # an empty map: zeros
        st = ctx.map_filter_outliers(_rad(0.15, 5))
        assert (st.n_in, st.n_finite, st.n_short, st.n_removed, st.mean, st.threshold) == (0, 0, 0, 0, 0.0, 0.0)
        assert ctx.map_size() == 0
        cal = R.Calib360(ctx, 240, 320)
        cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
        frames = []
        for k in range(2):
            pose = R.synth_path_pose(SEED, 2 * k)
            bgr, dep = cal.synth_frame(SEED, pose)
            f = R.Frame360(cal)
            frames.append(f)
            f.upload(bgr, dep)
            f.build(R.BUILD_UNDISTORT | R.BUILD_CLOUD)
            assert ctx.map_add_frame(f, pose, leaf)
        rng = np.random.default_rng(17)
        mx, _ = ctx.map_download()
        lo, hi = mx.min(0), mx.max(0)
        planted = rng.uniform(lo - 3.0, hi + 3.0, (20, 3)).astype(np.float32)
        assert ctx.map_add_cloud(planted, _colours(20), leaf)
        for prm in (_rad(0.15, 5), _sor(20, 1.0, 0.5)):
            mx, mc = ctx.map_download()
            n0 = len(mx)
            # invalid parameters: an error, and the map as it was
            bad = R.OutlierParams.default()
            bad.kind, bad.radius, bad.mean_k = prm.kind, -1.0, 0
            with pytest.raises(RuntimeError):
                ctx.map_filter_outliers(bad)
            assert ctx.map_size() == n0
            st = ctx.map_filter_outliers(prm)
            wx, wc, wst = ctx2.filter_outliers(mx, mc, prm)
            gx, gc = ctx.map_download()
            print(f"map kind {prm.kind}: {n0} -> {len(gx)} points, {st.n_short} short")
            assert 0 < len(gx) < n0 and ctx.map_size() == len(gx) == len(wx)
            assert _bits(gx).tobytes() == _bits(wx).tobytes() and gc.tobytes() == wc.tobytes()
            assert bytes(st) == bytes(wst) and st.n_in == n0 and st.n_removed == n0 - len(gx)
            # still one point per voxel in ascending (k, j, i) order
            ijk = _voxel_index(gx)
            order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
            assert np.array_equal(order, np.arange(len(gx))) and len(np.unique(ijk, axis=0)) == len(gx)
            # the map goes on from the result
            extra = rng.uniform(lo, hi, (500, 3)).astype(np.float32)
            ec = _colours(500, 6)
            assert ctx.map_add_cloud(extra, ec, leaf)
            ax, ac = ctx.map_download()
            vx, vc, ok = ctx2.filter_voxel(np.vstack([gx, extra]), np.concatenate([gc, ec]), leaf)
            assert ok and _bits(ax).tobytes() == _bits(vx).tobytes() and ac.tobytes() == vc.tobytes()
    finally:
        for f in frames or []:
            f.close()
        if cal is not None:
            cal.close()
        ctx.close()
        ctx2.close()


def test_dropin_runs():
    exe = os.path.join(BIN, "outlier_dropin")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, R.SAMPLES_DIR, "1", "1"], capture_output=True, text=True, timeout=100)
    print(p.stdout)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    assert "maps identical" in p.stdout
    m = re.search(r"radius \(0\.15, 5\): (\d+) -> (\d+) points", p.stdout)
    assert m and 0 < int(m.group(2)) <= int(m.group(1))


def test_app_cleans_the_map():
    exe = os.path.join(BIN, "KFsphereSLAM")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    args = ["--synthetic-frames", "0,4,8,12,16", "1"]
    plain = subprocess.run([exe, *args], capture_output=True, text=True, timeout=100)
    clean = subprocess.run([exe, *args, "--clean-map", "radius:0.15,5"], capture_output=True, text=True, timeout=100)
    assert plain.returncode == 0 and clean.returncode == 0, plain.stderr + clean.stderr
    lines = clean.stdout.splitlines()
    m = re.fullmatch(r"map cleaned: (\d+) -> (\d+) points \((\d+) short\)", lines[-1])
    assert m, lines[-3:]
    print(lines[-1])
    assert int(m.group(2)) <= int(m.group(1)) and int(m.group(3)) == 0
    assert "\n".join(lines[:-1]) == plain.stdout.rstrip("\n")
    sizes = re.search(r"global map: (\d+) points at the chained poses, (\d+) at the optimised poses", clean.stdout)
    assert int(sizes.group(2)) == int(m.group(1))
