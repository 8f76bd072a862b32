"""The frame front end (frame_kernels.hip: CLAMS undistortion, stitch, source-point compaction) on small ragged sensors,
through the public API and against the CPU oracle.  tests/test_oracle_frame_shapes.py asserts on the CPU that the cases
reach what they were made for (fill, branches, blocks, gate values).

1. Stitch, level 0 and the pyramid, bit for bit, on the six sensors of _cases.FRAME_SHAPES: spheres smaller than one
   64 x 16 tile, with an odd height, with a full tile row followed by a partial one, with two and three tile rows.
   Each with the rig's extrinsics and with the identity a calibration holds before it loads any (half of the pixels it
   fills come from rays behind the sensor, p2 <= 0).  Lean frames (setCompaction(False), W % 64 == 0) at 56x76 and
   96x128 through every first getter; 50x70 (W % 64 != 0) is never lean.
2. Undistortion against synthetic CLAMS models (_cases.CLAMS_CASES), bit for bit per sensor: the scalar kernel
   (cols % 4 == 2) undistorts here for the first time, k_undistort4 with quads that span two frustums, a second and
   third table geometry, and one whose bins do not divide the sensor (ny = ceil(rows / bin_h): the kernels took
   (rows / bin_h) * nx for the per-sensor table stride and read sensors 1..7 from the wrong frustums; it is the
   model's nx * ny now); a calibration of another size, or one without models, leaves depth_m = mm * 0.001f.
3. Source points against a float64 statement of the same operation (_cases.src_points_model): the count, the gray
   values bit for bit, and for every coordinate |got - model| <= 2^-21 * d.
   The bound is derived, not measured.  The kernel multiplies d by table entries that are sinf / cosf of the same
   float32 angle the model takes its float64 sine and cosine of: within 1 ulp, 2^-23 relative, each.  At most two
   entries meet in a coordinate (cos phi and sin / cos theta), and the two float32 products add 2^-24 each: 3 * 2^-23
   in all, rounded up to 2^-21.  A column off by one is an angle of 2 pi / C >= 7.8e-3 at C <= 800, four orders above
   the bound; swapped sin / cos tables or a flipped sign are of the order of d itself.
   Measured on an MI355X (recorded, not asserted; every case prints its own): the largest |got - model| / (2^-21 * d)
   over all cases is 0.3456 (level 0 of the 128x768 noise sphere), 0.33 on the stitched shapes.
   Run on every level of the six stitched shapes, on crafted spheres (a compaction block without a valid pixel next to
   one with 4096, no valid pixel at all, ranges on the strict 0.3 < d < 6.0 gate), and on levels whose compaction the
   build skipped (setCompaction(False)), asked for in the order 2, 0, 1, ... and compared with a full build's bytes."""
import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import (CLAMS_CASES, CRAFTED_KINDS, CRAFTED_SPHERES, FRAME_LEAN, FRAME_SHAPES, IDENTITY_RTI, clams_depth,
                    crafted_sphere, frame_images, noise_sphere, pyramid_depth, sphere_size, src_points_model,
                    write_clams_models)
from test_gpu_prep_fused import FIELDS, _check_against_oracle

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"{r}x{c}" for r, c in FRAME_SHAPES]
POINT_BOUND = 2.0 ** -21   # of the point's depth, per coordinate (derived in the docstring)


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


_CASES = {}


def _case(ctx, shape, extr):
    """The calibration, images and oracle results of a sensor shape, computed once per module and left unchanged."""
    key = (shape, extr)
    if key not in _CASES:
        rows, cols = shape
        cal = R.Calib360(ctx, rows, cols)
        if extr == "rig":
            cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
        _, rti, K = cal.extrinsics()
        if extr == "identity":   # the identity the library installs is the one the oracle is given
            assert np.array_equal(rti, IDENTITY_RTI)
            rti = IDENTITY_RTI
        b, d = frame_images(rows, cols)
        sb, sd = O.stitch(b, d, rti, K.reshape(3, 3).T)
        ref = O.sphere_pyramid(sb, sd, FRAME_SHAPES[shape])
        _CASES[key] = dict(cal=cal, rti=rti, K=K.reshape(3, 3).T, b=b, d=d, sb=sb, sd=sd, ref=ref)
    return _CASES[key]


# ---------------------------------------------------------------- 1. stitch, level 0 and the pyramid
@pytest.mark.parametrize("extr", ["rig", "identity"])
@pytest.mark.parametrize("shape", list(FRAME_SHAPES), ids=SHAPE_IDS)
def test_stitch_and_pyramid_bitexact(ctx, shape, extr):
    c = _case(ctx, shape, extr)
    n = FRAME_SHAPES[shape]
    f = R.Frame360(c["cal"])
    assert (f.sph_rows, f.sph_cols) == sphere_size(shape[0])
    f.upload(c["b"], c["d"])
    f.build()
    gb, gd = f.sphere()
    assert np.array_equal(gb, c["sb"]), np.argwhere((gb != c["sb"]).any(axis=2))[:8]
    assert np.array_equal(gd, c["sd"]), np.argwhere(gd != c["sd"])[:8]
    for l in range(n):
        got = f.level(l)
        assert got["gray"].shape == (f.sph_rows >> l, f.sph_cols >> l)
        for k in FIELDS:
            assert np.array_equal(got[k], c["ref"][l][k]), (l, k)
    with pytest.raises(RuntimeError):   # the pyramid stops where the test expects it to
        f.level(n)


@pytest.mark.parametrize("shape", list(FRAME_LEAN), ids=[f"{r}x{c}" for r, c in FRAME_LEAN])
def test_lean_frames_match_full_and_oracle(ctx, shape):
    """test_gpu_prep_fused.py's lean round on the ragged spheres: 74x448 and 128x768 are lean, 66x400 is not."""
    rows, cols = shape
    lean, n = FRAME_LEAN[shape], FRAME_SHAPES[shape]
    c = _case(ctx, shape, "rig")
    f, full = R.Frame360(c["cal"]), R.Frame360(c["cal"])
    f.setCompaction(False)
    # build -> getter -> re-upload -> build -> getter, each round entering through another getter
    for k, first in enumerate(("level0", "points0", "sphere")):
        b, d = frame_images(rows, cols, k)
        sb, sd = O.stitch(b, d, c["rti"], c["K"])
        ref = O.sphere_pyramid(sb, sd, n)
        for fr in (f, full):
            fr.upload(b, d)
            assert fr.built() == 0
            fr.build()
        assert full.built() & R.BUILT_LEVEL0
        assert bool(f.built() & R.BUILT_LEVEL0) == (not lean)
        with pytest.raises(RuntimeError):
            f.level(n)
        got = f.level(1)   # a level below 0 needs no level-0 output: the frame stays lean
        assert all(np.array_equal(got[key], ref[1][key]) for key in FIELDS)
        assert bool(f.built() & R.BUILT_LEVEL0) == (not lean)
        _check_against_oracle(f, full, ref, sb, sd, first)


# ---------------------------------------------------------------- 2. undistortion
def _depth_bits_equal(got, ref, what):
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("name", list(CLAMS_CASES))
def test_undistort_against_synthetic_models(ctx, name, tmp_path):
    c = CLAMS_CASES[name]
    rows, cols = c["rows"], c["cols"]
    paths = write_clams_models(tmp_path, name)
    d = clams_depth(name)
    plain = O.depth_to_m(d)
    cal = R.Calib360(ctx, rows, cols)
    cal.loadIntrinsicCalibration(str(tmp_path))
    f = R.Frame360(cal)
    f.upload(np.zeros((8, rows, cols, 3), np.uint8), d)
    f.build(R.BUILD_UNDISTORT)
    got = f.depth_m()
    for k in range(8):
        ref = O.Clams(paths[k]).undistort(plain[k])
        assert (ref != plain[k]).any()
        _depth_bits_equal(got[k], ref, (name, k))
    # the gate: models of another size are not applied (one more row pair: the same kernel; one more column pair: the
    # other one), nor is anything without models
    for r2, c2 in ((rows + 2, cols), (rows, cols + 2)):
        d2 = np.resize(d, (8, r2, c2))
        cal2 = R.Calib360(ctx, r2, c2)
        cal2.loadIntrinsicCalibration(str(tmp_path))
        f2 = R.Frame360(cal2)
        f2.upload(np.zeros((8, r2, c2, 3), np.uint8), d2)
        f2.build(R.BUILD_UNDISTORT)
        _depth_bits_equal(f2.depth_m(), O.depth_to_m(d2), (name, r2, c2))
    f3 = R.Frame360(R.Calib360(ctx, rows, cols))
    f3.upload(np.zeros((8, rows, cols, 3), np.uint8), d)
    f3.build(R.BUILD_UNDISTORT)
    _depth_bits_equal(f3.depth_m(), plain, (name, "no models"))


# ---------------------------------------------------------------- 3. source points
def _check_points(pts, lv, tag):
    g, model, dv = src_points_model(lv)
    assert pts.shape == (len(g), 4), (tag, pts.shape, len(g))
    assert np.array_equal(pts[:, 3].view(np.uint32), g.view(np.uint32)), tag
    if not len(g):
        return
    err = np.abs(pts[:, :3].astype(np.float64) - model) / dv.astype(np.float64)[:, None]
    print(f"{tag}: {len(g)} points, max |got - model| / (2^-21 d) = {err.max() / POINT_BOUND:.4f}")
    bad = np.argwhere(err > POINT_BOUND)
    assert len(bad) == 0, (tag, len(bad), bad[:8].tolist(), float(err.max()))


@pytest.mark.parametrize("shape", list(FRAME_SHAPES), ids=SHAPE_IDS)
def test_points_of_stitched_shapes(ctx, shape):
    c = _case(ctx, shape, "rig")
    f = R.Frame360(c["cal"])
    f.upload(c["b"], c["d"])
    f.build()
    for l in range(FRAME_SHAPES[shape]):
        _check_points(f.points(l), c["ref"][l], f"{shape[0]}x{shape[1]} level {l}")


@pytest.mark.parametrize("kind", CRAFTED_KINDS)
@pytest.mark.parametrize("rows,cols", CRAFTED_SPHERES, ids=[f"{r}x{c}" for r, c in CRAFTED_SPHERES])
def test_points_of_crafted_spheres(ctx, rows, cols, kind):
    n = pyramid_depth(rows, cols)
    bgr, dep = crafted_sphere(rows, cols, kind)
    ref = O.sphere_pyramid(bgr, dep, n)
    f = R.Frame360(R.Calib360.for_sphere(ctx, rows, cols))
    f.set_sphere(bgr, dep)
    for l in range(n):
        pts = f.points(l)
        if kind == "zeros":
            assert pts.shape == (0, 4), l
        _check_points(pts, ref[l], f"{kind} {rows}x{cols} level {l}")
    with pytest.raises(RuntimeError):
        f.points(n)


@pytest.mark.parametrize("kind", ["sensors_96x128", "sphere_128x768"])
def test_points_of_skipped_levels(ctx, kind):
    """A setCompaction(False) build compacts only the levels no batched pass streams (here levels 4 and 5; none of a
    3-level pyramid); the others are compacted one at a time when asked for."""
    if kind == "sensors_96x128":
        c = _case(ctx, (96, 128), "rig")
        cal, full_ref = c["cal"], c["ref"]

        def load(fr):
            fr.upload(c["b"], c["d"])
            fr.build()
    else:
        bgr, dep = noise_sphere(128, 768, 128768)
        cal, full_ref = R.Calib360.for_sphere(ctx, 128, 768), O.sphere_pyramid(bgr, dep, 6)

        def load(fr):
            fr.set_sphere(bgr, dep)
    f, full = R.Frame360(cal), R.Frame360(cal)
    f.setCompaction(False)
    for n in (6, 3):
        if n != 6:
            f.setNumPyr(n)
            full.setNumPyr(n)
        load(f)
        load(full)
        if kind == "sensors_96x128":
            assert not f.built() & R.BUILT_LEVEL0   # lean: level 0's points bring level 0 in
        for l in [2, 0, 1] + list(range(3, n)):
            pts = f.points(l)
            _check_points(pts, full_ref[l], f"skipped {kind} of {n} levels, level {l}")
            assert pts.tobytes() == full.points(l).tobytes(), (n, l)
            if kind == "sensors_96x128":
                assert bool(f.built() & R.BUILT_LEVEL0) == (l != 2)
        with pytest.raises(RuntimeError):
            f.points(n)
