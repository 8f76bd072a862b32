"""CPU side of tests/test_gpu_sensor_shapes.py: on the small ragged sensors, poses and capture cut-outs that file runs,
the cases reach what they were made for.  Asserted with the oracle and plain arithmetic only (no GPU), so a generator or
a pose that stops producing it fails here instead of letting the GPU comparison pass on a case that no longer bites.

Measured on the oracle:
  the larger motion keeps 0.48 .. 0.56 of the valid source pixels in view on every `noise` level of at least 256 px
  (0.51 .. 0.54 at level 0); the two small twists keep 0.90 .. 1.0.
  stability census (stable sensors of 8 under the 12-nudge rule / sensors the oracle returns ILL-POSED):
    dec  PHOTO_DEPTH 7 (sensor 6 drifts 5.0e-4 rad, 1.4e-3 m) / none     DEPTH_CONSISTENCY 8 / none
    crop PHOTO_DEPTH 7 (sensor 5 drifts 0.15 rad, 0.21 m)     / 4, 5, 7  DEPTH_CONSISTENCY 8 / 4, 7"""
import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import (PASS_TPB, SENSOR_CAPTURES, SENSOR_LARGE_POSE, SENSOR_MAX_PYR, SENSOR_SHAPES, pass_blocks,
                    pin_thread_classes, sensor_align_census, sensor_captures, sensor_images, sensor_levels,
                    sensor_poses)

SHAPE_IDS = [f"{r}x{c}" for r, c in SENSOR_SHAPES]
METHODS = (O.PHOTO, O.DEPTH, O.PHOTO_DEPTH)
# per shape and level: (workgroups per job, the classes its threads fall in)
T, P, PT, I = "tail_only", "pair_only", "pair_and_tail", "idle"
BLOCKS_AND_CLASSES = {
    (2, 2): [(1, {T, I})],
    (10, 14): [(1, {T, I}), (1, {T, I})],
    (50, 70): [(4, {P, PT}), (1, {P, PT})],
    (56, 76): [(5, {P, PT}), (2, {P, PT}), (1, {P, T})],
    (96, 128): [(12, {P}), (3, {P}), (1, {PT}), (1, {T, I}), (1, {T, I})],
    (100, 134): [(14, {P, PT}), (4, {P, PT})],
    (120, 160): [(19, {P, PT}), (5, {P, PT}), (2, {P, PT}), (1, {P, T})],
}


# 0 < n_vis < npx holds at every non-identity pose on every level of at least 256 px but these two (level, pose index):
# the 14 x 19 and 15 x 20 levels are level 2 and 3 of their pyramids, where every pixel is valid (a 2 x 2 mean is
# invalid only if all four are) and the first small twist moves a point by 0.01 rad * 16.4 px of focal length = 0.16 px,
# so none leaves: n_vis == npx there, asserted as such
WHOLE_IN_VIEW = {((14, 19), 1), ((15, 20), 1)}


def test_level_table():
    last = {(2, 2): (2, 2), (10, 14): (5, 7), (50, 70): (25, 35), (56, 76): (14, 19), (96, 128): (6, 8),
            (100, 134): (50, 67), (120, 160): (15, 20)}
    assert list(SENSOR_SHAPES) == list(last)
    for (rows, cols), n in SENSOR_SHAPES.items():
        assert rows % 2 == 0 and cols % 2 == 0            # r360_calib_create's requirement
        lv = sensor_levels(rows, cols)
        assert len(lv) == n <= SENSOR_MAX_PYR and lv[-1] == last[(rows, cols)], (rows, cols, lv)
        assert lv == [(rows >> l, cols >> l) for l in range(n)]
        assert 8 * rows * cols <= 8 * 120 * 160
    # what the last levels are here for: odd in both directions, odd columns only, odd rows only, below one wave
    assert [(r % 2, c % 2) for r, c in last.values()] == [(0, 0), (1, 1), (1, 1), (0, 1), (0, 0), (0, 1), (1, 0)]
    assert 5 * 7 < 64 and 6 * 8 < 64
    assert 8 * SENSOR_SHAPES[(96, 128)] == 40             # rig-frame jobs of one launch
    # the capture cut-outs are two of the shapes
    assert SENSOR_CAPTURES == {"dec": SENSOR_SHAPES[(120, 160)], "crop": SENSOR_SHAPES[(56, 76)]}


def test_workgroups_and_thread_classes():
    for shape, want in BLOCKS_AND_CLASSES.items():
        lv = sensor_levels(*shape)
        assert len(lv) == len(want)
        for (r, c), (nb, classes) in zip(lv, want):
            npx = r * c
            assert pass_blocks(npx) == min(256, -(-npx // 1024)) == nb, (shape, r, c)
            got, covered = pin_thread_classes(npx)
            assert covered == npx and sum(got.values()) == nb * PASS_TPB
            assert {k for k, v in got.items() if v} == classes, (shape, r, c, got)
    # the counts the table of cases names
    assert pin_thread_classes(14 * 19)[0] == dict(idle=0, tail_only=246, pair_only=10, pair_and_tail=0)
    assert pin_thread_classes(28 * 38)[0] == dict(idle=0, tail_only=0, pair_only=472, pair_and_tail=40)
    assert 96 * 128 == 4 * 12 * PASS_TPB and 48 * 64 == 4 * 3 * PASS_TPB      # exactly 4 strides
    assert round(3500 / (4 * PASS_TPB), 2) == 3.42 and round(13400 / (14 * PASS_TPB), 2) == 3.74
    # a last workgroup (or wave) that is only partly inside the image
    for npx in (3500, 4256, 13400, 3350, 1200, 266, 140, 35):
        assert npx % PASS_TPB and npx % 64


def test_generators_are_deterministic():
    for rows, cols in ((10, 14), (56, 76)):
        (b, d), (b2, d2) = sensor_images(rows, cols, "target"), sensor_images(rows, cols, "target")
        assert np.array_equal(b, b2) and np.array_equal(d, d2)
        assert b.shape == (8, rows, cols, 3) and b.dtype == np.uint8
        assert d.shape == (8, rows, cols) and d.dtype == np.uint16 and d.max() <= 6999
        assert 0.1 < (d == 0).mean() < 0.3
        for other in ("source", "other"):
            assert not np.array_equal(sensor_images(rows, cols, other)[1], d)
    for kind, shape in (("dec", (120, 160)), ("crop", (56, 76))):
        for b, d in sensor_captures(kind, R.SAMPLES_DIR):
            assert b.shape == (8,) + shape + (3,) and d.shape == (8,) + shape
            assert b.flags.c_contiguous and d.flags.c_contiguous


def test_poses_keep_every_point_in_front():
    """The oracle's depth term is NaN behind the camera (stdDevDepth * Z < 0): no pose may put a point there.  Every
    valid pixel of every shape's level 0, at the nearest and the farthest valid depth."""
    for rows, cols in SENSOR_SHAPES:
        K = O.Pinhole.rgbd360(rows, cols)
        v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
        for z in (0.3, 6.0):
            pts = np.stack([(u - K.ox) * z / K.fx, (v - K.oy) * z / K.fy, np.full_like(u, z), np.ones_like(u)], -1)
            for Pm in sensor_poses():
                assert (pts @ Pm.astype(np.float64).T)[..., 2].min() > 0.05, (rows, cols, z)


@pytest.mark.parametrize("shape", list(SENSOR_SHAPES), ids=SHAPE_IDS)
def test_visibility_windows(shape):
    rows, cols = shape
    n = SENSOR_SHAPES[shape]
    lv = sensor_levels(rows, cols)
    (bt, dt), (bs, ds) = sensor_images(rows, cols, "target"), sensor_images(rows, cols, "source")
    K = O.Pinhole.rgbd360(rows, cols)
    poses = sensor_poses()
    for k in (0, 3, 7):
        pt, ps = O.sensor_pyramid(bt[k], dt[k], n), O.sensor_pyramid(bs[k], ds[k], n)
        for l in range(n):
            assert ps[l]["gray"].shape == lv[l]
            npx = lv[l][0] * lv[l][1]
            dep = ps[l]["depth"]
            nvalid = int(((dep > np.float32(0.3)) & (dep < np.float32(6.0))).sum())
            assert 0 < nvalid <= npx
            for j, Pm in enumerate(poses):
                H, g, nvis = O.hessgrad_pinhole(ps[l], pt[l], K, l, Pm, O.PHOTO_DEPTH)
                e, nP, nD, rP, rD = O.error_pinhole(ps[l], pt[l], K, l, Pm, O.PHOTO_DEPTH)
                assert nP == nvis and np.isfinite(rP) and np.isfinite(rD), (k, l, j)
                if j == 0:
                    assert nvis == nvalid                     # the identity keeps every valid pixel
                    continue
                if npx < 256:
                    continue
                if (lv[l], j) in WHOLE_IN_VIEW:
                    assert nvis == nvalid == npx, (k, l, j, nvis)
                    continue
                assert 0 < nvis < npx, (k, l, j, nvis)
                if j == SENSOR_LARGE_POSE:
                    assert 0.25 * nvalid <= nvis <= 0.75 * nvalid, (k, l, nvis, nvalid)
            if npx >= 256:                                    # the pass is not vacuous: H has weight
                H, g, _ = O.hessgrad_pinhole(ps[l], pt[l], K, l, poses[1], O.PHOTO_DEPTH)
                assert np.abs(H).max() > 0 and np.abs(g).max() > 0


def test_2x2_has_no_gradient():
    """Every pixel of a 2 x 2 image is a border pixel: gradients zero, every point fails the saliency test, H = g = 0
    with every method, at every pose, while pixels are still in view."""
    (bt, dt), (bs, ds) = sensor_images(2, 2, "target"), sensor_images(2, 2, "source")
    K = O.Pinhole.rgbd360(2, 2)
    seen = 0
    for k in range(8):
        pt, ps = O.sensor_pyramid(bt[k], dt[k], 1)[0], O.sensor_pyramid(bs[k], ds[k], 1)[0]
        assert not any(pt[key].any() for key in ("gx", "gy", "dgx", "dgy"))
        for Pm in sensor_poses():
            for m in METHODS:
                H, g, nvis = O.hessgrad_pinhole(ps, pt, K, 0, Pm, m)
                assert not H.any() and not g.any()
                seen += nvis
    assert seen > 0


@pytest.mark.parametrize("kind", list(SENSOR_CAPTURES))
def test_stability_census(kind):
    """What tests/test_gpu_sensor_shapes.py's whole alignments rely on: at least 6 of the 8 sensors are compared by
    pose in each run, and `crop` has ILL-POSED sensors (lm_step_wave's rank exit)."""
    want = {("dec", O.PHOTO_DEPTH): (7, []), ("dec", O.DEPTH): (8, []),
            ("crop", O.PHOTO_DEPTH): (7, [4, 5, 7]), ("crop", O.DEPTH): (8, [4, 7])}
    for m in (O.PHOTO_DEPTH, O.DEPTH):
        c = sensor_align_census(kind, m, R.SAMPLES_DIR)
        stable = [k for k in range(8) if c[k]["stable"]]
        ill = [k for k in range(8) if c[k]["ref"][0] == 1]
        print(kind, m, "stable", stable, "ill-posed", ill, "drifts", [x["drift"] for x in c])
        assert (len(stable), ill) == want[(kind, m)], (kind, m, stable, ill)
        assert len(stable) >= 6
        if kind == "crop":
            assert any(k in stable for k in ill)              # an ILL-POSED sensor is among the compared ones
        # the solves iterate: the comparison is of Levenberg-Marquardt paths, not of untouched starts
        assert sum(sum(x["ref"][4].iters[:SENSOR_CAPTURES[kind]]) > 0 for x in c) >= 6
    if kind == "crop":   # the rig-frame call on `crop`: every level's loop runs, and the call succeeds
        (b1, d1), (b2, d2) = sensor_captures("crop", R.SAMPLES_DIR)
        rt = O.read_extrinsics(R.EXTRINSICS_DIR)
        rti = np.stack([np.linalg.inv(m.astype(np.float64)).astype(np.float32) for m in rt])
        ok, _, _, st = O.register_dense_robot(b1, d1, b2, d2, rt, rti, sensor_poses()[1], O.PHOTO,
                                              O.IcpParams.default(n_pyr=3))
        assert ok and list(st.ran[:4]) == [1, 1, 1, 0]
