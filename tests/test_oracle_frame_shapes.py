"""CPU side of tests/test_gpu_frame_shapes.py: on the small ragged sensors, synthetic CLAMS models and crafted spheres
that file runs, the oracle's stitch, undistortion and the source-point model are not vacuous and reach the branches the
cases were made for.  What that file relies on is asserted here on the oracle alone (no GPU), so a generator that stops
producing it fails this test instead of letting the GPU comparison pass on empty output.

Measured on the oracle:
  stitch, sphere pixels filled with the rig's extrinsics / with the identity (half of the identity's come from rays
  behind the sensor, p2 <= 0), and the largest range in mm:
    2x2     32 of 32 / 12 of 32 (6 behind)   6213      10x14   87.6 % / 26.8 %   8127      50x70    94.7 % / 26.5 %   8587
    56x76   95.8 % / 27.2 %                  8578      96x128  95.7 % / 27.2 %   8643      100x134  95.6 % / 27.2 %   8656
  valid source points per level, rig extrinsics: 24 (2x2), 546 (10x14), 15240 6167 (50x70), 19175 7768 (56x76),
  57000 22861 5993 1526 384 96 (96x128: the last two levels are all valid), 61374 (100x134).
  undistortion branches (zero / idx0 < 0 / idx1 >= nb / low count / interpolated / past the last bin), the smallest and
  the largest of the 8 sensors:
    50x70              301-359 / 231-284 / 736-877 / 1210-1441 / 672-878 / 493-581
    48x64              281-335 / 205-228 / 669-719 / 1155-1254 / 601-684 / 453-493
    56x76              417-435 / 207-259 / 2581-2693 / 587-714 / 255-395 / 2352-2437
    50x70_ragged_bins  320-385 / 233-281 / 753-827 / 1301-1463 / 620-836 / 488-575"""
import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import (CLAMS_CASES, CLAMS_COUNTS, CLAMS_EDGE_MM, CRAFTED_KINDS, CRAFTED_SPHERES, FRAME_LEAN, FRAME_SHAPES,
                    IDENTITY_RTI, LIB_PI, SRC_BLOCK, SRC_GATE_MM, clams_branches, clams_depth, clams_tables,
                    crafted_sphere, frame_images, pyramid_depth, sphere_size, src_points_model, write_clams_models)

SHAPE_IDS = [f"{r}x{c}" for r, c in FRAME_SHAPES]
CHANGING = ("idx0_neg", "idx1_past", "low_count", "interpolated", "past_last_bin")


def _rig_rti():
    """The rig's inverse poses as the oracle's stitch takes them (float64 inverse: within an ulp of the library's)."""
    rt = O.read_extrinsics(R.EXTRINSICS_DIR).astype(np.float64)
    return np.concatenate([O.mat16(np.linalg.inv(m)) for m in rt])


def test_shapes_are_what_the_gpu_file_says():
    for (rows, cols), n in FRAME_SHAPES.items():
        H, W = sphere_size(rows)
        assert (H, W) == (int(8 * rows / 6), 8 * rows) and W % 16 == 0
        assert pyramid_depth(H, W) == n, (rows, cols)
    sph = {s: sphere_size(s[0]) for s in FRAME_SHAPES}
    assert sph[(2, 2)] == (2, 16) and sph[(10, 14)] == (13, 80) and sph[(100, 134)] == (133, 800)
    # tile rows of 64: one partial; full + 2; full + 10; two full; two full + 5
    assert [(sph[s][0] // 64, sph[s][0] % 64) for s in FRAME_SHAPES] == [(0, 2), (0, 13), (1, 2), (1, 10), (2, 0), (2, 5)]
    # compaction blocks of level 0: 50x70 has 7, the last partial; 96x128 exactly 24
    assert divmod(66 * 400, SRC_BLOCK) == (6, 1824) and divmod(128 * 768, SRC_BLOCK) == (24, 0)
    for s, lean in FRAME_LEAN.items():
        assert (sph[s][1] % 64 == 0) == lean
    assert [c % 4 for _, c in FRAME_SHAPES] == [2, 2, 2, 0, 0, 2]
    for rows, cols in CRAFTED_SPHERES:
        assert (rows, cols) in sph.values()
    # the model's angle step: the library's pi literal and numpy's give the same float at every level width in use
    widths = {W >> l for (_, W), n in zip(sph.values(), FRAME_SHAPES.values()) for l in range(n)}
    for C in widths:
        assert np.float32(2 * LIB_PI / C) == np.float32(2 * np.pi / C), C


def test_generators_are_deterministic():
    for rows, cols in ((10, 14), (56, 76)):
        (b, d), (b2, d2) = frame_images(rows, cols), frame_images(rows, cols)
        assert np.array_equal(b, b2) and np.array_equal(d, d2)
        assert b.shape == (8, rows, cols, 3) and b.dtype == np.uint8 and b.min() >= 1
        assert d.shape == (8, rows, cols) and d.dtype == np.uint16 and d.max() <= 6999
        assert not np.array_equal(frame_images(rows, cols, 1)[1], d)
    for name in CLAMS_CASES:
        assert np.array_equal(clams_depth(name), clams_depth(name))
        assert all(np.array_equal(a, b) for a, b in zip(clams_tables(name, 3), clams_tables(name, 3)))
        assert not np.array_equal(clams_tables(name, 3)[0], clams_tables(name, 4)[0])   # another seed per sensor
    a, b = crafted_sphere(66, 400, "blocks"), crafted_sphere(66, 400, "blocks")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", list(FRAME_SHAPES), ids=SHAPE_IDS)
def test_oracle_stitch_is_not_vacuous(shape):
    rows, cols = shape
    H, W = sphere_size(rows)
    b, d = frame_images(rows, cols)
    assert 0.17 < (d == 0).mean() < 0.23 or rows == 2
    K = O.camera_matrix(rows, cols)
    for extr, rti in (("rig", _rig_rti()), ("identity", IDENTITY_RTI)):
        sb, sd = O.stitch(b, d, rti, K)
        assert sb.shape == (H, W, 3) and sd.shape == (H, W)
        filled = sb.any(axis=2)                         # BGR is 1..255: a pixel the stitch wrote
        assert not sd[~filled].any()
        assert sd.max() < 9000, sd.max()                # 6999 mm * sqrt(1 + du^2 + dv^2): far from the uint16 cast's end
        fill = filled.mean()
        if extr == "rig":
            assert fill == 1.0 if rows == 2 else 0.85 < fill < 0.97, (extr, fill)
        else:
            assert 0.25 < fill < 0.40, (extr, fill)
            # the rays behind the sensor (p2 = cos phi cos theta <= 0 under the identity) fill pixels too: the mirrored
            # u, v pass the bounds test as the ones in front do
            theta = ((np.arange(W) + np.float32(-rows * 15 // 2 + 0.5)) * np.float32(2 * LIB_PI / W)).astype(np.float32)
            behind = np.cos(theta) <= 0
            assert filled[:, behind].sum() > 0 and filled[:, ~behind].sum() > 0, extr
        # every level of the pyramid has valid source points
        if extr == "rig":
            for lv in O.sphere_pyramid(sb, sd, FRAME_SHAPES[shape]):
                g, pts, dv = src_points_model(lv)
                assert 16 <= len(g) <= lv["depth"].size


@pytest.mark.parametrize("name", list(CLAMS_CASES))
def test_oracle_undistort_takes_every_branch(name, tmp_path):
    c = CLAMS_CASES[name]
    rows, cols = c["rows"], c["cols"]
    assert c["nx"] * c["bin_w"] >= cols and c["ny"] * c["bin_h"] >= rows
    assert (c["nx"] - 1) * c["bin_w"] < cols and (c["ny"] - 1) * c["bin_h"] < rows   # every frustum is used
    paths = write_clams_models(tmp_path, name)
    d = clams_depth(name)
    assert d.max() == 65535 and tuple(d[0].reshape(-1)[:len(CLAMS_EDGE_MM)]) == CLAMS_EDGE_MM
    assert 0.08 < (d == 0).mean() < 0.12
    for k in range(8):
        counts, mult = clams_tables(name, k)
        assert set(np.unique(counts)) == set(np.float32(CLAMS_COUNTS)) and mult.min() >= 0.9 and mult.max() <= 1.1
        z = O.depth_to_m(d[k])
        assert np.array_equal(z, d[k].astype(np.float32) * np.float32(0.001))
        cl = O.Clams(paths[k])
        out = cl.undistort(z)
        br = clams_branches(name, z, counts)
        parts = [br[key] for key in ("zero", "idx0_neg", "idx1_past", "low_count", "interpolated")]
        assert np.array_equal(sum(p.astype(int) for p in parts), np.ones((rows, cols), int))   # a partition
        assert not (br["past_last_bin"] & ~br["idx1_past"]).any()
        for key, m in br.items():
            assert m.sum() >= 100, (k, key, int(m.sum()))
        assert np.array_equal(out[br["zero"]], z[br["zero"]])
        for key in CHANGING:
            assert (out[br[key]] != z[br[key]]).any(), (k, key)
        # the pixels whose count is exactly 50 on one side and no lower on the other are interpolated, not scaled
        v, u = np.mgrid[0:rows, 0:cols]
        cnt = counts[v // c["bin_h"], u // c["bin_w"]]
        assert (br["interpolated"] & (cnt == 50).any(axis=2)).any(), k
        # the gate: the oracle leaves an image of another size alone
        other = np.ones((rows + 2, cols), np.float32)
        assert np.array_equal(cl.undistort(other), other)
    if name == "48x64":    # every quad of 4 columns spans two frustums
        assert c["bin_w"] == 2
    if name == "56x76":    # bin edges at columns that are no multiple of 4
        assert [e % 4 for e in range(c["bin_w"], cols, c["bin_w"])] == [3, 2, 1]
    if name == "50x70_ragged_bins":   # the table stride a sensor owns is not (rows / bin_h) * nx
        assert c["nx"] * c["ny"] != (rows // c["bin_h"]) * c["nx"] and c["ny"] == -(-rows // c["bin_h"])
    else:
        assert c["nx"] * c["ny"] == (rows // c["bin_h"]) * c["nx"]


@pytest.mark.parametrize("rows,cols", CRAFTED_SPHERES, ids=[f"{r}x{c}" for r, c in CRAFTED_SPHERES])
def test_crafted_spheres_hold_what_they_claim(rows, cols):
    n = pyramid_depth(rows, cols)
    assert n == {(66, 400): 2, (128, 768): 6}[(rows, cols)]
    assert rows * cols >= 3 * SRC_BLOCK
    for kind in CRAFTED_KINDS:
        bgr, dep = crafted_sphere(rows, cols, kind)
        assert bgr.shape == (rows, cols, 3) and dep.shape == (rows, cols) and dep.dtype == np.uint16
        ref = O.sphere_pyramid(bgr, dep, n)
        d0 = ref[0]["depth"].reshape(-1)
        valid = (d0 > np.float32(0.3)) & (d0 < np.float32(6.0))
        if kind == "blocks":
            assert not valid[SRC_BLOCK:2 * SRC_BLOCK].any() and valid[2 * SRC_BLOCK:3 * SRC_BLOCK].all()
            assert 0 < valid[:SRC_BLOCK].sum() < SRC_BLOCK and 0 < valid[3 * SRC_BLOCK:].sum() < valid[3 * SRC_BLOCK:].size
            assert {0, 299, 6001} <= set(np.unique(dep.reshape(-1)[SRC_BLOCK:2 * SRC_BLOCK]))
        elif kind == "zeros":
            assert not dep.any()
            for lv in ref:
                assert len(src_points_model(lv)[0]) == 0
        else:
            mm = dep.reshape(-1)
            assert set(np.unique(mm)) == set(SRC_GATE_MM)
            assert valid[(mm == 301) | (mm == 5999)].all() and not valid[(mm == 0) | (mm == 299) | (mm == 6001)].any()
            # 300 and 6000 mm: whatever the float32 product and the strict compare make of them, all pixels alike
            for edge in (300, 6000):
                assert len(set(valid[mm == edge])) == 1
            assert all(len(src_points_model(lv)[0]) > 0 for lv in ref)
        g, pts, dv = src_points_model(ref[0])
        assert len(g) == int(valid.sum()) and np.array_equal(g, ref[0]["gray"].reshape(-1)[valid])
        if len(g):
            # points at the pixel's depth, and a model off by one column is four orders outside the GPU file's bound
            assert np.allclose(np.linalg.norm(pts, axis=1), dv, rtol=1e-12)
            th = 2 * np.pi / cols
            moved = np.stack([pts[:, 0], pts[:, 1] * np.cos(th) + pts[:, 2] * np.sin(th),
                              pts[:, 2] * np.cos(th) - pts[:, 1] * np.sin(th)], axis=1)   # theta + one pixel
            assert (np.abs(moved - pts).max(axis=1) > 1e3 * 2.0 ** -21 * dv).all()
