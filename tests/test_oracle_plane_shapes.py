"""CPU side of tests/test_gpu_plane_shapes.py: on the ragged sensor sizes and the crafted label fields that file runs,
the oracle's plane stage is not vacuous and reaches the paths the fields were made for.  The floors that file relies
on are asserted here on the oracle alone (no GPU), so a generator that stops producing them fails this test instead
of letting the GPU comparison pass on empty output.

Measured on the oracle (sensors with regions / contour-less regions / traced regions / pixels changed by the
refinement / PbMap planes, for seeds 360 << 16 and that + 7):
    66x90    7, 7 sensors    5, 8    3, 0     2 744, 2 992       4, 5
    130x250  8, 8           18, 20  12, 9    19 674, 20 292     21, 23
    34x400   3, 3            2, 1    1, 2     3 973, 739         1, 2
    258x70   8, 8            6, 8   16, 14    6 926, 7 934       8, 6
    32x162   0, 0            -       -        0, 0               0, 0
    100x132  8, 8            7, 7    6, 6     4 552, 4 814       8, 8
    194x258  8, 8           17, 20  14, 13   23 551, 25 657     15, 17
    512x768  8, 8           28, 28  27, 25  140 422, 129 441    19, 19
    516x768  8, 8           28, 29  29, 23  141 839, 132 936    19, 18
Not every sensor with regions has both kinds (130x250, sensor 3: three regions, none traced), so the two kinds are
asserted per frame, and per sensor only their sum."""
import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import (PLANE_SEEDS, PLANE_SHAPES, STRIPE_CASES, depth_metres, per_sensor_oracle, span_keys, stripe_frame,
                    stripe_oracle, stripe_sensor)

# (rows, cols) -> per seed: sensors with regions, at least this many pixels changed by the refinement
FLOORS = {(66, 90): ((7, 2000), (7, 2000)), (130, 250): ((8, 15000), (8, 15000)), (34, 400): ((3, 500), (3, 500)),
          (258, 70): ((8, 5000), (8, 5000)), (32, 162): ((0, 0), (0, 0)), (100, 132): ((8, 3000), (8, 3000)),
          (194, 258): ((8, 20000), (8, 20000)), (512, 768): ((8, 100000), (8, 100000)),
          (516, 768): ((8, 100000), (8, 100000))}
# sizes whose frames hold regions without a contour (voxel fallback) and traced regions, in every sensor's share of
# one frame or another; 6 or more PbMap planes
FULL = {(130, 250), (258, 70), (100, 132), (194, 258), (512, 768), (516, 768)}


@pytest.fixture(scope="module")
def rt():
    return O.read_extrinsics(R.EXTRINSICS_DIR)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_plane_stage_is_not_vacuous(rt, shape, k):
    rows, cols = shape
    seed = PLANE_SEEDS[k]
    b, d = R.synth_frame_rt(rows, cols, rt, seed, R.synth_path_pose(seed, 0))
    assert d.any() and b.any()
    dm = depth_metres(d)
    ref = per_sensor_oracle(b, dm)
    nreg = [len(r["regs"]) for r in ref]
    nocont = sum(1 for r in ref for g in r["regs"] if len(g["contour"]) == 0)
    traced = sum(1 for r in ref for g in r["regs"] if len(g["contour"]) > 0)
    grown = sum(int((r["lf"] != r["lc"]).sum()) for r in ref)
    with_regions, min_grown = FLOORS[shape][k]
    assert sum(1 for n in nreg if n) == with_regions, nreg
    if shape == (32, 162):
        assert nreg == [0] * 8 and grown == 0
        assert all(np.isnan(r["nrm"][..., 0]).all() for r in ref)   # the normals' border of 8 eats the 16-row image
        return
    assert grown >= min_grown > 0, grown
    if shape in FULL:
        assert nocont >= 6 and traced >= 6, (nocont, traced)
        assert 6 <= len(O.PbMap(dm, b, rt)) <= 23
    elif shape in ((66, 90), (34, 400)):
        assert 0 in nreg and max(nreg) >= 1 and nocont >= 1       # empty and non-empty sensors side by side
    if shape == (194, 258):
        assert 15 <= len(O.PbMap(dm, b, rt)) <= 17
    if shape == (130, 250):
        assert all(2 <= n <= 6 for n in nreg), nreg


def test_both_contour_kinds_at_the_small_sizes():
    """Over the two seeds, 66x90 and 34x400 show a traced region and a contour-less one."""
    rt8 = O.read_extrinsics(R.EXTRINSICS_DIR)
    for rows, cols in ((66, 90), (34, 400)):
        kinds = set()
        for seed in PLANE_SEEDS:
            b, d = R.synth_frame_rt(rows, cols, rt8, seed, R.synth_path_pose(seed, 0))
            for r in per_sensor_oracle(b, depth_metres(d)):
                kinds |= {len(g["contour"]) > 0 for g in r["regs"]}
        assert kinds == {True, False}, (rows, cols)


def test_stripe_generator():
    xyz, nrm = stripe_sensor(21, 160, 4)
    a, b = stripe_frame("a"), stripe_frame("a")
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    assert xyz.dtype == np.float32 and nrm.dtype == np.float32 and xyz.shape == (21, 160, 4)
    # unit normals towards the viewpoint, the points on n . p = -2 within float rounding, stripes 17 degrees apart
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=-1) - 1).max() < 1e-6
    d = np.einsum("ijk,ijk->ij", xyz[..., :3].astype(np.float64), nrm.astype(np.float64))
    assert np.abs(d + 2).max() < 1e-5
    ang = np.rad2deg(np.arccos(np.clip(nrm[0, 3].astype(np.float64) @ nrm[0, 4].astype(np.float64), -1, 1)))
    assert 16.5 < ang < 17.5 and np.array_equal(nrm[0, 0], nrm[0, 3]) and not np.array_equal(nrm[0, 3], nrm[0, 4])
    # every case has an all-NaN sensor, a one-plane sensor and striped sensors of both signs
    for case, c in STRIPE_CASES.items():
        kinds = [k for k, _, _ in c["sensors"]]
        assert kinds.count("n") >= 1 and kinds.count("p") == 1 and kinds.count("s") >= 5, case
        assert len({(p, f) for k, p, f in c["sensors"] if k == "s"}) >= 2, case
    assert STRIPE_CASES["a"]["sensors"][0] == STRIPE_CASES["a"]["sensors"][1] == ("s", 0, 0)
    assert STRIPE_CASES["c"]["sensors"][7][0] == "s"              # the contour pool's last share is a full one
    rgb = a[2]
    assert (rgb[0, 0, :4, :3] == 0).all() and (rgb[..., 3] == 0).all() and len(np.unique(rgb)) == 256


def _figures(res):
    out = []
    for lc, lf, regs in res:
        cnt = np.bincount(lc[lc >= 0].ravel(), minlength=1)
        out.append(dict(labels=int(lc.max()) + 1, big=int((cnt > 80).sum()), regions=len(regs),
                        nocont=sum(1 for g in regs if len(g["contour"]) == 0),
                        points=sum(len(g["contour"]) for g in regs), top=max([g["label"] for g in regs], default=-1)))
    return out


def _span_max(res):
    lc8, lf8 = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    big = [set(np.nonzero(np.bincount(r[0][r[0] >= 0].ravel(), minlength=1) > 80)[0].tolist()) for r in res]
    mod = [{g["label"] for g in r[2]} for r in res]
    return max(span_keys(lc8, big)), max(span_keys(lf8, mod))


@pytest.mark.parametrize("case", list(STRIPE_CASES))
def test_crafted_fields_reach_their_paths(case):
    c = STRIPE_CASES[case]
    xyz, nrm, _ = stripe_frame(case)
    res = stripe_oracle(xyz, nrm)
    F = _figures(res)
    N = c["h"] * c["w"]
    striped0 = [F[s] for s, (k, p, f) in enumerate(c["sensors"]) if k == "s" and p == 0]
    for s, (kind, _, _) in enumerate(c["sensors"]):
        if kind == "n":
            assert F[s]["labels"] == 0 and F[s]["regions"] == 0
        if kind == "p":     # one region over the whole sensor: no contour, the voxel fallback
            assert (F[s]["labels"], F[s]["regions"], F[s]["nocont"], F[s]["points"]) == (1, 1, 1, 0)
    if case == "a":
        assert N == 3360 and N % 512 != 0
        for f in F[:2]:
            assert (f["labels"], f["big"], f["regions"], f["nocont"]) == (40, 40, 40, 1)
        # the 512-pixel span over the seam of sensors 0 and 1: 80 keys for k_gm<false> (large labels) and for
        # k_gm<true> (models), more than the table's 64 slots
        assert _span_max(res) == (80, 80)
        assert [f["regions"] for f in F] == [40, 40, 0, 1, 39, 39, 0, 39]
    elif case == "b":
        for f in striped0:
            assert (f["regions"], f["points"], f["top"], f["nocont"]) == (64, 10304, 63, 0)
        assert all(f["regions"] <= 64 for f in F)
    elif case == "c":
        for f in striped0:
            assert (f["regions"], f["points"]) == (60, 23940)
        assert 12288 < 23940 <= 2 * N == 24000                     # above TR_LIST, inside the sensor's pool share
        assert F[7]["points"] == 2 * N - 60
    elif case == "d":
        for f in striped0:
            assert f["regions"] == 70
        assert max(f["regions"] for f in F) > 64
    elif case == "e":
        for f in striped0:
            assert (f["labels"], f["big"]) == (960, 640)
        assert max(f["big"] for f in F) > 512
    if case in "abc":
        assert all(f["regions"] <= 64 and f["big"] <= 512 for f in F)   # no capacity is exceeded


@pytest.mark.parametrize("h,w,sw", [(81, 70, 4), (240, 320, 8)])
def test_case_a_pattern_fits_the_error_cases_frames(h, w, sw):
    """Case (a)'s sensors at the frame sizes of (d) and (e) (8-pixel stripes at 240 x 320: 4-pixel ones would be 80
    models) stay within every capacity, with regions in every striped sensor."""
    xyz, nrm, _ = stripe_frame("a", h, w, sw)
    F = _figures(stripe_oracle(xyz, nrm))
    assert all(f["regions"] <= 64 and f["big"] <= 512 for f in F)
    assert [f["regions"] > 10 for f in F] == [True, True, False, False, True, True, False, True]
