"""GPU parity tests of the plane stage (plane_kernels.hip, plane_seg.hip, plane_match.hip) away from the two cloud
sizes of test_gpu_planes.py: ragged sensors through the public API, and crafted label fields through the
segmentation hook (Frame360.segment_eval), against the CPU oracle.  Every comparison is exact (bit for bit,
NaN == NaN).  tests/test_oracle_plane_shapes.py pins on the CPU what the oracle gives for these inputs, so nothing
here passes on empty output.

Paths (the launchers' conditions, plane_seg.hip):
  * k_gm's 64-pixel chunks straddling two sensors (N % 64 != 0): every ragged size but 512x768 / 516x768;
  * gm_deposit's global-atomic fallback (more than 64 keys in a 512-pixel span): crafted (a), (b), (c);
  * k_trace's second walk (s_nch > TR_NCH, more than 12 288 contour points in a sensor): crafted (c);
  * k_trace<true> at N = TR_NB_MAX: 512x768; k_trace<false> (N > TR_NB_MAX): 516x768;
  * k_ccl_local alone (h <= 16, no k_ccl_border): 32x162; a one-row last CCL band: 66x90, 34x400;
  * partial last NUMC chunk: every size with N % 256 != 0;
  * k_refine_pipe<.., 4> at h = 256: 512x768; k_refine_pipe<.., 8> (h = 258): 516x768;
  * nmodels == 64: crafted (b); sensors without a model: 66x90, 34x400, 32x162, the all-NaN sensors of the fields;
  * error bits 4 and 2 and the builds after them: crafted (d), (e)."""
import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import (PLANE_SEEDS, PLANE_SHAPES, STRIPE_CASES, cmp_per_pixel, cmp_planes, cmp_regions, depth_metres,
                    per_sensor_oracle, plane_pair_rel, same, stripe_frame, stripe_oracle)

pytestmark = pytest.mark.gpu

PLANE_FLAGS = R.BUILD_UNDISTORT | R.BUILD_CLOUD | R.BUILD_PLANES


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


@pytest.fixture(scope="module")
def rt():
    return O.read_extrinsics(R.EXTRINSICS_DIR)


def _calib(ctx, rows, cols):
    """Extrinsics only: depth_m = mm * 0.001f."""
    cal = R.Calib360(ctx, rows, cols)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    return cal


def _scene(cal, seed, frame=0, rel=None):
    P = R.synth_path_pose(seed, frame)
    return cal.synth_frame(seed, P if rel is None else P @ rel)


def _built(cal, b, d):
    f = R.Frame360(cal)
    f.upload(b, d)
    f.getPlanes()
    return f


def _snapshot(f):
    """Everything a build leaves that the tests compare: cloud, colours, normals, distance map, labels, refined
    labels, the sensors' regions and the PbMap planes."""
    return dict(cloud=f.cloud(), labels=f.labels(), regions=[f.regions(k) for k in range(8)], planes=f.planes())


def _same_build(f, snap, what=None):
    for a, b in zip(f.cloud(), snap["cloud"]):
        assert same(a, b), what
    for a, b in zip(f.labels(), snap["labels"]):
        assert np.array_equal(a, b), what
    for k in range(8):
        got, ref = f.regions(k), snap["regions"][k]
        assert len(got) == len(ref), what
        for g, o in zip(got, ref):
            assert g.keys() == o.keys()
            for key in g:
                assert np.array_equal(g[key], o[key]), (what, k, key)
    cmp_planes(f.planes(), snap["planes"])


# ------------------------------------------------------------------ 1. ragged sensors through the public API
@pytest.mark.parametrize("seed", PLANE_SEEDS, ids=["seed0", "seed7"])
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_sensors_bitexact(ctx, rt, shape, seed):
    """What test_per_pixel_stages_bitexact and test_pbmap_planes_identical assert, at sensor sizes whose clouds are
    no multiple of any tile: cloud, colours, capped distance map, normals, CCL labels, refined labels, every region
    field, and the PbMap planes with their hulls."""
    cal = _calib(ctx, *shape)
    b, d = _scene(cal, seed)
    f = _built(cal, b, d)
    dm = depth_metres(d)
    cmp_per_pixel(f, per_sensor_oracle(b, dm))
    cmp_planes(f.planes(), O.PbMap(dm, b, rt).planes())


def test_batched_ragged_builds_equal_lone_builds(ctx):
    """One r360_frames_build call over frames of 66x90 (nine: a batch of 8 and a batch of 1), 130x250 and 258x70
    interleaved, frames of two contexts; twice (the second call reuses the voxel tables and plane buffers).  Cloud,
    labels, regions and PbMap planes equal the lone builds'."""
    ctx2 = R.Context(0)
    seed = PLANE_SEEDS[1]
    lone, batch = {}, {}
    for shape, count in (((66, 90), 9), ((130, 250), 2), ((258, 70), 2)):
        cals = (_calib(ctx, *shape), _calib(ctx2, *shape))
        for i in range(count):
            b, d = _scene(cals[0], seed, i)
            lone[shape, i] = _snapshot(_built(cals[0], b, d))
            g = R.Frame360(cals[i % 2])
            g.upload(b, d)
            batch[shape, i] = g
    S, M, T = (66, 90), (130, 250), (258, 70)
    order = [(S, 0), (M, 0), (S, 1), (S, 2), (T, 0), (S, 3), (S, 4), (M, 1), (S, 5), (S, 6), (S, 7), (T, 1), (S, 8)]
    assert sorted(order) == sorted(batch)
    for rep in range(2):
        R.frames_build([batch[k] for k in order], PLANE_FLAGS)
        for k in order:
            _same_build(batch[k], lone[k], (k, rep))


def test_rebuild_with_other_content(ctx):
    """One frame built with scene A, scene B, an all-zero depth frame (every sensor empty) and A again equals a fresh
    frame's build on a fresh context each time: no buffer of the stage and no cell of the context's voxel table
    carries anything from the build before.  Then one context across sizes (194x258, 66x90, 194x258): its voxel table
    and lists were sized by the larger frame."""
    shape = (130, 250)
    cal = _calib(ctx, *shape)
    A, B = _scene(cal, 1), _scene(cal, 2)
    Z = (A[0], np.zeros_like(A[1]))
    fresh = []
    for b, d in (A, B, Z):
        c2 = R.Context(0)
        fresh.append(_snapshot(_built(_calib(c2, *shape), b, d)))
    assert sum(len(r) for r in fresh[0]["regions"]) > 8 and fresh[0]["planes"] and fresh[1]["planes"]
    assert not np.array_equal(fresh[0]["labels"][1], fresh[1]["labels"][1])
    assert all(len(r) == 0 for r in fresh[2]["regions"]) and not fresh[2]["planes"]
    f = R.Frame360(cal)
    for step, ((b, d), ref) in enumerate(zip((A, B, Z, A), (fresh[0], fresh[1], fresh[2], fresh[0]))):
        f.upload(b, d)
        f.getPlanes()
        _same_build(f, ref, step)
    # across sizes on one (new) context
    c3 = R.Context(0)
    big, small = (194, 258), (66, 90)
    refs, scenes = {}, {}
    for shp in (big, small):
        scenes[shp] = _scene(_calib(ctx, *shp), PLANE_SEEDS[0])
        refs[shp] = _snapshot(_built(_calib(R.Context(0), *shp), *scenes[shp]))
    assert sum(1 for g in sum(refs[big]["regions"], []) if g["n_contour"] == 0) >= 8   # the voxel fallback ran
    frames = {shp: R.Frame360(_calib(c3, *shp)) for shp in (big, small)}
    for step, shp in enumerate((big, small, big)):
        frames[shp].upload(*scenes[shp])
        frames[shp].getPlanes()
        _same_build(frames[shp], refs[shp], (step, shp))


def test_latency_mode_is_result_neutral_ragged(ctx):
    """test_latency_mode_is_result_neutral's three builds at 130x250: a context with latency mode off (kernel by
    kernel), and on the default context the first build (graph capture) and the second (graph replay)."""
    shape = (130, 250)
    ctx2 = R.Context(0)
    ctx2.latency_mode(False)
    cal, cal2 = _calib(ctx, *shape), _calib(ctx2, *shape)
    for seed in PLANE_SEEDS:
        b, d = _scene(cal, seed)
        off = _snapshot(_built(cal2, b, d))
        assert off["planes"]
        again = R.Frame360(cal)
        for rep in range(2):
            again.upload(b, d)
            again.getPlanes()
            _same_build(again, off, (seed, rep))


@pytest.mark.parametrize("mode", [R.PLANAR_3DoF, R.DEFAULT_6DoF])
def test_match_tables_and_register_pbmap_ragged(ctx, rt, mode):
    """The 194x258 pair (scene A and A moved by 4 degrees and (0, 0.25, 0.15) m): SubgraphMatcher tables, matches,
    verdict, pose and information equal the oracle's.  Agreement, not success, is asserted."""
    cal = _calib(ctx, 194, 258)
    frames, maps = [], []
    for rel in (None, plane_pair_rel()):
        b, d = _scene(cal, PLANE_SEEDS[0], 0, rel)
        frames.append(_built(cal, b, d))
        maps.append(O.PbMap(depth_metres(d), b, rt))
    assert len(maps[0]) >= 10 and len(maps[1]) >= 10
    reg = R.RegisterRGBD360(ctx)
    reg.setReference(frames[0], 25)
    reg.setTarget(frames[1], 25)
    gt = reg.match_tables(mode)
    ot = O.match_tables(maps[0], maps[1], 25, mode)
    for key in ("sid", "tid", "unary", "binary"):
        assert np.array_equal(gt[key], ot[key]), key
    assert ot["unary"].any()
    calls0, trunc0, _ = ctx.match_stats()
    ok = reg.RegisterPbMap(frames[0], frames[1], 25, mode)
    r = O.register_pbmap(maps[0], maps[1], 25, mode)
    calls1, trunc1, max_nodes = ctx.match_stats()
    # the interpretation tree searched to the end (no node-budget cut) on both sides
    assert calls1 == calls0 + 1 and trunc1 == trunc0 and not r["truncated"] and max_nodes >= r["nodes"]
    assert ok == bool(r["good"])
    assert reg.getMatchedPlanes() == r["matches"]
    assert reg.getAreaMatched() == r["area_matched"]
    if ok:
        assert np.array_equal(reg.getPose(), r["pose"])
        assert np.array_equal(reg.getInfoMat(), r["info"])


# ------------------------------------------------------------------ 2. crafted fields through the segmentation hook
def _ref_stats(xyz, rgb, sel, T):
    """PlaneOut::stats, bmin and bmax of the pixels `sel` of one sensor, restated from plane_math.h with Python
    integers: the point into the rig frame in float32 in Eigen's order (((T0 x + T4 y) + T8 z) + T12 for the
    column-major pose T), q36(v) = trunc(v 2^36), exact sums of the q and their products; moments_add_rgb's
    trunc(float(c) * (1.0f / float(r + g + b)) 2^33) and the sum of r + g + b."""
    p = xyz[sel][:, :3]
    T = np.asarray(T, np.float32)
    q = []
    for r in range(3):
        v = ((T[r] * p[:, 0] + T[4 + r] * p[:, 1]) + T[8 + r] * p[:, 2]) + T[12 + r]
        assert v.dtype == np.float32
        q.append(np.trunc(v.astype(np.float64) * 68719476736.0).astype(np.int64))   # |q| < 2^40: exact
    s1 = [int(q[k].sum()) for k in range(3)]
    # exact sums of products: q = hi 2^20 + lo (hi signed below 2^20, 0 <= lo < 2^20), so every partial sum over
    # fewer than 2^20 pixels stays below 2^62 in int64; the parts are put together as Python integers
    assert len(p) < (1 << 20) and all(np.abs(x).max(initial=0) < (1 << 40) for x in q)
    hi, lo = [x >> 20 for x in q], [x & ((1 << 20) - 1) for x in q]
    s2 = [(int((hi[a] * hi[b]).sum()) << 40) + (int((hi[a] * lo[b] + lo[a] * hi[b]).sum()) << 20)
          + int((lo[a] * lo[b]).sum()) for a in range(3) for b in range(a, 3)]
    col = rgb[sel][:, :3]
    tot = col.astype(np.int64).sum(1)
    nz = tot != 0
    inv = np.float32(1.0) / tot[nz].astype(np.float32)
    c = [int(np.trunc((col[nz, k].astype(np.float32) * inv).astype(np.float64) * 8589934592.0).astype(np.int64).sum())
         for k in range(3)] + [int(tot.sum())]
    return dict(n=len(p), s1=s1, s2=s2, c=c, bmin=p.min(0), bmax=p.max(0))


def _cmp_crafted(f, xyz, nrm, rgb, res, T8, what):
    """labels(), regions(k) and region_detail(k, m) of a frame after segment_eval against O.segment's labels, refined
    labels, region records and contours, the restated statistics and numpy bounds."""
    lab, labf = f.labels()
    got_nrm = f.cloud()[2]
    for s in range(8):
        lc, lf, regs = res[s]
        assert np.array_equal(lab[s], lc), (what, "ccl", s)
        assert np.array_equal(labf[s], lf), (what, "refined labels", s)
        # the normals as given, their fourth component p.n as the oracle's comparator computes it
        pd = xyz[s][..., 0] * nrm[s][..., 0] + xyz[s][..., 1] * nrm[s][..., 1] + xyz[s][..., 2] * nrm[s][..., 2]
        assert same(got_nrm[s][..., :3], nrm[s]) and same(got_nrm[s][..., 3], pd), (what, "normals", s)
        cmp_regions(f.regions(s), regs, (what, s), nan_equal=True)
        flat = xyz[s].reshape(-1, 4)
        for m, o in enumerate(regs):
            g = f.region_detail(s, m)
            assert same(g["contour"], flat[o["contour"]]), (what, "contour", s, m)
            ref = _ref_stats(xyz[s], rgb[s], lf == o["label"], T8[16 * s:16 * s + 16])
            assert (g["n"], g["s1"], g["s2"], g["c"]) == (ref["n"], ref["s1"], ref["s2"], ref["c"]), (what, s, m)
            assert np.array_equal(g["bmin"], ref["bmin"]) and np.array_equal(g["bmax"], ref["bmax"]), (what, s, m)


@pytest.fixture(scope="module")
def crafted_refs():
    return {}


def _crafted(crafted_refs, case, h=None, w=None, sw=None):
    key = (case, h, w, sw)
    if key not in crafted_refs:
        xyz, nrm, rgb = stripe_frame(case, h, w, sw)
        crafted_refs[key] = (xyz, nrm, rgb, stripe_oracle(xyz, nrm))
    return crafted_refs[key]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_crafted_fields(ctx, crafted_refs, case):
    """(a) 80 keys in the 512-pixel span over the seam of two striped sensors: gm_deposit's overflow path in
    k_gm<false> and k_gm<true>.  (b) 64 models exactly, labels and closeness bits up to 63.  (c) 23 940 contour
    points per striped sensor: k_trace's second walk; sensor 7's last contour ends 60 points before the pool's end.
    Run twice on the frame: the second run meets the first one's buffers."""
    c = STRIPE_CASES[case]
    cal = _calib(ctx, 2 * c["h"], 2 * c["w"])
    T8 = cal.extrinsics()[0]
    xyz, nrm, rgb, res = _crafted(crafted_refs, case)
    f = R.Frame360(cal)
    nrm4 = np.concatenate([nrm, np.full(nrm.shape[:3] + (1,), 123.0, np.float32)], -1)   # a fourth component to ignore
    for rep in range(2):
        assert f.segment_eval(xyz, nrm4 if rep else nrm, rgb) == 0
        _cmp_crafted(f, xyz, nrm, rgb, res, T8, (case, rep))
        assert f.planes() == []                                    # the host assembly did not run
    if case == "b":
        assert [len(f.regions(s)) for s in range(8)] == [64, 0, 64, 1, 64, 64, 0, 64]
    with pytest.raises(ValueError):
        f.segment_eval(xyz[:, :-1], nrm[:, :-1], rgb[:, :-1])       # fields of another size than the frame's


@pytest.mark.parametrize("case,bit,sw", [("d", 4, 4), ("e", 2, 8)])
def test_capacity_errors_leave_no_state(ctx, crafted_refs, case, bit, sw):
    """(d) 70 models: error bit 4; (e) 640 labels above 80 points: error bit 2.  segment_eval fails with the
    capacity message; case (a)'s sensors on the same frame give what they gave before the failure, and an ordinary
    build of a synthetic scene on that frame equals a fresh frame's on a fresh context."""
    c = STRIPE_CASES[case]
    h, w = c["h"], c["w"]
    cal = _calib(ctx, 2 * h, 2 * w)
    T8 = cal.extrinsics()[0]
    good = _crafted(crafted_refs, "a", h, w, sw)
    bad = stripe_frame(case)
    b, d = _scene(cal, PLANE_SEEDS[0])
    fresh = _snapshot(_built(_calib(R.Context(0), 2 * h, 2 * w), b, d))
    assert sum(len(r) for r in fresh["regions"]) >= 8
    f = R.Frame360(cal)
    assert f.segment_eval(*good[:3]) == 0
    _cmp_crafted(f, *good, T8, (case, "before"))
    before = (f.labels(), [f.regions(s) for s in range(8)])
    with pytest.raises(RuntimeError, match="capacity exceeded") as ei:
        f.segment_eval(*bad)
    assert ei.value.code & bit, ei.value.code
    assert ei.value.code & ~(2 | 4) == 0
    with pytest.raises(RuntimeError, match="capacity exceeded"):
        f.regions(0)                                               # the failed stage has no regions to show
    assert f.segment_eval(*good[:3]) == 0
    _cmp_crafted(f, *good, T8, (case, "after"))
    for x, y in zip(f.labels(), before[0]):
        assert np.array_equal(x, y)
    f.upload(b, d)
    f.getPlanes()
    _same_build(f, fresh, (case, "build after"))
    # and a failure straight after an ordinary build, then the build again
    with pytest.raises(RuntimeError, match="capacity exceeded"):
        f.segment_eval(*bad)
    f.upload(b, d)
    f.getPlanes()
    _same_build(f, fresh, (case, "second build after"))
