"""GPU parity tests of the plane stage's fused per-pixel passes (plane_seg.hip): k_refine_prep<true> (state, closeness
mask and their skewed copies in one pass), k_refine_finish (raster states and refined labels in one pass, leaving the
sensors k_refine_fb redoes to it), and of the large-label bookkeeping (k_big_count / k_big_list) at label counts no
other test reaches.

Every comparison is exact, against the CPU oracle (O.segment) and against a sequential restatement of the refinement:
the states and closeness masks restated here from the oracle's labels and models, swept by test_gpu_refine's
_refine_ref.  Nothing is compared with the code under test.

Fields go through the segmentation hook (Frame360.segment_eval, R.frames_segment_eval for a batch): points on planes
n . p = -2 with normals 17 degrees apart, so the sign pattern of the normals' x component decides the labels: equal
signs of 4-neighbours join, a checkerboard makes every pixel a label of its own.  Frame360.refine_states() shows the
swept states and the wavefront sweeps' flags.

The wrap push of the second sweep (column 0 of row r + 1 into (r, w - 1)) is corrected by re-runs of the pipelined
sweep and, past 64 of them or after a hand-off that gave up, by k_refine_fb; both set the sensor's flags, which is what
test_wrap_push_through_frame_build asserts (as r360_refine_eval's count does).  One re-run settles any field (see
test_fallback_kernel_through_frame_build), so k_refine_fb is reached through the test hook R.refine_force_fallback;
its own sweeps are also covered from raster inputs by test_gpu_refine.py."""
import numpy as np
import pytest

import rgbd360_amd as R
from _cases import PLANE_SEEDS, PLANE_SHAPES, cmp_per_pixel, cmp_regions, depth_metres, per_sensor_oracle, stripe_oracle
from test_gpu_refine import _refine_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


def _calib(ctx, rows, cols):
    cal = R.Calib360(ctx, rows, cols)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    return cal


# ------------------------------------------------------------------ fields
def _sensor(sgn):
    """One sensor's cloud [h, w, 4] and unit normals [h, w, 3] from the sign pattern sgn [h, w] (+-1; 0: no point):
    tests/_cases.py's stripe_sensor with the pattern given.  Pixel (v, u) looks along the pinhole ray and lies on the
    plane n . p = -2 of its own normal n = normalize((sgn 0.15, 0, -1))."""
    h, w = sgn.shape
    f = 525.0 * (2 * w / 640.0) / 2
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    v, u = np.mgrid[0:h, 0:w]
    ln = np.sqrt(0.15 ** 2 + 1.0)
    n = np.stack([sgn * 0.15 / ln, np.zeros((h, w)), np.full((h, w), -1.0 / ln)], -1)
    ray = np.stack([(u - cx) / f, (v - cy) / f, np.ones((h, w))], -1)
    z = -2.0 / np.einsum("ijk,ijk->ij", ray, n)
    xyz = np.zeros((h, w, 4), np.float32)
    xyz[..., :3] = ray * z[..., None]
    n = n.astype(np.float32)
    xyz[sgn == 0, :3] = np.nan
    n[sgn == 0] = np.nan
    return xyz, n


def _plane(h, w):
    return np.ones((h, w))


def _none(h, w):
    return np.zeros((h, w))


def _checker(h, w):
    v, u = np.mgrid[0:h, 0:w]
    return np.where((u + v) % 2 == 0, 1.0, -1.0)


def _stripes(h, w, sw, phase=0):
    u = np.mgrid[0:h, 0:w][1]
    return np.where(((u + phase) // sw) % 2 == 0, 1.0, -1.0)


def _speckled(h, w, seed, p=0.2):
    """One plane with pixels of the other sign sprinkled in: labels of a few pixels that lie close to the plane's
    model, which the refinement's sweeps hand to it.  Pixel 0 stays on the plane: a sensor whose pixel 0 is a label
    of its own and whose pixel 1 starts a region makes the stage report contour overflow (error bits 8 | 16) where
    the oracle traces 120 points, with the kernels before these passes too; that is k_trace's
    business, not these passes'."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random((h, w)) < p, -1.0, 1.0)
    s[0, 0] = 1.0
    return s


def _wrap(h, w):
    """A plane over the columns left of the middle, no points right of it, and the last column on the plane again: a
    label of h pixels of its own (non-planar below 81 rows), every pixel close to the plane's model.  Nothing reaches
    (r, w - 1) in the first sweep (the chain and the push from the left stop at the gap) nor from below in the second
    (that push needs a labelled left neighbour), so column 0 of row r + 1, which is planar, pushes into it over the
    flat-index wrap, in every row but the last."""
    s = np.zeros((h, w))
    s[:, :w // 2] = 1.0
    s[:, w - 1] = 1.0
    return s


def _frame(patterns):
    fields = [_sensor(p) for p in patterns]
    xyz = np.stack([f[0] for f in fields])
    nrm = np.stack([f[1] for f in fields])
    rgb = np.random.default_rng(77).integers(0, 256, xyz.shape, dtype=np.uint8)
    rgb[..., 3] = 0
    return xyz, nrm, rgb


# ------------------------------------------------------------------ the sequential restatement
def _init_ref(xyz, lc, regs):
    """d_refine_init restated: state -1 no label, -2 a label without model, m the label of model m; bit m of the mask
    where |v_m . p| < 0.02f, the dot product summed in float32 from the left, the comparison in double."""
    assert len(regs) <= 64
    S = np.where(lc < 0, -1, -2).astype(np.int8)
    M = np.zeros(lc.shape, np.uint64)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    for m, g in enumerate(regs):
        S[lc == g["label"]] = m
        v = np.asarray(g["model"], np.float32)
        with np.errstate(invalid="ignore"):
            d = ((v[0] * x + v[1] * y) + v[2] * z) + v[3]
            assert d.dtype == np.float32
            close = np.abs(d.astype(np.float64)) < np.float64(np.float32(0.02))
        M |= close.astype(np.uint64) << np.uint64(m)
    return S, M


def _refined_ref(xyz, lc, regs):
    """(states before the sweeps, states after, refined labels) of one sensor, sequentially."""
    S0, M = _init_ref(xyz, lc, regs)
    # the sweeps only hand on states >= 0: without a model nothing changes
    S = _refine_ref(S0, M) if regs else S0.copy()
    of_model = np.array([g["label"] for g in regs] + [-1], np.int32)
    lf = np.where(S >= 0, of_model[np.maximum(S, 0)], np.where(S == -2, lc, -1)).astype(np.int32)
    return S0, S, lf


def _reference(xyz, nrm):
    """Per sensor: the oracle's (labels, refined labels, regions) and the restatement's (states, refined labels);
    the two references agree on the refined labels."""
    res = stripe_oracle(xyz, nrm)
    seq = []
    for s in range(8):
        lc, lf, regs = res[s]
        S0, S, lf_seq = _refined_ref(xyz[s], lc, regs)
        assert np.array_equal(lf_seq, lf), ("restatement against the oracle", s)
        seq.append((S0, S, lf_seq))
    return res, seq


def _check(f, res, seq, what):
    lab, labf = f.labels()
    states, flags = f.refine_states()
    for s in range(8):
        lc, lf, regs = res[s]
        assert np.array_equal(lab[s], lc), (what, "ccl", s)
        assert np.array_equal(states[s], seq[s][1]), (what, "states", s, np.argwhere(states[s] != seq[s][1])[:5])
        assert np.array_equal(labf[s], lf), (what, "refined labels", s, np.argwhere(labf[s] != lf)[:5])
        cmp_regions(f.regions(s), regs, (what, s), nan_equal=True)
    return flags


@pytest.fixture(scope="module")
def refs():
    return {}


def _ref_of(refs, key, patterns):
    if key not in refs:
        xyz, nrm, rgb = _frame(patterns())
        refs[key] = (xyz, nrm, rgb) + _reference(xyz, nrm)
    return refs[key]


# ------------------------------------------------------------------ 1. the wrap push through a frame build
WRAP_SENSOR = 3


def _wrap_patterns(h=21, w=160):
    return [_stripes(h, w, 4), _speckled(h, w, 1), _none(h, w), _wrap(h, w), _stripes(h, w, 4, 1), _plane(h, w),
            _none(h, w), _speckled(h, w, 2)]


def _plain_patterns(h=21, w=160):
    """The same frame with the last column of the wrap sensor empty: no wrap push can fire."""
    p = _wrap_patterns(h, w)
    p[WRAP_SENSOR][:, -1] = 0
    return p


def test_wrap_push_through_frame_build(ctx, refs):
    """A sensor whose second sweep's wrap push fires in every row, beside seven sensors without one, alone and in a
    batch of two with a frame without any: labels, swept states, refined labels and regions equal the oracle's and
    the sequential restatement's, the correction is flagged for that sensor of that frame only, and the batch leaves
    what the lone build leaves.  Twice: the second run meets the first one's buffers."""
    h, w = 21, 160
    A = _ref_of(refs, "wrap", _wrap_patterns)
    Bp = _ref_of(refs, "plain", _plain_patterns)
    S0, S1, _ = A[4][WRAP_SENSOR]
    # the restatement says so too: the sweeps took every (r, w - 1) above the last row from -2 to the plane's model
    assert (S0[:-1, -1] == -2).all() and (S1[:-1, -1] == S1[0, 0]).all() and S1[0, 0] >= 0 and S1[-1, -1] == -2
    cal = _calib(ctx, 2 * h, 2 * w)
    fa, fb = R.Frame360(cal), R.Frame360(cal)
    for rep in range(2):
        assert fa.segment_eval(*A[:3]) == 0
        flags = _check(fa, A[3], A[4], ("lone", rep))
        corrected = (flags[:8] != 0) | (flags[8:16] != 0)
        assert corrected[WRAP_SENSOR] and not np.delete(corrected, WRAP_SENSOR).any(), flags
        assert not flags[16:].any()
        order = (fa, fb) if rep == 0 else (fb, fa)           # the wrap frame first, then second in the batch
        fields = (A, Bp) if rep == 0 else (Bp, A)
        codes = R.frames_segment_eval(order, *[np.stack([x[k] for x in fields]) for k in range(3)])
        assert not codes.any()
        flags = _check(fa, A[3], A[4], ("batch", rep))
        corrected = (flags[:8] != 0) | (flags[8:16] != 0)
        assert corrected[WRAP_SENSOR] and not np.delete(corrected, WRAP_SENSOR).any(), flags
        flags = _check(fb, Bp[3], Bp[4], ("batch, plain frame", rep))
        assert not flags.any(), flags


FORCED = (1, WRAP_SENSOR)   # a speckled sensor (the sweeps change it, no wrap push) and the wrap sensor


@pytest.mark.parametrize("first_sweep", [False, True], ids=["second_sweep", "both_sweeps"])
def test_fallback_kernel_through_frame_build(ctx, refs, first_sweep):
    """k_refine_fb inside a frame build.  No field sends a build there (a wrap push's value never depends on another
    row's wrap push, so one re-run settles every row: test_wrap_push_through_frame_build), so the test hook hands
    sensors 1 and 3 of the wrap frame to it after their wavefront sweeps: as after re-runs that ran out at the middle
    row (rows up to it come back from the first sweep's states and are swept again), and as after a first sweep that
    gave up (both sweeps again from the raster states k_refine_prep wrote).  k_refine_finish must leave those
    sensors alone and k_refine_fb must write their states and refined labels; the other six sensors and the second
    frame of the batch go the ordinary way.  Before every build the frames hold another field's states and labels
    (a checkerboard: every pixel its own label), so nothing stale can pass for the result."""
    h, w = 21, 160
    A = _ref_of(refs, "wrap", _wrap_patterns)
    Bp = _ref_of(refs, "plain", _plain_patterns)
    other = _frame([_checker(h, w)] * 8)
    cal = _calib(ctx, 2 * h, 2 * w)
    fa, fb = R.Frame360(cal), R.Frame360(cal)
    mask = sum(1 << s for s in FORCED)

    def flags_ok(flags, forced):
        for s in range(8):
            assert (flags[s] != 0) == (s in forced), (s, flags)
            assert (flags[16 + s] != 0) == (s in forced and first_sweep), (s, flags)

    try:
        for slot in (0, 1):                                   # the forced frame first, then second in the batch
            assert fa.segment_eval(*other) == 0 and fb.segment_eval(*other) == 0
            assert not np.array_equal(fa.labels()[1], np.stack([r[1] for r in A[3]]))
            R.refine_force_fallback(mask, first_sweep)
            assert fa.segment_eval(*A[:3]) == 0                # alone
            flags_ok(_check(fa, A[3], A[4], ("lone", slot)), FORCED)
            R.refine_force_fallback(0)
            assert fa.segment_eval(*other) == 0
            R.refine_force_fallback(mask << (8 * slot), first_sweep)
            order, fields = ((fa, fb), (A, Bp)) if slot == 0 else ((fb, fa), (Bp, A))
            codes = R.frames_segment_eval(order, *[np.stack([x[k] for x in fields]) for k in range(3)])
            assert not codes.any()
            flags_ok(_check(fa, A[3], A[4], ("batch", slot)), FORCED)
            flags_ok(_check(fb, Bp[3], Bp[4], ("batch, plain frame", slot)), ())
            R.refine_force_fallback(0)
    finally:
        R.refine_force_fallback(0)


# ------------------------------------------------------------------ 2. short and ragged diagonals
def _small_patterns(h, w):
    return lambda: [_speckled(h, w, 3), _plane(h, w), _none(h, w), _stripes(h, w, 3), _speckled(h, w, 4, 0.4),
                    _checker(h, w), _wrap(h, w), _stripes(h, w, 1)]


@pytest.mark.parametrize("h,w", [(2, 2), (2, 64), (33, 2), (17, 45)], ids=lambda v: str(v))
def test_small_clouds(ctx, refs, h, w):
    """Clouds whose diagonals are short (2 x 2), all ragged (2 x 64, 33 x 2: every diagonal has at most two pixels)
    or no multiple of anything (17 x 45), through the hook, twice on one frame."""
    xyz, nrm, rgb, res, seq = _ref_of(refs, ("small", h, w), _small_patterns(h, w))
    if h * w > 80:
        assert any(len(r[2]) for r in res)                   # some sensor has a model to refine towards
    if (h, w) == (17, 45):
        assert any(not np.array_equal(q[0], q[1]) for q in seq)   # and the sweeps change something
    f = R.Frame360(_calib(ctx, 2 * h, 2 * w))
    for rep in range(2):
        assert f.segment_eval(xyz, nrm, rgb) == 0
        _check(f, res, seq, (h, w, rep))


@pytest.mark.parametrize("shape", [(34, 90), (66, 90), (34, 400)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_sensor_builds(ctx, shape):
    """Ordinary builds of synthetic scenes at sensors of 34 x 90 (clouds of 17 x 45), 66 x 90 and 34 x 400 against
    the per-sensor oracle, every per-pixel stage and region field."""
    assert shape == (34, 90) or shape in PLANE_SHAPES
    cal = _calib(ctx, *shape)
    b, d = cal.synth_frame(PLANE_SEEDS[0], R.synth_path_pose(PLANE_SEEDS[0], 0))
    f = R.Frame360(cal)
    f.upload(b, d)
    f.getPlanes()
    cmp_per_pixel(f, per_sensor_oracle(b, depth_metres(d)))


# ------------------------------------------------------------------ 3. label counts
NUMC = 256   # label ids per workgroup of k_big_count / k_big_list (plane_seg.hip)


def _mixed(h, w, bands):
    """One-pixel labels (a checkerboard) with stripes 6 wide over the row ranges `bands`: labels above 80 points for
    14 rows and more.  Labels are numbered in raster order of their first pixels, so a band's stripes come after the
    one-pixel labels above it."""
    s = _checker(h, w)
    for k, (r0, r1) in enumerate(bands):
        s[r0:r1] = _stripes(r1 - r0, w, 6, 3 * k)
    return s


def _count_patterns(h=75, w=100):
    return [_checker(h, w), _none(h, w), _mixed(h, w, [(0, 15), (60, 75)]), _plane(h, w),
            _mixed(h, w, [(0, 15), (19, 34)]), _checker(h, w), _none(h, w), _mixed(h, w, [(60, 75)])]


def test_label_counts(ctx, refs):
    """Sensors without a label (nlab = 0, no model); sensors of 7500 one-pixel labels (nlab = N: 30 chunks of 256
    ids, none large); sensors whose large labels lie in the first chunk and in a far or the next chunk (the later
    ranks carry the earlier chunks' counts); one whose large labels all come after 23 chunks of small ones."""
    xyz, nrm, rgb, res, seq = _ref_of(refs, "counts", _count_patterns)
    nlab = [int(r[0].max()) + 1 for r in res]
    big = [sorted(g["label"] for g in r[2]) for r in res]
    assert nlab[1] == 0 and nlab[6] == 0 and not res[1][2] and (res[1][0] == -1).all()
    assert nlab[0] == 75 * 100 > NUMC and not big[0]
    assert big[2][0] < NUMC and big[2][-1] // NUMC >= 16
    assert big[4][0] < NUMC <= big[4][-1] < 2 * NUMC
    assert big[7][0] // NUMC >= 23
    f = R.Frame360(_calib(ctx, 150, 200))
    for rep in range(2):
        assert f.segment_eval(xyz, nrm, rgb) == 0
        _check(f, res, seq, ("counts", rep))
    assert [len(f.regions(s)) for s in range(8)] == [len(r[2]) for r in res]


def _overflow_patterns(h=162, w=260):
    """520 one-pixel-wide stripes of 81 rows in two sensors (two bands of 260): more than R360_MAX_BIG = 512."""
    v, u = np.mgrid[0:h, 0:w]
    many = np.where((u + v // 81) % 2 == 0, 1.0, -1.0)
    return [_plane(h, w), many, _none(h, w), _none(h, w), _none(h, w), many, _none(h, w), _none(h, w)]


def _overflow_good_patterns(h=162, w=260):
    return [_plane(h, w), _stripes(h, w, 20), _none(h, w), _none(h, w), _none(h, w), _speckled(h, w, 5, 0.02),
            _none(h, w), _none(h, w)]


def test_too_many_large_labels(ctx, refs):
    """520 labels above 80 points in a sensor: error bit 2 and nothing else, the stage fails with the capacity
    message; the frame then builds a good field exactly as the oracle and the restatement have it (what a fresh
    frame gives), before and after the failure."""
    h, w = 162, 260
    bad = _frame(_overflow_patterns())
    good = _ref_of(refs, "overflow_good", _overflow_good_patterns)
    f = R.Frame360(_calib(ctx, 2 * h, 2 * w))
    assert f.segment_eval(*good[:3]) == 0
    _check(f, good[3], good[4], "before")
    for rep in range(2):
        with pytest.raises(RuntimeError, match="capacity exceeded") as ei:
            f.segment_eval(*bad)
        assert ei.value.code & 2 and ei.value.code & ~(2 | 4) == 0, ei.value.code   # 4: the models overflow after it
        with pytest.raises(RuntimeError, match="capacity exceeded"):
            f.regions(0)
        assert f.segment_eval(*good[:3]) == 0
        _check(f, good[3], good[4], ("after", rep))
