"""The sparse level-0 pass (PF 6): the pyramid build leaves two saliency flags per level-0 pixel in the packed image's
spare bits, and the pass gathers the target's gradients and runs the terms only for the visible pixels whose flag is
set, queued and walked in full 64-lane chunks (icp_kernels.hip).

Shapes: the 64 x 384 sphere (sensors of 48 x 64, and the same size given as images for the crafted targets) and a
ragged neighbour of 52 x 320 (5 waves per row, waves of 7 and of 8 chunks on the batched grid), the smallest where
PF 6 runs.  Everything is compared with the CPU oracle on the same images, with the bars of test_gpu_dense.py and
test_gpu_icp_shapes.py (icp_check of _cases.py: counts exact, squared error 1e-6, H and g 1e-5 of scale); a job's sums
are bit-identical lone-batched, in a batch of one and in a batch of three.

The image forms keep the lean transform at every size, and with a few dozen contributing terms the lean |p'| can miss
the 1e-6 bar on the squared error (PF 5 switches to the exact terms below 512 points).  So every
crafted case has either no contributing term at all or at least 512, by the oracle's own count, asserted here."""
import functools

import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import ROOM_SOURCE, icp_check, noise_sphere, room_sphere

pytestmark = pytest.mark.gpu

TPB = 256
EXACT_BELOW = 512            # R360_EXACT_BELOW
POSES = [np.eye(4, dtype=np.float32), O.exp_se3([0.02, -0.03, 0.05, 0.01, -0.015, 0.02])]
METHODS = (R.PHOTO_CONSISTENCY, R.DEPTH_CONSISTENCY, R.PHOTO_DEPTH)
ROWS, COLS = 64, 384
N_PYR = 2


def _gray3(v):
    return np.repeat(np.asarray(v, np.uint8)[..., None], 3, axis=-1)   # CV_RGB2GRAY of b = g = r = v is v


def _const():
    return _gray3(np.full((ROWS, COLS), 100)), np.full((ROWS, COLS), 2000, np.uint16)


def _ramp():
    """Gray and range strictly monotone down the rows (3 / 255 and 40 mm per row): every pixel with a live gradient
    is salient for both tests.  A column pattern of period 5 (0, 6, 12, 3, 9) rides on top, so that the horizontal
    gradients are not all zero: with rows alone the rotation about the sphere's axis has a Jacobian of rounding
    residues only, H's entry for it is ~1e-10 of the others and no float sum meets a bar scaled by it."""
    r = np.arange(ROWS)[:, None] * np.ones(COLS, np.int64)[None, :]
    h = (3 * ((2 * np.arange(COLS)) % 5))[None, :]
    return _gray3(20 + 3 * r + h), (1000 + 40 * r + 5 * h).astype(np.uint16)


# salient runs of the stripes target: (row, first salient column, salient pixels).  On the batched grid of 12
# workgroups (stride 3072 pixels = 8 rows) workgroup 3 owns columns 0..255 of rows 2 + 8 k and workgroup 6 those of
# rows 4 + 8 k: its waves 0, 1, 2 collect 63, 64 and 65 needed entries over several chunks, and wave 0 of workgroup 6
# collects entries in its last chunk only (k = 7).  The runs avoid the seam columns (48 s - 1, 48 s); the rows
# 6 + 8 k carry the bulk that brings every cost function over EXACT_BELOW terms.
STRIPE_RUNS = [(2, 1, 40), (18, 1, 23),
               (2, 100, 28), (18, 97, 31), (34, 100, 5),
               (2, 145, 46), (18, 145, 19),
               (60, 1, 30)] + [(r, 64 * j + 2, 40) for r in range(6, 56, 8) for j in range(6) if j != 2] + \
              [(r, 146, 40) for r in range(6, 56, 8)]


def _stripes():
    """Flat rows (gray 10, range 2 m) with ramps of 3 / 255 and 30 mm per column: a run of n salient pixels is a ramp
    of n + 1 columns after a flat pixel (its last pixel is a maximum, not salient); the rows above and below are
    flat, so no vertical gradient is live."""
    g = np.full((ROWS, COLS), 10, np.int64)
    d = np.full((ROWS, COLS), 2000, np.int64)
    for r, c0, n in STRIPE_RUNS:
        j = np.arange(n + 1)
        g[r, c0:c0 + n + 1] = 20 + 3 * j
        d[r, c0:c0 + n + 1] = 2030 + 30 * j
    return _gray3(g), d.astype(np.uint16)


def _sensor_images(seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (8, 48, 64, 3), dtype=np.uint8)
    d = rng.integers(0, 7000, (8, 48, 64)).astype(np.uint16)
    d[rng.random((8, 48, 64)) < 0.2] = 0
    return b, d


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


@pytest.fixture(scope="module")
def rig(ctx):
    """The 48 x 64 rig: calibration, and the oracle's stitch of sensor images."""
    cal = R.Calib360(ctx, 48, 64)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    _, rti, K = cal.extrinsics()
    Km = K.reshape(3, 3).T
    return cal, (lambda b, d: O.stitch(b, d, rti, Km))


@pytest.fixture(scope="module")
def bank(ctx, rig):
    """case -> (target frame, source frame, oracle level 0 of the target, of the source).  All frames are built with
    setCompaction(False), as the sequence runner's ring frames are: a lone pass streams level 0 as PF 6 too."""
    cal48, stitch = rig
    cals = {(ROWS, COLS): R.Calib360.for_sphere(ctx, ROWS, COLS), (52, 320): R.Calib360.for_sphere(ctx, 52, 320)}
    made = {}

    def given(images):
        bgr, dep = images
        f = R.Frame360(cals[dep.shape])
        f.setCompaction(False)
        f.set_sphere(bgr, dep)
        return f, O.sphere_pyramid(bgr, dep, 1)[0]

    def sensed(seed):
        b, d = _sensor_images(seed)
        f = R.Frame360(cal48)
        f.setCompaction(False)
        f.upload(b, d)
        f.build()
        return f, O.sphere_pyramid(*stitch(b, d), 1)[0]

    def get(case):
        if case not in made:
            if case == "noise":
                (t, lt), (s, ls) = sensed(4801), sensed(4802)
            elif case == "ragged":
                (t, lt), (s, ls) = given(noise_sphere(52, 320, 52320)), given(noise_sphere(52, 320, 52321))
            else:
                t, lt = given({"const": _const, "ramp": _ramp, "stripes": _stripes}[case]())
                s, ls = given(room_sphere(ROWS, COLS, *ROOM_SOURCE, holes=0.0))
            made[case] = (t, s, lt, ls)
        return made[case]

    yield get
    for t, s, _, _ in made.values():
        t.close()
        s.close()


def _prm(ti=None, td=None):
    p, po = R.IcpParams.default(), O.IcpParams.default(n_pyr=N_PYR)
    p.n_pyr = N_PYR
    for q in (p, po):
        if ti is not None:
            q.thres_sal_int = ti
        if td is not None:
            q.thres_sal_depth = td
    return p, po


def _oracle(lt, ls, P, method, po):
    _, e2, nv = O.error_sphere(ls, lt, P, method, po)
    H, g, nvis = O.hessgrad_sphere(ls, lt, P, method, po)
    return H, g, e2, nv, nvis


def _flags_of(level0, ti=np.float32(0.01), td=np.float32(0.01)):
    """contribute_lean's sal_p (bit 0) and sal_d (bit 1) of an oracle level."""
    a = lambda k: np.abs(level0[k].astype(np.float32))
    sal_p = ~((a("gx") < ti) & (a("gy") < ti))
    sal_d = ~((a("dgx") < td) & (a("dgy") < td))
    return sal_p.astype(np.uint8) | (sal_d.astype(np.uint8) << 1)


def _passes(ctx, t, s, lt, ls, method, p, po, fillers, what):
    """Every pose: the lone pass, a batch of one and a batch of three (the job in the middle slot) against the oracle;
    the batched sums bit-identical in both batches.  Returns the oracle's (n_valid, n_visible) per pose."""
    reg = R.RegisterPhotoICP(ctx)
    reg.params = p
    reg.setTargetFrame(t)
    reg.setSourceFrame(s)
    assert reg.pass_grid(0, 0, False)[0] == 6 and reg.pass_grid(0, 0, True)[0] == 6
    npx = lt["gray"].size
    counts = []
    for pi, P in enumerate(POSES):
        ref = _oracle(lt, ls, P, method, po)
        counts.append((ref[3], ref[4]))
        got = reg.eval(0, P, method)
        print(what, "pose", pi, "lone", got[3], got[4], "oracle", ref[3], ref[4], "e2", got[2], ref[2])
        icp_check(*got, *ref, npx)
        one = R.align_eval_batch(ctx, [(t, s)], 0, [P], method, p)
        icp_check(one[0][0], one[1][0], one[2][0], int(one[3][0]), int(one[4][0]), *ref, npx)
        pairs = [fillers[0], (t, s), fillers[1]]
        three = R.align_eval_batch(ctx, pairs, 0, [POSES[1], P, POSES[0]], method, p)
        for a, b in zip(one, three):
            assert np.array_equal(np.asarray(a[0]), np.asarray(b[1])), (what, pi)
        if ref[3] == 0:
            assert got[2] == 0.0 and not got[0].any() and not got[1].any()
            assert one[2][0] == 0.0 and not one[0][0].any() and not one[1][0].any()
    return counts


# ---------------------------------------------------------------- 1. the flags
def _check_flags(f, level0):
    fl, thr = f.saliency()
    assert thr == (np.float32(0.01), np.float32(0.01))
    want = _flags_of(level0)
    assert fl.shape == want.shape and np.array_equal(fl, want), int((fl != want).sum())
    return want


def test_flags_match_oracle_and_rebuilds_leave_no_stale_bits(ctx, rig):
    """Stitched frames (lean and full) and a frame given as images: the flags equal the oracle's sal_p / sal_d of the
    level-0 gradients bit for bit, again after the same frame object is rebuilt with other content (a noise sphere,
    then a constant one, whose flags are all clear), and the unpacked level-0 values stay the oracle's."""
    cal48, stitch = rig
    for compact in (False, True):
        f = R.Frame360(cal48)
        f.setCompaction(compact)
        for seed in (4811, 4812):
            b, d = _sensor_images(seed)
            f.upload(b, d)
            f.build()
            ref = O.sphere_pyramid(*stitch(b, d), 1)[0]
            want = _check_flags(f, ref)
            assert 0 < int((want & 1).sum()) < want.size and 0 < int((want >> 1).sum()) < want.size
            got = f.level(0)   # a lean frame stitches again in full here: the packed image and its flags stay
            assert all(np.array_equal(got[k], ref[k]) for k in ("gray", "depth", "gx", "gy", "dgx", "dgy"))
            _check_flags(f, ref)
        f.close()
    cal = R.Calib360.for_sphere(ctx, 52, 320)
    f = R.Frame360(cal)
    f.setCompaction(False)
    const = (_gray3(np.full((52, 320), 77)), np.full((52, 320), 1500, np.uint16))
    for images in (noise_sphere(52, 320, 1), noise_sphere(52, 320, 2), const):
        f.set_sphere(*images)
        want = _check_flags(f, O.sphere_pyramid(*images, 1)[0])
    assert not want.any()
    f.close()


# ---------------------------------------------------------------- 2. pass parity
def _wave_counts(need, nb):
    """Needed entries per (workgroup, wave) and per chunk of the batched grid, at a pose that maps every pixel onto
    itself: chunk k of wave w of workgroup b is the 64 pixels from b 256 + 64 w + k nb 256."""
    flat = need.reshape(-1)
    stride = nb * TPB
    out = {}
    for b in range(nb):
        for w in range(TPB // 64):
            b0 = b * TPB + 64 * w
            out[(b, w)] = [int(flat[i:i + 64].sum()) for i in range(b0, flat.size, stride)]
    return out


def test_stripes_hit_the_queue_edges(ctx, bank):
    """The stripes target does what it was drawn for, by the oracle's gradients: on the batched grid, waves with
    exactly 63, 64 and 65 needed entries, and a wave whose entries all come from its last chunk."""
    t, s, lt, _ = bank("stripes")
    reg = R.RegisterPhotoICP(ctx)
    reg.setTargetFrame(t)
    reg.setSourceFrame(s)
    pf, nb = reg.pass_grid(0, 0, True)
    assert (pf, nb) == (6, 12)
    fl = _flags_of(lt)
    assert np.array_equal(fl & 1, fl >> 1)   # the range ramps sit on the gray ramps
    waves = _wave_counts(fl & 1, nb)
    totals = {k: sum(v) for k, v in waves.items()}
    assert (totals[(3, 0)], totals[(3, 1)], totals[(3, 2)]) == (63, 64, 65), totals
    assert all(len(v) == 8 for v in waves.values())
    assert waves[(6, 0)] == [0] * 7 + [30], waves[(6, 0)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["const", "ramp", "stripes", "noise", "ragged"])
def test_pass_parity(ctx, bank, case, method):
    t, s, lt, ls = bank(case)
    p, po = _prm()
    fillers = [bank("noise")[:2], bank("stripes")[:2]] if case != "ragged" else [(s, t), (t, s)]
    counts = _passes(ctx, t, s, lt, ls, method, p, po, fillers, (case, method))
    fl = _flags_of(lt)
    if case == "const":
        assert not fl.any() and all(nv == 0 and nvis > 0 for nv, nvis in counts), counts
    if case == "ramp":   # every pixel with a live gradient is flagged: the queue takes (nearly) every visible pixel
        assert int((fl == 3).sum()) >= (ROWS - 2) * (COLS - 2 - 14)
    if case in ("const", "ramp", "stripes"):
        assert all(nv == 0 or nv >= EXACT_BELOW for nv, _ in counts), counts
    if case != "const":
        assert all(nv >= EXACT_BELOW for nv, _ in counts), counts


# ---------------------------------------------------------------- 3. thresholds
@pytest.mark.parametrize("ti,td", [(0.01, 0.01), (0.02, 0.03), (0.005, 0.002), (0.03, 0.004), (0.004, 0.03)],
                         ids=["equal", "above", "below", "depth-below", "int-below"])
def test_alignment_thresholds_other_than_the_flags(ctx, bank, ti, td):
    """The flags are built for the default thresholds.  An alignment at or above them uses the flags (a superset of
    its salient pixels) and one below them in either threshold treats every pixel as flagged: each equals the oracle
    run with the alignment's thresholds."""
    t, s, lt, ls = bank("noise")
    p, po = _prm(ti, td)
    fillers = [(s, t), bank("stripes")[:2]]
    for method in METHODS:
        counts = _passes(ctx, t, s, lt, ls, method, p, po, fillers, ("thr", ti, td, method))
        assert all(nv >= EXACT_BELOW for nv, _ in counts), counts


# ---------------------------------------------------------------- 4. a flagged frame as the source
@pytest.mark.parametrize("case", ["noise", "ramp"])
def test_flagged_frame_as_source(ctx, bank, case):
    """The source word's luma is read under the flags: the pair reversed, so that the frame whose flags are set (for
    the ramp, on nearly every pixel) is streamed as the source."""
    t, s, lt, ls = bank(case)
    assert _flags_of(lt).any()
    fl, _ = t.saliency()
    assert fl.any()
    p, po = _prm()
    for method in METHODS:
        _passes(ctx, s, t, ls, lt, method, p, po, [(t, s), (t, s)], ("reversed", case, method))
