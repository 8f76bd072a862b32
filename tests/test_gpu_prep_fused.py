"""The sphere's dense preparation as tiled launches: level 0's gradients, level 1 and its gradients from one
workgroup per level-0 tile, the deeper levels and their gradients from one workgroup per tile of the coarsest level
(three levels per launch).  Every level and field against the CPU oracle, bit for bit, on shapes that exercise what
the tiles can get wrong: a one-level and a two-row pyramid, odd last levels, widths and heights that are no
multiple of any tile (edge tiles in both directions), several workgroups per launch, and 6-level pyramids, whose
last level comes from a second tail launch."""
import os

import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import noise_sphere as sphere_images

pytestmark = pytest.mark.gpu

FIELDS = ("gray", "depth", "gx", "gy", "dgx", "dgy")
# (sphere rows, sphere columns, pyramid levels the library builds for it)
SHAPES = [(2, 8, 1), (4, 16, 2), (20, 72, 2), (52, 416, 3), (72, 480, 4), (80, 576, 5), (96, 768, 6), (64, 384, 6),
          (130, 1040, 2)]


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


@pytest.mark.parametrize("rows,cols,n_levels", SHAPES, ids=[f"{r}x{c}" for r, c, _ in SHAPES])
def test_ragged_shapes_bitexact(ctx, rows, cols, n_levels):
    bgr, dep = sphere_images(rows, cols, 1000 * rows + cols)
    cal = R.Calib360.for_sphere(ctx, rows, cols)
    f = R.Frame360(cal)
    f.set_sphere(bgr, dep)
    ref = O.sphere_pyramid(bgr, dep, n_levels)
    for l in range(n_levels):
        got = f.level(l)
        assert got["gray"].shape == (rows >> l, cols >> l)
        for k in FIELDS:
            assert np.array_equal(got[k], ref[l][k]), (l, k)
    with pytest.raises(RuntimeError):   # the pyramid stops where the test expects it to
        f.level(n_levels)
    if n_levels > 2:   # a shorter pyramid of the same frame: the tail launch with fewer levels than it can take
        f.setNumPyr(n_levels - 1)
        f.set_sphere(bgr, dep)
        for l in range(n_levels - 1):
            got = f.level(l)
            for k in FIELDS:
                assert np.array_equal(got[k], ref[l][k]), (l, k)


# ---------------------------------------------------------------- lean frames
# A frame that only enters batched alignments (setCompaction(False)) whose level 0 those passes stream as the packed
# image is built lean: its stitch stores only the packed level-0 image.  The sphere images and level 0's {gray, depth}
# appear with the first call that reads them (BUILT_LEVEL0 of Frame360.built()), identical to a full build's.
def _sample_images():
    return [O.load_bin(os.path.join(R.SAMPLES_DIR, n)) for n in ("sphere_images_1.bin", "sphere_images_10.bin")]


def _random_images(rows, cols, seed):
    out = []
    for k in range(3):
        rng = np.random.default_rng(seed + k)
        b = rng.integers(0, 256, (8, rows, cols, 3), dtype=np.uint8)
        d = rng.integers(0, 7000, (8, rows, cols)).astype(np.uint16)
        d[rng.random((8, rows, cols)) < 0.2] = 0
        out.append((b, d))
    return out


LEAN_CASES = {
    "qvga_samples": (240, 320, _sample_images, True),                      # sphere 320 x 1920
    "48x64": (48, 64, lambda: _random_images(48, 64, 4864), True),         # sphere 64 x 384
    "36x48": (36, 48, lambda: _random_images(36, 48, 3648), False),        # sphere 48 x 288: rows of 4.5 waves, full
}


def _check_against_oracle(f, full, ref, sb, sd, first):
    """Every getter of f against the oracle (points: the oracle's valid pixels and gray values, and the full build's
    records), starting with `first`, the getter that has to bring level 0 in."""
    n = len(ref)

    def level(l):
        got = f.level(l)
        for k in FIELDS:
            assert np.array_equal(got[k], ref[l][k]), (l, k)

    def points():
        pts = f.points(0)
        d, g = ref[0]["depth"].reshape(-1), ref[0]["gray"].reshape(-1)
        valid = (d > np.float32(0.3)) & (d < np.float32(6.0))
        assert pts.shape[0] == int(valid.sum()) and np.array_equal(pts[:, 3], g[valid])
        assert np.array_equal(pts, full.points(0))

    def sphere():
        gb, gd = f.sphere()
        assert np.array_equal(gb, sb) and np.array_equal(gd, sd)

    getters = {"level0": lambda: level(0), "points0": points, "sphere": sphere}
    getters[first]()
    assert f.built() & R.BUILT_LEVEL0
    for name, g in getters.items():
        if name != first:
            g()
    for l in range(1, n):
        level(l)


@pytest.mark.parametrize("case", list(LEAN_CASES))
def test_lean_frames_match_full_and_oracle(ctx, case):
    rows, cols, images, lean = LEAN_CASES[case]
    cal = R.Calib360(ctx, rows, cols)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    _, rti, K = cal.extrinsics()
    Km = K.reshape(3, 3).T
    f, full = R.Frame360(cal), R.Frame360(cal)
    f.setCompaction(False)
    imgs = images()
    # build -> getter -> re-upload -> build -> getter, each round entering through another getter
    for (b, d), first in zip(imgs + imgs[:1], ("level0", "points0", "sphere")):
        sb, sd = O.stitch(b, d, rti, Km)
        n = 1
        while n < 6 and (sb.shape[0] >> n) >= 2 and (sb.shape[1] >> n) >= 8 and (sb.shape[1] >> n) % 4 == 0 and \
                (sb.shape[0] >> (n - 1)) % 2 == 0 and (sb.shape[1] >> (n - 1)) % 2 == 0:
            n += 1
        ref = O.sphere_pyramid(sb, sd, n)
        for fr in (f, full):
            fr.upload(b, d)
            assert fr.built() == 0
            fr.build()
        assert full.built() & R.BUILT_LEVEL0
        assert bool(f.built() & R.BUILT_LEVEL0) == (not lean)
        with pytest.raises(RuntimeError):
            f.level(n)   # n is the library's level count
        if n > 1:        # a level below 0 needs no level-0 output: the frame stays lean
            got = f.level(1)
            assert all(np.array_equal(got[k], ref[1][k]) for k in FIELDS)
            assert bool(f.built() & R.BUILT_LEVEL0) == (not lean)
        _check_against_oracle(f, full, ref, sb, sd, first)


@pytest.mark.parametrize("occlusion", [0, 1])
def test_alignment_materialises_a_lean_target(ctx, occlusion):
    """alignFrames360 of a full source against a lean target (a lone alignment's level-0 pass reads the target's
    {gray, depth} image: PF 5, or PF 3 with the occlusion projection) equals the alignment against a full target bit
    for bit: pose, Hessian, gradient and iteration counts."""
    cal = R.Calib360(ctx, 240, 320)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    cal.loadIntrinsicCalibration(R.INTRINSICS_DIR)
    (b1, d1), (b2, d2) = _sample_images()
    src, full, lean = R.Frame360(cal), R.Frame360(cal), R.Frame360(cal)
    lean.setCompaction(False)
    src.upload(b2, d2); full.upload(b1, d1); lean.upload(b1, d1)
    for f in (src, full, lean):
        f.build()
    assert not lean.built() & R.BUILT_LEVEL0
    out = []
    for trg in (full, lean):
        reg = R.RegisterPhotoICP(ctx)
        reg.setNumPyr(5)
        reg.setGrayVariance(3.0 / 255)
        reg.setTargetFrame(trg); reg.setSourceFrame(src)
        reg.alignFrames360(np.eye(4), R.PHOTO_DEPTH, occlusion)
        out.append((reg.getOptimalPose().copy(), reg.getHessian().copy(), reg.getGradient().copy(),
                    list(reg.stats.iters), list(reg.stats.evals)))
    assert lean.built() & R.BUILT_LEVEL0
    (pa, Ha, ga, ia, ea), (pb, Hb, gb, ib, eb) = out
    assert np.array_equal(pa, pb) and np.array_equal(Ha, Hb) and np.array_equal(ga, gb)
    assert ia == ib and ea == eb and sum(ia) > 0
