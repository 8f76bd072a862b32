"""CPU side of tests/test_gpu_icp_shapes.py: the shared input generator is deterministic, and on the room pair the
oracle's passes and alignments are not vacuous at the small ragged spheres that file runs (the floors and iteration
counts it relies on are asserted here on the oracle alone, where no GPU is needed)."""
import numpy as np
import pytest

from oracle import oracle360 as O
from _cases import ROOM_MOTION, ROOM_SOURCE, ROOM_TARGET, noise_sphere, room_pair, room_sphere

GEOMS = {"20x72": (20, 72, 2), "16x64": (16, 64, 4), "32x64": (32, 64, 4), "40x256": (40, 256, 4),
         "52x416": (52, 416, 3), "64x384": (64, 384, 6), "80x576": (80, 576, 5), "130x1040": (130, 1040, 2)}
POSES = [np.eye(4, dtype=np.float32), O.exp_se3([0.02, -0.03, 0.05, 0.01, -0.015, 0.02])]
# levels too small for a pass to mean much: the plain pass finds no valid pixel, with 12 to 125 in view (its sums are
# exactly 0 where nothing is valid, which the GPU file checks)
DEGENERATE = {(4, 16), (2, 8), (8, 16), (4, 8), (2, 12)}


def test_generators_are_deterministic():
    for rows, cols in ((20, 72), (52, 416)):
        a, b = room_pair(rows, cols), room_pair(rows, cols)
        for (ab, ad), (bb, bd) in zip(a, b):
            assert np.array_equal(ab, bb) and np.array_equal(ad, bd)
            assert ab.shape == (rows, cols, 3) and ab.dtype == np.uint8
            assert ad.shape == (rows, cols) and ad.dtype == np.uint16
        na, nb = noise_sphere(rows, cols, 5), noise_sphere(rows, cols, 5)
        assert np.array_equal(na[0], nb[0]) and np.array_equal(na[1], nb[1])
        assert not np.array_equal(noise_sphere(rows, cols, 6)[1], na[1])
    # the two eyes see one room: different images, holes where the seed puts them, about `holes` of the pixels
    (tb, td), (sb, sd) = room_pair(64, 384)
    assert not np.array_equal(tb, sb) and not np.array_equal(td == 0, sd == 0)
    for d in (td, sd):
        assert 0.08 < (d == 0).mean() < 0.12
        assert 1300 <= d[d > 0].min() and d.max() <= 5200   # mm: every wall is 1.3 .. 5.2 m from both eyes
    solid = room_sphere(64, 384, *ROOM_TARGET, holes=0.0)[1]
    assert (solid > 0).all() and np.array_equal(solid[td > 0], td[td > 0])
    # the centre pixel's ray (phi ~ 0, theta ~ 0) runs along +z: the wall at z = 3.4 m, from z = 0.3 m
    assert abs(int(solid[32, 192]) - 3100) <= 2


def test_room_geometry_matches_the_sphere_model():
    """A hit point rendered from the target eye, moved into the source eye's frame, projects where the source image
    shows the same wall: the generator follows the library's pixel-to-ray convention (the oracle aligns the pair)."""
    rows, cols = 64, 384
    solid_t = room_sphere(rows, cols, *ROOM_TARGET, holes=0.0)[1].astype(np.float64) / 1000
    solid_s = room_sphere(rows, cols, *ROOM_SOURCE, holes=0.0)[1].astype(np.float64) / 1000
    ares = 2 * np.pi / cols
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    phi, th = (rows / 2 - 0.5 - r) * ares, c * ares - np.pi
    d = np.stack([np.sin(phi), np.cos(phi) * np.sin(th), np.cos(phi) * np.cos(th)], -1)
    h = np.asarray(ROOM_TARGET[0]) + solid_t[..., None] * d          # hit points in room coordinates
    v = h - np.asarray(ROOM_SOURCE[0])
    rng = np.linalg.norm(v, axis=-1)
    rr = np.rint(rows / 2 - 0.5 - np.arcsin(v[..., 0] / rng) / ares).astype(int)
    cc = np.rint((np.arctan2(v[..., 1], v[..., 2]) + np.pi) / ares).astype(int) % cols
    ok = (rr >= 0) & (rr < rows)
    err = np.abs(solid_s[rr[ok], cc[ok]] - rng[ok])
    assert ok.mean() > 0.8 and np.median(err) < 0.02   # within a pixel's change of range, except at wall edges


@pytest.mark.parametrize("name", list(GEOMS))
def test_oracle_passes_are_not_vacuous(name):
    rows, cols, n = GEOMS[name]
    (tb, td), (sb, sd) = room_pair(rows, cols)
    pt, ps = O.sphere_pyramid(tb, td, n), O.sphere_pyramid(sb, sd, n)
    for l in range(n):
        shape = (rows >> l, cols >> l)
        for method in (0, 1, 2):
            for P in POSES:
                for occ in (0, 1, 2):
                    if occ == 0:
                        _, _, nv = O.error_sphere(ps[l], pt[l], P, method)
                        _, _, nvis = O.hessgrad_sphere(ps[l], pt[l], P, method)
                    else:
                        _, nv = O.error_sphere_occ(ps[l], pt[l], P, method, occ)
                        _, _, nvis = O.hessgrad_sphere_occ(ps[l], pt[l], P, method, occ)
                    if shape[0] >= 8 and shape[1] >= 32:
                        assert nv >= 64 and nvis >= 100, (l, method, occ, nv, nvis)
                    if shape in DEGENERATE and occ == 0:   # (the Occ variants count other things as valid)
                        assert nv == 0 and 9 <= nvis <= shape[0] * shape[1], (l, method, occ, nv, nvis)


@pytest.mark.parametrize("name,n_pyr", [("52x416", 3), ("64x384", 5), ("80x576", 5)])
@pytest.mark.parametrize("fixed", [0, 6])
def test_oracle_recovers_the_room_displacement(name, n_pyr, fixed):
    """alignFrames360 (PHOTO_DEPTH, sigma 3/255) from the identity: the displacement between the two eyes within
    5 mm, no rotation, iterating at least twice on two levels (measured: iters [2, 1, 3] at 52x416, [1, 1, 2, 2, 0] at
    64x384, [1, 2, 3, 1, 1] at 80x576; 1.2 / 2.7 / 0.7 mm)."""
    rows, cols, _ = GEOMS[name]
    (tb, td), (sb, sd) = room_pair(rows, cols)
    p = O.IcpParams.default(n_pyr=n_pyr, std_dev_photo=np.float32(3.0 / 255), fixed_iters_level0=fixed)
    rc, pose, H, g, st = O.align360(tb, td, sb, sd, None, O.PHOTO_DEPTH, p)
    assert rc == 0
    assert np.linalg.norm(pose[:3, 3] - np.array(ROOM_MOTION)) <= 5e-3, pose[:3, 3]
    assert O.rot_angle(pose, np.eye(4)) <= 2e-3
    iters = list(st.iters)[:n_pyr]
    assert sum(1 for k in iters if k >= 2) >= 2, iters
