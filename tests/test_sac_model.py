"""tests/sac_model.py, the statement of the RANSAC plane segmentation, against hand-counted answers (no GPU)."""
import math

import numpy as np

import sac_model as M


def lattice(nx, ny, step=1 / 16, origin=(0.0, 0.0, 0.0), axes=(0, 1)):
    """nx x ny points, `step` apart, in the plane spanned by the two coordinate axes, from `origin`."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * step
    p = np.tile(np.asarray(origin, np.float64), (len(g), 1))
    p[:, axes[0]] += g[:, 0]
    p[:, axes[1]] += g[:, 1]
    return p.astype(np.float32)


def test_sampler_gives_three_distinct_positions():
    for m in (3, 4, 5, 2 ** 30):
        for h in range(300):
            s = M.sample3(5, 1, h, m)
            assert len(set(s)) == 3 and all(0 <= v < m for v in s), (m, h, s)
    for slot in range(3):                                  # every position of m = 5 turns up in every slot
        assert {M.sample3(0, 0, h, 5)[slot] for h in range(300)} == set(range(5))
    assert {tuple(sorted(M.sample3(9, 2, h, 3))) for h in range(50)} == {(0, 1, 2)}
    assert M.sample3(1, 0, 0, 1000) != M.sample3(2, 0, 0, 1000) or M.sample3(1, 0, 1, 1000) != M.sample3(2, 0, 1, 1000)


def test_mix_is_splitmix64():
    # the published first outputs of SplitMix64 from state 0 are mix(0), mix(golden), ...: the first is 0xE220A8397B1DCDAF
    assert M.mix(0) == 0xE220A8397B1DCDAF


def test_closed_threshold_on_a_dyadic_lattice():
    thr = 2.0 ** -6
    floor = lattice(8, 8)
    above = floor.copy(); above[:, 2] = thr                                 # exactly at the threshold: in
    beyond = floor.copy(); beyond[:, 2] = np.nextafter(np.float32(thr), np.float32(1))   # one float beyond: out
    below = floor.copy(); below[:, 2] = -np.nextafter(np.float32(thr), np.float32(1))
    xyz = np.concatenate([floor, above, beyond, below])
    _, _, count, near = M.evaluate(xyz, coef_in=[[0, 0, 1, 0], [0, 0, -1, 0], [0, 0, 1, -thr]], distance_threshold=thr)
    assert count.tolist() == [128, 128, 192]
    assert near == 64 + 64 + 64                             # the points at the threshold are within the band of it ...
    _, _, count, near = M.evaluate(xyz, coef_in=[[0, 0, 1, 0.25]], distance_threshold=thr)
    assert count.tolist() == [0] and near == 0              # ... and no others


def test_duplicates_and_collinear_triples_score_nothing():
    c = M.planes3([[1, 2, 3], [0, 0, 0], [0, 0, 0]], [[1, 2, 3], [1, 1, 1], [0, 0, 0]], [[4, 5, 6], [2, 2, 2], [0, 0, 0]])
    assert np.isnan(c).all()
    xyz = np.concatenate([np.tile(np.float32([[1, 1, 1]]), (200, 1)), np.float32([[0, 0, 0], [2, 2, 2]])])   # one line
    s, coef, count, _ = M.evaluate(xyz, n_hyp=128, distance_threshold=0.01)
    assert np.isnan(coef).all() and not count.any() and (s >= 0).all()
    r = M.segment(xyz, distance_threshold=0.01, min_inliers=3)
    assert r.n_planes == 0 and r.last is not None and r.last.size == 0 and r.last.raw_size == 0
    assert r.last.best_hypothesis == 0 and r.n_evaluated == 1024 and (r.labels == -1).all()


def room(rng, jitter=2.0 ** -9):
    parts = [lattice(40, 40), lattice(30, 30, origin=(-0.5, 0, 0.25), axes=(1, 2)),
             lattice(12, 12, origin=(3.5, 3, 0.25), axes=(0, 2)), rng.uniform(0.3, 2.0, (56, 3)).astype(np.float32)]
    xyz = np.concatenate(parts).astype(np.float64)
    xyz += rng.uniform(-jitter, jitter, xyz.shape)
    return xyz.astype(np.float32)


ROOM = dict(distance_threshold=2.0 ** -6, min_inliers=100, seed=2016)


def test_peel_and_its_four_stops():
    xyz = room(np.random.default_rng(1))
    r = M.segment(xyz, **ROOM)
    assert [p.size for p in r.planes] == [1600, 900, 144]                    # stop 2: the 56 left are below min_inliers
    assert r.last is None and r.n_in_planes == 2644
    assert [int((r.labels == k).sum()) for k in range(3)] == [1600, 900, 144]
    assert (r.labels[:1600] == 0).all() and (r.labels[1600:2500] == 1).all() and (r.labels[2500:2644] == 2).all()
    assert r.n_evaluated == sum(p.evaluated for p in r.planes) == 384 and r.k_decided()
    assert abs(r.planes[0].coef[2] - 1) < 1e-4 and abs(r.planes[1].coef[0] - 1) < 1e-4 and abs(r.planes[2].coef[1] - 1) < 1e-4
    r2 = M.segment(xyz, max_planes=2, **ROOM)                               # stop 1
    assert [p.size for p in r2.planes] == [1600, 900] and r2.last is None
    big = dict(ROOM, min_inliers=1000)
    r3 = M.segment(xyz, **big)                                              # stop 4: the second plane is too small
    assert [p.size for p in r3.planes] == [1600] and r3.last is not None and r3.last.size == 900
    assert r3.n_evaluated == r3.planes[0].evaluated + r3.last.evaluated and (r3.labels[1600:] == -1).all()
    r4 = M.segment(xyz, stop_fraction=0.5, **ROOM)                          # stop 3: 1100 left <= 0.5 * 2700
    assert [p.size for p in r4.planes] == [1600] and r4.last is None
    r5 = M.segment(xyz[:1700], **dict(ROOM, min_inliers=150))               # stop 2: the pool of 100 is below min_inliers
    assert [p.size for p in r5.planes] == [1600] and r5.last is None and r5.n_evaluated == r5.planes[0].evaluated


def test_a_tie_goes_to_the_lower_hypothesis():
    a, b = lattice(6, 6), lattice(6, 6, origin=(0, 0, 1.0))
    xyz = np.concatenate([a, b])
    r = M.segment(xyz, distance_threshold=0.01, min_inliers=10, optimize=0, max_planes=1, max_iterations=128)
    _, coef, count, _ = M.evaluate(xyz, n_hyp=128, distance_threshold=0.01)
    assert count.max() == 36 and (count == 36).sum() > 1
    first = int(np.flatnonzero(count == 36)[0])
    assert r.planes[0].best_hypothesis == first and r.planes[0].raw_size == 36
    assert np.array_equal(r.planes[0].coef, M.orient(coef[first]))


def test_constraints_pick_floor_or_wall_against_a_larger_competitor():
    floor, wall = lattice(10, 10), lattice(20, 20, origin=(-1, 0, 0.5), axes=(1, 2))
    xyz = np.concatenate([floor, wall])
    kw = dict(distance_threshold=0.01, min_inliers=50, max_planes=1, axis=(0, 0, 2.0))
    assert M.segment(xyz, **kw).planes[0].size == 400
    r = M.segment(xyz, constraint=M.PERPENDICULAR, **kw)                    # normal along z: the floor
    assert r.planes[0].size == 100 and (r.labels[:100] == 0).all() and abs(r.planes[0].coef[2]) > 0.99
    xyz2 = np.concatenate([lattice(20, 20), lattice(10, 10, origin=(-1, 0, 0.5), axes=(1, 2))])
    assert M.segment(xyz2, **kw).planes[0].size == 400
    r = M.segment(xyz2, constraint=M.PARALLEL, **kw)                        # parallel to z: the wall
    assert r.planes[0].size == 100 and (r.labels[400:] == 0).all() and abs(r.planes[0].coef[0]) > 0.99


def test_gate_excludes_crossed_and_non_finite_normals():
    xyz = lattice(10, 10)
    nrm = np.tile(np.float32([[0, 0, 1]]), (100, 1))
    nrm[:10] = [1, 0, 0]                                    # crossed
    nrm[10:15] = [0, 0, -1]                                 # flipped: the gate is sign-agnostic
    nrm[15, 1] = np.nan
    nrm[16, 0] = np.inf
    _, _, count, _ = M.evaluate(xyz, normals=nrm, coef_in=[[0, 0, 1, 0]], distance_threshold=0.01)
    assert count.tolist() == [88]
    r = M.segment(xyz, normals=nrm, distance_threshold=0.01, min_inliers=10, max_planes=2)
    assert r.planes[0].size == 88 and (r.labels[:10] == -1).all() and (r.labels[15:17] == -1).all()
    assert (r.labels[10:15] == 0).all() and r.n_finite == 100


def test_orientation_rule():
    assert M.orient([0, 0, -1, 2]).tolist() == [0, 0, 1, -2]
    assert M.orient([-0.5, 0.5, 0.1, 1]).tolist() == [0.5, -0.5, -0.1, -1]      # a tie: the lower axis leads
    assert M.orient([0.5, -0.5, 0.1, 1]).tolist() == [0.5, -0.5, 0.1, 1]
    assert M.orient([0.1, -0.9, 0.2, -3]).tolist() == [-0.1, 0.9, -0.2, 3]


def test_non_finite_rows_are_dropped():
    xyz = lattice(12, 12)
    xyz[5, 0], xyz[17, 2], xyz[30, 1] = np.nan, np.inf, -np.inf
    r = M.segment(xyz, distance_threshold=0.01, min_inliers=10)
    assert r.n_in == 144 and r.n_finite == 141 and r.planes[0].size == 141 and (r.labels[[5, 17, 30]] == -1).all()


def test_k_rule_stops_after_one_round_or_runs_out():
    xyz = lattice(20, 20)
    r = M.segment(xyz, distance_threshold=0.01, min_inliers=10, max_planes=1)
    assert r.planes[0].evaluated == 128 and r.planes[0].k < 1 and r.k_decided()
    for it in (1, 127, 128, 129, 130):
        r = M.segment(xyz, distance_threshold=1e-6, probability=0.999, min_inliers=3, max_planes=1, max_iterations=it)
        ev = (r.planes + [r.last])[0].evaluated
        assert ev == (it if ev < 128 or (r.planes + [r.last])[0].rounds[0][1] > 128 else 128)
    assert math.isclose(M.EPS, 2.0 ** -52)
