"""RANSAC plane segmentation on the GPU (r360_cloud_sac_planes, r360_cloud_sac_eval, r360_ctx_map_sac_planes,
r360_ctx_map_filter_planes) against the brute-force numpy statement tests/sac_model.py.

Every case first asserts, on the model alone, that its undecided sets are empty: no (point, hypothesis) pair scored has a
distance, gate or constraint value within 1e-12 of its threshold, no point lies within 1e-9 of a refined plane's
threshold, and at every round boundary |k - evaluated| > 1e-9 k.  (The condition a seed must meet is at most 1 % of the
points; the seeds here were chosen on the CPU so that there are none, and the cases assert none.)  The crafted
hypotheses of the closed-threshold case are the exception: their points lie exactly at the threshold by construction,
and every operation on their dyadic numbers is exact on both sides.

Bounds, derived and not measured:
  * samples, count, labels, size, raw_size, best_hypothesis, evaluated and the stats: exact.  Both sides draw with the
    same integer arithmetic, decide an inlier with the same float64 operations on the same float32 inputs, and counts are
    integer sums.
  * coefficients of r360_cloud_sac_eval and of optimize = 0: bit for bit.  Both sides run the same IEEE operations in
    the stated order; float64 division and square root are correctly rounded on both.
  * optimize = 1.  The refined plane comes from one covariance summed and solved on both sides, so the bounds are those
    tests/test_gpu_clusters.py derives, restated: the centroid's two sums of the same N terms differ by at most
    B = (N - 1) 2^-53 sum |x| (the model's sum_bound) and the division rounds once more,
    |centroid - model| <= B / N + 2^-52 |centroid|; per entry the covariances differ by E = cov_bound (N + 7) /
    ((N - 1) N) (the six moments in two orders, plus 8 units of 2^-53 per term for means that differ in the last
    place); with w = E / l2, where the model marks the solve decided (l1 - l0 >= 1e-5 l2), eigenvalues agree within
    (1e-12 + w) l2, the eigenvector's components within 1e-8 + w, the curvature within 1e-12 + w.  The record's normal is
    that eigenvector of the best hypothesis' inliers (the model's `fit`), its sign fixed by the orientation rule, which
    the case asserts is decided (the leading |component| leads by 1e-6); d = -n . centroid moves by at most
    (1e-8 + w) sum |centroid| + sum of the centroid's bounds + 2^-50 (sum |centroid| + |d|).  centroid, eig and curvature
    of the record are those of the final inliers, with their own N, bounds and w.  Labels are exact, because no point
    lies within 1e-9 of the refined threshold."""
import numpy as np
import pytest

import rgbd360_amd as R
import sac_model as M

pytestmark = pytest.mark.gpu

THR = 2.0 ** -6


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _fields(st):
    return [getattr(st, f) for f, _ in st._fields_]


def _prm(**kw):
    return R.SacParams.make(**kw)


# ------------------------------------------------------------------ clouds
def lattice(nx, ny, step=1 / 16, origin=(0.0, 0.0, 0.0), axes=(0, 1)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * step
    p = np.tile(np.asarray(origin, np.float64), (len(g), 1))
    p[:, axes[0]] += g[:, 0]
    p[:, axes[1]] += g[:, 1]
    return p


def _jitter(parts, rng, jitter=2.0 ** -9):
    xyz = np.concatenate(parts).astype(np.float64)
    return (xyz + rng.uniform(-jitter, jitter, xyz.shape)).astype(np.float32)


def room(seed=1, shuffle=True):
    """Floor 40 x 40, walls 30 x 30 and 12 x 12, 56 loose points, every coordinate jittered by up to 2^-9; shuffled."""
    rng = np.random.default_rng(seed)
    xyz = _jitter([lattice(40, 40), lattice(30, 30, origin=(-0.5, 0, 0.25), axes=(1, 2)),
                   lattice(12, 12, origin=(3.5, 3, 0.25), axes=(0, 2)), rng.uniform(0.3, 2.0, (56, 3))], rng)
    return xyz[rng.permutation(len(xyz))] if shuffle else xyz


ROOM = dict(distance_threshold=THR, min_inliers=100, seed=2016)


def slab(n, seed):
    """n points: about three quarters on a jittered tilted plane, the rest loose around it."""
    rng = np.random.default_rng(seed)
    k = (3 * n) // 4
    uv = rng.uniform(0, 2, (k, 2))
    on = np.stack([uv[:, 0], uv[:, 1], 0.25 * uv[:, 0] - 0.125 * uv[:, 1] + 0.5], 1)
    return _jitter([on, rng.uniform(0, 2, (n - k, 3))], rng)


# ------------------------------------------------------------------ the comparison
def _check_refined(pl, m):
    """One record of an optimize = 1 call against the model's plane, within the docstring's bounds."""
    fit = m.fit
    assert fit["eig_decided"] and m.eig_decided, "the eigen-solve is not decided: choose another seed"
    lead = np.sort(np.abs(m.coef[:3]))
    assert lead[2] - lead[1] >= 1e-6, "the orientation rule is not decided: choose another seed"
    nr = float(m.raw_size)
    w_fit = fit["cov_bound"] * (nr + 7) / ((nr - 1) * nr) / fit["eig"][2]
    e_n = np.abs(pl["coef"][:3] - m.coef[:3])
    c1 = np.abs(fit["centroid"]).sum()
    b_d = (1e-8 + w_fit) * c1 + (fit["sum_bound"] / nr + 2.0 ** -52 * np.abs(fit["centroid"])).sum() + \
        2.0 ** -50 * (c1 + abs(m.coef[3]))
    e_d = abs(pl["coef"][3] - m.coef[3])
    print(f"plane of {m.size}: normal {e_n.max():.2e} (bound {1e-8 + w_fit:.2e}), d {e_d:.2e} (bound {b_d:.2e})")
    assert (e_n <= 1e-8 + w_fit).all() and e_d <= b_d
    _check_moments(pl, m)


def _check_moments(pl, m):
    """centroid, eig and curvature of one record, those of the final inliers, within the docstring's bounds."""
    n = float(m.size)
    e_c = np.abs(pl["centroid"] - m.centroid)
    b_c = m.sum_bound / n + 2.0 ** -52 * np.abs(m.centroid)
    assert (e_c <= b_c).all(), (e_c, b_c)
    assert np.isfinite(pl["eig"]).all() and np.isfinite(pl["curvature"])
    if not m.eig_decided:
        return
    l2 = m.eig[2]
    w = m.cov_bound * (n + 7) / ((n - 1) * n) / l2
    e_eig = np.abs(pl["eig"] - m.eig) / l2
    e_cur = abs(pl["curvature"] - m.curvature)
    print(f"plane of {m.size}: centroid {(e_c / np.maximum(b_c, 1e-300)).max():.2f} of its bound, eig {e_eig.max():.2e} l2, "
          f"curvature {e_cur:.2e}, w {w:.2e}")
    assert (e_eig <= 1e-12 + w).all() and e_cur <= 1e-12 + w


def _check(ctx, xyz, normals=None, **kw):
    """Product parity of one case against its model; returns (model, labels, planes, stats)."""
    m = M.segment(xyz, normals, **kw)
    assert m.near_pairs == 0 and m.near_refined == 0, ("undecided comparisons: choose another seed", m.near_pairs,
                                                       m.near_refined)
    assert m.k_decided(), "a round boundary's k is undecided: choose another seed"
    labels, planes, st = ctx.sac_planes(xyz, _prm(**kw), normals)
    assert _fields(st) == [m.n_in, m.n_finite, m.n_planes, m.n_in_planes, m.n_evaluated]
    assert np.array_equal(labels, m.labels), np.flatnonzero(labels != m.labels)[:10]
    assert len(planes) == m.n_planes
    for pl, mp in zip(planes, m.planes):
        assert (pl["size"], pl["raw_size"], pl["best_hypothesis"], pl["evaluated"]) == \
            (mp.size, mp.raw_size, mp.best_hypothesis, mp.evaluated)
        if mp.refined:
            _check_refined(pl, mp)
        else:
            assert _bits(pl["coef"]) == _bits(mp.coef), (pl["coef"], mp.coef)
            _check_moments(pl, mp)
    return m, labels, planes, st


def _check_eval(ctx, xyz, normals=None, n_hyp=128, **kw):
    s, coef, count, near = M.evaluate(xyz, normals, n_hyp=n_hyp, **kw)
    assert near == 0, ("undecided comparisons: choose another seed", near)
    gs, gcoef, gcount = ctx.sac_eval(xyz, _prm(**kw), normals, n_hyp=n_hyp)
    assert np.array_equal(gs, s), np.flatnonzero((gs != s).any(1))[:10]
    assert np.array_equal(gcount, count), np.flatnonzero(gcount != count)[:10]
    assert _bits(gcoef) == _bits(coef), np.flatnonzero((gcoef.view(np.uint64) != coef.view(np.uint64)).any(1))[:10]
    return s, coef, count


# ------------------------------------------------------------------ tiny pools
def test_empty_and_all_non_finite(ctx):
    for xyz in (np.zeros((0, 3), np.float32), np.full((70, 3), np.nan, np.float32)):
        m, labels, planes, st = _check(ctx, xyz, min_inliers=3)
        assert st.n_planes == 0 and st.n_evaluated == 0 and (labels == -1).all()
        s, coef, count = ctx.sac_eval(xyz, _prm(), n_hyp=5)
        assert (s == -1).all() and np.isnan(coef).all() and not count.any()


def test_two_and_three_finite_rows(ctx):
    xyz = np.full((9, 3), np.nan, np.float32)
    xyz[2], xyz[7] = [0, 0, 0], [1, 0, 0]
    m, labels, planes, st = _check(ctx, xyz, min_inliers=3)
    assert (st.n_finite, st.n_planes, st.n_evaluated) == (2, 0, 0)
    xyz[4] = [0, 1, 0.5]
    m, labels, planes, st = _check(ctx, xyz, min_inliers=3, distance_threshold=THR, optimize=0)
    assert st.n_planes == 1 and planes[0]["size"] == 3 and sorted(np.flatnonzero(labels == 0)) == [2, 4, 7]
    _check(ctx, xyz, min_inliers=3, distance_threshold=THR)
    s, _, count = _check_eval(ctx, xyz, n_hyp=7, distance_threshold=THR)
    assert (np.sort(s, 1) == [2, 4, 7]).all() and (count == 3).all()


def test_three_collinear_and_identical_points(ctx):
    m, labels, planes, st = _check(ctx, np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), min_inliers=3, max_iterations=130)
    assert st.n_planes == 0 and st.n_evaluated == 130 and m.last.raw_size == 0
    xyz = np.concatenate([np.tile(np.float32([[1, 1, 1]]), (200, 1)), np.float32([[0, 0, 0], [2, 2, 2]])])
    xyz = xyz[np.random.default_rng(3).permutation(202)]
    m, labels, planes, st = _check(ctx, xyz, min_inliers=3, distance_threshold=0.01)
    assert st.n_planes == 0 and st.n_evaluated == 1024
    _, coef, count = _check_eval(ctx, xyz, distance_threshold=0.01)
    assert np.isnan(coef).all() and not count.any()


# ------------------------------------------------------------------ pool sizes around a wave and a workgroup, and a striding grid
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_pool_sizes_around_a_workgroup(ctx, n):
    xyz = slab(n, 40 + n)
    _check_eval(ctx, xyz, n_hyp=128, distance_threshold=THR)
    m, *_ = _check(ctx, xyz, distance_threshold=THR, min_inliers=20, max_planes=2)
    assert m.n_planes >= 1


def test_a_pool_larger_than_the_capped_grid(ctx):
    n = 70001                                   # more than 256 workgroups of 256 rows: the count kernel strides
    xyz = slab(n, 5)
    xyz[::1000, 1] = np.nan
    _check_eval(ctx, xyz, n_hyp=130, distance_threshold=THR)
    m, labels, planes, st = _check(ctx, xyz, distance_threshold=THR, min_inliers=1000, max_planes=2)
    assert m.n_planes == 1 and planes[0]["size"] > 50000        # its moments span several chunks


# ------------------------------------------------------------------ rounds and iteration limits
@pytest.mark.parametrize("it", [1, 127, 128, 129, 130])
def test_iteration_limits(ctx, it):
    xyz = slab(300, 8)
    m, labels, planes, st = _check(ctx, xyz, distance_threshold=2.0 ** -12, probability=0.999, min_inliers=3, max_planes=1,
                                   max_iterations=it, optimize=0)
    assert st.n_evaluated == it                  # so thin a plane never satisfies the k rule
    _check_eval(ctx, xyz, n_hyp=it, distance_threshold=2.0 ** -12)


def test_k_rule_stops_after_the_first_round(ctx):
    m, labels, planes, st = _check(ctx, slab(400, 9), distance_threshold=THR, min_inliers=100, max_planes=1)
    assert st.n_evaluated == 128 and planes[0]["evaluated"] == 128 and m.planes[0].k < 128


# ------------------------------------------------------------------ crafted hypotheses
def test_crafted_hypotheses_closed_threshold_ties_and_no_inlier(ctx):
    floor = lattice(8, 8).astype(np.float32)
    above, beyond, below = floor.copy(), floor.copy(), floor.copy()
    above[:, 2] = THR                                                        # exactly at the threshold: in
    beyond[:, 2] = np.nextafter(np.float32(THR), np.float32(1))              # one float beyond: out
    below[:, 2] = -np.nextafter(np.float32(THR), np.float32(1))
    xyz = np.concatenate([floor, above, beyond, below])[np.random.default_rng(6).permutation(256)]
    coef_in = np.array([[0, 0, 1, 0], [0, 0, -1, 0], [0, 0, 1, -THR], [0, 0, 1, 0.25], [np.nan] * 4, [1, 0, 0, 100.0]])
    _, _, count, _ = M.evaluate(xyz, coef_in=coef_in, distance_threshold=THR)
    assert count.tolist() == [128, 128, 192, 0, 0, 0]      # two equal counts, two planes with no inlier, one NaN
    s, coef, gcount = ctx.sac_eval(xyz, _prm(distance_threshold=THR), coef_in=coef_in)
    assert gcount.tolist() == count.tolist() and _bits(coef) == _bits(coef_in) and (s == -1).all()
    many = np.tile(coef_in, (50, 1))                        # 300 hypotheses: three rounds, the last one short
    assert ctx.sac_eval(xyz, _prm(distance_threshold=THR), coef_in=many)[2].tolist() == count.tolist() * 50


def test_a_tie_goes_to_the_lower_hypothesis(ctx):
    xyz = np.concatenate([lattice(6, 6), lattice(6, 6, origin=(0, 0, 1.0))]).astype(np.float32)
    kw = dict(distance_threshold=0.01, min_inliers=10, optimize=0, max_planes=1, max_iterations=128)
    _, coef, count = _check_eval(ctx, xyz, distance_threshold=0.01)
    assert (count == 36).sum() > 1
    m, labels, planes, st = _check(ctx, xyz, **kw)
    assert planes[0]["best_hypothesis"] == int(np.flatnonzero(count == 36)[0])


# ------------------------------------------------------------------ non-finite rows
def test_non_finite_rows_anywhere(ctx):
    xyz = room(2)
    rng = np.random.default_rng(12)
    bad = rng.choice(len(xyz), 300, replace=False)
    xyz[bad[:100], 0], xyz[bad[100:200], 1], xyz[bad[200:], 2] = np.nan, np.inf, -np.inf
    m, labels, planes, st = _check(ctx, xyz, **ROOM)
    assert st.n_finite == len(xyz) - 300 and (labels[bad] == -1).all() and st.n_planes == 3
    _check_eval(ctx, xyz, **ROOM)


# ------------------------------------------------------------------ the peel
def test_room_peel(ctx):
    xyz = room(1)
    m, labels, planes, st = _check(ctx, xyz, **ROOM)
    assert planes["size"].tolist() == [1600, 900, 144] and st.n_in_planes == 2644
    assert all(p.evaluated == 128 for p in m.planes)        # each plane decided after one round
    m, labels, planes, st = _check(ctx, xyz, optimize=0, **ROOM)
    assert st.n_planes == 3


@pytest.mark.parametrize("kw,sizes", [(dict(max_planes=2), [1600, 900]), (dict(min_inliers=1000), [1600]),
                                      (dict(stop_fraction=0.5), [1600])])
def test_room_peel_stops(ctx, kw, sizes):
    m, labels, planes, st = _check(ctx, room(1), **dict(ROOM, **kw))
    assert planes["size"].tolist() == sizes


def test_room_constraints(ctx):
    xyz = room(1)
    kw = dict(ROOM, axis=(0.0, 0.0, 3.0), eps_angle=0.1)
    m, labels, planes, st = _check(ctx, xyz, constraint=M.PERPENDICULAR, **kw)
    assert planes["size"].tolist() == [1600]                # the 900-point wall is not found
    m, labels, planes, st = _check(ctx, xyz, constraint=M.PARALLEL, **kw)
    assert planes["size"].tolist() == [900, 144]            # the floor is not found
    _, coef, _ = _check_eval(ctx, xyz, constraint=M.PARALLEL, **kw)
    assert np.isnan(coef).any() and np.isfinite(coef).any()


# ------------------------------------------------------------------ the gate
def test_gate_excludes_crossed_and_non_finite_normals(ctx):
    rng = np.random.default_rng(15)
    xyz = _jitter([lattice(20, 20)], rng, 2.0 ** -11)
    nrm = np.tile(np.float32([[0, 0, 1]]), (400, 1))
    nrm[:40] = [1, 0, 0]                                    # crossed
    nrm[40:60] = [0, 0, -1]                                 # flipped: the gate is sign-agnostic
    nrm[60:70, 1] = np.nan
    nrm[70:80, 0] = np.inf
    nrm[80:90, 2] = -np.inf
    perm = rng.permutation(400)
    xyz, nrm = xyz[perm], nrm[perm]
    kw = dict(distance_threshold=THR, min_inliers=30, max_planes=2)
    m, labels, planes, st = _check(ctx, xyz, nrm, **kw)
    assert planes["size"].tolist() == [330] and st.n_finite == 400
    assert (labels[np.isin(perm, np.arange(40))] == -1).all() and (labels[np.isin(perm, np.arange(60, 90))] == -1).all()
    assert (labels[np.isin(perm, np.arange(40, 60))] == 0).all()
    _check_eval(ctx, xyz, nrm, **kw)
    assert ctx.sac_planes(xyz, _prm(**kw))[1]["size"].tolist() == [400]     # plain: all of them


# ------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bytes_and_another_seed_other_samples(ctx):
    xyz = room(3)
    a, b = ctx.sac_planes(xyz, _prm(**ROOM)), ctx.sac_planes(xyz, _prm(**ROOM))
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and _fields(a[2]) == _fields(b[2])
    e1, e2 = ctx.sac_eval(xyz, _prm(**ROOM)), ctx.sac_eval(xyz, _prm(**ROOM))
    assert all(_bits(x) == _bits(y) for x, y in zip(e1, e2))
    e3 = ctx.sac_eval(xyz, _prm(**dict(ROOM, seed=2017)))
    assert not np.array_equal(e1[0], e3[0])


def test_record_capacity_error_still_reports_the_count(ctx):
    import ctypes as C
    xyz, prm = room(1), _prm(**ROOM)
    npl, info = C.c_size_t(), np.zeros(2, R.SAC_PLANE_DTYPE)
    rc = R.lib().r360_cloud_sac_planes(ctx.h, xyz.ctypes.data_as(R._FP), None, len(xyz), C.byref(prm), None,
                                       C.c_void_p(info.ctypes.data), 2, C.byref(npl), None)
    assert rc < 0 and npl.value == 3


# ------------------------------------------------------------------ the map
def _fill_map(ctx):
    ctx.map_reset()
    xyz = room(1)
    rgba = np.random.default_rng(30).integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    assert ctx.map_add_cloud(xyz, rgba, leaf=0.05)
    return ctx.map_download()


MAP = dict(distance_threshold=THR, min_inliers=100, seed=2016)


def test_map_planes_equal_the_cloud_call_on_the_downloaded_map(ctx):
    xyz, rgba = _fill_map(ctx)
    prm = _prm(**MAP)
    st = ctx.map_sac_planes(prm)
    labels, info = ctx.map_plane_labels(), ctx.map_planes()
    l2, i2, s2 = ctx.sac_planes(xyz, prm)
    assert _bits(labels) == _bits(l2) and _bits(info) == _bits(i2) and _fields(st) == _fields(s2)
    assert _bits(ctx.map_plane_labels()) == _bits(labels)   # still the map's after a cloud call
    assert st.n_planes >= 2 and st.n_in == len(xyz)
    x2, c2 = ctx.map_download()
    assert _bits(x2) == _bits(xyz) and _bits(c2) == _bits(rgba)


def test_map_plane_labels_are_invalidated_by_map_changes(ctx):
    prm = _prm(**MAP)
    xyz, _ = _fill_map(ctx)
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_plane_labels()
    cprm = R.ClusterParams.make(0.1, 20)
    ctx.map_cluster(cprm)
    clabels = ctx.map_labels()
    ctx.map_sac_planes(prm)
    assert len(ctx.map_plane_labels()) == len(xyz)
    assert _bits(ctx.map_labels()) == _bits(clabels)        # the cluster stage's labels are untouched and still valid
    ctx.map_cluster(cprm)
    ctx.map_plane_labels()                                  # and clustering leaves the plane labels valid
    ctx.map_add_cloud(np.float32([[9, 9, 9]]), None, leaf=0.05)
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_plane_labels()
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_planes()
    ctx.map_sac_planes(prm)
    ctx.map_filter_outliers(R.OutlierParams.radius_filter(0.15, 2))
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_plane_labels()
    ctx.map_sac_planes(prm)
    ctx.map_filter_clusters(cprm)
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_plane_labels()
    ctx.map_sac_planes(prm)
    ctx.map_reset()
    with pytest.raises(RuntimeError, match="no valid plane labels"):
        ctx.map_plane_labels()


def test_map_planes_with_normals(ctx):
    xyz, _ = _fill_map(ctx)
    prm = _prm(**MAP, normal_angle=0.3)
    with pytest.raises(RuntimeError, match="no valid normals"):
        ctx.map_sac_planes(prm, use_normals=True)
    with pytest.raises(RuntimeError, match="no valid normals"):
        ctx.map_filter_planes(prm, use_normals=True)
    assert ctx.map_size() == len(xyz)                        # the failed calls left the map alone
    ctx.map_estimate_normals((1.0, 1.0, 1.0), R.NormalParams.make(12, 0.2))
    nrm, _ = ctx.map_normals()
    st = ctx.map_sac_planes(prm, use_normals=True)
    labels, info = ctx.map_plane_labels(), ctx.map_planes()
    l2, i2, s2 = ctx.sac_planes(xyz, prm, nrm)
    assert _bits(labels) == _bits(l2) and _bits(info) == _bits(i2) and _fields(st) == _fields(s2)
    assert _bits(ctx.map_normals()[0]) == _bits(nrm)         # and the normals are still valid


def test_map_filter_planes_keep_and_drop_partition_the_map(ctx):
    prm = _prm(**MAP)
    halves = []
    for keep in (False, True):
        xyz, rgba = _fill_map(ctx)
        ctx.map_estimate_normals((1.0, 1.0, 1.0), R.NormalParams.make(12, 0.2))
        ctx.map_cluster(R.ClusterParams.make(0.1, 20))
        ctx.map_sac_planes(prm)
        on = ctx.map_plane_labels() >= 0
        assert 0 < on.sum() < len(xyz)
        st = ctx.map_filter_planes(prm, keep_planes=keep)
        assert (st.n_in, st.n_in_planes) == (len(xyz), int(on.sum()))
        x2, c2 = ctx.map_download()
        want = on if keep else ~on
        assert _bits(x2) == _bits(xyz[want]) and _bits(c2) == _bits(rgba[want])     # order and bits kept
        for what, fn in (("no valid normals", ctx.map_normals), ("no valid labels", ctx.map_labels),
                         ("no valid plane labels", ctx.map_plane_labels)):
            with pytest.raises(RuntimeError, match=what):
                fn()
        halves.append(want)
    assert (halves[0] ^ halves[1]).all()                     # the two results partition the map


def test_empty_map(ctx):
    ctx.map_reset()
    prm = _prm(**MAP)
    for st in (ctx.map_sac_planes(prm), ctx.map_filter_planes(prm), ctx.map_filter_planes(prm, keep_planes=True)):
        assert _fields(st) == [0] * 5
    ctx.map_sac_planes(prm)
    assert len(ctx.map_plane_labels()) == 0 and len(ctx.map_planes()) == 0 and ctx.map_size() == 0
