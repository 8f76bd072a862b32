"""Euclidean cluster extraction on the GPU (r360_cloud_clusters, r360_cloud_clusters_eval, r360_ctx_map_cluster,
r360_ctx_map_filter_clusters) against the brute-force numpy statement tests/cluster_model.py.

Bounds, derived and not measured:
  * root, comp_size, labels, the stats and every record's size, root, min and max: exact on every point.  Both sides
    decide an edge with the same float64 operations on the same float32 inputs (the squared distance, and in the
    conditional form the dot product and the C library's cos), components do not depend on the order the edges are
    found in, sizes are integers and min / max are comparisons.
  * conditional form: the model reports the points that touch an edge whose dot product lies within 1e-12 of the
    threshold.  A case first asserts, on the model alone, that they are at most 1 % of the points (the seeds were chosen
    on the CPU so that there are none), then compares root and comp_size on the points whose whole component is decided,
    and labels and records when every point is.
  * centroid: both sides add the same N coordinates per axis in different fixed orders, so the two sums differ by at
    most B = (N - 1) 2^-53 sum |x| (the model's sum_bound); the division by N rounds once more:
    |centroid - model| <= B / N + 2^-52 |centroid|.
  * covariance: the six moments are again the same N terms in two orders: (N - 1) 2^-53 sum |term| (the model's
    cov_bound, over the largest of the six).  The terms themselves are formed from means that may differ in the last
    place; in exact arithmetic that moves C by the square of the difference only, but the subtraction and the product
    round differently: 8 more units of 2^-53 per term.  Per entry of C: E = cov_bound (N + 7) / ((N - 1) N).
  * eigen-solve, on the clusters the model marks eig_decided (l1 - l0 >= 1e-5 l2, the sign rule decided): the bounds
    tests/test_gpu_normals.py derives for one matrix solved twice, 1e-12 l2 on the eigenvalues, 1e-8 on the
    eigenvector's components and 1e-12 on the curvature, each widened by w = E / l2 for the two sides' matrices
    differing by E.  The record tests first assert that at most 1 % of their clusters are undecided.
  * a cluster of fewer than 3 members has NaN eig, normal and curvature, exactly."""
import math

import numpy as np
import pytest

import cluster_model as CM
import rgbd360_amd as R

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -3


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ------------------------------------------------------------------ clouds
def _box(n=300, seed=11, side=1.0):
    return np.random.default_rng(seed).uniform(0, side, (n, 3)).astype(np.float32)


def _chain(n=300, step=TOL):
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = np.arange(n, dtype=np.float32) * np.float32(step)
    return p


def _chain_tenths(n=300):
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = (np.arange(n) * 0.1).astype(np.float32)          # gaps of 0.1 rounded to float32: some above, some below
    return p


def _dense():
    rng = np.random.default_rng(2)
    same = np.tile(np.float32([[0.3, 0.3, 0.3]]), (200, 1))
    near = (np.float32([0.3, 0.3, 0.3]) + rng.uniform(0, 0.02, (50, 3))).astype(np.float32)
    far = np.float32([[5, 5, 5], [5.01, 5, 5]])
    return np.concatenate([same, near, far])[rng.permutation(252)]


def _face_pairs():
    """Pairs exactly TOL apart along each axis that straddle a face of the cells (edge TOL (1 + 2^-20)), far from
    each other, and pairs one float beyond."""
    rows = []
    for axis in range(3):
        for j in range(1, 13):
            a = np.zeros(3)
            a[(axis + 1) % 3] = 10.0 * j + 40.0 * axis
            a[axis] = TOL * j - TOL / 2
            b = a.copy()
            b[axis] += TOL
            rows += [a, b]
            c, d = a.copy(), b.copy()
            c[(axis + 2) % 3] = d[(axis + 2) % 3] = 7.0
            d[axis] = np.nextafter(np.float32(d[axis]), np.float32(np.inf))
            rows += [c, d]
    return np.float32(rows)


def _equal_sizes():
    """Components of sizes 3, 5, 3, 5, 3, 1, 8 in input order, then shuffled."""
    rows = []
    for c, s in enumerate([3, 5, 3, 5, 3, 1, 8]):
        rows += [[3.0 * c + 0.05 * k, 0.0, 0.0] for k in range(s)]
    p = np.float32(rows)
    return p[np.random.default_rng(4).permutation(len(p))]


def _with_nans(p, every=7):
    q = p.copy()
    q[::every, 1] = np.nan
    q[3::2 * every, 2] = np.inf
    return q


def _cube_faces():
    """Six 10 x 10 face lattices of the unit cube, inset by half a step so that neighbouring faces' border rows are
    sqrt(2) * 0.05 apart; the normals are the faces' axes, exactly."""
    u = (0.05 + 0.1 * np.arange(10)).astype(np.float32)
    g = np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)
    xyz, nrm = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.zeros((100, 3), np.float32)
            p[:, axis] = side
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = g[:, 0], g[:, 1]
            v = np.zeros((100, 3), np.float32)
            v[:, axis] = 1.0
            xyz.append(p)
            nrm.append(v)
    return np.concatenate(xyz), np.concatenate(nrm)


def _random_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _blobs(seed=23):
    """Five anisotropic blobs of different sizes, far apart: every cluster's eigenvalues are well separated."""
    rng = np.random.default_rng(seed)
    out = []
    for c, n in enumerate([700, 400, 400, 150, 40]):
        p = rng.uniform(-1, 1, (n, 3)) * [0.30, 0.12, 0.04]
        a = 0.4 * c
        rot = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        out.append(p @ rot.T + [2.0 * c, -1.0 * c, 0.5 * c])
    p = np.concatenate(out).astype(np.float32)
    return p[rng.permutation(len(p))]


# ------------------------------------------------------------------ the comparison
def _check_records(info, m, assert_decided=False):
    nc = m.n_clusters
    assert len(info) == nc
    assert np.array_equal(info["size"], m.size) and np.array_equal(info["root"], m.croot)
    assert _bits(info["min"]) == _bits(m.min) and _bits(info["max"]) == _bits(m.max)
    if nc == 0:
        return
    n = m.size.astype(np.float64)[:, None]
    e_c = np.abs(info["centroid"] - m.centroid)
    b_c = m.sum_bound / n + 2.0 ** -52 * np.abs(m.centroid)
    small = m.size < 3
    for f in ("eig", "normal"):
        assert np.isnan(info[f][small]).all() and np.isfinite(info[f][~small]).all()
    assert np.isnan(info["curvature"][small]).all() and np.isfinite(info["curvature"][~small]).all()
    d = m.eig_decided
    frac = float((~small & ~d).sum()) / max(int((~small).sum()), 1)
    if assert_decided:
        assert frac <= 0.01, ("too many eigen-undecided clusters: choose another seed", frac)
    nn = m.size[d].astype(np.float64)
    l2 = m.eig[d, 2]
    w = m.cov_bound[d] * (nn + 7) / ((nn - 1) * nn) / l2
    e_eig = np.abs(info["eig"][d] - m.eig[d]) / l2[:, None]
    e_nrm = np.abs(info["normal"][d] - m.normal[d])
    e_cur = np.abs(info["curvature"][d] - m.curvature[d])
    print(f"{nc} clusters, {int(d.sum())} eigen-decided: centroid {(e_c / np.maximum(b_c, 1e-300)).max():.2f} of its bound, "
          f"eig {e_eig.max(initial=0.0):.2e} l2, normal {e_nrm.max(initial=0.0):.2e}, curvature {e_cur.max(initial=0.0):.2e}, "
          f"w {w.max(initial=0.0):.2e}")
    assert (e_c <= b_c).all()
    assert (e_eig <= (1e-12 + w)[:, None]).all() and (e_nrm <= (1e-8 + w)[:, None]).all() and (e_cur <= 1e-12 + w).all()


def _check(ctx, xyz, tol, min_size=1, max_size=2 ** 30, normals=None, eps=None, assert_decided=False):
    """Hook and product parity of one case against its model; returns (model, labels, info, stats)."""
    n = len(xyz)
    kw = {} if normals is None else dict(normals=normals, eps_angle=eps)
    m = CM.extract(xyz, tol, min_size, max_size, **kw)
    assert m.undecided.sum() <= 0.01 * n, ("too many undecided points: choose another seed", int(m.undecided.sum()))
    prm = R.ClusterParams.make(tol, min_size, max_size, eps_angle=eps)
    labels, info, st, root, comp = ctx.clusters_eval(xyz, prm, normals)
    ok = m.component_decided()
    assert np.array_equal(root[ok], m.root[ok]), np.flatnonzero((root != m.root) & ok)[:10]
    assert np.array_equal(comp[ok], m.comp_size[ok]), np.flatnonzero((comp != m.comp_size) & ok)[:10]
    assert (st.n_in, st.n_finite) == (n, int(m.finite.sum()))
    if not m.undecided.any():
        assert np.array_equal(labels, m.labels), np.flatnonzero(labels != m.labels)[:10]
        assert (st.n_components, st.n_clusters, st.n_clustered) == (m.n_components, m.n_clusters, m.n_clustered)
        _check_records(info, m, assert_decided)
    # the product call: the same labels and records, byte for byte
    l2, i2, s2 = ctx.clusters(xyz, prm, normals)
    assert _bits(l2) == _bits(labels) and _bits(i2) == _bits(info)
    assert [getattr(s2, f) for f, _ in s2._fields_] == [getattr(st, f) for f, _ in st._fields_]
    return m, labels, info, st


# ------------------------------------------------------------------ sizes and edges
def test_one_point(ctx):
    m, labels, info, st = _check(ctx, np.float32([[0.5, -2.0, 3.0]]), 0.1)
    assert labels.tolist() == [0] and info["size"].tolist() == [1] and info["centroid"][0].tolist() == [0.5, -2.0, 3.0]
    m, labels, info, st = _check(ctx, np.float32([[0.5, -2.0, 3.0]]), 0.1, min_size=2)
    assert labels.tolist() == [-1] and len(info) == 0 and st.n_components == 1


def test_two_points_at_the_tolerance_and_one_float_beyond(ctx):
    at = np.float32([[0, 0, 0], [TOL, 0, 0]])
    m, labels, info, _ = _check(ctx, at, TOL)
    assert labels.tolist() == [0, 0] and info["size"].tolist() == [2]
    beyond = at.copy()
    beyond[1, 0] = np.nextafter(np.float32(TOL), np.float32(1))
    m, labels, info, _ = _check(ctx, beyond, TOL)
    assert labels.tolist() == [0, 1] and info["size"].tolist() == [1, 1]


@pytest.mark.parametrize("n", [63, 64, 65, 256, 257])
def test_wave_and_workgroup_edges(ctx, n):
    m, *_ = _check(ctx, _box(300)[:n], 0.12)
    assert m.n_clusters > 1


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_at_a_dyadic_tolerance(ctx, order):
    p = _chain()
    if order == "descending":
        p = p[::-1].copy()
    elif order == "shuffled":
        p = p[np.random.default_rng(8).permutation(len(p))]
    m, labels, info, st = _check(ctx, p, TOL)
    assert st.n_components == 1 and info["size"].tolist() == [300] and (labels == 0).all()


def test_chain_at_a_non_dyadic_tolerance(ctx):
    m, *_ = _check(ctx, _chain(), 0.1)                          # 2^-3 apart: nothing links
    assert m.n_clusters == 300
    m, *_ = _check(ctx, _chain_tenths(), 0.1)                   # float32(0.1 k): the model says which links hold
    assert 1 < m.n_clusters < 300


# ------------------------------------------------------------------ dense and far
def test_coincident_points_and_a_crowded_cell(ctx):
    m, labels, info, st = _check(ctx, _dense(), 0.05)
    assert info["size"].tolist() == [250, 2]


def test_translated_cloud(ctx):
    p = (_box(400, 12).astype(np.float64) + [-1000.0, 2000.0, 900.0]).astype(np.float32)
    m, *_ = _check(ctx, p, 0.12)
    assert m.n_clusters > 1


def test_pairs_across_a_cell_face(ctx):
    m, labels, info, st = _check(ctx, _face_pairs(), TOL)
    assert (info["size"] == 2).sum() == 36 and (info["size"] == 1).sum() == 72


# ------------------------------------------------------------------ size bounds and ordering
def test_equal_sizes_are_ordered_by_root(ctx):
    m, labels, info, st = _check(ctx, _equal_sizes(), 0.06)
    assert info["size"].tolist() == [8, 5, 5, 3, 3, 3, 1]
    assert (np.diff(info["root"][1:3]) > 0).all() and (np.diff(info["root"][3:6]) > 0).all()


def test_min_size_above_every_component(ctx):
    m, labels, info, st = _check(ctx, _equal_sizes(), 0.06, min_size=9)
    assert (labels == -1).all() and len(info) == 0 and (st.n_clusters, st.n_clustered, st.n_components) == (0, 0, 7)


def test_max_size_rejects_the_largest(ctx):
    m, labels, info, st = _check(ctx, _equal_sizes(), 0.06, min_size=3, max_size=5)
    assert info["size"].tolist() == [5, 5, 3, 3, 3] and st.n_clustered == 19


def test_all_nan_input(ctx):
    m, labels, info, st = _check(ctx, np.full((70, 3), np.nan, np.float32), 0.1)
    assert (labels == -1).all() and len(info) == 0 and (st.n_finite, st.n_components) == (0, 0)


def test_nan_rows_interleaved(ctx):
    m, labels, info, st = _check(ctx, _with_nans(_box(300, 13)), 0.12)
    assert (labels[~m.finite] == -1).all() and st.n_finite == int(m.finite.sum()) < 300


# ------------------------------------------------------------------ conditional form
def test_cube_faces_split_by_normals(ctx):
    xyz, nrm = _cube_faces()
    m, labels, info, st = _check(ctx, xyz, 0.11)
    assert info["size"].tolist() == [600]
    m, labels, info, st = _check(ctx, xyz, 0.11, normals=nrm, eps=0.1)
    assert info["size"].tolist() == [100] * 6 and info["root"].tolist() == [0, 100, 200, 300, 400, 500]


def test_random_normals(ctx):
    xyz = _box(1500, 14)
    m, *_ = _check(ctx, xyz, 0.1, normals=_random_normals(1500, 15), eps=1.0)
    assert not m.undecided.any() and 1 < m.n_clusters < 1500 and m.size[0] > 1


def test_nan_normals_are_singletons(ctx):
    xyz = _box(300, 16, side=0.5)
    nrm = np.tile(np.float32([[0, 0, 1]]), (300, 1))
    nrm[::5, 1] = np.nan
    nrm[2::25, 0] = np.inf
    m, labels, info, st = _check(ctx, xyz, 0.12, normals=nrm, eps=0.1)
    bad = ~np.isfinite(nrm).all(1)
    assert (m.comp_size[bad] == 1).all() and m.size[0] > 1


# ------------------------------------------------------------------ records
def test_records_of_anisotropic_blobs(ctx):
    m, labels, info, st = _check(ctx, _blobs(), 0.1, min_size=10, assert_decided=True)
    assert info["size"].tolist() == [700, 400, 400, 150, 40] and m.eig_decided.all()
    assert (info["normal"].max(1) == np.abs(info["normal"]).max(1)).all()     # the sign rule


def test_records_across_chunks_of_the_moment_sums(ctx):
    """One cluster of more members than a workgroup of the sums takes (4096), and a small one."""
    rng = np.random.default_rng(23)
    big = rng.uniform(-1, 1, (5000, 3)) * [0.20, 0.10, 0.03]
    small = rng.uniform(-1, 1, (300, 3)) * [0.03, 0.10, 0.05] + [3.0, 0.0, 0.0]
    p = np.concatenate([big, small]).astype(np.float32)[rng.permutation(5300)]
    prm = R.ClusterParams.make(0.1, 100)
    labels, info, st = ctx.clusters(p, prm)
    assert info["size"].tolist() == [5000, 300]
    # the model of the records alone: the components are known by construction
    want = (p[:, 0] > 1.5).astype(np.int32)
    assert np.array_equal(labels, want)
    for r in (0, 1):
        q = p[labels == r].astype(np.float64)
        nq = len(q)
        mean = q.sum(0) / nq
        b = (nq - 1) * 2.0 ** -53 * np.abs(q).sum(0) / nq + 2.0 ** -52 * np.abs(mean)
        assert (np.abs(info["centroid"][r] - mean) <= b).all()
        dq = q - mean
        lam = np.linalg.eigvalsh(dq.T @ dq / nq)
        e = (nq + 7) * 2.0 ** -53 * np.abs(dq[:, :, None] * dq[:, None, :]).sum(0).max() / nq
        assert (np.abs(info["eig"][r] - lam) <= 1e-12 * lam[2] + e).all()
        assert _bits(info["min"][r]) == _bits(p[labels == r].min(0)) and _bits(info["max"][r]) == _bits(p[labels == r].max(0))


# ------------------------------------------------------------------ determinism and permutation
def test_two_calls_give_the_same_bytes(ctx):
    p = _with_nans(_box(2000, 17))
    prm = R.ClusterParams.make(0.08, 2)
    a = ctx.clusters(p, prm)
    b = ctx.clusters(p, prm)
    assert a[2].n_clusters > 5
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])
    nrm = _random_normals(2000, 18)
    prm = R.ClusterParams.make(0.1, 2, eps_angle=1.2)
    a = ctx.clusters(p, prm, nrm)
    b = ctx.clusters(p, prm, nrm)
    assert a[2].n_clusters > 5 and _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])


def test_permuted_input_gives_the_same_partition(ctx):
    p = _box(1000, 19)
    prm = R.ClusterParams.make(0.07, 2)
    perm = np.random.default_rng(20).permutation(len(p))
    la, ia, _ = ctx.clusters(p, prm)
    lb, ib, _ = ctx.clusters(p[perm], prm)
    assert len(ia) > 5 and CM.partition(p, la) == CM.partition(p[perm], lb)
    assert np.array_equal(ia["size"], ib["size"])


# ------------------------------------------------------------------ the map
def _map_cloud():
    rng = np.random.default_rng(30)
    a = rng.uniform(0, 0.5, (1500, 3))
    b = rng.uniform(0, 0.5, (1200, 3)) + [2.0, 0.0, 0.0]
    c = rng.uniform(0, 0.1, (30, 3)) + [5.0, 1.0, 0.0]
    xyz = np.concatenate([a, b, c]).astype(np.float32)
    rgba = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    return xyz, rgba


MAP_PRM = dict(tolerance=0.1, min_size=20)


def _fill_map(ctx):
    ctx.map_reset()
    assert ctx.map_add_cloud(*_map_cloud(), leaf=0.05)
    return ctx.map_download()


def test_map_cluster_equals_the_cloud_call_on_the_downloaded_map(ctx):
    xyz, rgba = _fill_map(ctx)
    prm = R.ClusterParams.make(**MAP_PRM)
    st = ctx.map_cluster(prm)
    labels, info = ctx.map_labels(), ctx.map_clusters()
    l2, i2, s2 = ctx.clusters(xyz, prm)
    assert _bits(labels) == _bits(l2) and _bits(info) == _bits(i2)
    assert [getattr(st, f) for f, _ in st._fields_] == [getattr(s2, f) for f, _ in s2._fields_]
    assert _bits(ctx.map_labels()) == _bits(labels)              # still the map's after a cloud call
    m = CM.extract(xyz, **MAP_PRM)
    assert np.array_equal(labels, m.labels) and m.n_clusters == 2 and m.n_components == 3
    assert 0 < (labels == -1).sum() < 20 and (xyz[labels == -1, 0] > 4.5).all()   # the small far blob's voxels
    assert st.n_clusters == 2 and st.n_in == len(xyz)
    x2, c2 = ctx.map_download()
    assert _bits(x2) == _bits(xyz) and _bits(c2) == _bits(rgba)  # clustering leaves the map alone


def test_map_labels_are_invalidated_by_map_changes(ctx):
    prm = R.ClusterParams.make(**MAP_PRM)
    xyz, _ = _fill_map(ctx)
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_labels()
    ctx.map_cluster(prm)
    assert len(ctx.map_labels()) == len(xyz)
    ctx.map_add_cloud(np.float32([[9, 9, 9]]), None, leaf=0.05)
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_labels()
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_clusters()
    ctx.map_cluster(prm)
    ctx.map_labels()
    ctx.map_filter_outliers(R.OutlierParams.radius_filter(0.15, 2))
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_labels()
    ctx.map_cluster(prm)
    ctx.map_labels()
    ctx.map_reset()
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_labels()


def test_map_cluster_with_normals(ctx):
    xyz, _ = _fill_map(ctx)
    prm = R.ClusterParams.make(**MAP_PRM, eps_angle=0.8)
    with pytest.raises(RuntimeError, match="no valid normals"):
        ctx.map_cluster(prm, use_normals=True)
    with pytest.raises(RuntimeError, match="no valid normals"):
        ctx.map_filter_clusters(prm, use_normals=True)
    assert ctx.map_size() == len(xyz)                            # the failed calls left the map alone
    ctx.map_estimate_normals((0.0, 0.0, 5.0), R.NormalParams.make(12, 0.2))
    nrm, _ = ctx.map_normals()
    st = ctx.map_cluster(prm, use_normals=True)
    labels, info = ctx.map_labels(), ctx.map_clusters()
    l2, i2, s2 = ctx.clusters(xyz, prm, nrm)
    assert _bits(labels) == _bits(l2) and _bits(info) == _bits(i2) and st.n_clusters == s2.n_clusters
    plain = ctx.clusters(xyz, prm)[2]
    assert st.n_components > plain.n_components                  # the normals cut edges
    assert _bits(ctx.map_normals()[0]) == _bits(nrm)             # and are still valid


def test_map_filter_clusters_keeps_the_labelled_rows(ctx):
    xyz, rgba = _fill_map(ctx)
    prm = R.ClusterParams.make(**MAP_PRM)
    ctx.map_estimate_normals((0.0, 0.0, 5.0), R.NormalParams.make(12, 0.2))
    ctx.map_cluster(prm)
    labels = ctx.map_labels()
    keep = labels >= 0
    assert 0 < keep.sum() < len(xyz)
    st = ctx.map_filter_clusters(prm)
    assert (st.n_in, st.n_clusters, st.n_clustered) == (len(xyz), 2, int(keep.sum()))
    x2, c2 = ctx.map_download()
    assert _bits(x2) == _bits(xyz[keep]) and _bits(c2) == _bits(rgba[keep])
    with pytest.raises(RuntimeError, match="no valid normals"):
        ctx.map_normals()
    with pytest.raises(RuntimeError, match="no valid labels"):
        ctx.map_labels()
    # the filtered map goes on: it clusters into the same two pieces, every point kept
    st = ctx.map_cluster(prm)
    assert (st.n_clusters, st.n_clustered) == (2, int(keep.sum())) and (ctx.map_labels() >= 0).all()


def test_empty_map(ctx):
    ctx.map_reset()
    prm = R.ClusterParams.make(**MAP_PRM)
    for st in (ctx.map_cluster(prm), ctx.map_filter_clusters(prm)):
        assert [getattr(st, f) for f, _ in st._fields_] == [0] * 5
    ctx.map_cluster(prm)
    assert len(ctx.map_labels()) == 0 and len(ctx.map_clusters()) == 0 and ctx.map_size() == 0


def test_record_capacity_error_still_reports_the_count(ctx):
    import ctypes as C
    p = _equal_sizes()
    prm = R.ClusterParams.make(0.06, 1)
    nk, info = C.c_size_t(), np.zeros(2, R.CLUSTER_INFO_DTYPE)
    rc = R.lib().r360_cloud_clusters(ctx.h, p.ctypes.data_as(R._FP), None, len(p), C.byref(prm), None,
                                     C.c_void_p(info.ctypes.data), 2, C.byref(nk), None)
    assert rc < 0 and nk.value == 7
    rc = R.lib().r360_cloud_clusters(ctx.h, p.ctypes.data_as(R._FP), None, len(p), C.byref(prm), None, None, 0,
                                     C.byref(nk), None)
    assert rc == 0 and nk.value == 7
