"""tests/cluster_model.py, the statement of the Euclidean cluster extraction, against hand-counted answers (no GPU)."""
import math

import numpy as np

import cluster_model as CM

TOL = 2.0 ** -3


def _lattice(nx, ny, step, origin=(0.0, 0.0, 0.0), axes=(0, 1)):
    """nx x ny points `step` apart in the plane of `axes`, float32."""
    p = np.zeros((nx * ny, 3), np.float32)
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * np.float32(step)
    p[:, axes[0]], p[:, axes[1]] = g[:, 0], g[:, 1]
    return p + np.float32(origin)


def test_two_blobs_and_a_bridge_point():
    a = _lattice(3, 3, 0.1)                                   # 9 points around the origin
    b = _lattice(3, 3, 0.1, origin=(0.5, 0.0, 0.0))           # 9 points, 0.3 m from a's last column
    r = CM.extract(np.concatenate([a, b]), 0.11, 1, 100)
    assert r.n_clusters == 2 and r.n_components == 2 and r.size.tolist() == [9, 9] and r.croot.tolist() == [0, 9]
    assert r.labels.tolist() == [0] * 9 + [1] * 9
    bridge = np.float32([[0.3, 0.1, 0.0], [0.4, 0.1, 0.0]])    # 0.2 -> 0.3 -> 0.4 -> 0.5
    r = CM.extract(np.concatenate([a, b, bridge]), 0.11, 1, 100)
    assert r.n_clusters == 1 and r.size.tolist() == [20] and r.croot.tolist() == [0] and (r.labels == 0).all()
    assert (r.root == 0).all() and (r.comp_size == 20).all()
    assert r.clusters[0].tolist() == list(range(20))
    r = CM.extract(np.concatenate([a, b, bridge[:1]]), 0.11, 1, 100)   # half a bridge: it joins a only
    assert r.size.tolist() == [10, 9] and r.labels[18] == 0


def test_chain_at_exactly_the_tolerance_and_one_float_beyond():
    x = np.arange(10, dtype=np.float32) * np.float32(TOL)     # dyadic: every gap is exactly 2^-3
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    r = CM.extract(p, TOL, 1, 100)
    assert r.n_clusters == 1 and r.size.tolist() == [10]
    below = float(np.nextafter(np.float32(TOL), np.float32(0)))
    r = CM.extract(p, below, 1, 100)
    assert r.n_clusters == 10 and (r.size == 1).all() and r.croot.tolist() == list(range(10))
    q = p.copy()
    q[5:, 0] = np.nextafter(q[5, 0], np.float32(np.inf)) + (q[5:, 0] - q[5, 0])   # one gap one float wider
    assert float(q[5, 0]) - float(q[4, 0]) > TOL
    r = CM.extract(q, TOL, 1, 100)
    assert r.size.tolist() == [5, 5] and r.croot.tolist() == [0, 5]


def test_size_ties_are_ordered_by_root_and_sizes_descend():
    # components in input order: sizes 2, 3, 2, 3, 1, far apart
    sizes = [2, 3, 2, 3, 1]
    rows = []
    for c, s in enumerate(sizes):
        rows += [[10.0 * c + 0.05 * k, 0.0, 0.0] for k in range(s)]
    r = CM.extract(np.float32(rows), 0.06, 1, 100)
    assert r.size.tolist() == [3, 3, 2, 2, 1] and r.croot.tolist() == [2, 7, 0, 5, 10]
    assert r.labels.tolist() == [2, 2, 0, 0, 0, 3, 3, 1, 1, 1, 4]
    assert [c.tolist() for c in r.clusters] == [[2, 3, 4], [7, 8, 9], [0, 1], [5, 6], [10]]


def test_size_bounds_are_closed():
    rows = []
    for c, s in enumerate([4, 3, 2]):
        rows += [[10.0 * c + 0.05 * k, 0.0, 0.0] for k in range(s)]
    p = np.float32(rows)
    assert CM.extract(p, 0.06, 3, 4).size.tolist() == [4, 3]
    assert CM.extract(p, 0.06, 4, 4).size.tolist() == [4]
    assert CM.extract(p, 0.06, 2, 3).size.tolist() == [3, 2]
    r = CM.extract(p, 0.06, 5, 100)
    assert r.n_clusters == 0 and (r.labels == -1).all() and r.n_components == 3 and r.comp_size.tolist() == [4] * 4 + [3] * 3 + [2] * 2
    r = CM.extract(p, 0.06, 1, 3)
    assert r.labels.tolist() == [-1] * 4 + [0] * 3 + [1] * 2 and r.n_clustered == 5


def test_nan_rows_are_dropped():
    p = np.float32([[0, 0, 0], [np.nan, 0, 0], [0.05, 0, 0], [0, np.inf, 0], [0.1, 0, 0]])
    r = CM.extract(p, 0.06, 1, 100)
    assert r.labels.tolist() == [0, -1, 0, -1, 0] and r.root.tolist() == [0, -1, 0, -1, 0]
    assert r.comp_size.tolist() == [3, -1, 3, -1, 3] and r.finite.tolist() == [True, False, True, False, True]
    r = CM.extract(np.full((4, 3), np.nan, np.float32), 0.06, 1, 100)
    assert r.n_clusters == 0 and r.n_components == 0 and (r.labels == -1).all()


def test_partition_of_a_permuted_cloud_is_the_same_set_of_sets():
    rng = np.random.default_rng(5)
    p = rng.uniform(0, 1, (400, 3)).astype(np.float32)
    r = CM.extract(p, 0.08, 2, 1000)
    assert 2 <= r.n_clusters
    perm = rng.permutation(len(p))
    q = CM.extract(p[perm], 0.08, 2, 1000)
    assert CM.partition(p, r.labels) == CM.partition(p[perm], q.labels)
    assert sorted(r.size.tolist()) == sorted(q.size.tolist())


def _two_walls():
    """A floor lattice (z = 0, normal +z) and a wall lattice (x = 0, normal +x) that touch along the y axis."""
    floor = _lattice(5, 5, 0.1, axes=(0, 1))
    wall = _lattice(5, 5, 0.1, origin=(0.0, 0.0, 0.1), axes=(2, 1))     # x = 0, z = 0.1 .. 0.5
    xyz = np.concatenate([floor, wall])
    nrm = np.zeros_like(xyz)
    nrm[:25, 2] = 1.0
    nrm[25:, 0] = 1.0
    return xyz, nrm


def test_perpendicular_lattices_split_only_with_normals():
    xyz, nrm = _two_walls()
    r = CM.extract(xyz, 0.11, 1, 100)
    assert r.n_clusters == 1 and r.size.tolist() == [50]
    r = CM.extract(xyz, 0.11, 1, 100, normals=nrm, eps_angle=0.1)
    assert r.n_clusters == 2 and r.size.tolist() == [25, 25] and r.croot.tolist() == [0, 25] and not r.undecided.any()
    # the records of the floor: a plane, so eig[0] = 0, the normal is +z and the curvature 0
    assert r.eig[0, 0] == 0.0 and np.allclose(r.normal[0], [0, 0, 1]) and r.curvature[0] == 0.0
    assert np.allclose(r.centroid[0], [0.2, 0.2, 0.0]) and r.min[0].tolist() == [0, 0, 0]
    assert np.allclose(r.max[0], [0.4, 0.4, 0.0])


def test_opposite_normals_do_not_connect():
    xyz = np.float32([[0, 0, 0], [0.05, 0, 0], [0.1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0, 0, -1], [0, 0, 1]])
    r = CM.extract(xyz, 0.06, 1, 100, normals=nrm, eps_angle=0.1)
    assert r.n_clusters == 3                                   # 0 - 2 are 0.1 apart: beyond the tolerance
    r = CM.extract(xyz, 0.11, 1, 100, normals=nrm, eps_angle=0.1)
    assert r.size.tolist() == [2, 1] and r.labels.tolist() == [0, 1, 0]
    wide = np.float32([[0, 0, 1], [0, math.sin(2.9), math.cos(2.9)], [0, 0, 1]])   # 2.9 rad apart: within 3.0
    r = CM.extract(xyz, 0.06, 1, 100, normals=wide, eps_angle=3.0)
    assert r.n_clusters == 1
    r = CM.extract(xyz, 0.06, 1, 100, normals=wide, eps_angle=2.8)
    assert r.n_clusters == 3


def test_nan_normal_is_a_singleton():
    xyz = np.float32([[0, 0, 0], [0.05, 0, 0], [0.1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0, np.nan, 1], [0, 0, 1]])
    r = CM.extract(xyz, 0.06, 1, 100, normals=nrm, eps_angle=0.1)
    assert r.n_clusters == 3 and r.labels.tolist() == [0, 1, 2] and (r.comp_size == 1).all()
    assert np.isnan(r.eig).all() and np.isnan(r.normal).all() and np.isnan(r.curvature).all()
    assert r.centroid[1].tolist() == [float(np.float32(0.05)), 0.0, 0.0]


def test_undecided_edges_are_reported():
    xyz = np.float32([[0, 0, 0], [0.05, 0, 0], [5, 0, 0]])
    eps = 0.3
    c = math.cos(float(np.float32(eps)))
    nrm = np.float32([[1, 0, 0], [c, math.sqrt(1 - c * c), 0], [1, 0, 0]])   # the dot product lands on the threshold
    dot = float(nrm[0, 0]) * float(nrm[1, 0])
    r = CM.extract(xyz, 0.06, 1, 100, normals=nrm, eps_angle=eps)
    assert r.undecided.tolist() == [abs(dot - c) <= CM.DOT_BAND] * 2 + [False]
    assert r.component_decided()[2]


def test_defaults():
    d = CM.DEFAULTS
    assert d["tolerance"] == 0.10 and d["min_size"] == 100 and d["max_size"] == 2 ** 30
    assert abs(d["eps_angle"] - math.radians(10)) == 0.0
