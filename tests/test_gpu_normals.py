"""Surface normals on the GPU (r360_cloud_normals, r360_ctx_map_estimate_normals, r360_cloud_normals_eval) against the
brute-force numpy statement tests/normal_model.py.

Bounds, derived and not measured:
  * count, the dropped and the short rows: exact on every point.  The squared distances are the same float64 operations
    on both sides and the order (squared distance, input index) is total.
  * knn: exact on the model's knn_decided points (every point of the exact lattices: an exact tie is decided by the
    index rule).
  * On the model's eig_decided points ((l1 - l0) >= 1e-5 l2, the flip decided): both sides add the same moments in the
    same order, so they solve the same matrix C.  A float64 symmetric eigen-solver returns eigenvalues within a few
    ulps of |C| = l2: 1e-12 l2 leaves four digits.  An eigenvector is off by about 1e-14 l2 / (l1 - l0) <= 1e-9
    (the GICP test's argument): 1e-8 per component.  curvature = |l0| / trace <= 1/3 inherits the eigenvalues' error
    over the trace >= l2: 1e-12.
  * float32 outputs: within 2^-22 of the model's float64 values (components are at most 1: half a float32 ulp, 2^-25,
    plus the bound above); NaN exactly where the model has no normal.
  * At most 1 % of a case's points with a normal may be undecided; every case asserts that first, on the model alone
    (the seeds were chosen on the CPU so that it holds)."""
import ctypes as C
import functools

import numpy as np
import pytest

import normal_model as NM
import rgbd360_amd as R

pytestmark = pytest.mark.gpu

ORIGIN = ((0.0, 0.0, 0.0),)


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _model(name, k, radius, views=ORIGIN):
    """The model of a case, computed once however many tests read it."""
    return NM.estimate(CLOUDS[name](), k, radius, np.float32(views))


def _check(ctx, xyz, k, radius, views, m, knn_everywhere=False):
    """Hook and product parity of one case against its model m; returns (knn, count, normals32, curvature32, stats)."""
    views = np.float32(views).reshape(-1, 3)
    n = len(xyz)
    assert m.undecided_fraction() <= 0.01, ("too many undecided points: choose another seed", m.undecided_fraction())
    prm = R.NormalParams.make(k, radius)
    knn, count, nrm, eig, curv = ctx.normals_eval(xyz, views, prm)
    assert np.array_equal(count, m.count), np.flatnonzero(count != m.count)[:10]
    none = m.count < 3                                           # dropped or short
    assert np.isnan(nrm[none]).all() and np.isnan(eig[none]).all() and np.isnan(curv[none]).all()
    assert np.isfinite(nrm[~none]).all() and np.isfinite(eig[~none]).all() and np.isfinite(curv[~none]).all()
    sel = np.ones(n, bool) if knn_everywhere else m.knn_decided
    assert np.array_equal(knn[sel], m.knn[sel]), np.flatnonzero((knn != m.knn).any(1) & sel)[:10]
    assert (knn[m.count < 0] == -1).all()
    d = m.eig_decided
    l2 = m.eig[d, 2:3]
    e_eig = np.abs(eig[d] - m.eig[d]) / l2 if d.any() else np.zeros((0, 3))
    e_nrm = np.abs(nrm[d] - m.normal[d])
    e_curv = np.abs(curv[d] - m.curvature[d])
    gn, gc, st = ctx.estimate_normals(xyz, views, prm)
    e32 = max(np.abs(gn[d] - m.normal[d]).max(initial=0.0), np.abs(gc[d] - m.curvature[d]).max(initial=0.0))
    print(f"n={n} k={k} r={radius}: {int(d.sum())} decided of {int((~none).sum())}, {int(m.short.sum())} short; "
          f"eig {e_eig.max(initial=0.0):.2e} l2, normal {e_nrm.max(initial=0.0):.2e}, curvature {e_curv.max(initial=0.0):.2e}, "
          f"float32 {e32:.2e}")
    assert (e_eig <= 1e-12).all() and (e_nrm <= 1e-8).all() and (e_curv <= 1e-12).all()
    assert e32 <= 2.0 ** -22
    assert np.array_equal(np.isnan(gn).any(1), none) and np.array_equal(np.isnan(gc), none)
    assert np.isnan(gn[none]).all()
    # the float32 outputs are the float32 of the hook's float64 values
    assert _bits(gn[~none]) == _bits(nrm[~none].astype(np.float32)) and _bits(gc[~none]) == _bits(curv[~none].astype(np.float32))
    assert (st.n_in, st.n_finite, st.n_short) == (n, int(m.finite.sum()), int(m.short.sum()))
    assert st.sum_neighbors == int(m.count[m.count > 0].sum())
    return knn, count, gn, gc, st


def _case(ctx, name, k, radius, views=ORIGIN, **kw):
    return _check(ctx, CLOUDS[name](), k, radius, views, _model(name, k, radius, views), **kw)


# ------------------------------------------------------------------ clouds
@functools.lru_cache(maxsize=None)
def box_cloud():
    """257 random points in a 1 m box; the sizes take its prefixes."""
    return np.random.default_rng(12).uniform(0, 1, (257, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def big_cloud():
    return np.random.default_rng(5).uniform(0, 1, (2000, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def plane_lattice(side=13, e=2.0 ** -4):
    """side x side points in z = 0, spacing e, centred on x = 0: coordinates and squared distances are exact."""
    g = np.arange(side) - side // 2
    i, j = np.meshgrid(g, g, indexing="ij")
    return (np.stack([i.ravel(), j.ravel(), np.zeros(side * side)], 1) * e).astype(np.float32)


@functools.lru_cache(maxsize=None)
def two_walls(per=700, seed=8):
    """z = 0 and z = 0.1, 0.5 m x 0.5 m each, 1 mm of noise; shuffled."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 0.5, (2 * per, 3))
    p[:, 2] = rng.normal(0, 0.001, 2 * per)
    p[per:, 2] += 0.1
    upper = np.arange(2 * per) >= per
    o = rng.permutation(2 * per)
    return p[o].astype(np.float32), upper[o]


@functools.lru_cache(maxsize=None)
def surface_cloud(n=1000, seed=11):
    """A bumpy sheet z = 0.1 sin(3x) cos(2y) over 1 m x 1 m with 2 mm of noise."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, (n, 3))
    p[:, 2] = 0.1 * np.sin(3 * p[:, 0]) * np.cos(2 * p[:, 1]) + rng.normal(0, 0.002, n)
    return p.astype(np.float32)


@functools.lru_cache(maxsize=None)
def non_finite_cloud():
    p = box_cloud().copy()
    bad = np.arange(3, len(p), 7)
    p[bad[0::3], 0] = np.nan
    p[bad[1::3], 1] = np.inf
    p[bad[2::3], 2] = -np.inf
    return p


CLOUDS = {
    "box": box_cloud, "big": big_cloud, "lattice": plane_lattice, "walls": lambda: two_walls()[0], "surface": surface_cloud,
    "shifted": lambda: (surface_cloud() + np.float32(1000.0)).astype(np.float32),
    "clusters": lambda: np.vstack([surface_cloud(500, 13), surface_cloud(500, 14) + np.float32([1000.0, -20.0, 3.0])]).astype(np.float32),
    "non_finite": non_finite_cloud,
}
for _n in (2, 3, 63, 64, 65, 257):
    CLOUDS[f"box{_n}"] = functools.partial(lambda q: box_cloud()[:q], _n)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("k", [3, 20, 64])
def test_sizes(ctx, k):
    views = ((0.5, 0.5, 3.0),)
    for n in (2, 3, 63, 64, 65, 257):
        knn, count, gn, gc, st = _case(ctx, f"box{n}", k, 2.0, views)      # beyond the box's diameter: setKSearch(k)
        if n == 2:
            assert (count == 2).all() and st.n_short == 2 and np.isnan(gn).all()
        if n == 3:
            assert (count == 3).all() and st.n_short == 0
    # nothing at all
    gn, gc, st = ctx.estimate_normals(np.zeros((0, 3), np.float32), views, R.NormalParams.make(k, 0.5))
    assert gn.shape == (0, 3) and gc.shape == (0,) and (st.n_in, st.n_finite, st.n_short, st.sum_neighbors) == (0, 0, 0, 0)
    assert all(len(a) == 0 for a in ctx.normals_eval(np.zeros((0, 3), np.float32), views, R.NormalParams.make(k, 0.5)))


def test_two_thousand_points_and_the_cap_at_64(ctx):
    _case(ctx, "big", 20, 0.25)
    # about 130 points lie within 0.25 m of a point inside the box: k = 64 cuts most neighbourhoods, the radius the
    # ones near the box's corners and edges
    m = _model("big", 64, 0.25)
    assert (m.count == 64).mean() > 0.8 and (m.count < 64).sum() > 100
    _case(ctx, "big", 64, 0.25)


def test_exact_lattice_ties_by_index(ctx):
    """Every distance is exact and ties massively: knn must equal the model's on every point."""
    views = ((0.1, 0.2, 2.0),)
    for k, r in ((5, 1.0), (9, 1.0), (20, 1.0), (64, 1.0), (64, 0.25), (7, 2.0 ** -4)):
        knn, count, gn, gc, _ = _case(ctx, "lattice", k, r, views, knn_everywhere=True)
        assert np.array_equal(gn, np.tile(np.float32([0, 0, 1]), (169, 1))) and not gc.any()
    m = _model("lattice", 64, 0.25, views)
    assert m.count.max() == 49 and m.count[84] == 49            # the centre: 48 others within exactly four spacings (closed)
    m = _model("lattice", 7, 2.0 ** -4, views)
    assert m.count[84] == 5 and m.count[0] == 3


def test_parallel_walls_do_not_bridge(ctx):
    xyz, upper = two_walls()
    above = ((0.25, 0.25, 5.0),)
    m = _model("walls", 20, 0.04, above)
    has = m.knn >= 0
    assert (upper[np.maximum(m.knn, 0)] == upper[:, None])[has].all()     # the model's neighbourhoods stay on their wall
    knn, *_ = _case(ctx, "walls", 20, 0.04, above)
    assert (upper[np.maximum(knn, 0)] == upper[:, None])[knn >= 0].all()
    assert (m.normal[m.valid, 2] > 0.9).all()                 # both walls face the viewpoint above them


def test_shifted_by_a_kilometre(ctx):
    """The same sheet at +1000 m on every axis (float32 spacing 6e-5 m): the moments are centred, so the bounds hold."""
    _case(ctx, "surface", 20, 0.25, ((0.5, 0.5, 2.0),))
    _case(ctx, "shifted", 20, 0.25, ((1000.5, 1000.5, 1002.0),))


def test_two_clusters_a_kilometre_apart(ctx):
    views = ((0.5, 0.5, 2.0), (1000.5, -19.5, 5.0))
    knn, *_ = _case(ctx, "clusters", 20, 0.25, views)
    first = np.arange(1000) < 500
    assert ((knn < 500) == first[:, None])[knn >= 0].all()
    m = _model("clusters", 20, 0.25, views)
    assert (m.view[m.valid & first] == 0).all() and (m.view[m.valid & ~first] == 1).all()


def test_non_finite_rows(ctx):
    p = non_finite_cloud()
    bad = ~np.isfinite(p).all(1)
    assert bad.sum() == 37
    knn, count, gn, gc, st = _case(ctx, "non_finite", 20, 0.5)
    assert (count[bad] == -1).all() and not np.isin(knn, np.flatnonzero(bad)).any()
    nothing = np.full((5, 3), np.nan, np.float32)
    gn, gc, st = ctx.estimate_normals(nothing, ORIGIN, R.NormalParams.make(20, 0.5))
    assert np.isnan(gn).all() and np.isnan(gc).all() and (st.n_in, st.n_finite, st.n_short, st.sum_neighbors) == (5, 0, 0, 0)
    assert (ctx.normals_eval(nothing, ORIGIN, R.NormalParams.make(20, 0.5))[1] == -1).all()


def test_small_radius_leaves_short_points(ctx):
    m = _model("box", 20, 0.08)
    assert 0.2 < m.short.mean() < 0.9 and m.valid.sum() > 20
    _case(ctx, "box", 20, 0.08)
    # far beyond the cloud's diameter: setKSearch
    m = _model("box", 20, 100.0)
    assert (m.count == 20).all()
    _case(ctx, "box", 20, 100.0)


def test_nearest_of_two_viewpoints(ctx):
    """The plane z = 0 with v0 = (-1, 0, 1) and v1 = (1, 0, -1): x < 0 looks up, x > 0 down, x = 0 ties to v0: up."""
    p = plane_lattice()
    views = ((-1.0, 0.0, 1.0), (1.0, 0.0, -1.0))
    _, _, gn, gc, _ = _case(ctx, "lattice", 9, 1.0, views, knn_everywhere=True)
    x = p[:, 0]
    assert (x == 0).sum() == 13
    assert np.array_equal(gn[x <= 0], np.tile(np.float32([0, 0, 1]), (int((x <= 0).sum()), 1)))
    assert np.array_equal(gn[x > 0], np.tile(np.float32([0, 0, -1]), (int((x > 0).sum()), 1)))
    # 4096 viewpoints, the last one the nearest
    many = np.zeros((4096, 3), np.float32)
    many[:, 2] = -5.0 - np.arange(4096)[::-1]
    gn, _, _ = ctx.estimate_normals(p, many, R.NormalParams.make(9, 1.0))
    assert np.array_equal(gn, np.tile(np.float32([0, 0, -1]), (169, 1)))


def test_deterministic_and_order_independent(ctx):
    prm = R.NormalParams.make(20, 0.25)
    xyz = surface_cloud()
    views = np.float32([[0.5, 0.5, 2.0], [0.2, 0.1, 1.0]])
    a, b = ctx.estimate_normals(xyz, views, prm), ctx.estimate_normals(xyz, views, prm)
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and bytes(a[2]) == bytes(b[2])
    ea, eb = ctx.normals_eval(xyz, views, prm), ctx.normals_eval(xyz, views, prm)
    assert all(_bits(u) == _bits(v) for u, v in zip(ea, eb))
    # no two of the cloud's distances tie, so a neighbourhood's order does not depend on the input indices
    q = xyz[:600]
    d2 = np.stack([NM.sq_dists(q, i) for i in range(len(q))])
    iu = np.triu_indices(len(q), 1)
    assert len(np.unique(d2[iu])) == len(iu[0])
    p = np.random.default_rng(2).permutation(len(q))
    gn, gc, _ = ctx.estimate_normals(q, views, prm)
    pn, pc, _ = ctx.estimate_normals(q[p], views, prm)
    assert _bits(pn) == _bits(gn[p]) and _bits(pc) == _bits(gc[p])
    kn = ctx.normals_eval(q, views, prm)
    kp = ctx.normals_eval(q[p], views, prm)
    assert all(_bits(kp[i]) == _bits(kn[i][p]) for i in (1, 2, 3, 4))
    assert np.array_equal(np.where(kp[0] >= 0, p[np.maximum(kp[0], 0)], -1), kn[0][p])


def test_context_map():
    leaf = 0.05
    ctx, ctx2 = R.Context(0), R.Context(0)
    try:
        views = np.float32([[0.5, 0.5, 2.0], [0.5, 0.5, -2.0]])
        prm = R.NormalParams.make(12, 0.2)
        # an empty map: zero stats, and nothing to download
        st = ctx.map_estimate_normals(views, prm)
        assert (st.n_in, st.n_finite, st.n_short, st.sum_neighbors) == (0, 0, 0, 0)
        gn, gc = ctx.map_normals()
        assert gn.shape == (0, 3) and gc.shape == (0,)
        crafted = surface_cloud(3000, 21)                       # several points per 5 cm voxel: the map holds their means
        assert ctx.map_add_cloud(crafted, None, leaf)
        with pytest.raises(RuntimeError, match="no valid normals"):
            ctx.map_normals()
        st = ctx.map_estimate_normals(views, prm)
        mx, _ = ctx.map_download()
        assert 300 < len(mx) < len(crafted) and st.n_in == len(mx) == ctx.map_size()
        gn, gc = ctx.map_normals()
        wn, wc, wst = ctx2.estimate_normals(mx, views, prm)
        assert _bits(gn) == _bits(wn) and _bits(gc) == _bits(wc) and bytes(st) == bytes(wst)
        m = NM.estimate(mx, 12, 0.2, views)
        _check(ctx2, mx, 12, 0.2, views, m)
        # a cloud call on the map's context leaves the map's normals alone
        ctx.estimate_normals(crafted[:100], views, R.NormalParams.make(5, 0.5))
        an, ac = ctx.map_normals()
        assert _bits(an) == _bits(gn) and _bits(ac) == _bits(gc)
        # invalid parameters: an error, and map and normals as they were
        with pytest.raises(RuntimeError):
            ctx.map_estimate_normals(views, R.NormalParams.make(2, 0.2))
        with pytest.raises(RuntimeError):
            ctx.map_estimate_normals(np.zeros((0, 3), np.float32), prm)
        an, ac = ctx.map_normals()
        assert _bits(an) == _bits(gn) and ctx.map_size() == len(mx)
        # a short capacity: an error that still reports the size
        n = C.c_size_t()
        few = np.zeros((4, 3), np.float32)
        assert R.lib().r360_ctx_map_download_normals(ctx.h, R._fptr(few), None, 4, C.byref(n)) < 0
        assert n.value == len(mx) and b"capacity" in R.lib().r360_last_error() and not few.any()
        # whatever changes the map drops the normals
        assert ctx.map_add_cloud(surface_cloud(50, 22), None, leaf)
        with pytest.raises(RuntimeError, match="no valid normals"):
            ctx.map_normals()
        ctx.map_estimate_normals(views, prm)
        assert len(ctx.map_normals()[0]) == ctx.map_size()
        ctx.map_filter_outliers(R.OutlierParams.radius_filter(0.15, 5))
        with pytest.raises(RuntimeError, match="no valid normals"):
            ctx.map_normals()
        ctx.map_estimate_normals(views, prm)
        assert len(ctx.map_normals()[0]) == ctx.map_size()
        ctx.map_reset()
        with pytest.raises(RuntimeError, match="no valid normals"):
            ctx.map_normals()
    finally:
        ctx.close()
        ctx2.close()
