"""tests/normal_model.py against closed forms, and the normal estimation's C-ABI checks that need no GPU
(include/rgbd360_hip.h, "surface normals and curvature"): the documented defaults and every R360_EINVAL case, which
return before anything touches a device."""
import ctypes as C
import subprocess

import numpy as np

import normal_model as NM
import rgbd360_amd as R

EINVAL = -2


def plane_lattice(side=5, e=2.0 ** -4):
    """side x side points in z = 0 with spacing e, row-major in (x, y): every coordinate and every squared distance
    is exact in float32 and float64."""
    g = np.arange(side)
    i, j = np.meshgrid(g, g, indexing="ij")
    return (np.stack([i.ravel(), j.ravel(), np.zeros(side * side)], 1) * e).astype(np.float32)


# ------------------------------------------------------------------ the model, by hand
def test_plane_lattice_is_exact():
    p = plane_lattice()
    for k, r in ((5, 1.0), (9, 1.0), (25, 1.0), (64, 0.07), (64, 0.1)):
        for view, sign in (((0.1, 0.1, 1.0), 1.0), ((0.1, 0.1, -3.0), -1.0)):
            m = NM.estimate(p, k, r, [view])
            assert m.valid.all() and m.eig_decided.all()
            assert np.array_equal(m.normal, np.tile([0.0, 0.0, sign], (25, 1)))
            assert np.array_equal(m.curvature, np.zeros(25)) and np.array_equal(m.eig[:, 0], np.zeros(25))
            assert np.array_equal(m.normal32, np.tile(np.float32([0, 0, sign]), (25, 1)))


def test_lattice_ties_go_to_the_lower_index():
    """Point 12 is the centre (2, 2): its four axis neighbours 7, 11, 13, 17 tie at e^2, its diagonal ones 6, 8, 16, 18
    at 2 e^2, then 2, 10, 14, 22 at 4 e^2.  Point 0 is the corner: 1 and 5 tie, then 6, then 2 and 10."""
    p = plane_lattice()
    m = NM.estimate(p, 9, 1.0, [[0, 0, 1]])
    assert m.knn[12].tolist() == [12, 7, 11, 13, 17, 6, 8, 16, 18]
    assert m.knn[0].tolist() == [0, 1, 5, 6, 2, 10, 7, 11, 12]
    assert m.knn_decided.all() and (m.count == 9).all()
    m = NM.estimate(p, 4, 1.0, [[0, 0, 1]])                    # the cut falls inside a tie: 7, 11, 13 of 7, 11, 13, 17
    assert m.knn[12].tolist() == [12, 7, 11, 13] and m.knn_decided[12]
    # the radius is closed: exactly e reaches the axis neighbours and nothing else
    m = NM.estimate(p, 64, 2.0 ** -4, [[0, 0, 1]])
    assert m.knn[12, :6].tolist() == [12, 7, 11, 13, 17, -1] and m.count[12] == 5
    assert m.count[0] == 3 and m.knn[0, :4].tolist() == [0, 1, 5, -1]
    m = NM.estimate(p, 64, 0.99 * 2.0 ** -4, [[0, 0, 1]])
    assert (m.count == 1).all() and m.short.all() and np.isnan(m.normal).all() and np.isnan(m.curvature).all()


def test_sphere_shell_points_inwards_to_a_centre_viewpoint():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(600, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    m = NM.estimate(p, 12, 0.5, [[0, 0, 0]])
    assert m.valid.all()
    dots = (m.normal * p.astype(np.float64)).sum(1)
    assert (dots < 0).all() and (dots < -0.95).mean() > 0.95     # towards the centre, and nearly radial
    out = NM.estimate(p, 12, 0.5, [[0, 0, 0], [0, 0, 50], [0, 0, -50]])
    assert (out.view == 0).all() and np.array_equal(out.normal, m.normal)
    far = NM.estimate(p, 12, 0.5, [[0, 0, 50]])                  # one far viewpoint: the upper cap looks outwards
    top = p[:, 2] > 0.5
    assert ((far.normal * p).sum(1)[top] > 0).all()
    assert (m.curvature > 0).all() and (m.curvature < 0.05).all()


def test_three_points_give_the_triangles_normal():
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]])
    m = NM.estimate(tri, 3, 10.0, [[0, 0, 10]])
    want = np.cross(tri[1] - tri[0], tri[2] - tri[0]).astype(np.float64)
    want /= np.linalg.norm(want)
    assert (m.count == 3).all() and np.abs(m.normal - want).max() < 1e-15
    assert np.abs(m.eig[:, 0]).max() < 1e-16 and np.abs(m.curvature).max() < 1e-15
    assert m.knn.tolist() == [[0, 1, 2], [1, 0, 2], [2, 0, 1]]
    # k = 3 of more points, a dropped row between them, and a point that is short
    more = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, 1, 0.5], [40, 40, 40]])
    m = NM.estimate(more, 3, 10.0, [[0, 0, 10]])
    assert m.count.tolist() == [3, -1, 3, 3, 1] and m.short.tolist() == [False, False, False, False, True]
    assert np.abs(m.normal[[0, 2, 3]] - want).max() < 1e-15 and np.isnan(m.normal[[1, 4]]).all()
    assert m.knn[0].tolist() == [0, 2, 3] and m.knn[1].tolist() == [-1, -1, -1] and m.knn[4].tolist() == [4, -1, -1]


def test_two_viewpoints_split_a_plane():
    p = plane_lattice(5) - np.float32([2 * 2.0 ** -4, 0, 0])     # x in {-2, -1, 0, 1, 2} e
    m = NM.estimate(p, 9, 1.0, [[-1, 0, 1], [1, 0, -1]])
    x = p[:, 0]
    assert (m.view[x <= 0] == 0).all() and (m.view[x > 0] == 1).all()          # x = 0 ties: the lower index
    assert (m.normal[x <= 0, 2] == 1.0).all() and (m.normal[x > 0, 2] == -1.0).all()


# ------------------------------------------------------------------ the C ABI without a device
def test_defaults():
    p = R.NormalParams.default()
    assert (p.k, p.radius) == (20, 0.25)
    q = R.NormalParams.make(7, 0.5)
    assert (q.k, q.radius) == (7, 0.5)
    R.lib().r360_normal_default_params(None)                    # tolerated


def _calls(L, ctx, prm, view, n_view, n=4):
    xyz = np.zeros((4, 3), np.float32)
    st = R.NormalStats()
    nrm, curv = np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    fx = R._fptr(xyz)
    return (L.r360_cloud_normals(ctx, fx, n, prm, view, n_view, R._fptr(nrm), R._fptr(curv), C.byref(st)),
            L.r360_ctx_map_estimate_normals(ctx, prm, view, n_view, C.byref(st)),
            L.r360_cloud_normals_eval(ctx, fx, n, prm, view, n_view, None, None, None, None, None))


def test_invalid_arguments_are_einval_without_a_device():
    """A null context, null parameters, null viewpoints and every parameter outside its domain return R360_EINVAL from
    the argument check, which runs before anything touches a device.  `fake` stands in for a context: the checks that
    fail here never read it."""
    L = R.lib()
    good = R.NormalParams.default()
    v = np.zeros((1, 3), np.float32)
    vp = R._fptr(v)
    bad3 = (EINVAL, EINVAL, EINVAL)
    assert _calls(L, None, C.byref(good), vp, 1) == bad3
    assert b"null ctx" in L.r360_last_error()
    buf = C.create_string_buffer(1 << 16)
    fake = C.c_void_p(C.addressof(buf))
    assert _calls(L, fake, None, vp, 1) == bad3
    assert b"null params" in L.r360_last_error()
    assert _calls(L, fake, C.byref(good), None, 1) == bad3
    assert b"viewpoints" in L.r360_last_error()
    for n_view in (0, -1, 4097):
        assert _calls(L, fake, C.byref(good), vp, n_view) == bad3, n_view
    for name, value in (("k", 2), ("k", 0), ("k", -5), ("k", 65), ("radius", 0.0), ("radius", -0.25),
                        ("radius", float("nan")), ("radius", float("inf"))):
        p = R.NormalParams.default()
        setattr(p, name, value)
        assert _calls(L, fake, C.byref(p), vp, 1) == bad3, (name, value)
    # more than 2^30 points: the two calls that take a cloud
    fx, big = R._fptr(np.zeros((4, 3), np.float32)), (1 << 30) + 1
    assert L.r360_cloud_normals(fake, fx, big, C.byref(good), vp, 1, None, None, None) == EINVAL
    assert L.r360_cloud_normals_eval(fake, fx, big, C.byref(good), vp, 1, None, None, None, None, None) == EINVAL
    n = C.c_size_t()
    assert L.r360_ctx_map_download_normals(None, None, None, 0, C.byref(n)) == EINVAL
    assert L.r360_ctx_map_download_normals(fake, None, None, 0, None) == EINVAL


def test_normals_call_sequence_compiles(root):
    """tests/dropin/normals_dropin.cpp: the PCL-shaped NormalEstimation calls through the façade, with g++ alone."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/normals_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
