"""Generalized-ICP on the GPU beyond the one room of tests/test_gpu_gicp.py: the direct / grid switch, grids one cell
thick, an axis at the 1024-cell cap, a grid that is mostly empty, exact ties and duplicates, k at both ends of its
range, a gate below the cell edge, no gate, a gate met exactly, quarter and half turns, queries clamped beyond the
target's box, the grid-stride wrap of the pass and of the sum, the iteration limits, a zero residual and the argument
errors.  Inputs and rules: tests/_gicp_cases.py (their conditions are asserted on the CPU in tests/test_gicp_model.py);
reference: tests/gicp_model.py, and for gicp_epsilon = 1 a closed form written here with numpy alone.  The bars are
test_gpu_gicp.py's, through its _check_cloud and _check_eval: kNN and correspondences exact on decided points,
|C - C_model| <= 2^-22, cost within 1e-6 relative, H and g within 1e-5 of their maxima, pose within 1e-4 rad and 1e-3 m,
iterations and converged equal.

Measured on the MI355X (printed by the tests; none of these is a bar).  kNN lists equal on every decided point of every
cloud, on every point of both lattices and of the duplicates; every correspondence and every count equal to the
model's, the two undecided points of the last shift included.  Worst |C - C_model| 2.98e-8 (the float32 store), 0 on
the exact plane and the sheet.  Worst relative f / H / g against the model 1.37e-13 / 1.19e-13 / 1.97e-13 over the
poses, gates, k = 4 and 32 and the 70001-point source; against the closed form at gicp_epsilon = 1: 2.8e-16 / 1.1e-15
/ 4.7e-16 (the model's f against it: 9.6e-16).  Pose drift under the iteration limits at most 1.1e-9 rad, 2.9e-9 m,
iterations, inner steps and converged equal; the 70001-point alignment's fitness within 4.7e-9 relative of the model's
at the returned pose.  No defect found: the library is unchanged.  Wall time of this file: 2.2 s for its 37 tests,
the slowest (the 70001-point source: model, two evals, one alignment) 0.93 s.
"""
import ctypes as C
import re

import numpy as np
import pytest

import rgbd360_amd as R

import _gicp_cases as GC
import gicp_model as GM
from test_gpu_gicp import BAR_M, BAR_RAD, _align, _check_cloud, _check_eval, _full, _stats_tuple, lib_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def _rc(call, *a, **kw):
    """The status a Context call ends with: its own return where it succeeds, the code of the RuntimeError it raises."""
    try:
        call(*a, **kw)
        return 0
    except RuntimeError as e:
        m = re.search(r"failed \((-?\d+)\)", str(e))
        assert m, e
        return int(m.group(1))


# ---- the cloud stage --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GC.CLOUDS))
def test_cloud_stage_crafted(ctx, name):
    xyz, m = GC.cloud(name), GC.model_cloud(name)
    ctx.gicp_set_source(xyz)
    lattice = name.startswith("lattice")
    dec = (GC.knn_decided_ties(m), GC.cov_decided_ties(m))
    if name in GC.TIED:
        assert dec[0].all(), name           # every point's list is compared
    cov, knn = _check_cloud(ctx, 0, m, name, decided=dec, covariances=name != "lattice3d")
    if lattice:
        assert np.array_equal(knn, m.knn), name
    if name == "lattice_plane":
        eps = float(np.float32(1e-3))
        err = np.abs(_full(cov) - np.diag([1.0, 1.0, eps])).max()
        print(f"{name}: max |C - diag(1, 1, eps)| = {err:.3g}")
        assert err <= 2.0 ** -22
    if name == "dups":
        first = {}
        for i, r in enumerate(xyz):
            first.setdefault(r.tobytes(), i)
        lowest = np.array([first[r.tobytes()] for r in xyz])
        assert (lowest != np.arange(xyz.shape[0])).sum() == 100
        assert np.array_equal(knn[:, 0], lowest)


@pytest.mark.parametrize("k", GC.K_ENDS)
def test_cloud_stage_k_ends(ctx, k):
    prm = lib_params(GC.make_params(k=k))
    for n in (k, 600, 2000):
        ctx.gicp_set_target(GC.room(n, 31), prm)
        _check_cloud(ctx, 1, GC.model_room(n, 31, k), f"k={k} n={n}")


@pytest.mark.parametrize("k", GC.K_ENDS)
def test_eval_stage_k_ends(ctx, k):
    p = GC.make_params(k=k)
    s, t = GC.pair(*GC.K_PAIR)
    ctx.gicp_set_source(s, lib_params(p))
    ctx.gicp_set_target(t, lib_params(p))
    ms, mt = GC.model_pair_with(*GC.K_PAIR, k=k)
    _check_cloud(ctx, 0, ms, f"k={k} source")
    _check_cloud(ctx, 1, mt, f"k={k} target")
    _check_eval(ctx, ms, mt, np.eye(4), f"k={k} eval identity", p=p)
    _check_eval(ctx, ms, mt, GC.pose2(), f"k={k} eval pose 2", p=p)


@pytest.mark.parametrize("k", (GC.KMIN - 1, GC.KMAX + 1))
def test_k_out_of_range(ctx, k):
    prm = lib_params(GC.make_params(k=k))
    assert _rc(ctx.gicp_set_source, GC.room(600, 31), prm) == -2
    assert _rc(ctx.gicp_set_target, GC.room(600, 31), prm) == -2


# ---- the eval stage: turns, clamped queries, gates ------------------------------------------------------------------

@pytest.fixture(scope="module")
def eval_pair(ctx):
    def put():
        s, t = GC.pair(*GC.EVAL_PAIR)
        ctx.gicp_set_source(s)
        ctx.gicp_set_target(t)
        return GC.model_pair(*GC.EVAL_PAIR)
    return put


@pytest.mark.parametrize("gate", GC.GATES)
@pytest.mark.parametrize("pose", ("rz90", "rz180", "tx", "tyz"))
def test_eval_stage_poses_and_gates(ctx, eval_pair, pose, gate):
    ms, mt = eval_pair()
    X = GC.eval_poses()[pose]
    corr_only = pose in GC.EVAL_CORR_ONLY
    nc = _check_eval(ctx, ms, mt, X, f"eval {pose} gate {gate}", p=GC.make_params(gate=gate), sums_need_decided=corr_only)
    if gate == float("inf"):
        assert nc == ms.xyz.shape[0]


def test_gate_met_exactly_and_two_way_ties(ctx):
    s, t = GC.gate_lattice()
    ctx.gicp_set_source(s)
    ctx.gicp_set_target(t)
    corr, f, H, g, nc = ctx.gicp_eval(np.eye(4), lib_params(GC.make_params(gate=0.125)))
    print(f"gate 0.125: n_corr {nc}")
    assert nc == 0 and (corr == -1).all() and f == 0.0    # d^2 = 2^-6 = gate^2 exactly, and the gate is strict
    above = float(np.nextafter(np.float32(0.125), np.float32(1.0)))
    corr, f, H, g, nc = ctx.gicp_eval(np.eye(4), lib_params(GC.make_params(gate=above)))
    want = GC.gate_lattice_expected()
    print(f"gate {above!r}: n_corr {nc}, {(want != np.arange(648)).sum()} ties won by the other row")
    assert nc == 648 and np.array_equal(corr, want)


def _closed_form_eps1(s, t, corr, X):
    """f, g, H at X for C = I on both sides: M = (I + R R^T)^-1 for every pair, J = [I | -[p]x]."""
    R3, tr = X[:3, :3], X[:3, 3]
    M = np.linalg.inv(np.eye(3) + R3 @ R3.T)
    ok = corr >= 0
    p = s[ok].astype(np.float64) @ R3.T + tr
    r = p - t[corr[ok]].astype(np.float64)
    f, g, H = 0.0, np.zeros(6), np.zeros((6, 6))
    for pi, ri in zip(p, r):
        J = np.zeros((3, 6))
        J[:, :3] = np.eye(3)
        J[:, 3:] = -np.array([[0, -pi[2], pi[1]], [pi[2], 0, -pi[0]], [-pi[1], pi[0], 0]])
        f += ri @ M @ ri
        g += J.T @ M @ ri
        H += J.T @ M @ J
    return f, g, H


def test_epsilon_one_gives_the_closed_form(ctx):
    p = GC.make_params(eps=1.0)
    s, t = GC.pair(*GC.K_PAIR)
    ctx.gicp_set_source(s, lib_params(p))
    ctx.gicp_set_target(t, lib_params(p))
    for which in (0, 1):
        _, cov, _ = ctx.gicp_cloud(which)
        assert np.array_equal(_full(cov), np.broadcast_to(np.eye(3), (cov.shape[0], 3, 3)))
    X = GC.pose2().astype(np.float32).astype(np.float64)
    corr, f, H, g, nc = ctx.gicp_eval(X, lib_params(p))
    ms, mt = GC.model_pair_with(*GC.K_PAIR, eps=1.0)
    mcorr, mf, _, _, mn, d2, second = GM.eval_at(ms, mt, X, p)
    assert GC.corr_decided(d2, second, p.max_corr_dist).all()
    assert nc == mn and np.array_equal(corr, mcorr)
    cf, cg, cH = _closed_form_eps1(s, t, corr, X)
    ef, eg, eH = abs(f - cf) / cf, np.abs(g - cg).max() / np.abs(cg).max(), np.abs(H - cH).max() / np.abs(cH).max()
    print(f"eps = 1: n_corr {nc}, against the closed form cost rel {ef:.3g} H {eH:.3g} g {eg:.3g}; "
          f"model f against it {abs(mf - cf) / cf:.3g}")
    assert abs(mf - cf) <= 1e-6 * cf
    assert ef <= 1e-6 and eH <= 1e-5 and eg <= 1e-5


# ---- the wrap of the pass and of the sum ----------------------------------------------------------------------------

def test_wrap_of_the_pass_and_the_sum(ctx):
    ns, nt = GC.WRAP_PAIR
    s, t = GC.pair(ns, nt)
    assert s.shape[0] > GC.PASS_WRAP
    ctx.gicp_set_source(s)
    ctx.gicp_set_target(t)
    ms, mt = GC.model_pair(ns, nt)
    _check_cloud(ctx, 0, ms, f"source {ns}")
    _check_eval(ctx, ms, mt, np.eye(4), f"eval ({ns},{nt}) identity")
    _check_eval(ctx, ms, mt, GC.pose2(), f"eval ({ns},{nt}) pose 2")
    pose, st, rc = ctx.gicp_align(np.eye(4))
    mfit = GM.fitness(ms, mt, pose.astype(np.float64))
    eg = (GM.rot_angle(pose, GC.G()), float(np.linalg.norm(pose[:3, 3] - GC.G()[:3, 3])))
    print(f"align ({ns},{nt}): iterations {st.iterations} inner {st.inner_steps} converged {st.converged}; vs G "
          f"{eg[0]:.3g} rad {eg[1]:.3g} m; fitness {st.fitness:.9g} (model at this pose {mfit:.9g}, "
          f"rel {abs(st.fitness - mfit) / mfit:.3g})")
    assert rc == 0 and st.n_corr > GC.PASS_WRAP
    assert abs(st.fitness - mfit) <= 1e-6 * mfit


# ---- iteration limits and a zero residual --------------------------------------------------------------------------

@pytest.mark.parametrize("max_inner,max_it,want", [(0, 10, (1, True, 0)), (20, 1, (1, False, None)), (1, 3, (3, None, 3))])
def test_iteration_limits(ctx, eval_pair, max_inner, max_it, want):
    ms, mt = eval_pair()
    p = GC.make_params(max_it=max_it, max_inner=max_inner)
    init = np.eye(4, dtype=np.float32) if max_inner else GC.pose2().astype(np.float32)
    pose, st, rc = ctx.gicp_align(init, lib_params(p))
    ref = GM.align(ms, mt, init.astype(np.float64), p)
    dr = GM.rot_angle(pose, ref.pose)
    dt = float(np.linalg.norm(pose[:3, 3].astype(np.float64) - ref.pose[:3, 3]))
    print(f"limits inner {max_inner} outer {max_it}: iterations {st.iterations} (model {ref.iterations}) inner "
          f"{st.inner_steps} (model {ref.inner_steps}) converged {st.converged} (model {ref.converged}); drift "
          f"{dr:.3g} rad {dt:.3g} m")
    assert rc == 0 and ref.status == 0
    assert (st.iterations, bool(st.converged)) == (ref.iterations, ref.converged)
    assert st.iterations == want[0]
    assert want[1] is None or bool(st.converged) == want[1]
    assert want[2] is None or st.inner_steps == ref.inner_steps == want[2]
    assert dr <= BAR_RAD and dt <= BAR_M
    if max_inner == 0:
        assert pose.tobytes() == init.tobytes()


def test_identical_clouds_have_a_zero_residual(ctx):
    c = GC.room(700, 9)
    ctx.gicp_set_source(c)
    ctx.gicp_set_target(c)
    pose, st, rc = ctx.gicp_align(np.eye(4))
    print(f"identical clouds: status {rc} {_stats_tuple(st)}")
    assert rc == 0 and (st.iterations, bool(st.converged), st.inner_steps, st.n_corr) == (1, True, 0, 700)
    assert st.cost == 0.0 and st.fitness == 0.0
    assert pose.tobytes() == np.eye(4, dtype=np.float32).tobytes()
    m = GM.Cloud(c, GC.params32())
    ref = GM.align(m, m, np.eye(4), GC.params32())
    assert (ref.status, ref.iterations, ref.converged, ref.inner_steps, ref.cost, ref.fitness) == (0, 1, True, 0, 0.0, 0.0)


# ---- argument errors ----------------------------------------------------------------------------------------------

def _bad_params():
    d = {}
    for k in (GC.KMIN - 1, GC.KMAX + 1, 0, -1):
        d[f"k={k}"] = GC.make_params(k=k)
    for eps in (0.0, float("nan"), float("inf"), -1e-3):
        d[f"eps={eps}"] = GC.make_params(eps=eps)
    for gate in (0.0, -0.4, float("nan")):
        d[f"gate={gate}"] = GC.make_params(gate=gate)
    d["max_iterations=0"] = GC.make_params(max_it=0)
    d["max_inner_iterations=-1"] = GC.make_params(max_inner=-1)
    return d


def test_errors_leave_the_context_usable(ctx):
    fresh = R.Context(0)
    try:
        # nothing set yet
        assert _rc(fresh.gicp_align, np.eye(4)) == -2 and _rc(fresh.gicp_eval, np.eye(4)) == -2
        ref = _align(fresh, *GC.EVAL_PAIR, False)
    finally:
        fresh.close()
    s, t = GC.pair(*GC.EVAL_PAIR)
    ctx.gicp_set_source(s)
    ctx.gicp_set_target(t)
    good = ctx.gicp_eval(np.eye(4))
    for label, p in _bad_params().items():
        q = lib_params(p)
        codes = (_rc(ctx.gicp_set_source, s, q), _rc(ctx.gicp_set_target, t, q), _rc(ctx.gicp_eval, np.eye(4), q),
                 _rc(ctx.gicp_align, np.eye(4), q))
        print(label, codes)
        assert codes == (-2, -2, -2, -2), (label, codes)
    nan_pose = np.eye(4)
    nan_pose[1, 3] = np.nan
    inf_pose = np.eye(4)
    inf_pose[0, 0] = np.inf
    for X in (nan_pose, inf_pose):
        assert _rc(ctx.gicp_eval, X) == -2 and _rc(ctx.gicp_align, X) == -2
    # a refused call changed nothing: the clouds are still set and give the same bytes
    again = ctx.gicp_eval(np.eye(4))
    assert again[0].tobytes() == good[0].tobytes() and again[1] == good[1] and again[4] == good[4]
    assert again[2].tobytes() == good[2].tobytes() and again[3].tobytes() == good[3].tobytes()
    # capacity one short: -4, and the count is still reported
    n = C.c_size_t()
    xyz = np.zeros((s.shape[0], 3), np.float32)
    rc = R.lib().r360_gicp_get_cloud(ctx.h, 0, xyz.ctypes.data_as(C.POINTER(C.c_float)), None, None, s.shape[0] - 1, C.byref(n))
    assert rc == -4 and n.value == s.shape[0]
    rc = R.lib().r360_gicp_get_cloud(ctx.h, 2, None, None, None, 0, C.byref(n))
    assert rc == -2
    # too few finite rows: -3, the source is unset, and nothing reads its stale buffers
    few = GC.room(25, 1)
    few[:6, 1] = np.nan
    assert _rc(ctx.gicp_set_source, few) == -3
    rc = R.lib().r360_gicp_get_cloud(ctx.h, 0, None, None, None, 0, C.byref(n))
    assert rc == 0 and n.value == 0
    assert _rc(ctx.gicp_eval, np.eye(4)) == -2 and _rc(ctx.gicp_align, np.eye(4)) == -2
    rc = R.lib().r360_gicp_get_cloud(ctx.h, 1, None, None, None, 0, C.byref(n))
    assert rc == 0 and n.value == t.shape[0]     # the target is untouched
    # recovery: the same context gives a fresh context's bytes
    out = _align(ctx, *GC.EVAL_PAIR, False)
    assert out[0].tobytes() == ref[0].tobytes() and _stats_tuple(out[1]) == _stats_tuple(ref[1]) and out[2] == ref[2]
