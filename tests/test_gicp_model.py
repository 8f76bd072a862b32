"""The Generalized-ICP statement (tests/gicp_model.py) on known answers, its intake and tie rules, its convergence
on the test pair, the conditions the GPU tests' inputs must meet (tests/_gicp_cases.py), the drop-in's compile and
the library's host-side pieces that need no GPU (default parameters, the exported ABI)."""
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

import _gicp_cases as GC
import gicp_model as GM


def _plane(n_side=20, seed=3):
    rng = np.random.default_rng(seed)
    g = (np.arange(n_side) - n_side / 2) * 0.1
    x, y = np.meshgrid(g, g)
    p = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.5)], axis=1)
    p[:, :2] += rng.uniform(-0.03, 0.03, size=(x.size, 2))
    return p.astype(np.float32)   # z = 0.5 stays exact


def test_plane_gives_the_known_covariance():
    p = _plane()
    assert p.shape[0] == 400
    C, lam, _ = GM.covariances(p, 20, 1e-3)
    assert np.abs(C - np.diag([1.0, 1.0, 1e-3])).max() <= 1e-12
    # rotated by a known R, in float64 (covariances takes the points as given: a float32 cast would bend the plane
    # by its rounding, 2e-7 of a 0.3 m neighbourhood)
    Rk = GM.exp_se3((0, 0, 0, 0.3, -0.5, 0.7))[:3, :3]
    C2, _, _ = GM.covariances(p.astype(np.float64) @ Rk.T, 20, 1e-3)
    assert np.abs(C2 - Rk @ np.diag([1.0, 1.0, 1e-3]) @ Rk.T).max() <= 1e-12


def test_intake_drops_non_finite_rows_in_order():
    p = GC.room(40, 4)
    q = p.copy()
    q[3, 1] = np.nan
    q[17, 0] = np.inf
    q[39, 2] = -np.inf
    kept = GM.intake(q, 20)
    assert kept.tobytes() == np.delete(p, [3, 17, 39], axis=0).tobytes()
    with pytest.raises(ValueError):
        GM.intake(GC.room(19, 1), 20)
    assert GM.intake(q[:22], 20).shape[0] == 20   # 22 rows less rows 3 and 17: 20 finite points are enough
    with pytest.raises(ValueError):
        GM.intake(q[:21], 20)                     # 19 are not


def test_ties_go_to_the_lower_index():
    g = np.array([(x, y, z) for z in range(2) for y in range(3) for x in range(4)], np.float32)
    assert g.shape[0] == 24
    rng = np.random.default_rng(9)
    g = g[rng.permutation(24)]   # the index order is not the lattice order
    for k in (4, 7, 20):
        idx, d2, _ = GM.knn(g, k)
        for i in range(24):
            dd = ((g.astype(np.float64) - g[i]) ** 2).sum(axis=1)
            order = sorted(range(24), key=lambda j: (dd[j], j))
            assert list(idx[i]) == order[:k], (k, i)
            assert idx[i, 0] == i and d2[i, 0] == 0.0
    # nearest-target ties as well: a query midway between lattice points
    j, d2, second = GM.nearest(g.astype(np.float64), GM.cKDTree(g.astype(np.float64)), np.array([[0.5, 0.5, 0.5]]))
    dd = ((g.astype(np.float64) - 0.5) ** 2).sum(axis=1)
    assert j[0] == int(np.flatnonzero(dd == dd.min())[0]) and d2[0] == second[0] == 0.75


def test_alignment_converges_to_the_sampling_floor():
    ms, mt = GC.model_pair(1999, 2113)
    r = GM.align(ms, mt, np.eye(4), GC.params32())
    assert r.status == 0 and r.converged and r.iterations < 10, r
    assert r.inner_steps == sum(r.inner_per_iteration)
    er = GM.rot_angle(r.pose, GC.G())
    et = float(np.linalg.norm(r.pose[:3, 3] - GC.G()[:3, 3]))
    print(f"iterations {r.iterations}, inner steps {r.inner_per_iteration}, error {er:.3g} rad {et:.3g} m")
    assert er < 1e-3 and et < 1e-3, (er, et)


def test_a_noisier_generator_misses_the_floor():
    """The 1e-3 bar binds the generator: with 2 cm of jitter the same alignment ends further from G."""
    s, t = GC.pair(1999, 2113, jitter=0.02)
    p = GC.params32()
    r = GM.align(GM.Cloud(s, p), GM.Cloud(t, p), np.eye(4), p)
    er = GM.rot_angle(r.pose, GC.G())
    et = float(np.linalg.norm(r.pose[:3, 3] - GC.G()[:3, 3]))
    assert not (r.converged and r.iterations < 10 and er < 1e-3 and et < 1e-3), (r, er, et)


@pytest.mark.parametrize("ns,nt", GC.SIZES)
def test_inputs_are_decided(ns, nt):
    """At most 1 % of a case's points may be undecided, at every size the GPU tests use."""
    p = GC.params32()
    for c in GC.model_pair(ns, nt):
        n = c.xyz.shape[0]
        assert (~GC.knn_decided(c)).sum() <= GC.MAX_UNDECIDED * n
        assert (~GC.cov_decided(c)).sum() <= GC.MAX_UNDECIDED * n
    ms, mt = GC.model_pair(ns, nt)
    for X in (np.eye(4), GC.pose2().astype(np.float32).astype(np.float64)):
        _, _, _, _, _, d2, second = GM.eval_at(ms, mt, X, p)
        assert (~GC.corr_decided(d2, second, p.max_corr_dist)).sum() <= GC.MAX_UNDECIDED * ns


def test_partial_gate_case():
    ms, mt = GC.model_pair(64, 129)
    _, _, _, _, n, _, _ = GM.eval_at(ms, mt, np.eye(4), GC.params32())
    assert 16 <= n <= 48   # about half of the 64 points are inside the gate


def test_default_params_are_the_issues():
    p = R.GicpParams.default()
    assert (p.k_correspondences, p.max_iterations, p.max_inner_iterations) == (20, 10, 20)
    assert p.gicp_epsilon == np.float32(1e-3) and p.max_corr_dist == np.float32(0.4)
    assert p.rotation_epsilon == 2e-3 and p.transformation_epsilon == 1e-9
    q = GM.Params()
    assert (q.k_correspondences, q.gicp_epsilon, q.max_corr_dist, q.max_iterations, q.max_inner_iterations,
            q.rotation_epsilon, q.transformation_epsilon) == (20, 1e-3, 0.4, 10, 20, 2e-3, 1e-9)
    for name in ("r360_gicp_set_source", "r360_gicp_set_target", "r360_gicp_align", "r360_gicp_get_cloud",
                 "r360_gicp_eval", "r360_gicp_default_params"):
        assert name in R.ABI_SYMBOLS and hasattr(R.lib(), name)


def test_model_exp_is_the_librarys():
    mu = (0.12, -0.08, 0.05, 0.03, -0.02, 0.04)
    assert np.abs(GM.exp_se3(mu) - R.exp_se3(mu, False)).max() <= 1e-7   # the library returns float32


def test_host_logic_check_runs(root, tmp_path):
    """tools/gicp_host_check.cpp (intake, grid sizing and counting sort, the 6x6 solve, the inner loop's accept / stop
    rule on a canned quadratic) builds with g++ alone and passes; the same file is what the host sanitizers run."""
    exe = tmp_path / "gicp_host_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"{root}/tools/gicp_host_check.cpp",
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "gicp host check ok" in p.stdout, p.stderr + p.stdout


def test_gicp_dropin_compiles(root):
    """tests/dropin/gicp_dropin.cpp: RegisterPairRGBD360's Generalized-ICP call sequence through compat.h, g++ alone."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/gicp_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
