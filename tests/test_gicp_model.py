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


def _host_check_exe(root, tmp_path):
    exe = tmp_path / "gicp_host_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"{root}/tools/gicp_host_check.cpp",
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_crafted_clouds_get_the_grids_they_claim(root, tmp_path):
    """Every crafted cloud of _gicp_cases.CLOUDS through the library's own gicp_build_grid (tools/gicp_host_check.cpp
    with file arguments, which also checks the invariant ring_bound2 rests on): the shape is the table's and the numpy
    port's, to the bit of h."""
    exe = _host_check_exe(root, tmp_path)
    names = list(GC.CLOUDS)
    files = []
    for name in names:
        files.append(str(tmp_path / f"{name}.f32"))
        GC.cloud(name).tofile(files[-1])
    p = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr + p.stdout
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("grid ")]
    assert len(lines) == len(names), p.stdout
    for name, ln in zip(names, lines):
        dim, h = tuple(int(v) for v in ln[1:4]), np.float32(float(ln[4]))
        pdim, ph, _, _ = GC.choose_grid(GC.cloud(name))
        print(name, GC.cloud(name).shape[0], dim, h)
        assert dim == pdim and h == ph, (name, dim, pdim, h, ph)
        want = GC.CLOUDS[name][1]
        assert want is None or dim == want, (name, dim, want)
    grid = {name: GC.choose_grid(GC.cloud(name)) for name in names}
    # what each cloud is there for
    assert GC.cloud("room512").shape[0] == GC.DIRECT and GC.cloud("room513").shape[0] == GC.DIRECT + 1
    assert (GC.cloud("sheet")[:, 2] == 0.5).all() and grid["sheet"][0][2] == 1
    for name in ("rod", "rod1024", "ribbon"):   # the capped axis: h at the bisection's lower bound, to float rounding
        c = GC.cloud(name)
        emax = float((c.max(axis=0) - c.min(axis=0)).max())
        assert abs(float(grid[name][1]) * (GC.MAXDIM - 1) / emax - 1.0) <= 2.0 ** -22, name
    assert {grid["rod"][0][0], grid["rod1024"][0][0]} == {GC.MAXDIM - 1, GC.MAXDIM}
    # two clusters a kilometre apart: the cell columns between them are empty
    c, (dim, _, inv, mn) = GC.cloud("two_clusters"), grid["two_clusters"]
    used = np.unique(np.clip(np.floor((c[:, 0] - mn[0]) * inv), 0, dim[0] - 1))
    assert dim[0] - used.size >= 490, (dim, used)
    order = np.argsort(c[:, 0], kind="stable")
    assert not np.array_equal(order, np.arange(c.shape[0]))   # shuffled: index order is not spatial order


@pytest.mark.parametrize("name", list(GC.CLOUDS))
def test_crafted_clouds_are_decided(name):
    m = GC.model_cloud(name)
    n = m.xyz.shape[0]
    old, kd, cd = GC.knn_decided(m), GC.knn_decided_ties(m), GC.cov_decided_ties(m)
    print(f"{name}: n={n} undecided kNN {(~old).sum()} by the gap alone, {(~kd).sum()} with ties, covariances {(~cd).sum()}")
    assert (old <= kd).all()   # the extended rule only adds
    if name in GC.TIED:
        assert kd.all() and (~old).sum() > 50   # the ties are there, and the extended rule decides every one
    else:
        assert (~kd).sum() <= GC.MAX_UNDECIDED * n and (~cd).sum() <= GC.MAX_UNDECIDED * n
    if name == "dups":
        assert cd.all()
        c = GC.cloud(name)
        assert c.shape[0] == 700 and np.unique(c, axis=0).shape[0] == 600   # 100 rows are exact copies
    if name.startswith("lattice"):
        assert GC.exact_cloud(GC.cloud(name)) and np.abs(GC.cloud(name)).max() < 2.0
    if name == "lattice_plane":
        assert cd.all()
        assert np.abs(m.C - np.diag([1.0, 1.0, GC.make_params().gicp_epsilon])).max() == 0.0


def test_eval_poses_leave_the_targets_box():
    """The four poses of the eval stage put hundreds of source points beyond five of the six faces of the target's
    box (where the query's cell is clamped), and the cases that compare sums have no undecided correspondence."""
    ms, mt = GC.model_pair(*GC.EVAL_PAIR)
    dim, h, _, _ = GC.choose_grid(mt.xyz)
    assert min(GC.GATES) < float(h) < GC.GATES[0]   # one gate below the target's cell edge, one above
    reached = np.zeros(6, int)
    counts = []
    for name, X in GC.eval_poses().items():
        out = GC.outside_faces(ms.xyz, mt.xyz, X)
        assert out.max() > 100, (name, out)
        reached = np.maximum(reached, out)
        for gate in GC.GATES:
            p = GC.make_params(gate=gate)
            _, _, _, _, n, d2, second = GM.eval_at(ms, mt, X, p)
            und = int((~GC.corr_decided(d2, second, p.max_corr_dist)).sum())
            print(f"{name} gate {gate}: outside {out.tolist()} n_corr {n} undecided {und}")
            counts.append(n)
            assert und <= GC.MAX_UNDECIDED * ms.xyz.shape[0]
            assert und == 0 or name in GC.EVAL_CORR_ONLY, (name, gate, und)
    assert (reached > 100).sum() == 5, reached
    assert min(counts) < 10 and max(counts) == ms.xyz.shape[0]


def test_gate_lattice_ties_at_exactly_the_gate():
    s, t = GC.gate_lattice()
    assert GC.exact_cloud(s) and GC.exact_cloud(t) and s.shape[0] == 648
    p = GC.make_params(gate=0.125)
    ms, mt = GM.Cloud(s, p), GM.Cloud(t, p)
    corr, _, _, _, n, d2, second = GM.eval_at(ms, mt, np.eye(4), p)
    assert n == 0 and (corr == -1).all() and (d2 == 2.0 ** -6).all()   # the gate is strict
    assert (second == d2).sum() == 576                                 # 8 of the 9 x columns tie two ways
    above = GC.make_params(gate=float(np.nextafter(np.float32(0.125), np.float32(1.0))))
    corr, _, _, _, n, _, _ = GM.eval_at(ms, mt, np.eye(4), above)
    assert n == 648 and np.array_equal(corr, GC.gate_lattice_expected())


@pytest.mark.parametrize("k", GC.K_ENDS)
def test_k_ends_are_decided(k):
    for c in GC.model_pair_with(*GC.K_PAIR, k=k) + tuple(GC.model_room(n, 31, k) for n in (k, 600, 2000)):
        n = c.xyz.shape[0]
        assert c.knn.shape == (n, k)
        assert (~GC.knn_decided(c)).sum() <= GC.MAX_UNDECIDED * n and (~GC.cov_decided(c)).sum() <= GC.MAX_UNDECIDED * n
    assert GC.choose_grid(GC.room(k, 31))[0] == (1, 1, 1) and GC.choose_grid(GC.room(600, 31))[0] != (1, 1, 1)
    assert GC.WRAP_PAIR[0] > GC.PASS_WRAP


def test_gicp_dropin_compiles(root):
    """tests/dropin/gicp_dropin.cpp: RegisterPairRGBD360's Generalized-ICP call sequence through compat.h, g++ alone."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/gicp_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
