"""Pose-graph optimisation on the GPU (kernels/pgo_kernels.hip, host/pgo.cpp) against its numpy statement
tests/pgo_model.py, on the graphs of tests/_pgo_cases.py.  Bars: F within 1e-6 relative, b and H within 1e-5 of max |b|
and max |H| (the project's bars for its dense passes and GICP); a damped solve within 1e-8 of max |delta| of
numpy.linalg.solve (the CPU prototype of the same PCG measured 1e-10; the margin covers another grouping of partial
sums); a whole optimisation's status, iterations and trials equal to the model's, the final F within 1e-6 relative and
every pose within 1e-4 rad and 1e-3 m (the north-star bar).  Every figure is printed before it is asserted."""
import os
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

import _pgo_cases as Cs
import pgo_model as M

pytestmark = pytest.mark.gpu

BAR_RAD, BAR_M = 1e-4, 1e-3


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


_OPEN = []


@pytest.fixture(autouse=True)
def _close_graphs():
    """Every graph a test made is destroyed when the test ends, passed or not, before the module's context goes."""
    yield
    while _OPEN:
        _OPEN.pop().close()


def _new(ctx):
    pg = R.PoseGraph(ctx)
    _OPEN.append(pg)
    return pg


def _make(ctx, g):
    pg = _new(ctx)
    for T, f in zip(g.poses, g.fixed):
        k = pg.addVertex(T)
        if f and k > 0:
            pg.setFixed(k)
    for (i, j, Z, Om) in g.edges:
        pg.addEdge(i, j, Z, Om)
    return pg


def _pose_diff(P, Q):
    dr = dt = 0.0
    for a, b in zip(P, Q):
        c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1) / 2
        s = np.linalg.norm(a[:3, :3].T @ b[:3, :3] - b[:3, :3].T @ a[:3, :3]) / (2 * np.sqrt(2))
        dr = max(dr, float(np.arctan2(s, c)))
        dt = max(dt, float(np.linalg.norm(a[:3, 3] - b[:3, 3])))
    return dr, dt


def _blocks(H):
    n = H.shape[0] // 6
    return np.array([[bool(np.any(H[6 * r:6 * r + 6, 6 * c:6 * c + 6] != 0)) for c in range(n)] for r in range(n)])


@pytest.mark.parametrize("name", Cs.ALL)
def test_evaluation_parity(ctx, name):
    g = Cs.get(name).graph
    pg = _make(ctx, g)
    F, b, H = pg.eval()
    mF, mb, mH = M.linearise(g)
    dF = abs(F - mF) / mF if mF else abs(F)
    sb, sH = np.max(np.abs(mb)), np.max(np.abs(mH))
    db = float(np.max(np.abs(b - mb))) / sb if sb else float(np.max(np.abs(b)))
    dH = float(np.max(np.abs(H - mH))) / sH
    print(f"{name}: F {F:.9g} |dF|/F {dF:.2e}  |db|/max|b| {db:.2e}  |dH|/max|H| {dH:.2e}")
    if mF == 0.0:
        assert F == 0.0 and not b.any()
    assert dF <= 1e-6 and db <= 1e-5 and dH <= 1e-5
    assert np.array_equal(H, H.T) or np.max(np.abs(H - H.T)) <= 1e-9 * sH
    if name in ("duplicates", "hub", "reversed", "fixed8"):
        assert np.array_equal(_blocks(H), _blocks(mH))
    pg.close()


def _solve_case(ctx, name, forms):
    g = Cs.get(name).graph
    pg = _make(ctx, g)
    mF, mb, mH = M.linearise(g)
    lam0 = 1e-5 * float(np.max(np.diag(mH)))
    _, nf = g.free_index()
    for lam in (lam0, 1e-4 * lam0):
        ref = np.linalg.solve(mH + lam * np.eye(mH.shape[0]), -mb)
        scale = float(np.max(np.abs(ref)))
        got = {}
        for form in forms:
            d, it, rel, used, ok = pg.solve(lam, R.GraphParams.default(cg_form=form))
            err = float(np.max(np.abs(d - ref))) / scale
            print(f"{name} lambda {lam:.3e} form {form}: {it} iterations of {6 * nf} unknowns (cap {12 * nf}), residual "
                  f"{rel:.2e}, max |d - d_model| / max |d_model| = {err:.2e}")
            assert ok and used == form and 0 < it <= 12 * nf and rel <= 1e-12
            assert err <= 1e-8
            got[form] = d
        if len(got) == 2:
            both = float(np.max(np.abs(got[1] - got[2]))) / scale
            print(f"{name} lambda {lam:.3e}: the two forms differ by {both:.2e}")
            assert both <= 1e-8
    pg.close()


@pytest.mark.parametrize("name", ["n9", "n65", "n257", "hub", "fixed8"])
def test_solve_parity_both_forms(ctx, name):
    _solve_case(ctx, name, (1, 2))


def test_solve_parity_513_multi_launch(ctx):
    _solve_case(ctx, "n513", (2,))
    g = Cs.get("n513").graph
    pg = _make(ctx, g)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):   # too large for one workgroup's LDS
        pg.solve(1.0, R.GraphParams.default(cg_form=1))
    assert pg.solve(1.0)[3] == 2                          # automatic: the multi-launch form
    pg.close()


def _compare_run(name, pg, st, model_poses, ms):
    P = pg.getPoses()
    dr, dt = _pose_diff(P, model_poses)
    dF = abs(st.F_final - ms["F"]) / ms["F"] if ms["F"] else abs(st.F_final)
    print(f"{name}: status {st.status} iterations {st.iterations} trials {st.trials} form {st.cg_form} F {st.F_initial:.6g} -> "
          f"{st.F_final:.6g} (|dF|/F {dF:.2e}) lambda {st.lambda_:.3e} CG {st.cg_iterations} in all, {st.cg_iterations_max} "
          f"at most; poses vs model {dr:.2e} rad {dt:.2e} m")
    assert (st.status, st.iterations, st.trials) == (ms["status"], ms["iterations"], ms["trials"])
    assert dF <= 1e-6
    assert dr <= BAR_RAD and dt <= BAR_M
    return P


@pytest.mark.parametrize("name", Cs.ALL)
def test_whole_optimisation(ctx, name):
    c = Cs.get(name)
    pg = _make(ctx, c.graph)
    st = pg.optimizeGraph()
    P = _compare_run(name, pg, st, c.poses, c.stats)
    if c.stats["iterations"] == 0:
        for a, b in zip(P, c.graph.poses):
            assert a.tobytes() == b.tobytes()
    for k, f in enumerate(c.graph.fixed):
        if f:
            assert P[k].tobytes() == c.graph.poses[k].tobytes()
    pg.close()


@pytest.mark.parametrize("form", [1, 2])
def test_whole_optimisation_in_either_form(ctx, form):
    c = Cs.get("n65")
    pg = _make(ctx, c.graph)
    st = pg.optimizeGraph(R.GraphParams.default(cg_form=form))
    assert st.cg_form == form
    _compare_run(f"n65 form {form}", pg, st, c.poses, c.stats)
    pg.close()


def test_determinism(ctx):
    c = Cs.get("n257")
    runs = []
    for _ in range(2):
        pg = _make(ctx, c.graph)
        st = pg.optimizeGraph()
        runs.append((pg.getPoses().tobytes(), bytes(st)))
        pg.close()
    assert runs[0] == runs[1]


def test_statuses(ctx):
    c = Cs.get("n65")
    pg = _make(ctx, c.graph)
    mp, ms = M.optimize(c.graph, max_iterations=1)
    assert ms["status"] == M.STATUS_ITERATION_LIMIT and not M.undecided(ms)
    st = pg.optimizeGraph(R.GraphParams.default(max_iterations=1))
    assert st.status == R.GRAPH_ITERATION_LIMIT == M.STATUS_ITERATION_LIMIT
    _compare_run("n65 max_iterations 1", pg, st, mp, ms)
    pg.close()
    pg = _make(ctx, c.graph)
    st = pg.optimizeGraph(R.GraphParams.default(cg_max_iterations=2))
    print("cg_max_iterations 2: status", st.status, "CG iterations", st.cg_iterations)
    assert st.status == R.GRAPH_CG_NOT_CONVERGED == M.STATUS_CG and st.iterations == 0 and st.cg_iterations == 2
    for a, b in zip(pg.getPoses(), c.graph.poses):
        assert a.tobytes() == b.tobytes()
    pg.close()


def test_input_checks_and_recovery(ctx):
    """Every R360_EINVAL (-2) of the intake and of the graph checks; after each the same handle goes on to optimise
    a valid graph as the model does."""
    c = Cs.get("n9")
    g = c.graph.copy()
    pg = _make(ctx, g)
    bad = np.eye(4)
    bad[1, 3] = np.nan
    info_bad = np.eye(6)
    info_bad[2, 2] = np.inf
    einval = pytest.raises(RuntimeError, match=r"\(-2\)")
    with einval:
        pg.addVertex(bad)
    with einval:
        pg.setPose(3, bad)
    with einval:
        pg.addEdge(0, 1, bad, np.eye(6))
    with einval:
        pg.addEdge(0, 1, np.eye(4), info_bad)
    with einval:
        pg.addEdge(0, 9, np.eye(4), np.eye(6))      # a missing vertex
    with einval:
        pg.addEdge(-1, 2, np.eye(4), np.eye(6))
    with einval:
        pg.addEdge(4, 4, np.eye(4), np.eye(6))      # i == j
    with einval:
        pg.setFixed(0, False)
    with einval:
        pg.optimizeGraph(R.GraphParams.default(max_iterations=0))
    assert pg.size() == (9, len(g.edges))
    st = pg.optimizeGraph()
    _compare_run("n9 after rejected intake", pg, st, c.poses, c.stats)
    pg.close()

    # graph-level checks: reported by optimise, mended on the same handle
    rng = np.random.default_rng(5)
    pg = _make(ctx, g)
    T9 = Cs.mul4(g.poses[8], Cs.noise4(rng, 0.2, 0.05))
    assert pg.addVertex(T9) == 9
    g.add_vertex(T9)
    with einval:
        pg.optimizeGraph()                          # a free vertex with no edge
    with einval:
        pg.eval()
    T10 = Cs.mul4(T9, Cs.noise4(rng, 0.2, 0.05))
    pg.addVertex(T10)
    g.add_vertex(T10)
    Z, Om = Cs.noise4(rng, 0.2, 0.05), Cs.info(rng)
    pg.addEdge(9, 10, Z, Om)
    g.add_edge(9, 10, Z, Om)
    with einval:
        pg.optimizeGraph()                          # the component {9, 10} has no fixed vertex
    for a, b in zip(pg.getPoses(), g.poses):
        assert a.tobytes() == b.tobytes()
    Z, Om = Cs.measure(rng, c.truth[8], c.truth[8], 0.01, 0.003), Cs.info(rng)
    pg.addEdge(8, 9, Z, Om)
    g.add_edge(8, 9, Z, Om)
    mp, ms = M.optimize(g)
    assert not M.undecided(ms)
    st = pg.optimizeGraph()
    _compare_run("n9 + 2 after graph-level errors", pg, st, mp, ms)
    pg.close()


@pytest.mark.parametrize("name,half", [("n65", 32), ("duplicates", 4)])
def test_incremental_use(ctx, name, half):
    """The reference's pattern: add vertices and edges, optimise, add more (chained on the optimised poses), optimise
    again; the model is run the same way on its own poses."""
    full = Cs.get(name).graph
    n = len(full.poses)
    pg = _new(ctx)
    g = M.Graph()
    for k in range(half + 1):
        pg.addVertex(full.poses[k])
        g.add_vertex(full.poses[k])
    first = [e for e in full.edges if max(e[0], e[1]) <= half]
    for (i, j, Z, Om) in first:
        pg.addEdge(i, j, Z, Om)
        g.add_edge(i, j, Z, Om)
    mp, ms = M.optimize(g)
    assert not M.undecided(ms) and ms["iterations"] > 0
    st = pg.optimizeGraph()
    P = _compare_run("incremental, first half", pg, st, mp, ms)
    g.poses = [p.copy() for p in mp]
    chain = {(e[0], e[1]): e for e in full.edges if e[1] == e[0] + 1}
    Tg, Tm = P[half], mp[half]
    for k in range(half + 1, n):
        Z = chain[(k - 1, k)][2]
        Tg, Tm = Cs.mul4(Tg, Z), Cs.mul4(Tm, Z)
        pg.addVertex(Tg)
        g.add_vertex(Tm)
    for (i, j, Z, Om) in full.edges:
        if max(i, j) > half:
            pg.addEdge(i, j, Z, Om)
            g.add_edge(i, j, Z, Om)
    mp, ms = M.optimize(g)
    assert not M.undecided(ms) and ms["iterations"] > 0
    st = pg.optimizeGraph()
    _compare_run("incremental, second half", pg, st, mp, ms)
    pg.close()


def test_save_and_load(ctx, tmp_path):
    c = Cs.get("fixed8")
    pg = _make(ctx, c.graph)
    a, b = tmp_path / "a.g2o", tmp_path / "b.g2o"
    pg.saveGraph(str(a))
    other = _new(ctx)
    other.loadGraph(str(a))
    other.saveGraph(str(b))
    assert a.read_bytes() == b.read_bytes()
    assert other.size() == pg.size()
    st = other.optimizeGraph()
    _compare_run("fixed8 loaded from its file", other, st, c.poses, c.stats)
    pg.close()
    other.close()


def test_facade_dropin(ctx, tmp_path):
    """tests/dropin/graph_optimizer_dropin.cpp (the reference's call sites through compat.h) builds with g++ alone under
    -Wall -Wextra -Werror, runs, and prints the poses the Python path gives on the 9-vertex case.  Both paths take the
    case rounded to float, as the reference's callers hold it, and add the edges in the drop-in's order."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "graph_optimizer_dropin"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/graph_optimizer_dropin.cpp", "-o", str(exe),
                        f"-L{os.path.dirname(R.LIB_PATH)}", "-lrgbd360_hip", f"-Wl,-rpath,{os.path.dirname(R.LIB_PATH)}"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    g = Cs.get("n9").graph
    f32 = lambda A: np.asarray(A, np.float32)
    edges = sorted(g.edges, key=lambda e: max(e[0], e[1]))   # stable: the order the drop-in adds them in
    txt = tmp_path / "graph.txt"
    with open(txt, "w") as f:
        for T in g.poses:
            f.write("V " + " ".join(f"{v:.9g}" for v in f32(T).T.reshape(-1)) + "\n")
        for (i, j, Z, Om) in edges:
            f.write(f"E {i} {j} " + " ".join(f"{v:.9g}" for v in f32(Z).T.reshape(-1)) + " " +
                    " ".join(f"{v:.9g}" for v in f32(Om).T.reshape(-1)) + "\n")
    out = subprocess.run([str(exe), str(txt), str(tmp_path / "out.g2o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ThreeDegreesOfFreedom throws" in out.stdout
    got = np.array([[float(v) for v in l.split()[2:]] for l in out.stdout.splitlines() if l.startswith("pose ")], np.float32)
    pg = _new(ctx)
    for T in g.poses:
        pg.addVertex(f32(T).astype(np.float64))
    for (i, j, Z, Om) in edges:
        pg.addEdge(i, j, f32(Z).astype(np.float64), f32(Om).astype(np.float64))
    st = pg.optimizeGraph()
    want = np.array([T.T.reshape(-1) for T in pg.getPoses()]).astype(np.float32)
    print(out.stdout.splitlines()[-13], "| python path: status", st.status, "iterations", st.iterations)
    assert st.iterations > 0 and got.shape == want.shape == (9, 16)
    assert np.array_equal(got, want)
    poses, fixed, ed = R.g2o_read(str(tmp_path / "out.g2o"))
    assert len(poses) == 9 and list(fixed) == [1] + [0] * 8 and len(ed) == len(edges)


def test_graph_outlives_its_context_safely():
    """Destroying a graph after its context (a test that failed before its close, an interpreter shutting down) frees
    the graph's buffers and reads nothing of the context."""
    c = R.Context(0)
    pg = _make(c, Cs.get("n9").graph)
    pg.optimizeGraph()
    c.close()
    pg.close()


@pytest.mark.parametrize("n,form", [(339, 1), (340, 2)])
def test_single_workgroup_limit(ctx, n, form):
    """338 free vertices are the most whose four CG vectors fit the single-workgroup form's LDS (65,024 B); one more
    goes to the multi-launch form, and asking for form 1 there is R360_EINVAL.  Both sides solve as numpy does."""
    g = Cs.build_sized(n, 1, [(0, 128), (0, 256), (64, 192), (1, n - 1)])[0]
    pg = _make(ctx, g)
    mF, mb, mH = M.linearise(g)
    lam = 1e-5 * float(np.max(np.diag(mH)))
    ref = np.linalg.solve(mH + lam * np.eye(mH.shape[0]), -mb)
    d, it, rel, used, ok = pg.solve(lam)
    err = float(np.max(np.abs(d - ref))) / float(np.max(np.abs(ref)))
    print(f"{n} vertices: form {used}, {it} iterations, residual {rel:.2e}, max |d - d_model| / max |d_model| = {err:.2e}")
    assert ok and used == form and err <= 1e-8
    if form == 2:
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            pg.solve(lam, R.GraphParams.default(cg_form=1))
    st = pg.optimizeGraph()
    assert st.cg_form == form and st.status == R.GRAPH_CONVERGED and st.F_final < st.F_initial
