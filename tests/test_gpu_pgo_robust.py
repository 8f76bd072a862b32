"""Robust kernels, per-edge chi2 and the active set of the pose-graph optimiser on the GPU (kernels/pgo_kernels.hip,
host/pgo.cpp) against their numpy statement tests/pgo_robust_model.py, on the outlier graphs of
tests/_pgo_robust_cases.py (9, 33 and 65 vertices, one wrong loop edge each).  Bars, as tests/test_gpu_pgo.py: F within
1e-6 relative, b and H within 1e-5 of max |b| and max |H|, a whole optimisation's status, iterations and trials equal
to the model's, the final F within 1e-6 relative and every pose within 1e-4 rad and 1e-3 m; chi2 and w per edge
within 1e-9 relative.  Every figure is printed before it is asserted."""
import os
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

import _pgo_cases as Cs
import _pgo_robust_cases as RC
import pgo_model as M
import pgo_robust_model as RM

pytestmark = pytest.mark.gpu

BAR_RAD, BAR_M = 1e-4, 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = r"\(-2\)"


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


_OPEN = []


@pytest.fixture(autouse=True)
def _close_graphs():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _make(ctx, g, kernels=None):
    pg = R.PoseGraph(ctx)
    _OPEN.append(pg)
    for T, f in zip(g.poses, g.fixed):
        k = pg.addVertex(T)
        if f and k > 0:
            pg.setFixed(k)
    for (i, j, Z, Om) in g.edges:
        pg.addEdge(i, j, Z, Om)
    for k, (kind, delta) in enumerate(kernels or []):
        pg.setEdgeRobustKernel(k, kind, delta)
    return pg


def _pose_diff(P, Q):
    dr = dt = 0.0
    for a, b in zip(P, Q):
        c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1) / 2
        s = np.linalg.norm(a[:3, :3].T @ b[:3, :3] - b[:3, :3].T @ a[:3, :3]) / (2 * np.sqrt(2))
        dr = max(dr, float(np.arctan2(s, c)))
        dt = max(dt, float(np.linalg.norm(a[:3, 3] - b[:3, 3])))
    return dr, dt


def _run_bytes(pg, params=None):
    st = pg.optimizeGraph(params)
    return pg.getPoses().tobytes(), bytes(st)


def _eval_bytes(pg):
    return b"".join(np.asarray(x).tobytes() for x in pg.eval())


def _is_loop(edge):
    return abs(edge[0] - edge[1]) != 1


def _kernels(g, config):
    """The per-edge kernels of a named configuration; 'straddle' puts loop edges on both sides of delta^2."""
    m = len(g.edges)
    if config in RC.KERNELS:
        return [RC.KERNELS[config]] * m
    if config == "mixed":      # loop edges robust (alternately Huber and Cauchy), chain edges without a kernel
        loops = [k for k, e in enumerate(g.edges) if _is_loop(e)]
        ks = [(RM.NONE, 1.0)] * m
        for n, k in enumerate(loops):
            ks[k] = (RM.CAUCHY, 3.0) if n % 2 else (RM.HUBER, 1.0)
        return ks
    assert config == "straddle"
    chi2 = RM.edge_stats(g)[0]
    loops = sorted(chi2[k] for k, e in enumerate(g.edges) if _is_loop(e))
    delta = float(np.sqrt(np.sqrt(loops[0] * loops[1])))      # delta^2 between the two smallest loop edges' chi2
    assert loops[0] < delta * delta < loops[1]
    return [(RM.HUBER, delta)] * m


@pytest.mark.parametrize("config", ["huber", "cauchy", "mixed", "straddle"])
@pytest.mark.parametrize("name", RC.ALL)
def test_evaluation_parity(ctx, name, config):
    g = RC.get(name).graph
    ks = _kernels(g, config)
    w = RM.edge_stats(g, ks)[1]
    assert (w < 1.0).any() and (w == 1.0).any()
    if config == "straddle":
        lw = [w[k] for k, e in enumerate(g.edges) if _is_loop(e)]
        assert min(lw) < 1.0 and max(lw) == 1.0
    pg = _make(ctx, g, ks)
    F, b, H = pg.eval()
    mF, mb, mH = RM.linearise(g, ks)
    dF = abs(F - mF) / mF
    sb, sH = np.max(np.abs(mb)), np.max(np.abs(mH))
    db, dH = float(np.max(np.abs(b - mb))) / sb, float(np.max(np.abs(H - mH))) / sH
    print(f"{name} {config}: F {F:.9g} (no kernel {M.linearise(g)[0]:.9g}) |dF|/F {dF:.2e}  |db|/max|b| {db:.2e}  "
          f"|dH|/max|H| {dH:.2e}")
    assert dF <= 1e-6 and db <= 1e-5 and dH <= 1e-5


def _rel(got, want):
    return max((abs(a - b) / abs(b) if b else abs(a)) for a, b in zip(got, want))


@pytest.mark.parametrize("key", list(RC.KERNELS))
@pytest.mark.parametrize("name", RC.ALL)
def test_edge_stats(ctx, name, key):
    """At the start poses (the chain edges' chi2 is rounding noise there) and at the model's optimum."""
    c = RC.get(name)
    ks = [RC.KERNELS[key]] * len(c.graph.edges)
    pg = _make(ctx, c.graph, ks)
    for label, poses in (("start", c.graph.poses), ("optimum", c.runs[key][0])):
        for k, T in enumerate(poses):
            pg.setPose(k, T)
        chi2, w = pg.getEdgeChi2()
        mc, mw = RM.edge_stats(c.graph, ks, poses=poses)
        dc, dw = _rel(chi2, mc), _rel(w, mw)
        print(f"{name} {key} {label}: chi2 {mc.min():.3g} .. {mc.max():.3g}, max relative difference chi2 {dc:.2e} w {dw:.2e}")
        assert dc <= 1e-9 and dw <= 1e-9
        assert int(np.argmax(chi2)) == c.wrong
    pg.setEdgeActive(c.wrong, False)
    chi2b, wb = pg.getEdgeChi2()
    assert wb[c.wrong] == 0.0 and np.array_equal(chi2b, chi2) and np.array_equal(np.delete(wb, c.wrong), np.delete(w, c.wrong))


@pytest.mark.parametrize("kind", [R.GRAPH_KERNEL_NONE, R.GRAPH_KERNEL_HUBER, R.GRAPH_KERNEL_CAUCHY])
def test_edge_stats_of_an_exact_chain(ctx, kind):
    g = Cs.get("exact_chain").graph
    pg = _make(ctx, g, [(kind, 3.0)] * len(g.edges))
    chi2, w = pg.getEdgeChi2()
    assert len(chi2) == len(g.edges) and not chi2.any() and (w == 1.0).all()
    F, b, _ = pg.eval()
    assert F == 0.0 and not b.any()


@pytest.mark.parametrize("key", list(RC.KERNELS))
@pytest.mark.parametrize("name", RC.ALL)
def test_whole_optimisation(ctx, name, key):
    c = RC.get(name)
    mp, ms = c.runs[key]
    pg = _make(ctx, c.graph, [RC.KERNELS[key]] * len(c.graph.edges))
    st = pg.optimizeGraph()
    P = pg.getPoses()
    dr, dt = _pose_diff(P, mp)
    dF = abs(st.F_final - ms["F"]) / ms["F"]
    chi2, w = pg.getEdgeChi2()
    order = np.argsort(-chi2)
    print(f"{name} {key}: status {st.status} iterations {st.iterations} trials {st.trials} F {st.F_initial:.6g} -> "
          f"{st.F_final:.6g} (|dF|/F {dF:.2e}); poses vs model {dr:.2e} rad {dt:.2e} m; worst translation error "
          f"{RC.worst_error(P, c.truth):.3f} m (start {c.err_start:.3f}, no kernel {c.err['none']:.3f}); chi2 of edge "
          f"{order[0]} {chi2[order[0]]:.4g} (w {w[order[0]]:.3g}), next {chi2[order[1]]:.4g}")
    assert (st.status, st.iterations, st.trials) == (ms["status"], ms["iterations"], ms["trials"])
    assert dF <= 1e-6 and dr <= BAR_RAD and dt <= BAR_M
    assert order[0] == c.wrong
    assert RC.worst_error(P, c.truth) < c.err_start


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", ["n65", "hub"])
def test_a_kernel_that_never_bites_changes_no_byte(ctx, name, form):
    g = Cs.get(name).graph
    m = len(g.edges)
    prm = R.GraphParams.default(cg_form=form)
    plain = _run_bytes(_make(ctx, g), prm)
    assert _run_bytes(_make(ctx, g, [(R.GRAPH_KERNEL_NONE, 1.0)] * m), prm) == plain
    assert _run_bytes(_make(ctx, g, [(R.GRAPH_KERNEL_HUBER, 1e6)] * m), prm) == plain
    pg = _make(ctx, g)                      # the default kernel reaches the edges added after it
    pg2 = R.PoseGraph(ctx)
    _OPEN.append(pg2)
    pg2.setRobustKernel(R.GRAPH_KERNEL_HUBER, 1e6)
    for T in g.poses:
        pg2.addVertex(T)
    for (i, j, Z, Om) in g.edges:
        pg2.addEdge(i, j, Z, Om)
    assert pg2.getEdgeRobustKernel(m - 1) == (R.GRAPH_KERNEL_HUBER, 1e6) and pg.getEdgeRobustKernel(m - 1)[0] == 0
    assert _eval_bytes(pg2) == _eval_bytes(pg)
    assert _run_bytes(pg2, prm) == plain


def test_deactivation(ctx):
    c = RC.get("n65")
    without = _make(ctx, c.clean)
    ev_without = _eval_bytes(without)
    run_without = _run_bytes(without)
    pg = _make(ctx, c.graph)
    ev_full = _eval_bytes(pg)
    assert ev_full != ev_without
    pg.setEdgeActive(c.wrong, False)
    assert not pg.getEdgeActive(c.wrong) and pg.getEdgeActive(0)
    assert _eval_bytes(pg) == ev_without
    assert _run_bytes(pg) == run_without
    full = _run_bytes(_make(ctx, c.graph))
    assert full != run_without
    again = _make(ctx, c.graph)
    again.setEdgeActive(c.wrong, False)
    again.setEdgeActive(c.wrong, True)
    assert _eval_bytes(again) == ev_full and _run_bytes(again) == full
    # an inactive edge in the middle of the list: the edges after it move up one place on the device
    g = c.graph.copy()
    k = len(g.edges) // 2
    mid = _make(ctx, g)
    mid.setEdgeActive(k, False)
    del g.edges[k]
    assert _eval_bytes(mid) == _eval_bytes(_make(ctx, g))


def test_deactivating_a_leafs_only_edge_is_einval(ctx):
    c = RC.get("n9")
    g = c.graph.copy()
    rng = np.random.default_rng(9)
    g.add_vertex(Cs.mul4(g.poses[8], Cs.noise4(rng, 0.2, 0.05)))
    g.add_edge(8, 9, Cs.noise4(rng, 0.2, 0.05), Cs.info(rng))
    leaf = len(g.edges) - 1
    fresh = _run_bytes(_make(ctx, g))
    pg = _make(ctx, g)
    pg.setEdgeActive(leaf, False)
    before = pg.getPoses().tobytes()
    for call in (pg.optimizeGraph, pg.eval, lambda: pg.solve(1.0)):
        with pytest.raises(RuntimeError, match=EINVAL):
            call()
    assert pg.getPoses().tobytes() == before
    chi2, w = pg.getEdgeChi2()                 # per-edge figures need no valid graph
    assert w[leaf] == 0.0 and chi2[leaf] > 0.0
    pg.setEdgeActive(leaf, True)
    assert _run_bytes(pg) == fresh
    # a component anchored only through an inactive edge
    pg = _make(ctx, g)
    pg.setEdgeActive(0, False)                 # the chain edge 0 - 1; the loop edges from 0 still hold the graph
    pg.optimizeGraph()
    for k, e in enumerate(g.edges):
        if 0 in e[:2]:
            pg.setEdgeActive(k, False)
    with pytest.raises(RuntimeError, match=EINVAL):
        pg.optimizeGraph()


def test_determinism(ctx):
    c = RC.get("n65")
    ks = _kernels(c.graph, "mixed")
    runs = [_run_bytes(_make(ctx, c.graph, ks)) for _ in range(2)]
    assert runs[0] == runs[1]
    ks = [RC.KERNELS["cauchy"]] * len(c.graph.edges)
    runs = [_run_bytes(_make(ctx, c.graph, ks), R.GraphParams.default(cg_form=2)) for _ in range(2)]
    assert runs[0] == runs[1]


def test_save_and_load(ctx, tmp_path):
    c = RC.get("n9")
    m = len(c.graph.edges)
    pg = _make(ctx, c.graph, [RC.KERNELS["cauchy"]] * m)
    a, b = tmp_path / "a.g2o", tmp_path / "b.g2o"
    pg.saveGraph(str(a))
    assert a.read_text().count("EDGE_SE3:QUAT") == m
    pg.setEdgeActive(c.wrong, False)
    pg.setEdgeActive(1, False)
    pg.saveGraph(str(b))
    assert b.read_text().count("EDGE_SE3:QUAT") == m - 2
    other = R.PoseGraph(ctx)
    _OPEN.append(other)
    other.loadGraph(str(b))
    assert other.size() == (9, m - 2)
    assert all(other.getEdgeRobustKernel(k) == (R.GRAPH_KERNEL_NONE, 1.0) and other.getEdgeActive(k) for k in range(m - 2))
    other.setRobustKernel(R.GRAPH_KERNEL_HUBER, 2.5)
    other.loadGraph(str(b))
    assert all(other.getEdgeRobustKernel(k) == (R.GRAPH_KERNEL_HUBER, 2.5) and other.getEdgeActive(k) for k in range(m - 2))
    _, _, ed = R.g2o_read(str(b))
    kept = [e for k, e in enumerate(c.graph.edges) if k not in (1, c.wrong)]
    assert [(e[0], e[1]) for e in ed] == [(e[0], e[1]) for e in kept]


def test_argument_checks(ctx):
    g = RC.get("n9").graph
    m = len(g.edges)
    plain = _run_bytes(_make(ctx, g))
    pg = _make(ctx, g)
    einval = pytest.raises(RuntimeError, match=EINVAL)
    for kind, delta in [(3, 1.0), (-1, 1.0), (R.GRAPH_KERNEL_HUBER, 0.0), (R.GRAPH_KERNEL_HUBER, float("nan")),
                        (R.GRAPH_KERNEL_CAUCHY, -1.0), (R.GRAPH_KERNEL_CAUCHY, float("inf")), (R.GRAPH_KERNEL_NONE, 0.0)]:
        with einval:
            pg.setEdgeRobustKernel(2, kind, delta)
        with einval:
            pg.setRobustKernel(kind, delta)
    for edge in (-1, m):
        with einval:
            pg.setEdgeRobustKernel(edge, R.GRAPH_KERNEL_HUBER, 1.0)
        with einval:
            pg.getEdgeRobustKernel(edge)
        with einval:
            pg.setEdgeActive(edge, False)
        with einval:
            pg.getEdgeActive(edge)
    assert pg.numEdges() == m
    assert all(pg.getEdgeRobustKernel(k) == (R.GRAPH_KERNEL_NONE, 1.0) and pg.getEdgeActive(k) for k in range(m))
    pg.addEdge(0, 1, g.edges[0][2], g.edges[0][3])       # the default kernel is still NONE
    assert pg.getEdgeRobustKernel(m) == (R.GRAPH_KERNEL_NONE, 1.0)
    pg.setEdgeActive(m, False)
    assert _run_bytes(pg) == plain
    n = R.C.c_int()
    assert R.lib().r360_graph_edge_stats(pg.h, None, None, 0, R.C.byref(n)) == 0 and n.value == m + 1
    chi2 = np.zeros(m + 1)
    assert R.lib().r360_graph_edge_stats(pg.h, chi2.ctypes.data_as(R.C.POINTER(R.C.c_double)), None, m, R.C.byref(n)) == -4
    assert R.lib().r360_graph_edge_stats(pg.h, chi2.ctypes.data_as(R.C.POINTER(R.C.c_double)), None, m + 1, R.C.byref(n)) == 0
    assert chi2[:m].all()


def test_facade_dropin(ctx, tmp_path):
    """tests/dropin/graph_robust_dropin.cpp (built by __graft_entry__.build() into build/bin) on the 9-vertex outlier
    graph rounded to float: it names the wrong edge and prints the poses the Python path gives for the same calls."""
    exe = os.path.join(ROOT, "build", "bin", "graph_robust_dropin")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    c = RC.get("n9")
    g = c.graph
    f32 = lambda A: np.asarray(A, np.float32)
    txt = tmp_path / "graph.txt"
    with open(txt, "w") as f:
        for T in g.poses:
            f.write("V " + " ".join(f"{v:.9g}" for v in f32(T).T.reshape(-1)) + "\n")
        for (i, j, Z, Om) in g.edges:
            f.write(f"E {i} {j} " + " ".join(f"{v:.9g}" for v in f32(Z).T.reshape(-1)) + " " +
                    " ".join(f"{v:.9g}" for v in f32(Om).T.reshape(-1)) + "\n")
    out = subprocess.run([exe, str(txt)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    print("\n".join(l for l in out.stdout.splitlines() if not l.startswith("pose ")))
    assert f"wrong edge {c.wrong}\n" in out.stdout
    got = np.array([[float(v) for v in l.split()[2:]] for l in out.stdout.splitlines() if l.startswith("pose ")], np.float32)
    pg = R.PoseGraph(ctx)
    _OPEN.append(pg)
    for T in g.poses:
        pg.addVertex(f32(T).astype(np.float64))
    for e in g.edges:
        pg.setRobustKernel(R.GRAPH_KERNEL_CAUCHY if _is_loop(e) else R.GRAPH_KERNEL_NONE, 3.0)
        pg.addEdge(e[0], e[1], f32(e[2]).astype(np.float64), f32(e[3]).astype(np.float64))
    pg.optimizeGraph()
    chi2, _ = pg.getEdgeChi2()
    assert int(np.argmax(chi2)) == c.wrong
    pg.setEdgeActive(c.wrong, False)
    for k in range(len(g.edges)):
        pg.setEdgeRobustKernel(k, R.GRAPH_KERNEL_NONE)
    pg.optimizeGraph()
    want = np.array([T.T.reshape(-1) for T in pg.getPoses()]).astype(np.float32)
    assert got.shape == want.shape == (9, 16) and np.array_equal(got, want)
