"""The numpy statement of the robust kernels and the active set (tests/pgo_robust_model.py): equal to pgo_model bit
for bit where no kernel bites, its gradient against central differences of the robust cost, the active set, and the
drop-in's syntax.  No GPU.  The outlier cases' own assertions run when _pgo_robust_cases is imported."""
import os
import subprocess

import numpy as np
import pytest

import _pgo_cases as Cs
import _pgo_robust_cases as RC
import pgo_model as M
import pgo_robust_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_run(a, b):
    (pa, sa), (pb, sb) = a, b
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb))
    for key in ("status", "iterations", "trials", "F0", "F", "lam", "lam0", "b0", "F_trace", "decisions"):
        assert sa[key] == sb[key], key
    if "b_final" in sb:
        assert sa["b_final"] == sb["b_final"]


@pytest.mark.parametrize("name", ["n9", "n65", "hub"])
def test_no_kernel_equals_the_plain_model_bit_for_bit(name):
    c = Cs.get(name)
    m = len(c.graph.edges)
    _same_run(RM.optimize(c.graph), (c.poses, c.stats))
    _same_run(RM.optimize(c.graph, [(RM.NONE, 1.0)] * m, [True] * m), (c.poses, c.stats))
    for a, b in zip(RM.linearise(c.graph), M.linearise(c.graph)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["n9", "n65", "hub"])
def test_huber_wider_than_every_residual_equals_the_plain_model_bit_for_bit(name):
    c = Cs.get(name)
    m = len(c.graph.edges)
    kernels = [(RM.HUBER, 1e6)] * m
    assert float(np.max(RM.edge_stats(c.graph)[0])) < 1e12     # every chi2 is below delta^2 at the start already
    _same_run(RM.optimize(c.graph, kernels), (c.poses, c.stats))


@pytest.mark.parametrize("key", ["huber", "cauchy"])
def test_gradient_matches_central_differences_of_the_robust_cost(key):
    """2 b against (F(+h) - F(-h)) / 2h, h = 1e-6, on n9 with its wrong edge: within 1e-6 of max |b|."""
    c = RC.get("n9")
    g = c.graph
    kernels = [RC.KERNELS[key]] * len(g.edges)
    chi2, w = RM.edge_stats(g, kernels)
    assert (w < 1.0).any() and (key == "cauchy" or (w == 1.0).any())   # the kernel bites, and for Huber not everywhere
    _, b, _ = RM.linearise(g, kernels)
    _, nf = g.free_index()
    h, num = 1e-6, np.zeros(6 * nf)
    for k in range(6 * nf):
        d = np.zeros(6 * nf)
        d[k] = h
        num[k] = (RM.cost(g, kernels, M.apply(g, g.poses, d)) - RM.cost(g, kernels, M.apply(g, g.poses, -d))) / (2 * h)
    err = float(np.max(np.abs(2 * b - num))) / float(np.max(np.abs(b)))
    print(f"n9 + wrong edge, {key}: max |2b - dF/dx| / max |b| = {err:.3e}")
    assert err <= 1e-6


def test_rho_and_weight():
    assert RM.rho(RM.NONE, 1.0, 7.0) == (7.0, 1.0)
    assert RM.rho(RM.HUBER, 2.0, 4.0) == (4.0, 1.0)               # c == delta^2: still quadratic
    r, w = RM.rho(RM.HUBER, 2.0, 16.0)
    assert (r, w) == (12.0, 0.5)
    r, w = RM.rho(RM.CAUCHY, 3.0, 0.0)
    assert (r, w) == (0.0, 1.0)
    r, w = RM.rho(RM.CAUCHY, 3.0, 9.0)
    assert r == 9.0 * np.log1p(1.0) and w == 0.5
    h = 1e-6
    for kind, delta, c in [(RM.HUBER, 1.5, 30.0), (RM.CAUCHY, 3.0, 30.0), (RM.CAUCHY, 0.5, 1e4)]:   # w is rho'
        num = (RM.rho(kind, delta, c + h)[0] - RM.rho(kind, delta, c - h)[0]) / (2 * h)
        assert abs(num - RM.rho(kind, delta, c)[1]) <= 1e-8
    with pytest.raises(ValueError):
        RM.rho(3, 1.0, 1.0)


def test_an_inactive_edge_does_not_exist():
    c = RC.get("n65")
    m = len(c.graph.edges)
    active = [True] * m
    active[c.wrong] = False
    _same_run(RM.optimize(c.graph, None, active), RM.optimize(c.clean))
    chi2, w = RM.edge_stats(c.graph, None, active)
    assert w[c.wrong] == 0.0 and chi2[c.wrong] > 0.0 and (np.delete(w, c.wrong) == 1.0).all()
    g = c.graph.copy()
    g.add_vertex(np.eye(4))
    g.add_edge(64, 65, np.eye(4), np.eye(6))
    with pytest.raises(ValueError):                               # the leaf's only edge is inactive
        RM.optimize(g, None, [True] * m + [False])


def test_robust_dropin_compiles_with_gxx_alone():
    """tests/dropin/graph_robust_dropin.cpp uses GraphOptimizer's setRobustKernel, setEdgeRobustKernel, setEdgeActive,
    getEdgeChi2 and numEdges through compat.h."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Werror", f"-I{ROOT}/include",
                        f"{ROOT}/tests/dropin/graph_robust_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
