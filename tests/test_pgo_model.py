"""The numpy statement of the pose-graph optimiser (tests/pgo_model.py): its Jacobians against central differences,
descent on every shared case, the exact chain, the input checks.  No GPU."""
import numpy as np
import pytest

import _pgo_cases as Cs
import pgo_model as M


def _perturbed(T, d):
    return M.boxplus(T, d)


def test_jacobians_match_central_differences():
    """100 random edges with residual rotations up to 2.5 rad, h = 1e-6: within 1e-8 (the prototype measured 2.5e-10)."""
    h, worst = 1e-6, 0.0
    for (Ti, Tj, Z) in Cs.random_edges(100):
        e, Ji, Jj = M.edge_terms(Ti, Tj, Z)
        assert np.linalg.norm(e[3:]) < np.pi - 1e-3
        for (J, which) in ((Ji, 0), (Jj, 1)):
            num = np.zeros((6, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                if which == 0:
                    ep = M.edge_terms(_perturbed(Ti, d), Tj, Z, False)[0]
                    em = M.edge_terms(_perturbed(Ti, -d), Tj, Z, False)[0]
                else:
                    ep = M.edge_terms(Ti, _perturbed(Tj, d), Z, False)[0]
                    em = M.edge_terms(Ti, _perturbed(Tj, -d), Z, False)[0]
                num[:, k] = (ep - em) / (2 * h)
            worst = max(worst, float(np.max(np.abs(num - J))))
    print(f"Jacobians vs central differences: max |diff| = {worst:.3e}")
    assert worst <= 1e-8


def test_small_angle_branches_are_continuous():
    """Exp, log and J_r^-1 agree across the series threshold to rounding."""
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    for th in (0.0, 1e-9, 0.999e-4, 1.001e-4, 1e-3):
        w = ax * th
        assert np.allclose(M.log_so3(M.exp_so3(w)), w, rtol=0, atol=1e-15)
    lo, hi = M.jr_inv(ax * 0.9999e-4), M.jr_inv(ax * 1.0001e-4)
    assert np.max(np.abs(lo - hi)) < 1e-8
    assert np.array_equal(M.jr_inv(np.zeros(3)), np.eye(3))


@pytest.mark.parametrize("name", Cs.ALL)
def test_descent(name):
    """F never rises over accepted steps and the gradient falls to 1e-4 of the initial one; every decision of the
    model is decided (asserted by _pgo_cases.get)."""
    c = Cs.get(name)
    tr = c.stats["F_trace"]
    print(name, "status", c.stats["status"], "iterations", c.stats["iterations"], "trials", c.stats["trials"],
          "F", [f"{f:.6g}" for f in tr])
    assert all(b <= a for a, b in zip(tr, tr[1:]))
    if c.stats["iterations"]:
        assert c.stats["status"] == M.STATUS_CONVERGED
        assert c.stats["b_final"] <= 1e-4 * c.stats["b0"]


@pytest.mark.parametrize("name", ["exact_chain", "n2"])
def test_exact_chain_returns_at_once(name):
    c = Cs.get(name)
    assert c.stats["status"] == M.STATUS_CONVERGED and c.stats["iterations"] == 0 and c.stats["trials"] == 0
    assert c.stats["F0"] == 0.0
    for a, b in zip(c.poses, c.graph.poses):
        assert a.tobytes() == b.tobytes()


def test_optimisation_brings_the_loop_cases_closer_to_the_path():
    c = Cs.get("n257")
    err = lambda P: max(np.linalg.norm(a[:3, 3] - b[:3, 3]) for a, b in zip(P, c.truth))
    e0, e1 = err(c.graph.poses), err(c.poses)
    print(f"n257: worst translation error {e0:.3f} m -> {e1:.3f} m")
    assert e1 < e0


def test_input_checks():
    g = Cs.get("n9").graph.copy()
    g.add_vertex(np.eye(4))                       # a free vertex with no edge
    with pytest.raises(ValueError):
        M.check(g)
    g.add_vertex(np.eye(4))
    g.add_edge(9, 10, np.eye(4), np.eye(6))       # a component of its own without a fixed vertex
    with pytest.raises(ValueError):
        M.check(g)
    g.fixed[10] = True
    M.check(g)
    g.add_edge(3, 3, np.eye(4), np.eye(6))
    with pytest.raises(ValueError):
        M.check(g)
