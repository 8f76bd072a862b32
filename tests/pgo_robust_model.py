"""Robust kernels and the active set of the pose-graph optimiser, stated in numpy over pgo_model: the
oracle of r360_graph_set_edge_kernel / _set_edge_active / _edge_stats and of eval, solve and optimize with them.

Per edge a kind and a width delta > 0.  With c = e^T Omega e (delta applies to sqrt(c), as in g2o's RobustKernelHuber
and RobustKernelCauchy):

  NONE    rho(c) = c                                                   w = rho'(c) = 1
  HUBER   rho(c) = c for c <= delta^2, else 2 delta sqrt(c) - delta^2  w = 1, else delta / sqrt(c)
  CAUCHY  rho(c) = delta^2 log1p(c / delta^2)                          w = 1 / (1 + c / delta^2)

F = sum rho(c); an edge adds Ja^T (w Omega e) to b and Ja^T ((w Omega) Jc) to H (no second-order term, as in g2o);
Levenberg-Marquardt is pgo_model.optimize's with the robust F.  An inactive edge does not exist: the model runs on
the graph without it.  kernels is a list of (kind, delta) per edge (None = NONE everywhere), active a list of bools
(None = all)."""
import numpy as np

import pgo_model as M

NONE, HUBER, CAUCHY = 0, 1, 2


def rho(kind, delta, c):
    """(rho(c), w)."""
    if kind == NONE:
        return c, 1.0
    d2 = delta * delta
    if kind == HUBER:
        if c <= d2:
            return c, 1.0
        s = np.sqrt(c)
        return 2.0 * delta * s - d2, delta / s
    if kind == CAUCHY:
        q = c / d2
        return d2 * np.log1p(q), 1.0 / (1.0 + q)
    raise ValueError("unknown kernel")


def _kernels(g, kernels):
    return [(NONE, 1.0)] * len(g.edges) if kernels is None else list(kernels)


def subgraph(g, kernels=None, active=None):
    """The graph of the active edges and their kernels."""
    kernels = _kernels(g, kernels)
    if active is None:
        return g, kernels
    h = g.copy()
    h.edges = [e for e, a in zip(g.edges, active) if a]
    return h, [k for k, a in zip(kernels, active) if a]


def edge_stats(g, kernels=None, active=None, poses=None):
    """chi2 and w of every edge at the poses; an inactive edge has its chi2 and w = 0."""
    poses = g.poses if poses is None else poses
    chi2, w = [], []
    for k, ((i, j, Z, Om), (kind, delta)) in enumerate(zip(g.edges, _kernels(g, kernels))):
        e, _, _ = M.edge_terms(poses[i], poses[j], Z, False)
        c = float(e @ (Om @ e))
        chi2.append(c)
        w.append(float(rho(kind, delta, c)[1]) if active is None or active[k] else 0.0)
    return np.array(chi2), np.array(w)


def cost(g, kernels=None, poses=None, active=None):
    g, kernels = subgraph(g, kernels, active)
    poses = g.poses if poses is None else poses
    F = 0.0
    for (i, j, Z, Om), (kind, delta) in zip(g.edges, kernels):
        e, _, _ = M.edge_terms(poses[i], poses[j], Z, False)
        F += float(rho(kind, delta, float(e @ (Om @ e)))[0])
    return F


def linearise(g, kernels=None, poses=None, active=None):
    """F, b [6 nf], H [6 nf, 6 nf] as pgo_model.linearise, with every edge's Omega e and Omega scaled by its w."""
    g, kernels = subgraph(g, kernels, active)
    poses = g.poses if poses is None else poses
    idx, nf = g.free_index()
    H = np.zeros((6 * nf, 6 * nf))
    b = np.zeros(6 * nf)
    F = 0.0
    for (i, j, Z, Om), (kind, delta) in zip(g.edges, kernels):
        e, Ji, Jj = M.edge_terms(poses[i], poses[j], Z)
        Oe = Om @ e
        r, w = rho(kind, delta, float(e @ Oe))
        F += float(r)
        Oe = w * Oe
        Om = w * Om
        for (a, Ja) in ((idx[i], Ji), (idx[j], Jj)):
            if a < 0:
                continue
            b[6 * a:6 * a + 6] += Ja.T @ Oe
            for (c, Jc) in ((idx[i], Ji), (idx[j], Jj)):
                if c >= 0:
                    H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += Ja.T @ (Om @ Jc)
    return F, b, H


def optimize(g, kernels=None, active=None, max_iterations=10, max_trials=10, gain_epsilon=1e-6, solve=np.linalg.solve):
    """pgo_model.optimize, line for line, over the active edges with the robust F, b and H.  The same stats dict."""
    g, kernels = subgraph(g, kernels, active)
    M.check(g)
    poses = [p.copy() for p in g.poses]
    st = dict(status=M.STATUS_CONVERGED, iterations=0, trials=0, F0=0.0, F=0.0, lam=0.0, decisions=[], F_trace=[],
              b0=0.0, lam0=0.0)
    _, nf = g.free_index()
    if nf == 0 or not g.edges:
        st["F0"] = st["F"] = cost(g, kernels, poses)
        return poses, st
    F, b, H = linearise(g, kernels, poses)
    st["F0"] = st["F"] = F
    st["F_trace"].append(F)
    st["b0"] = float(np.max(np.abs(b)))
    lam = 1e-5 * float(np.max(np.diag(H)))
    st["lam0"] = st["lam"] = lam
    nu = 2.0
    if F == 0.0 or st["b0"] == 0.0:
        return poses, st
    N = 6 * nf
    for it in range(max_iterations):
        accepted = False
        for _ in range(max_trials):
            delta = solve(H + lam * np.eye(N), -b)
            trial = M.apply(g, poses, delta)
            F1 = cost(g, kernels, trial)
            rho_gain = (F - F1) / float(delta @ (lam * delta - b))
            st["trials"] += 1
            st["decisions"].append(("rho", rho_gain, 0.0, 1.0))
            st["decisions"].append(("sign", F - F1, 0.0, 1e-3 * F))
            if np.isfinite(F1) and rho_gain > 0.0:
                lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho_gain - 1.0) ** 3)
                nu = 2.0
                accepted = True
                break
            lam *= nu
            nu *= 2.0
        st["lam"] = lam
        if not accepted:
            st["status"] = M.STATUS_STALLED
            break
        st["iterations"] += 1
        gain, Fold = F - F1, F
        poses, F = trial, F1
        st["F"] = F
        st["F_trace"].append(F)
        st["decisions"].append(("gain", gain, gain_epsilon * Fold, Fold))
        if gain <= gain_epsilon * Fold:
            st["status"] = M.STATUS_CONVERGED
            break
        if it == max_iterations - 1:
            st["status"] = M.STATUS_ITERATION_LIMIT
            break
        F, b, H = linearise(g, kernels, poses)
    st["b_final"] = float(np.max(np.abs(linearise(g, kernels, poses)[1])))
    return poses, st
