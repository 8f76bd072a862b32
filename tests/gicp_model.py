"""The statement of the library's Generalized-ICP as plain numpy + scipy.spatial.cKDTree, in float64
on the float32 inputs.  pcl::GeneralizedIterativeClosestPoint restated (PCL is not pinned), with a Gauss-Newton inner
solve where PCL runs BFGS.  Parameters carry PCL's names.  Not a test module: tests import it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.spatial import cKDTree

WORKERS = 1   # threads of the k-d tree queries (tools/gicp_bench.py raises it; the results do not depend on it)


@dataclass
class Params:
    k_correspondences: int = 20
    gicp_epsilon: float = 1e-3
    max_corr_dist: float = 0.4
    max_iterations: int = 10
    max_inner_iterations: int = 20
    rotation_epsilon: float = 2e-3
    transformation_epsilon: float = 1e-9

    def as_float32(self) -> "Params":
        """The values the C ABI's float fields hold (gicp_epsilon, max_corr_dist)."""
        return Params(self.k_correspondences, float(np.float32(self.gicp_epsilon)), float(np.float32(self.max_corr_dist)),
                      self.max_iterations, self.max_inner_iterations, self.rotation_epsilon, self.transformation_epsilon)


def exp_se3(mu) -> np.ndarray:
    """exp of se(3), mu = (v, w): the closed form of CPose3D::exp (r360_exp_se3 with pseudo = 0), 4x4 float64."""
    mu = np.asarray(mu, np.float64)
    v, w = mu[:3], mu[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-6:
        A, B, Cc = 1 - th2 / 6, 0.5 - th2 / 24, 1.0 / 6 - th2 / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * (W @ W)
    T[:3, 3] = (np.eye(3) + B * W + Cc * (W @ W)) @ v
    return T


def intake(xyz, k: int) -> np.ndarray:
    """Rows with a non-finite coordinate dropped, order kept; fewer than k finite points is an error."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    kept = xyz[np.isfinite(xyz).all(axis=1)]
    if kept.shape[0] < k:
        raise ValueError(f"{kept.shape[0]} finite points, fewer than k_correspondences = {k}")
    return kept


def _sorted_neighbours(P: np.ndarray, tree: cKDTree, Q: np.ndarray, k: int):
    """For each row of Q (float64) the k nearest rows of P by (squared distance, index), plus the squared distance of
    the next one (inf if none): (idx [m,k], d2 [m,k], d2_next [m])."""
    n = P.shape[0]
    kk = min(n, k + 8)
    _, cand = tree.query(Q, k=kk, workers=WORKERS)
    cand = cand.reshape(Q.shape[0], kk)
    dd = ((P[cand] - Q[:, None, :]) ** 2).sum(axis=2)
    o = np.lexsort((cand, dd), axis=1)
    cs = np.take_along_axis(cand, o, axis=1)
    ds = np.take_along_axis(dd, o, axis=1)
    idx, d2 = cs[:, :k].copy(), ds[:, :k].copy()
    nxt = ds[:, k].copy() if kk > k else np.full(Q.shape[0], np.inf)
    if kk < n:
        # equal distances from the (k+1)-th candidate to the last: the tie may reach past the candidates, so all pairs
        for i in np.nonzero(ds[:, kk - 1] == ds[:, k])[0]:
            da = ((P - Q[i]) ** 2).sum(axis=1)
            oa = np.lexsort((np.arange(n), da))
            idx[i], d2[i], nxt[i] = oa[:k], da[oa[:k]], da[oa[k]]
    return idx, d2, nxt


def knn(xyz: np.ndarray, k: int):
    """Each point's k nearest points of its own cloud (itself included at distance 0, ties to the lower index), in
    ascending (distance, index) order: (idx [n,k], d2 [n,k], d2 of the (k+1)-th [n])."""
    P = xyz.astype(np.float64)
    return _sorted_neighbours(P, cKDTree(P), P, k)


def covariances(xyz: np.ndarray, k: int, eps: float):
    """C_i = V diag(eps, 1, 1) V^T of each point's k-neighbourhood: (C [n,3,3], eigenvalues ascending [n,3], knn)."""
    P = xyz.astype(np.float64)
    idx, d2, nxt = knn(xyz, k)
    nb = P[idx]                                  # [n,k,3]
    d = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", d, d) / k
    lam, V = np.linalg.eigh(cov)
    v0 = V[:, :, 0]
    C = np.eye(3)[None] - (1.0 - eps) * v0[:, :, None] * v0[:, None, :]
    return C, lam, (idx, d2, nxt)


def nearest(T: np.ndarray, tree: cKDTree, Q: np.ndarray):
    """Nearest row of T for each row of Q, ties to the lower index: (j [m], d2 [m], d2 of the second nearest [m])."""
    k = min(2, T.shape[0])
    idx, d2, nxt = _sorted_neighbours(T, tree, Q, k)
    second = d2[:, 1] if k == 2 else nxt
    return idx[:, 0], d2[:, 0], second


class Cloud:
    def __init__(self, xyz, p: Params):
        self.xyz = intake(xyz, p.k_correspondences)
        self.P = self.xyz.astype(np.float64)
        self.tree = cKDTree(self.P)
        self.C, self.lam, (self.knn, self.knn_d2, self.knn_next) = covariances(self.xyz, p.k_correspondences, p.gicp_epsilon)


def correspondences(src: Cloud, tgt: Cloud, X: np.ndarray, p: Params):
    """(j [n] with -1 for none, M [n,3,3], d2 [n], second-nearest d2 [n]) at pose X."""
    R, t = X[:3, :3], X[:3, 3]
    Q = src.P @ R.T + t
    j, d2, second = nearest(tgt.P, tgt.tree, Q)
    ok = d2 < p.max_corr_dist ** 2
    S = tgt.C[j] + R[None] @ src.C @ R.T[None]
    M = np.linalg.inv(S)
    return np.where(ok, j, -1), M, d2, second


def evaluate(src: Cloud, tgt: Cloud, Y: np.ndarray, corr: np.ndarray, M: np.ndarray):
    """f, g [6], H [6,6] and the count at pose Y for fixed correspondences and weights."""
    ok = corr >= 0
    if not ok.any():
        return 0.0, np.zeros(6), np.zeros((6, 6)), 0
    s = src.P[ok]
    q = tgt.P[corr[ok]]
    Mi = M[ok]
    pY = s @ Y[:3, :3].T + Y[:3, 3]
    r = pY - q
    n = s.shape[0]
    J = np.zeros((n, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 0, 4] = pY[:, 2]; J[:, 0, 5] = -pY[:, 1]
    J[:, 1, 3] = -pY[:, 2]; J[:, 1, 5] = pY[:, 0]
    J[:, 2, 3] = pY[:, 1]; J[:, 2, 4] = -pY[:, 0]
    Mr = np.einsum("nij,nj->ni", Mi, r)
    f = float(np.einsum("ni,ni->", r, Mr))
    g = np.einsum("nia,ni->a", J, Mr)
    H = np.einsum("nia,nij,njb->ab", J, Mi, J)
    return f, g, H, n


def eval_at(src: Cloud, tgt: Cloud, X, p: Params):
    """What r360_gicp_eval returns at X: (corr, f, H, g, n_corr) plus (d2, second-nearest d2) for the decided test."""
    X = np.asarray(X, np.float64)
    corr, M, d2, second = correspondences(src, tgt, X, p)
    f, g, H, n = evaluate(src, tgt, X, corr, M)
    return corr, f, H, g, n, d2, second


def fitness(src: Cloud, tgt: Cloud, X) -> float:
    X = np.asarray(X, np.float64)
    _, d2, _ = nearest(tgt.P, tgt.tree, src.P @ X[:3, :3].T + X[:3, 3])
    return float(d2.mean())


@dataclass
class Result:
    pose: np.ndarray
    status: int
    iterations: int
    converged: bool
    inner_steps: int
    inner_per_iteration: list
    n_corr: int
    cost: float
    fitness: float


def align(src: Cloud, tgt: Cloud, init, p: Params) -> Result:
    """The outer iteration.  status 1: ill-posed (no correspondence, or a singular system in the first inner step)."""
    X = np.asarray(init, np.float64).copy()
    iterations, converged, inner_total, per_it, status = 0, False, 0, [], 0
    n_corr, cost = 0, 0.0
    while True:
        corr, M, _, _ = correspondences(src, tgt, X, p)
        Y = X.copy()
        f, g, H, n = evaluate(src, tgt, Y, corr, M)
        n_corr, cost = n, (f / n if n else 0.0)
        if n == 0:
            status = 1
            break
        steps = 0
        while steps < p.max_inner_iterations:
            try:
                d = -np.linalg.solve(H, g)
            except np.linalg.LinAlgError:
                d = np.full(6, np.nan)
            if not np.isfinite(d).all():
                if steps == 0:
                    status = 1
                break
            if np.abs(d).max() < 1e-10:
                break
            E = exp_se3(d).astype(np.float32).astype(np.float64)   # the library's exp_se3 returns float32
            Yc = E @ Y
            fc, gc, Hc, _ = evaluate(src, tgt, Yc, corr, M)
            if not fc < f:
                break
            Y, f, g, H = Yc, fc, gc, Hc
            steps += 1
        if status:
            break
        cost = f / n
        inner_total += steps
        per_it.append(steps)
        dR = np.abs(Y[:3, :3] - X[:3, :3]).max()
        dt = np.abs(Y[:3, 3] - X[:3, 3]).max()
        X = Y
        iterations += 1
        if iterations >= p.max_iterations:
            break
        if dR < p.rotation_epsilon and dt < p.transformation_epsilon:
            converged = True
            break
    return Result(X, status, iterations, converged, inner_total, per_it, n_corr, cost, fitness(src, tgt, X))


def rot_angle(A, B) -> float:
    """Angle of A^T B from its skew part and trace with atan2: arccos of the trace alone loses half the digits near
    zero, where a float32 pose's rounding (6e-8 per entry) would read as 3e-4 rad."""
    R = np.asarray(A, np.float64)[:3, :3].T @ np.asarray(B, np.float64)[:3, :3]
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), (np.trace(R) - 1) / 2))
