"""Pose-graph optimisation, stated in numpy (float64 throughout): the oracle of r360_graph_* (DESIGN.md §5d).

The reference's include/GraphOptimizer.h holds g2o VertexSE3 / EdgeSE3 and runs OptimizationAlgorithmLevenberg over
LinearSolverDense, optimize(10).  g2o is not vendored there, so the algorithm is restated here and not pinned:

  vertex    T_k = [R_k, t_k], world from keyframe; the rotation block is used as given; inverse = [R^T, -R^T t]
  edge      (i, j, Z, Omega) with T_j ~ T_i Z; Omega 6x6 ordered (translation, rotation), symmetrised on intake
  residual  E = Z^-1 T_i^-1 T_j = [R_E, t_E], e = [t_E ; log_SO3(R_E)], F = sum e^T Omega e
  increment T [+] d = T [Exp(d_w), d_t]  (local, on the right)
  solver    Levenberg-Marquardt after g2o over the free vertices; vertex 0 is always fixed

Every 3x3 product is written out with one fixed order of additions, (a0 b0 + a1 b1) + a2 b2, which the kernels
repeat without contraction: a chain whose edges are rel(T_i, T_j) of its own poses then has F == 0 exactly, here
and on the device.
"""
import numpy as np

SMALL_ANGLE = 1e-4          # below it Exp, log and J_r^-1 take their series
STATUS_CONVERGED, STATUS_ITERATION_LIMIT, STATUS_STALLED, STATUS_CG = 0, 1, 2, 3


def mul3(A, B):
    """A @ B for 3x3 (or 3x3 by 3-vector) with the fixed order (a0 b0 + a1 b1) + a2 b2."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    if B.ndim == 1:
        return (A[:, 0] * B[0] + A[:, 1] * B[1]) + A[:, 2] * B[2]
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rel(Ti, Tj):
    """T_i^-1 T_j as (R, t): R = R_i^T R_j, t = R_i^T (t_j - t_i)."""
    Rt = Ti[:3, :3].T
    return mul3(Rt, Tj[:3, :3]), mul3(Rt, Tj[:3, 3] - Ti[:3, 3])


def rel4(Ti, Tj):
    R, t = rel(Ti, Tj)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < SMALL_ANGLE:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        s = np.sin(0.5 * th)
        a, b = np.sin(th) / th, 2.0 * s * s / th2
    K = skew(w)
    return (np.eye(3) + a * K) + b * mul3(K, K)


def log_so3(R):
    """The rotation vector of R; theta from atan2(|v|, (tr - 1) / 2) with v = vee(R - R^T) / 2."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    th = np.arctan2(s, c)
    f = 1.0 + th * th / 6.0 if th < SMALL_ANGLE else th / s
    return f * v


def jr_inv(phi):
    """J_r^-1(phi) = I + 1/2 [phi]x + (1/th^2 - (1 + cos th) / (2 th sin th)) [phi]x^2."""
    th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]
    th = np.sqrt(th2)
    if th < SMALL_ANGLE:
        c = 1.0 / 12.0 + th2 / 720.0
    else:
        c = 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    K = skew(phi)
    return (np.eye(3) + 0.5 * K) + c * mul3(K, K)


def boxplus(T, d):
    """T [Exp(d_w), d_t]."""
    out = np.array(T, np.float64)
    R = T[:3, :3]
    out[:3, :3] = mul3(R, exp_so3(d[3:6]))
    out[:3, 3] = mul3(R, d[0:3]) + T[:3, 3]
    return out


class Graph:
    def __init__(self):
        self.poses, self.fixed, self.edges = [], [], []

    def add_vertex(self, T, fixed=False):
        self.poses.append(np.array(T, np.float64).reshape(4, 4))
        self.fixed.append(bool(fixed) or len(self.poses) == 1)
        return len(self.poses) - 1

    def add_edge(self, i, j, Z, Om):
        Om = np.array(Om, np.float64).reshape(6, 6)
        self.edges.append((int(i), int(j), np.array(Z, np.float64).reshape(4, 4), 0.5 * (Om + Om.T)))

    def copy(self):
        g = Graph()
        g.poses = [p.copy() for p in self.poses]
        g.fixed = list(self.fixed)
        g.edges = list(self.edges)
        return g

    def free_index(self):
        idx, k = [], 0
        for f in self.fixed:
            idx.append(-1 if f else k)
            k += 0 if f else 1
        return idx, k


def edge_terms(Ti, Tj, Z, want_jac=True):
    """e and, if asked, the 6x6 Jacobians (J_i, J_j) of one edge at the poses."""
    RB, tB = rel(Ti, Tj)
    RZt = Z[:3, :3].T
    RE = mul3(RZt, RB)
    tE = mul3(RZt, tB - Z[:3, 3])
    ew = log_so3(RE)
    e = np.concatenate([tE, ew])
    if not want_jac:
        return e, None, None
    Ji = jr_inv(ew)
    Jj = np.zeros((6, 6))
    Jj[:3, :3] = RE
    Jj[3:, 3:] = Ji
    Jiw = np.zeros((6, 6))
    Jiw[:3, :3] = -RZt
    Jiw[:3, 3:] = mul3(RZt, skew(tB))
    Jiw[3:, 3:] = -mul3(Ji, RB.T)
    return e, Jiw, Jj


def cost(g, poses=None):
    poses = g.poses if poses is None else poses
    F = 0.0
    for (i, j, Z, Om) in g.edges:
        e, _, _ = edge_terms(poses[i], poses[j], Z, False)
        F += float(e @ (Om @ e))
    return F


def linearise(g, poses=None):
    """F, b [6 nf], H [6 nf, 6 nf] dense over the free vertices in index order."""
    poses = g.poses if poses is None else poses
    idx, nf = g.free_index()
    H = np.zeros((6 * nf, 6 * nf))
    b = np.zeros(6 * nf)
    F = 0.0
    for (i, j, Z, Om) in g.edges:
        e, Ji, Jj = edge_terms(poses[i], poses[j], Z)
        Oe = Om @ e
        F += float(e @ Oe)
        for (a, Ja) in ((idx[i], Ji), (idx[j], Jj)):
            if a < 0:
                continue
            b[6 * a:6 * a + 6] += Ja.T @ Oe
            for (c, Jc) in ((idx[i], Ji), (idx[j], Jj)):
                if c >= 0:
                    H[6 * a:6 * a + 6, 6 * c:6 * c + 6] += Ja.T @ (Om @ Jc)
    return F, b, H


def apply(g, poses, delta):
    idx, _ = g.free_index()
    return [boxplus(T, delta[6 * k:6 * k + 6]) if k >= 0 else T.copy() for T, k in zip(poses, idx)]


def check(g):
    """The host's input checks; raises ValueError as the library returns R360_EINVAL."""
    n = len(g.poses)
    for T in g.poses:
        if not np.isfinite(T).all():
            raise ValueError("non-finite pose")
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    deg = [0] * n
    for (i, j, Z, Om) in g.edges:
        if not (0 <= i < n and 0 <= j < n) or i == j:
            raise ValueError("bad edge")
        if not (np.isfinite(Z).all() and np.isfinite(Om).all()):
            raise ValueError("non-finite edge")
        deg[i] += 1
        deg[j] += 1
        parent[find(i)] = find(j)
    for k in range(n):
        if not g.fixed[k] and deg[k] == 0:
            raise ValueError("free vertex without an edge")
    anchored = {find(k) for k in range(n) if g.fixed[k]}
    for k in range(n):
        if find(k) not in anchored:
            raise ValueError("component without a fixed vertex")


def optimize(g, max_iterations=10, max_trials=10, gain_epsilon=1e-6, solve=np.linalg.solve):
    """Levenberg-Marquardt after g2o.  Returns (poses, stats); stats['decisions'] lists every accept / reject and
    stop decision as (kind, value, threshold, scale): see undecided()."""
    check(g)
    poses = [p.copy() for p in g.poses]
    st = dict(status=STATUS_CONVERGED, iterations=0, trials=0, F0=0.0, F=0.0, lam=0.0, decisions=[], F_trace=[],
              b0=0.0, lam0=0.0)
    _, nf = g.free_index()
    if nf == 0 or not g.edges:
        st["F0"] = st["F"] = cost(g, poses)
        return poses, st
    F, b, H = linearise(g, poses)
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
            trial = apply(g, poses, delta)
            F1 = cost(g, trial)
            rho = (F - F1) / float(delta @ (lam * delta - b))
            st["trials"] += 1
            st["decisions"].append(("rho", rho, 0.0, 1.0))
            st["decisions"].append(("sign", F - F1, 0.0, 1e-3 * F))
            if np.isfinite(F1) and rho > 0.0:
                lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu = 2.0
                accepted = True
                break
            lam *= nu
            nu *= 2.0
        st["lam"] = lam
        if not accepted:
            st["status"] = STATUS_STALLED
            break
        st["iterations"] += 1
        gain, Fold = F - F1, F
        poses, F = trial, F1
        st["F"] = F
        st["F_trace"].append(F)
        st["decisions"].append(("gain", gain, gain_epsilon * Fold, Fold))
        if gain <= gain_epsilon * Fold:
            st["status"] = STATUS_CONVERGED
            break
        if it == max_iterations - 1:
            st["status"] = STATUS_ITERATION_LIMIT
            break
        F, b, H = linearise(g, poses)
    st["b_final"] = float(np.max(np.abs(linearise(g, poses)[1])))
    return poses, st


def undecided(st):
    """The decisions that rounding could turn.  rho > 0: rho is at least 1e-9 from 0, and F - F' is at least 1e-12
    of F, four orders above the rounding of an fp64 sum of this size.  The gain stop: F - F' is at least 1e-9 of F
    away from gain_epsilon F, which is stricter than 1e-9 of the threshold itself."""
    return [d for d in st["decisions"] if abs(d[1] - d[2]) < 1e-9 * d[3]]


# ---------------------------------------------------------------------------- g2o text (the reference's saveGraph)
def quat_of(R):
    """Shepperd's method, (qx, qy, qz, qw) with qw >= 0."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    d = [R[0, 0], R[1, 1], R[2, 2], tr]
    k = int(np.argmax(d))
    if k == 3:
        qw = 0.5 * np.sqrt(1.0 + tr)
        s = 0.25 / qw
        q = [(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s, qw]
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        qi = 0.5 * np.sqrt(((1.0 + R[i, i]) - R[j, j]) - R[l, l])
        s = 0.25 / qi
        q = [0.0, 0.0, 0.0, (R[l, j] - R[j, l]) * s]
        q[i], q[j], q[l] = qi, (R[j, i] + R[i, j]) * s, (R[l, i] + R[i, l]) * s
    q = np.array(q)
    return -q if q[3] < 0 else q


def rot_of(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
