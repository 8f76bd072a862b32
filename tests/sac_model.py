"""The statement of record of the RANSAC plane segmentation (pcl::SACSegmentation with SACMODEL_PLANE,
SACMODEL_PERPENDICULAR_PLANE, SACMODEL_PARALLEL_PLANE and SAC_RANSAC, and the peel loop of PCL's cluster-extraction
recipe; PCL is not pinned): brute force, numpy float64.  The library follows it.  Everything is
float64 of the float32 inputs, left to right, each operation rounded once.

  * a row with a non-finite coordinate is dropped: label -1, never sampled, never an inlier; n_finite counts the others;
  * plane of three points: u = p1 - p0, v = p2 - p0, n = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx),
    s = (nx^2 + ny^2) + nz^2; degenerate (scored 0, coefficients NaN) iff s is not a finite number > 0; otherwise
    n /= sqrt(s), d = -((nx p0x + ny p0y) + nz p0z);
  * distance |((a x + b y) + c z) + d|; inlier iff distance <= float64(float32(distance_threshold)) (closed);
  * normals gate (normals [n, 3] float32 given): an inlier also needs |(nx a + ny b) + nz c| >=
    math.cos(float64(float32(normal_angle))); a row whose normal has a non-finite component is never an inlier and stays
    in the pool;
  * axis constraint, with â = axis / sqrt((ax^2 + ay^2) + az^2) in float64: PERPENDICULAR |n.â| >= math.cos(eps),
    PARALLEL |n.â| <= math.sin(eps), n.â = (nx âx + ny ây) + nz âz; a hypothesis that fails scores 0 (NaN);
  * sampling: mix / draw / sample3 below; positions index the pool, the remaining rows in ascending input index;
  * search: rounds of ROUND hypotheses; after each round best = the highest count so far (ties to the lowest h),
    w = best / m, q = 1 - (w w) w clipped to [EPS, 1 - EPS], k = math.log(1 - probability) / math.log(q); go on while
    evaluated < max_iterations and evaluated < k;
  * refinement (optimize, best count >= 3): mean and covariance (two passes, / size) of the best hypothesis' inliers;
    the unit eigenvector of the smallest eigenvalue is the normal, d = -((nx mx + ny my) + nz mz); the inliers are
    selected again from the pool.  The refined plane is not re-checked against the constraint;
  * peel: for p = 0, 1, ... stop when p = max_planes, pool < max(3, min_inliers), float(pool) <= stop_fraction * n_finite,
    or the plane found has fewer than min_inliers final inliers (not recorded, its points stay unlabelled); otherwise the
    final inliers get label p and leave the pool;
  * record: coef oriented (the largest-magnitude component of the normal positive, ties to the lower axis, all four
    negated together), size, raw_size, best_hypothesis, evaluated, and centroid, eig ascending, curvature of the final
    inliers as tests/cluster_model.py computes them.

What a comparison needs in order to know that it is decided
  * near_pairs: the (point, hypothesis) pairs scored whose distance or gate value lies within BAND of its threshold, plus
    the hypotheses whose constraint value does;
  * near_refined: after refinement, the points within REF_BAND of a threshold;
  * per plane `rounds`: (evaluated, k) at every round boundary.
All three include the last search of a peel, whose plane was found too small.
"""
import math
import sys
from dataclasses import dataclass, field

import numpy as np

ROUND = 128
NONE, PERPENDICULAR, PARALLEL = 0, 1, 2
BAND = 1e-12
REF_BAND = 1e-9
EPS = sys.float_info.epsilon
M64 = (1 << 64) - 1
DEFAULTS = dict(distance_threshold=0.05, max_iterations=1024, probability=0.99, optimize=1, constraint=NONE,
                axis=(0.0, 0.0, 1.0), eps_angle=math.radians(10.0), normal_angle=math.radians(10.0), max_planes=8,
                min_inliers=100, stop_fraction=0.0, seed=0)


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, p, h, j, m):
    u = mix(mix(mix(mix(seed & M64) ^ p) ^ h) ^ j)
    return (u * m) >> 64


def sample3(seed, p, h, m):
    """Three distinct pool positions in [0, m), m >= 3, in sample order."""
    a, b, c = draw(seed, p, h, 0, m), draw(seed, p, h, 1, m - 1), draw(seed, p, h, 2, m - 2)
    if b >= a:
        b += 1
    lo, hi = min(a, b), max(a, b)
    if c >= lo:
        c += 1
    if c >= hi:
        c += 1
    return a, b, c


def planes3(p0, p1, p2):
    """[H, 4] float64 coefficients of the planes through float32 triples [H, 3]; NaN rows where degenerate."""
    p0, p1, p2 = (np.asarray(a, np.float32).reshape(-1, 3).astype(np.float64) for a in (p0, p1, p2))
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        ok = np.isfinite(s) & (s > 0)
        r = np.sqrt(s)
        nx, ny, nz = nx / r, ny / r, nz / r
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
    coef = np.stack([nx, ny, nz, d], 1)
    coef[~ok] = np.nan
    return coef


def orient(coef):
    """The record's sign: the largest-magnitude component of the normal positive, ties to the lower axis."""
    coef = np.array(coef, np.float64)
    lead = int(np.argmax(np.abs(coef[:3])))
    return -coef if coef[lead] < 0 else coef


class _Cloud:
    def __init__(self, xyz, normals, prm):
        self.xyz32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.n = self.xyz32.shape[0]
        self.fin = np.isfinite(self.xyz32).all(axis=1)
        self.p = self.xyz32.astype(np.float64)
        self.thr = float(np.float64(np.float32(prm["distance_threshold"])))
        self.nrm = None
        if normals is not None:
            n32 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            assert n32.shape[0] == self.n
            self.nfin = np.isfinite(n32).all(axis=1)
            self.nrm = n32.astype(np.float64)
            self.cos_n = math.cos(float(np.float64(np.float32(prm["normal_angle"]))))

    def inliers(self, idx, coef, band):
        """[H, len(idx)] bool inlier matrix of the rows idx for coefficients [H, 4], and the same shape `near`."""
        coef = np.asarray(coef, np.float64).reshape(-1, 4)
        a, b, c, d = (coef[:, k:k + 1] for k in range(4))
        x, y, z = (self.p[idx, k][None, :] for k in range(3))
        with np.errstate(all="ignore"):
            dist = np.abs(((a * x + b * y) + c * z) + d)
            inl = dist <= self.thr
            near = np.abs(dist - self.thr) <= band
            if self.nrm is not None:
                nx, ny, nz = (self.nrm[idx, k][None, :] for k in range(3))
                g = np.abs((nx * a + ny * b) + nz * c)
                ok = self.nfin[idx][None, :]
                near = (near & ok) | (inl & ok & (np.abs(g - self.cos_n) <= band))
                inl = inl & ok & (g >= self.cos_n)
        return inl, near


def _constraint(prm):
    if prm["constraint"] == NONE:
        return None
    ax = np.asarray(prm["axis"], np.float32).astype(np.float64)
    ln = math.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
    eps = float(np.float64(np.float32(prm["eps_angle"])))
    return ax / ln, math.cos(eps), math.sin(eps)


def hypotheses(C, pool, prm, p, h0, nh):
    """Hypotheses h0 .. h0 + nh of plane p over `pool`: samples [nh, 3] input indices, coef [nh, 4] (NaN when scored 0),
    and the number of constraint values within BAND of their threshold."""
    m = len(pool)
    seed = int(prm["seed"])
    pos = np.array([sample3(seed, p, h, m) for h in range(h0, h0 + nh)], np.int64).reshape(-1, 3)
    samples = pool[pos]
    coef = planes3(C.xyz32[samples[:, 0]], C.xyz32[samples[:, 1]], C.xyz32[samples[:, 2]])
    near = 0
    con = _constraint(prm)
    if con is not None:
        ax, ce, se = con
        with np.errstate(invalid="ignore"):
            dot = np.abs((coef[:, 0] * ax[0] + coef[:, 1] * ax[1]) + coef[:, 2] * ax[2])
            if prm["constraint"] == PERPENDICULAR:
                ok, t = dot >= ce, ce
            else:
                ok, t = dot <= se, se
            near = int((np.abs(dot - t) <= BAND).sum())
        coef[~ok] = np.nan
    return samples.astype(np.int32), coef, near


def moments(p):
    """Centroid, eigenvalues ascending, the unit eigenvector of eig[0], curvature, and the comparison bounds of
    tests/cluster_model.py for the float64 points p [c, 3], c >= 1."""
    c = p.shape[0]
    mean = p.sum(0) / float(c)
    sum_bound = (c - 1) * 2.0 ** -53 * np.abs(p).sum(0)
    d = p - mean
    prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                      d[:, 2] * d[:, 2]], 1)
    cov_bound = (c - 1) * 2.0 ** -53 * np.abs(prods).sum(0).max()
    out = dict(centroid=mean, eig=np.full(3, np.nan), normal=np.full(3, np.nan), curvature=np.nan, sum_bound=sum_bound,
               cov_bound=cov_bound, eig_decided=False)
    if c >= 3:
        s = prods.sum(0) / float(c)
        cov = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
        lam, vec = np.linalg.eigh(cov)
        tr = (lam[0] + lam[1]) + lam[2]
        out.update(eig=lam, normal=vec[:, 0].copy(), curvature=0.0 if tr == 0.0 else abs(lam[0]) / tr,
                   eig_decided=bool(lam[2] > 0 and (lam[1] - lam[0]) >= 1e-5 * lam[2]))
    return out


@dataclass
class Plane:
    coef: np.ndarray             # [4] oriented
    size: int
    raw_size: int
    best_hypothesis: int
    evaluated: int
    k: float
    rounds: list                 # (evaluated, k) per round boundary
    inliers: np.ndarray          # final inliers, ascending input indices
    centroid: np.ndarray
    eig: np.ndarray
    curvature: float
    sum_bound: np.ndarray
    cov_bound: float
    eig_decided: bool
    refined: bool
    fit: dict = field(default_factory=dict)     # moments() of the best hypothesis' inliers (the refinement's input)


@dataclass
class SacResult:
    labels: np.ndarray
    planes: list
    last: "Plane | None"         # the search that ended the peel by finding too small a plane
    n_in: int
    n_finite: int
    n_evaluated: int
    near_pairs: int
    near_refined: int

    @property
    def n_planes(self):
        return len(self.planes)

    @property
    def n_in_planes(self):
        return int((self.labels >= 0).sum())

    def k_decided(self):
        """Every round boundary's comparison of `evaluated` with k is decided."""
        every = self.planes + ([self.last] if self.last is not None else [])
        return all(abs(k - ev) > 1e-9 * k for pl in every for ev, k in pl.rounds)


def params(**kw):
    prm = dict(DEFAULTS)
    prm.update(kw)
    assert np.isfinite(prm["distance_threshold"]) and prm["distance_threshold"] > 0
    assert 1 <= prm["max_iterations"] <= 65536 and 0 < prm["probability"] < 1 and 1 <= prm["max_planes"] <= 64
    assert prm["min_inliers"] >= 3 and 0 <= prm["stop_fraction"] < 1 and prm["constraint"] in (NONE, PERPENDICULAR, PARALLEL)
    return prm


def search(C, pool, prm, p):
    """One plane over `pool`: (best count, best h, its coefficients, evaluated, rounds, near_pairs)."""
    m = len(pool)
    log_fail = math.log(1.0 - float(np.float64(np.float32(prm["probability"]))))
    best, best_h, best_coef = -1, 0, np.full(4, np.nan)
    evaluated, rounds, near_pairs = 0, [], 0
    while True:
        nh = min(ROUND, prm["max_iterations"] - evaluated)
        _, coef, near_c = hypotheses(C, pool, prm, p, evaluated, nh)
        inl, near = C.inliers(pool, coef, BAND)
        near_pairs += int(near.sum()) + near_c
        count = inl.sum(1)
        t = int(np.argmax(count))                       # the first maximum: ties to the lowest h
        if int(count[t]) > best:
            best, best_h, best_coef = int(count[t]), evaluated + t, coef[t].copy()
        evaluated += nh
        w = best / m
        q = min(max(1.0 - (w * w) * w, EPS), 1.0 - EPS)
        k = log_fail / math.log(q)
        rounds.append((evaluated, k))
        if not (evaluated < prm["max_iterations"] and evaluated < k):
            break
    return best, best_h, best_coef, evaluated, rounds, near_pairs


def segment(xyz, normals=None, **kw):
    prm = params(**kw)
    C = _Cloud(xyz, normals, prm)
    labels = np.full(C.n, -1, np.int32)
    pool = np.flatnonzero(C.fin)
    nf = len(pool)
    planes, last = [], None
    n_evaluated = near_pairs = near_refined = 0
    stop = float(np.float64(np.float32(prm["stop_fraction"])))
    for p in range(prm["max_planes"]):
        m = len(pool)
        if m < max(3, prm["min_inliers"]) or float(m) <= stop * nf:
            break
        best, best_h, coef, evaluated, rounds, near = search(C, pool, prm, p)
        n_evaluated += evaluated
        near_pairs += near
        sel = C.inliers(pool, coef, BAND)[0][0]
        assert int(sel.sum()) == best
        refined = bool(prm["optimize"]) and best >= 3
        fit = {}
        if refined:
            fit = moments(C.p[pool[sel]])
            nrm = fit["normal"]
            coef = np.array([nrm[0], nrm[1], nrm[2], -((nrm[0] * fit["centroid"][0] + nrm[1] * fit["centroid"][1])
                                                       + nrm[2] * fit["centroid"][2])])
            sel, nr = C.inliers(pool, coef, REF_BAND)
            sel = sel[0]
            near_refined += int(nr.sum())
        idx = pool[sel]
        size = len(idx)
        mo = moments(C.p[idx]) if size else dict(centroid=np.full(3, np.nan), eig=np.full(3, np.nan), curvature=np.nan,
                                                 sum_bound=np.zeros(3), cov_bound=0.0, eig_decided=False)
        pl = Plane(coef=orient(coef), size=size, raw_size=best, best_hypothesis=best_h, evaluated=evaluated, k=rounds[-1][1],
                   rounds=rounds, inliers=idx, centroid=mo["centroid"], eig=mo["eig"], curvature=mo["curvature"],
                   sum_bound=mo["sum_bound"], cov_bound=mo["cov_bound"], eig_decided=mo["eig_decided"], refined=refined,
                   fit=fit)
        if size < prm["min_inliers"]:
            last = pl
            break
        labels[idx] = p
        planes.append(pl)
        pool = pool[~sel]
    return SacResult(labels=labels, planes=planes, last=last, n_in=C.n, n_finite=nf, n_evaluated=n_evaluated,
                     near_pairs=near_pairs, near_refined=near_refined)


def evaluate(xyz, normals=None, n_hyp=ROUND, coef_in=None, **kw):
    """The parity hook of plane 0 over the whole finite cloud: (samples [n_hyp, 3], coef [n_hyp, 4], count [n_hyp],
    near_pairs).  With coef_in the coefficients are scored as given and samples are -1."""
    prm = params(**kw)
    C = _Cloud(xyz, normals, prm)
    pool = np.flatnonzero(C.fin)
    near_c = 0
    if coef_in is not None:
        coef = np.asarray(coef_in, np.float64).reshape(-1, 4).copy()
        n_hyp = coef.shape[0]
        samples = np.full((n_hyp, 3), -1, np.int32)
    elif len(pool) < 3:
        return np.full((n_hyp, 3), -1, np.int32), np.full((n_hyp, 4), np.nan), np.zeros(n_hyp, np.int32), 0
    else:
        samples, coef, near_c = hypotheses(C, pool, prm, 0, 0, n_hyp)
    count = np.zeros(n_hyp, np.int32)
    near = near_c
    for h0 in range(0, n_hyp, ROUND):
        inl, nr = C.inliers(pool, coef[h0:h0 + ROUND], BAND)
        count[h0:h0 + ROUND] = inl.sum(1)
        near += int(nr.sum())
    return samples, coef, count, near
