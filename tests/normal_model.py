"""The statement of record of the surface normals (pcl::NormalEstimation, restated from PCL 1.7 features/normal_3d.h,
unpinned): brute force, O(n^2), numpy float64.  The library follows it.

  * a row with a non-finite coordinate is dropped: normal and curvature NaN, count -1, and it is nobody's neighbour;
  * the squared distance of two points is that of tests/outlier_model.py (sq_dists): dx*dx + dy*dy + dz*dz in float64 of
    the float32 coordinates, left to right, each operation rounded once;
  * the neighbourhood of point i is i itself, then its nearest other points with squared distance
    <= float64(float32(radius))^2, at most k in all, in ascending (squared distance, input index) order;
  * one rule covers both PCL modes: a radius beyond the cloud's diameter is setKSearch(k), k = 64 is setRadiusSearch(r)
    for every point with at most 63 others within r.  Unlike PCL the search is always bounded, the neighbourhood is
    capped at 64, ties go to the lower index and the moments are float64 two-pass sums (PCL 1.7: float, one pass);
  * a point with m < 3 neighbours is short: normal and curvature NaN;
  * mean = (sum p_j) / m and C = sum (p_j - mean)(p_j - mean)^T / m, both added in neighbourhood order, one rounding
    per operation (products of two factors, no fused multiply-add);
  * l0 <= l1 <= l2 the eigenvalues of C (numpy.linalg.eigh), n the unit eigenvector of l0,
    curvature = |l0| / ((l0 + l1) + l2), 0 when the trace is 0;
  * orientation (flipNormalTowardsViewpoint): v = the nearest viewpoint by the same squared distance, ties to the lower
    index; n is negated iff ((vx-px)*nx + (vy-py)*ny) + (vz-pz)*nz < 0;
  * the float32 outputs are the float32 of the float64 values.

Decided points (what a comparison with another implementation may rely on)
  * knn_decided: the neighbourhood was not cut by k, or the last pair taken and the first one left out are equal (the
    index rule decides, exactly) or at least KNN_REL of the latter apart.  Both sides form the distances with the same
    operations, so the band 0 < gap < KNN_REL * d2 is empty in practice;
  * eig_decided: knn_decided, l2 > 0, (l1 - l0) >= 1e-5 * l2 (the eigenvector of l0 is conditioned by l2 / (l1 - l0)) and
    |(v - p) . n| >= 1e-9 * |v - p| (the flip is decided).
"""
from dataclasses import dataclass

import numpy as np

from outlier_model import sq_dists

KNN_REL = 2.0 ** -40
KMIN, KMAX, VIEWMAX = 3, 64, 4096


@dataclass
class NormalResult:
    finite: np.ndarray          # [n] bool
    count: np.ndarray           # [n] int32: m, -1 dropped row
    knn: np.ndarray             # [n, k] int32: the neighbourhood's input indices in its order, -1 padded
    short: np.ndarray           # [n] bool: finite and m < 3
    normal: np.ndarray          # [n, 3] float64, NaN for dropped and short rows
    eig: np.ndarray             # [n, 3] float64 ascending
    curvature: np.ndarray       # [n] float64
    view: np.ndarray            # [n] int32: the nearest viewpoint's index (-1 where there is no normal)
    knn_decided: np.ndarray     # [n] bool
    eig_decided: np.ndarray     # [n] bool

    @property
    def normal32(self):
        return self.normal.astype(np.float32)

    @property
    def curvature32(self):
        return self.curvature.astype(np.float32)

    @property
    def valid(self):
        return self.count >= 3

    def undecided_fraction(self):
        v = self.valid
        return float((v & ~self.eig_decided).sum()) / max(int(v.sum()), 1)


def estimate(xyz, k, radius, viewpoints):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(viewpoints, np.float32).reshape(-1, 3).astype(np.float64)
    assert KMIN <= k <= KMAX and 1 <= len(views) <= VIEWMAX and np.isfinite(radius) and radius > 0
    n = xyz.shape[0]
    fin = np.isfinite(xyz).all(axis=1)
    rows = np.flatnonzero(fin)
    p32 = xyz[rows]
    p = p32.astype(np.float64)
    nf = len(rows)
    lim2 = float(np.float64(np.float32(radius))) ** 2
    count = np.full(n, -1, np.int32)
    knn = np.full((n, k), -1, np.int32)
    local = np.full((nf, k), -1, np.int64)        # the neighbourhoods as rows of p
    m_of = np.zeros(nf, np.int64)
    knn_dec = np.zeros(n, bool)
    for a in range(nf):
        d2 = sq_dists(p32, a)
        d2[a] = np.inf
        order = np.argsort(d2, kind="stable")      # ascending distance, ties to the lower (input) index
        within = int(np.count_nonzero(d2 <= lim2))
        take = min(within, k - 1)
        nb = order[:take]
        m = take + 1
        m_of[a] = m
        local[a, 0] = a
        local[a, 1:m] = nb
        count[rows[a]] = m
        knn[rows[a], 0] = rows[a]
        knn[rows[a], 1:m] = rows[nb]
        if within > take:                          # cut by k: the first pair left out against the last one taken
            last, nxt = d2[order[take - 1]], d2[order[take]]
            knn_dec[rows[a]] = (nxt == last) or (nxt - last) >= KNN_REL * nxt
        else:
            knn_dec[rows[a]] = True
    # moments in neighbourhood order: slot by slot, so every point's sums are sequential
    ok = m_of >= 3
    md = np.maximum(m_of, 1).astype(np.float64)[:, None]
    s = np.zeros((nf, 3))
    for j in range(k):
        use = (j < m_of)[:, None]
        s = s + np.where(use, p[np.maximum(local[:, j], 0)], 0.0)
    mean = s / md
    c = np.zeros((nf, 6))                          # xx xy xz yy yz zz
    for j in range(k):
        use = (j < m_of)[:, None]
        d = p[np.maximum(local[:, j], 0)] - mean
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                         d[:, 2] * d[:, 2]], 1)
        c = c + np.where(use, prod, 0.0)
    c = c / md
    cov = np.zeros((nf, 3, 3))
    cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
    cov[:, 1, 0], cov[:, 1, 1], cov[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
    cov[:, 2, 0], cov[:, 2, 1], cov[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
    lam, vec = np.linalg.eigh(cov) if nf else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    nrm = vec[:, :, 0].copy()
    tr = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(tr == 0.0, 0.0, np.abs(lam[:, 0]) / tr)
    # the nearest viewpoint, ties to the lower index (argmin returns the first minimum)
    dv = views[None, :, :] - p[:, None, :]
    dv2 = (dv[:, :, 0] * dv[:, :, 0] + dv[:, :, 1] * dv[:, :, 1]) + dv[:, :, 2] * dv[:, :, 2]
    vi = np.argmin(dv2, axis=1) if nf else np.zeros(0, np.int64)
    to_v = dv[np.arange(nf), vi]
    dot = (to_v[:, 0] * nrm[:, 0] + to_v[:, 1] * nrm[:, 1]) + to_v[:, 2] * nrm[:, 2]
    nrm[dot < 0] *= -1.0
    with np.errstate(invalid="ignore"):
        dec = ok & (lam[:, 2] > 0) & ((lam[:, 1] - lam[:, 0]) >= 1e-5 * lam[:, 2]) & \
              (np.abs(dot) >= 1e-9 * np.sqrt(dv2[np.arange(nf), vi]))
    normal = np.full((n, 3), np.nan)
    eig = np.full((n, 3), np.nan)
    curvature = np.full(n, np.nan)
    view = np.full(n, -1, np.int32)
    good = rows[ok]
    normal[good], eig[good], curvature[good], view[good] = nrm[ok], lam[ok], curv[ok], vi[ok]
    eig_dec = np.zeros(n, bool)
    eig_dec[rows] = dec
    eig_dec &= knn_dec
    short = fin & (count < 3)
    return NormalResult(finite=fin, count=count, knn=knn, short=short, normal=normal, eig=eig, curvature=curvature,
                        view=view, knn_decided=knn_dec, eig_decided=eig_dec)
