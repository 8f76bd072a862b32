"""The statement of record of the two outlier filters (pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval,
restated from PCL 1.7, unpinned): brute force, O(n^2), numpy float64.  The library follows it.

Common to both
  * a row with a non-finite coordinate is dropped (PCL keeps it as an inlier);
  * kept points keep their input order and their bits;
  * the squared distance of two points is dx*dx + dy*dy + dz*dz with dx, dy, dz formed in float64 from the float32
    coordinates and the three products added left to right, each operation rounded once;
  * which of several equidistant neighbours is taken changes nothing below.

Statistical (k, mul, D)
  * d_i = the mean of the float64 square roots of the k smallest squared distances from point i to other points, summed
    ascending (here with math.fsum: the correctly rounded sum);
  * a point whose k-th nearest other point has squared distance > float64(float32(D))^2 is short (so is every point of a
    cloud with fewer than k + 1 finite points): removed, d_i = +inf, no part of the statistics (PCL searches unbounded);
  * over the m other points mean = sum d / m, stddev = sqrt(sum (d - mean)^2 / (m - 1)), 0 when m < 2; with m = 0
    nothing is kept;
  * threshold = mean + float64(float32(mul)) * stddev; point i is kept iff d_i <= threshold.

Radius (r, min_neighbors)
  * c_i = the number of other points with squared distance <= float64(float32(r))^2 (closed);
  * point i is kept iff c_i >= min_neighbors (PCL counts the point itself and keeps iff count > min: the same rule).
"""
import math
from dataclasses import dataclass, field

import numpy as np

BAND_REL = 1e-9


@dataclass
class OutlierResult:
    finite: np.ndarray                  # [n] bool: the row has three finite coordinates
    keep: np.ndarray                    # [n] bool
    d: np.ndarray = None                # [n] float64: d_i, +inf short, NaN dropped row (statistical)
    c: np.ndarray = None                # [n] int32: c_i, -1 dropped row (radius)
    short: np.ndarray = None            # [n] bool
    mean: float = 0.0
    stddev: float = 0.0
    threshold: float = 0.0
    band: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))   # rows with |d - threshold| <= 1e-9 threshold


def _finite_rows(xyz):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return xyz, np.isfinite(xyz).all(axis=1)


def sq_dists(p, i):
    """Squared distances from row i of p (float32 [m, 3]) to every row, as the statement above forms them."""
    q = p.astype(np.float64)
    dx = q[:, 0] - q[i, 0]
    dy = q[:, 1] - q[i, 1]
    dz = q[:, 2] - q[i, 2]
    return (dx * dx + dy * dy) + dz * dz


def statistical(xyz, k, mul, max_dist):
    xyz, fin = _finite_rows(xyz)
    n = xyz.shape[0]
    rows = np.flatnonzero(fin)
    p = xyz[rows]
    m_pts = p.shape[0]
    lim2 = float(np.float64(np.float32(max_dist))) ** 2
    d = np.full(n, np.nan)
    short = np.zeros(n, bool)
    for a in range(m_pts):
        d2 = np.delete(sq_dists(p, a), a)
        if d2.shape[0] < k:
            d[rows[a]] = np.inf
            continue
        near = np.sort(d2)[:k]
        if near[k - 1] > lim2:
            d[rows[a]] = np.inf
            continue
        d[rows[a]] = math.fsum(math.sqrt(v) for v in near) / k
    short = np.isinf(d)
    good = np.flatnonzero(np.isfinite(d))
    m = good.shape[0]
    mean = math.fsum(d[good]) / m if m else 0.0
    stddev = math.sqrt(math.fsum((v - mean) ** 2 for v in d[good]) / (m - 1)) if m >= 2 else 0.0
    threshold = mean + float(np.float64(np.float32(mul))) * stddev
    keep = np.isfinite(d) & (d <= threshold)
    band = good[np.abs(d[good] - threshold) <= BAND_REL * threshold]
    return OutlierResult(finite=fin, keep=keep, d=d, short=short, mean=mean, stddev=stddev, threshold=threshold, band=band)


def radius(xyz, r, min_neighbors):
    xyz, fin = _finite_rows(xyz)
    n = xyz.shape[0]
    rows = np.flatnonzero(fin)
    p = xyz[rows]
    lim2 = float(np.float64(np.float32(r))) ** 2
    c = np.full(n, -1, np.int32)
    for a in range(p.shape[0]):
        c[rows[a]] = int(np.count_nonzero(sq_dists(p, a) <= lim2)) - 1   # the point itself is at distance 0
    keep = fin & (c >= min_neighbors)
    return OutlierResult(finite=fin, keep=keep, c=c, short=np.zeros(n, bool))
