"""The statement of record of the Euclidean cluster extraction (pcl::EuclideanClusterExtraction and the normal-aware
pcl::extractEuclideanClusters overload, restated from PCL 1.7 segmentation/extract_clusters.h, unpinned): brute force,
O(n^2), numpy float64.  The library follows it.

  * a row with a non-finite coordinate is dropped: label -1, root -1, member of nothing;
  * the squared distance of two points is that of tests/outlier_model.py (sq_dists): dx*dx + dy*dy + dz*dz in float64 of
    the float32 coordinates, left to right, each operation rounded once;
  * plain form: there is an edge i - j iff i != j, both rows are finite and d2(i, j) <= float64(float32(tolerance))^2
    (closed);
  * conditional form (normals [n, 3] float32 given): an edge needs in addition
    (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j >= math.cos(float64(float32(eps_angle))), the dot product in float64 of the
    float32 components, each operation rounded once.  Normals are taken as given: not normalised, not sign-agnostic.  A
    row whose normal has a non-finite component has no edges.  An edge whose dot product lies within DOT_BAND of the
    threshold is undecided;
  * a component is a connected component of that graph over the finite rows; its root is its smallest input index;
  * a component is a cluster iff min_size <= size <= max_size; clusters are ordered by size descending, ties by root
    ascending; members within a cluster are in ascending input index; label[i] is the cluster's rank, -1 for a dropped
    row and for a row of a rejected component;
  * per cluster: size, root, min / max (float32 compared as float32), centroid = (sum p) / size,
    C = sum (p - centroid)(p - centroid)^T / size (float64, two passes), eig the eigenvalues of C ascending
    (numpy.linalg.eigh), normal the unit eigenvector of eig[0] with its largest-magnitude component made positive (ties
    to the lower axis), curvature = |eig[0]| / ((eig[0] + eig[1]) + eig[2]), 0 when the trace is 0.  A cluster with fewer
    than 3 members has NaN eig, normal and curvature.

Bounds a comparison with another implementation may use (the other side adds the same terms in another fixed order)
  * sum_bound [c, 3]: (size - 1) * 2^-53 * sum |coordinate| per axis, the most two orders of the centroid's sum differ by;
  * cov_bound [c]: (size - 1) * 2^-53 * the largest sum |product| over the six moments, likewise;
  * eig_decided [c]: size >= 3, eig[2] > 0 and eig[1] - eig[0] >= 1e-5 * eig[2] (the eigenvector of eig[0] is
    conditioned by eig[2] / (eig[1] - eig[0])), and the sign rule is decided (the largest |component| leads the next by
    1e-6).
"""
import math
from dataclasses import dataclass

import numpy as np

from outlier_model import sq_dists

DOT_BAND = 1e-12
DEFAULTS = dict(tolerance=0.10, min_size=100, max_size=2 ** 30, eps_angle=math.radians(10.0))


@dataclass
class ClusterResult:
    finite: np.ndarray          # [n] bool
    root: np.ndarray            # [n] int32: the smallest index of the row's component, -1 dropped
    comp_size: np.ndarray       # [n] int32: its size before the size bounds, -1 dropped
    labels: np.ndarray          # [n] int32
    clusters: list              # per cluster the member indices, ascending (int64 arrays)
    size: np.ndarray            # [c] int32
    croot: np.ndarray           # [c] int32
    min: np.ndarray             # [c, 3] float32
    max: np.ndarray             # [c, 3] float32
    centroid: np.ndarray        # [c, 3] float64
    eig: np.ndarray             # [c, 3] float64 ascending
    normal: np.ndarray          # [c, 3] float64
    curvature: np.ndarray       # [c] float64
    sum_bound: np.ndarray       # [c, 3]
    cov_bound: np.ndarray       # [c]
    eig_decided: np.ndarray     # [c] bool
    undecided: np.ndarray       # [n] bool: the point touches an undecided edge (conditional form)
    n_components: int = 0

    @property
    def n_clusters(self):
        return len(self.clusters)

    @property
    def n_clustered(self):
        return int((self.labels >= 0).sum())

    def component_decided(self):
        """[n] bool: no point of the row's component touches an undecided edge (dropped rows: True)."""
        bad_roots = np.unique(self.root[self.undecided])
        return ~np.isin(self.root, bad_roots) | (self.root < 0)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def extract(xyz, tolerance=DEFAULTS["tolerance"], min_size=DEFAULTS["min_size"], max_size=DEFAULTS["max_size"],
            normals=None, eps_angle=DEFAULTS["eps_angle"]):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    assert np.isfinite(tolerance) and tolerance > 0 and 1 <= min_size <= max_size
    fin = np.isfinite(xyz).all(axis=1)
    t = float(np.float64(np.float32(tolerance)))
    lim2 = t * t
    nrm = thr = None
    if normals is not None:
        nrm32 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert nrm32.shape[0] == n and 0.0 <= eps_angle <= math.pi
        nrm = nrm32.astype(np.float64)
        nfin = np.isfinite(nrm32).all(axis=1)
        thr = math.cos(float(np.float64(np.float32(eps_angle))))
    parent = np.arange(n)
    undecided = np.zeros(n, bool)
    for i in range(n):
        if not fin[i] or i == 0:
            continue
        d2 = sq_dists(xyz[:i + 1], i)[:i]                    # every edge once, from its higher end
        with np.errstate(invalid="ignore"):
            edge = fin[:i] & (d2 <= lim2)
        if nrm is not None:
            if not nfin[i]:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                dot = (nrm[:i, 0] * nrm[i, 0] + nrm[:i, 1] * nrm[i, 1]) + nrm[:i, 2] * nrm[i, 2]
                near = edge & nfin[:i] & (np.abs(dot - thr) <= DOT_BAND)
                edge = edge & nfin[:i] & (dot >= thr)
            if near.any():
                undecided[i] = True
                undecided[:i][near] = True
        for j in np.flatnonzero(edge):
            a, b = _find(parent, i), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.full(n, -1, np.int32)
    for i in range(n):
        if fin[i]:
            root[i] = _find(parent, i)
    comp_size = np.full(n, -1, np.int32)
    roots, counts = np.unique(root[fin], return_counts=True)
    size_of = dict(zip(roots.tolist(), counts.tolist()))
    for i in range(n):
        if fin[i]:
            comp_size[i] = size_of[int(root[i])]
    kept = sorted(((c, r) for r, c in size_of.items() if min_size <= c <= max_size), key=lambda cr: (-cr[0], cr[1]))
    labels = np.full(n, -1, np.int32)
    clusters = []
    nc = len(kept)
    size = np.zeros(nc, np.int32)
    croot = np.zeros(nc, np.int32)
    mn = np.zeros((nc, 3), np.float32)
    mx = np.zeros((nc, 3), np.float32)
    centroid = np.zeros((nc, 3))
    eig = np.full((nc, 3), np.nan)
    normal = np.full((nc, 3), np.nan)
    curvature = np.full(nc, np.nan)
    sum_bound = np.zeros((nc, 3))
    cov_bound = np.zeros(nc)
    eig_dec = np.zeros(nc, bool)
    for rank, (c, r) in enumerate(kept):
        idx = np.flatnonzero(root == r)
        labels[idx] = rank
        clusters.append(idx)
        size[rank], croot[rank] = c, r
        p32 = xyz[idx]
        mn[rank], mx[rank] = p32.min(0), p32.max(0)
        p = p32.astype(np.float64)
        mean = p.sum(0) / float(c)
        centroid[rank] = mean
        sum_bound[rank] = (c - 1) * 2.0 ** -53 * np.abs(p).sum(0)
        d = p - mean
        prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                          d[:, 2] * d[:, 2]], 1)
        cov_bound[rank] = (c - 1) * 2.0 ** -53 * np.abs(prods).sum(0).max()
        if c < 3:
            continue
        s = prods.sum(0) / float(c)
        cov = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
        lam, vec = np.linalg.eigh(cov)
        v = vec[:, 0].copy()
        a = np.abs(v)
        lead = int(np.argmax(a))                              # the first maximum: ties to the lower axis
        if v[lead] < 0:
            v = -v
        tr = (lam[0] + lam[1]) + lam[2]
        eig[rank], normal[rank] = lam, v
        curvature[rank] = 0.0 if tr == 0.0 else abs(lam[0]) / tr
        others = np.delete(a, lead)
        eig_dec[rank] = bool(lam[2] > 0 and (lam[1] - lam[0]) >= 1e-5 * lam[2] and a[lead] - others.max() >= 1e-6)
    return ClusterResult(finite=fin, root=root, comp_size=comp_size, labels=labels, clusters=clusters, size=size,
                         croot=croot, min=mn, max=mx, centroid=centroid, eig=eig, normal=normal, curvature=curvature,
                         sum_bound=sum_bound, cov_bound=cov_bound, eig_decided=eig_dec, undecided=undecided,
                         n_components=len(size_of))


def partition(xyz, labels):
    """The clustering as a set of frozensets of coordinate triples (bits), for comparisons across permutations."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = set()
    for lab in np.unique(labels[labels >= 0]):
        rows = xyz[labels == lab].view(np.uint32)
        out.add(frozenset(map(tuple, rows.tolist())))
    return out
