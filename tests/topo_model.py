"""Topological submaps, stated in numpy (float64 throughout): the oracle of r360_topo_* and r360_topomap_*
(DESIGN.md §5f).

The reference's include/TopologicalMap360.h cuts the sensed-space-overlap (SSO) graph of the current area and its
neighbours with mrpt::graphs::CGraphPartitioner::RecursiveSpectralPartition(SSO, parts, 0.8, false, true, true, 3).
MRPT is not vendored there, so the algorithm is restated here and not pinned:

  bisect     L = diag(row sums of A) - A (the plain Laplacian), full symmetric eigendecomposition, eigenvalues
             ascending; v = the eigenvector of the second-smallest eigenvalue (the only one for n = 1), m = mean(v);
             node i goes to side 1 when v_i >= m, else to side 2; an empty side -> side 1 = {i <= n/2}; cut = ncut
  ncut       c = sum over P x Q, aa / bb = the inside edges of P / Q counted once, the diagonal included;
             0 when c == 0, else c/(aa+c) + c/(bb+c)
  partition  bisect; cut > threshold or a side below min_cluster nodes -> one part; else recurse into both sides;
             at the end the parts are ordered by their first element (RearrangePartition, TopologicalMap360.h:372-387)

The bookkeeping of Map360 + TopologicalMap360 (TopoMap below) keeps the SSO in one symmetric table keyed by global
keyframe ids; the neighbour relation and the representative keyframes are functions of that table and of the
keyframes' areas.
"""
import numpy as np

THRESHOLD_NCUT, MIN_CLUSTER = 0.8, 3
MAX_NODES = 256


def laplacian(A):
    A = np.asarray(A, np.float64)
    return np.diag(A.sum(axis=1)) - A


def ncut(A, P, Q):
    A = np.asarray(A, np.float64)
    P, Q = list(P), list(Q)
    c = float(A[np.ix_(P, Q)].sum()) if P and Q else 0.0
    if c == 0.0:
        return 0.0
    aa = float(np.triu(A[np.ix_(P, P)]).sum())
    bb = float(np.triu(A[np.ix_(Q, Q)]).sum())
    return c / (aa + c) + c / (bb + c)


def sides_of(v):
    """The two index lists of a Fiedler vector, with the empty-side fallback."""
    v = np.asarray(v, np.float64)
    n = len(v)
    m = v.mean()
    s1 = [i for i in range(n) if v[i] >= m]
    s2 = [i for i in range(n) if not v[i] >= m]
    if not s1 or not s2:
        s1 = [i for i in range(n) if i <= n // 2]
        s2 = [i for i in range(n) if i > n // 2]
    return s1, s2


def bisect(A, info=None):
    """(side1, side2, cut).  info (a dict, optional) receives the eigenvalues, the Fiedler vector and the figures the
    parity tests rely on: margin = min |v_i - mean|, gap = the smaller distance of lambda_2 to its neighbours over
    lambda_max."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    w, V = np.linalg.eigh(laplacian(A))
    k = min(1, n - 1)
    v = V[:, k]
    s1, s2 = sides_of(v)
    cut = ncut(A, s1, s2)
    if info is not None:
        lmax = float(w[-1])
        gaps = [abs(w[k] - w[j]) for j in (k - 1, k + 1) if 0 <= j < n and j != k]
        info.update(eigenvalues=w, fiedler=v, margin=float(np.abs(v - v.mean()).min()),
                    gap=(min(gaps) / lmax if gaps and lmax > 0 else np.inf), lmax=lmax)
    return s1, s2, cut


def partition(A, threshold=THRESHOLD_NCUT, min_cluster=MIN_CLUSTER, recursive=True, bisections=None):
    """The parts (ascending index lists, ordered by their first element).  bisections (a list, optional) receives one
    dict per bisection, ordered by the cluster's lowest node and, among nested clusters, the larger first (which side
    of a bisection is side 1 hangs on the eigenvector's sign; this order does not): nodes (the cluster's indices in
    the input graph), side1, side2 (likewise), cut, split, margin, gap."""
    A = np.asarray(A, np.float64)

    def rec(nodes):
        sub = A[np.ix_(nodes, nodes)]
        info = {}
        s1, s2, cut = bisect(sub, info)
        split = not (cut > threshold or len(s1) < min_cluster or len(s2) < min_cluster)
        if bisections is not None:
            bisections.append(dict(nodes=list(nodes), side1=[nodes[i] for i in s1], side2=[nodes[i] for i in s2], cut=cut,
                                   split=split, margin=info["margin"], gap=info["gap"]))
        if not split:
            return [list(nodes)]
        g1, g2 = [nodes[i] for i in s1], [nodes[i] for i in s2]
        if not recursive:
            return [g1, g2]
        return rec(g1) + rec(g2)

    parts = rec(list(range(A.shape[0])))
    if bisections is not None:
        bisections.sort(key=lambda b: (b["nodes"][0], -len(b["nodes"])))
    return sorted(parts, key=lambda p: p[0])


def part_of(parts, n):
    out = np.full(n, -1, np.int32)
    for k, p in enumerate(parts):
        out[p] = k
    return out


def assert_well_posed(A, threshold=THRESHOLD_NCUT, min_cluster=MIN_CLUSTER):
    """What a parity case must satisfy at every bisection of its recursion, so that the comparison does not hang on a
    rounding: no Fiedler entry within 1e-6 of the mean, lambda_2 apart from its neighbours by 1e-4 lambda_max, no cut
    within 1e-6 of the threshold.  Returns the bisections."""
    bis = []
    partition(A, threshold, min_cluster, True, bis)
    for b in bis:
        assert b["margin"] >= 1e-6, ("margin", len(b["nodes"]), b["margin"])
        assert b["gap"] >= 1e-4, ("gap", len(b["nodes"]), b["gap"])
        assert abs(b["cut"] - threshold) >= 1e-6, ("cut", len(b["nodes"]), b["cut"])
    return bis


class TopoMap:
    """The bookkeeping of r360_topomap_* (Map360 + TopologicalMap360): keyframes with an area each, one symmetric
    SSO table over global keyframe ids, the current area."""

    def __init__(self):
        self.area_of = []
        self.sso = {}
        self.n_areas = 1
        self.current_area = 0

    def add_keyframe(self):
        self.area_of.append(self.current_area)
        return len(self.area_of) - 1

    def drop_last(self):
        assert self.area_of
        k = len(self.area_of) - 1
        self.area_of.pop()
        self.sso = {ij: s for ij, s in self.sso.items() if k not in ij}

    def add_connection(self, a, b, sso):
        n = len(self.area_of)
        assert 0 <= a < n and 0 <= b < n and a != b and np.isfinite(sso) and sso >= 0
        self.sso[(min(a, b), max(a, b))] = np.float32(sso)

    def get(self, a, b):
        return self.sso.get((min(a, b), max(a, b)), np.float32(0))

    def keyframes(self, area):
        return [k for k, a in enumerate(self.area_of) if a == area]

    def neighbors(self, area):
        out = {area}
        for (a, b), s in self.sso.items():
            if s > 0:
                if self.area_of[a] == area:
                    out.add(self.area_of[b])
                if self.area_of[b] == area:
                    out.add(self.area_of[a])
        return sorted(out)

    def selected(self, area):
        kfs = self.keyframes(area)
        if not kfs:
            return -1
        best, best_sum = kfs[0], 0.0
        for a in kfs:
            s = 0.0
            for b in kfs:
                s += float(self.get(a, b)) if a != b else 0.0
            if s > best_sum:
                best, best_sum = a, s
        return best

    def vicinity(self):
        kfs = [k for area in self.neighbors(self.current_area) for k in self.keyframes(area)]
        A = np.zeros((len(kfs), len(kfs)), np.float32)
        for i, a in enumerate(kfs):
            for j, b in enumerate(kfs):
                if a != b:
                    A[i, j] = self.get(a, b)
        return kfs, A

    def partition(self, threshold=THRESHOLD_NCUT, min_cluster=MIN_CLUSTER, recursive=True):
        """Returns the number of new areas."""
        areas = self.neighbors(self.current_area)
        kfs, A = self.vicinity()
        if len(kfs) < 3:
            return 0
        parts = partition(A, threshold, min_cluster, recursive)
        k = len(parts) - len(areas)
        if k <= 0:
            return 0
        ids = areas + list(range(self.n_areas, self.n_areas + k))
        self.n_areas += k
        top = max(kfs)
        for area, part in zip(ids, parts):
            for i in part:
                self.area_of[kfs[i]] = area
                if kfs[i] == top:
                    self.current_area = area
        return k
