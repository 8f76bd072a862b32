"""Inputs of the Generalized-ICP tests (tests/test_gicp_model.py, tests/test_gpu_gicp.py, tests/test_gpu_gicp_shapes.py)
and the rules that say which points a rounding cannot change ("decided").  Not a test module."""
from __future__ import annotations

import functools

import numpy as np

import gicp_model as GM

SIZES = [(20, 20), (21, 33), (63, 65), (64, 129), (1999, 2113), (20011, 19997)]
ALIGN_SIZES = [(1999, 2113), (20011, 19997)]
G_TWIST = (0.12, -0.08, 0.05, 0.03, -0.02, 0.04)
POSE2_TWIST = (0.01, 0.0, -0.01, 0.002, 0.001, -0.002)
REL = 2.0 ** -18          # 16 float32 ulps: a float32 squared distance from float32 coordinates carries about 4
MAX_UNDECIDED = 0.01


def room(n: int, seed: int, jitter: float = 0.002) -> np.ndarray:
    """n points uniform on the six faces of the box |x| <= 3, |y| <= 2, |z| <= 1.5, Gaussian jitter on every
    coordinate, float32."""
    rng = np.random.default_rng(seed)
    half = np.array([3.0, 2.0, 1.5])
    # faces by area: the pair normal to axis a has area 4 * half[b] * half[c] each
    area = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    side = rng.integers(0, 2, size=n) * 2 - 1
    p = rng.uniform(-1.0, 1.0, size=(n, 3)) * half
    p[np.arange(n), axis] = side * half[axis]
    p += rng.normal(0.0, jitter, size=(n, 3))
    return p.astype(np.float32)


def G() -> np.ndarray:
    return GM.exp_se3(G_TWIST)


def pose2() -> np.ndarray:
    return GM.exp_se3(POSE2_TWIST) @ G()


def transform(xyz: np.ndarray, T: np.ndarray) -> np.ndarray:
    return (xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def pair(ns: int, nt: int, jitter: float = 0.002):
    """Source = room(ns, 1); target = room(nt, 2), an independent sampling of the same surfaces, moved by G: the pose
    that maps the source into the target is G."""
    return room(ns, 1, jitter), transform(room(nt, 2, jitter), G())


def params32() -> GM.Params:
    return GM.Params().as_float32()


@functools.lru_cache(maxsize=None)
def model_pair(ns: int, nt: int):
    """(source Cloud, target Cloud) of the model for a size, computed once per process and left unchanged."""
    s, t = pair(ns, nt)
    p = params32()
    return GM.Cloud(s, p), GM.Cloud(t, p)


def knn_decided(c: GM.Cloud) -> np.ndarray:
    """The k-th and (k+1)-th neighbour are further apart than rounding reaches (always, when the cloud has k points)."""
    return (c.knn_next - c.knn_d2[:, -1]) >= REL * c.knn_next


def cov_decided(c: GM.Cloud) -> np.ndarray:
    lam = c.lam
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    return knn_decided(c) & (gap >= 1e-6)


def corr_decided(d2: np.ndarray, second: np.ndarray, max_corr_dist: float) -> np.ndarray:
    g2 = max_corr_dist ** 2
    return ((second - d2) >= REL * second) & (np.abs(d2 - g2) >= REL * g2)


# ---- crafted clouds, poses, gates and the extended rule (tests/test_gpu_gicp_shapes.py) -----------------------------

DIRECT, MAXDIM, KMIN, KMAX, PASS_WRAP = 512, 1024, 4, 32, 256 * 256   # R360_GICP_DIRECT, _MAXDIM, k's range, MAXB * 256


def _shuffled(p: np.ndarray, seed: int) -> np.ndarray:
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])], np.float32)


def lattice(nx: int, ny: int, nz: int, spacing: float, origin=(0.0, 0.0, 0.0), seed: int = 11) -> np.ndarray:
    """nx * ny * nz lattice points, rows shuffled so that the index order is not the lattice order."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return _shuffled(g * spacing + np.asarray(origin), seed)


def _sheet():
    rng = np.random.default_rng(21)
    return np.stack([rng.uniform(0, 3, 900), rng.uniform(0, 2, 900), np.full(900, 0.5)], axis=1).astype(np.float32)


def _rod(seed=24):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 10, 2000), rng.uniform(0, 0.004, 2000), rng.normal(0, 0.0002, 2000)],
                    axis=1).astype(np.float32)


def _ribbon():
    rng = np.random.default_rng(25)
    return np.stack([rng.uniform(0, 10, 7000), rng.uniform(0, 0.05, 7000), rng.normal(0, 0.0005, 7000)],
                    axis=1).astype(np.float32)


def _two_clusters():
    far = room(1000, 4) + np.array([1000.0, 0.0, 0.0], np.float32)
    return _shuffled(np.concatenate([room(1000, 3), far]), 24)


def _dups():
    p = room(600, 6)
    rows = np.random.default_rng(25).integers(0, 600, 100)
    return _shuffled(np.concatenate([p, p[rows]]), 26)


# name -> (builder, the grid gicp_choose_grid gives it: asserted in tests/test_gicp_model.py)
CLOUDS = {
    "room512": (lambda: room(512, 1), (1, 1, 1)),
    "room513": (lambda: room(513, 2), (11, 7, 6)),
    "sheet": (_sheet, (37, 25, 1)),
    "rod": (_rod, (1023, 1, 1)),
    "rod1024": (lambda: _rod(22), (1024, 1, 1)),   # the same recipe where the float rounding falls the other way
    "ribbon": (_ribbon, (1023, 6, 1)),
    "shifted": (lambda: room(2000, 5) + np.float32(1000.0), (18, 12, 10)),
    "two_clusters": (_two_clusters, (501, 2, 2)),
    "dups": (_dups, None),
    "lattice3d": (lambda: lattice(9, 9, 8, 2.0 ** -4), None),
    "lattice_plane": (lambda: lattice(26, 26, 1, 2.0 ** -4, (0.0, 0.0, 0.25), seed=12), None),
}
TIED = ("dups", "lattice3d", "lattice_plane")   # zero undecided under knn_decided_ties


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> np.ndarray:
    c = CLOUDS[name][0]()
    c.setflags(write=False)
    return c


def make_params(k=20, eps=1e-3, gate=0.4, max_it=10, max_inner=20) -> GM.Params:
    return GM.Params(k_correspondences=k, gicp_epsilon=eps, max_corr_dist=gate, max_iterations=max_it,
                     max_inner_iterations=max_inner).as_float32()


@functools.lru_cache(maxsize=None)
def model_cloud(name: str, k: int = 20) -> GM.Cloud:
    return GM.Cloud(cloud(name), make_params(k=k))


def choose_grid(xyz: np.ndarray):
    """gicp_choose_grid (host/gicp_host.h) in numpy, float for float: (dim (3,), h, inv, mn)."""
    p = np.asarray(xyz, np.float32)
    n = p.shape[0]
    mn, mx = p.min(axis=0), p.max(axis=0)
    ext = (mx - mn).astype(np.float32)
    emax = np.float32(ext.max())
    if n <= DIRECT or not emax > 0:
        h = np.float32(2.0) * emax if emax > 0 else np.float32(1.0)
        return (1, 1, 1), h, np.float32(1.0) / h, mn

    def cells(h):
        return int(np.prod(np.minimum(np.floor(ext.astype(np.float64) / h) + 1.0, MAXDIM)))

    lo, hi = float(emax) / (MAXDIM - 1), 2.0 * float(emax)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if cells(mid) <= n:
            hi = mid
        else:
            lo = mid
    h = np.float32(hi)
    inv = np.float32(1.0) / h
    v = np.floor((ext * inv).astype(np.float32))
    dim = np.minimum(np.maximum(v, 0), MAXDIM - 1).astype(int) + 1
    return tuple(int(d) for d in dim), h, inv, mn


def exact_cloud(xyz: np.ndarray) -> bool:
    """Every coordinate is a multiple of 2^-10 below 2^10: differences have at most 21 bits, their squares 42 and a sum
    of three 44, so a squared distance is exact in fp64 whatever the order or fusing of its operations."""
    s = np.asarray(xyz, np.float64) * 1024.0
    return bool((s == np.round(s)).all() and (np.abs(s) < 2.0 ** 20).all())


def knn_decided_ties(c: GM.Cloud) -> np.ndarray:
    """knn_decided extended to ties that the index rule settles on both sides: the k-th and the (k+1)-th neighbour
    have bit-identical coordinates (each side computes one distance from the same operands twice), or the cloud's
    squared distances are exact in fp64 (exact_cloud)."""
    dec = knn_decided(c).copy()
    if exact_cloud(c.xyz):
        dec[:] = True
        return dec
    n, k = c.knn.shape
    for i in np.flatnonzero(~dec):
        dd = ((c.P - c.P[i]) ** 2).sum(axis=1)
        o = np.lexsort((np.arange(n), dd))
        assert np.array_equal(o[:k], c.knn[i])
        dec[i] = c.xyz[o[k - 1]].tobytes() == c.xyz[o[k]].tobytes()
    return dec


def cov_decided_ties(c: GM.Cloud) -> np.ndarray:
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (c.lam[:, 1] - c.lam[:, 0]) / c.lam[:, 2]
    return knn_decided_ties(c) & (gap >= 1e-6)


def _f32(T: np.ndarray) -> np.ndarray:
    return np.asarray(T, np.float32).astype(np.float64)   # the ABI's pose is float32


def _rz(deg: float) -> np.ndarray:
    T = np.eye(4)
    a = np.deg2rad(deg)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def _tr(x, y, z) -> np.ndarray:
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


EVAL_PAIR = (1999, 2113)
GATES = (0.4, 0.05, float("inf"))


def eval_poses():
    """name -> pose (float32 values in float64) for the eval stage on EVAL_PAIR: a quarter and a half turn, and two
    shifts that put hundreds of source points beyond faces of the target's box."""
    return {"rz90": _f32(_rz(90) @ G()), "rz180": _f32(_rz(180) @ G()), "tx": _f32(_tr(2.5, 0, 0) @ G()),
            "tyz": _f32(_tr(0, -1.5, -1) @ G())}


def outside_faces(src_xyz: np.ndarray, tgt_xyz: np.ndarray, X: np.ndarray) -> np.ndarray:
    """Counts of transformed source points beyond the target's bounding box: [x-, x+, y-, y+, z-, z+]."""
    q = src_xyz.astype(np.float64) @ X[:3, :3].T + X[:3, 3]
    mn, mx = tgt_xyz.min(axis=0).astype(np.float64), tgt_xyz.max(axis=0).astype(np.float64)
    return np.array([f(a) for a in range(3) for f in (lambda a: int((q[:, a] < mn[a]).sum()),
                                                      lambda a: int((q[:, a] > mx[a]).sum()))])


def gate_lattice():
    """Target: a 9 x 9 x 8 lattice of spacing 0.25, shuffled; source: the same rows + (0.125, 0, 0).  At the identity
    every source point is exactly 0.125 from its own target and, in 8 of the 9 x columns, from the next one too."""
    t = lattice(9, 9, 8, 0.25, seed=13)
    return (t + np.array([0.125, 0.0, 0.0], np.float32)).astype(np.float32), t


def gate_lattice_expected() -> np.ndarray:
    """The correspondences of gate_lattice at the identity with the gate just above 0.125: source row i is 0.125 from
    target row i and from the target one step further along x, if there is one; the lower index of the two wins."""
    _, t = gate_lattice()
    at = {r.tobytes(): i for i, r in enumerate(t)}
    step = np.array([0.25, 0.0, 0.0], np.float32)
    return np.array([min(i, at.get((r + step).tobytes(), i)) for i, r in enumerate(t)], np.int32)


EVAL_CORR_ONLY = ("tyz",)   # eval_poses whose model has undecided correspondences: compared on correspondences only
K_ENDS = (KMIN, KMAX)
K_PAIR = (600, 700)
WRAP_PAIR = (70001, 3001)   # the source is past PASS_WRAP: k_gicp_pass and k_gicp_sum go round their grid-stride loops


@functools.lru_cache(maxsize=None)
def model_pair_with(ns: int, nt: int, k: int = 20, eps: float = 1e-3):
    """model_pair at another k_correspondences / gicp_epsilon."""
    s, t = pair(ns, nt)
    p = make_params(k=k, eps=eps)
    return GM.Cloud(s, p), GM.Cloud(t, p)


@functools.lru_cache(maxsize=None)
def model_room(n: int, seed: int, k: int = 20) -> GM.Cloud:
    return GM.Cloud(room(n, seed), make_params(k=k))
