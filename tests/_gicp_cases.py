"""Inputs of the Generalized-ICP tests (tests/test_gicp_model.py, tests/test_gpu_gicp.py) and the rule that says which
points a rounding cannot change ("decided").  Not a test module."""
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
