"""Synthetic control-plane correspondences from a known rig, shared by the rig-calibration tests.

A rig is the construction specs perturbed by seeded rotations of 1-3 degrees and translations of 1-3 cm.  A plane
n_w . x + D = 0 of the rig frame is seen by sensor k (pose [R_k, t_k]) as n_k = R_k^T n_w, d_k = D + n_w . t_k; a
row holds the two sensors' (n, d), an inlier count (col 8) and a pixel-centre figure (col 9).
"""
import os

import numpy as np

import rigcal_model as M

# The reference's control-plane files (Adjacent_Int, and All_Int's pairs (0,2), (0,5), (1,5)).  Every number in them
# is a float printed as %.16e, so they are kept as float32 arrays in one archive, keyed "i_j", and written out as the
# reference's text files on demand: golden_dir().
_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_NPZ = os.path.join(_HERE, "golden", "control_planes.npz")
# SHA-256 of the reference's own files (Calibration/ControlPlanes/Adjacent_Int, and All_Int for 0_2, 0_5, 1_5), taken
# from them when the archive was made: golden_dir()'s files must hash to these (tests/test_rigcal_io.py).
GOLDEN_SHA256 = {
    "0_1": "54bced06c8012c88e717342add793bde1f584679b30e85dac36e2bf252a2b9bc",
    "0_2": "6ab7433ed8946c3e79b63245a68e33d01261040529ce967a9b6b9dd39a97c49d",
    "0_5": "a3c321009d1082edccc784b7970ec99b9591ffcc5c6df499f757137d240fa884",
    "0_7": "68d0fee0e5f18553eec779a7a936f7250deea73af4f2a2d6284ea9265c5075ce",
    "1_2": "f163748f5ae37503f05ae7f539c5a7424bc4c6f8f5180121ce69c3e6f6810b02",
    "1_5": "1bc8074dee53ef7a93c6f7a86f4771e0172bd3016e8ea10aa14b5fc926936307",
    "2_3": "382851c47d48ea6f15609ec49d16d0f7c6ac0cc03cfa90f61a10f1983bcdf272",
    "3_4": "b5c65a211a268662ab9543928e57b4b290d88518bb0ab7a7caa72e3330ee7eab",
    "4_5": "ff31e3e4d4775cb0c76e42386da47b692c37476311f035edc7f3c320c6695e18",
    "5_6": "9e1d847dfeea16eed18b617d97aa37adebef74367fb92050a38918e47b32d801",
    "6_7": "ba0827bcd97239a214c63cbd8fa971d748a998c9f896164d00ff5917ef4960f5",
}
_golden_dir = None
ADJACENT = [(k, k + 1) for k in range(7)] + [(0, 7)]


def golden_rows():
    with np.load(GOLDEN_NPZ) as z:
        return {tuple(int(x) for x in k.split("_")): z[k].astype(np.float64) for k in z.files}


def golden_dir():
    """A directory of correspondences_i_j.txt written from the archive, made once per process."""
    global _golden_dir
    if _golden_dir is None:
        import atexit
        import shutil
        import tempfile
        d = tempfile.mkdtemp(prefix="control_planes_")
        atexit.register(shutil.rmtree, d, True)
        for (i, j), r in golden_rows().items():
            with open(os.path.join(d, f"correspondences_{i}_{j}.txt"), "w") as f:
                f.writelines(" ".join("%.16e" % v for v in row) + "\n" for row in r)
        _golden_dir = d
    return _golden_dir


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def perturbed_rig(seed, deg=(1.0, 3.0), cm=(1.0, 3.0)):
    rng = np.random.default_rng(seed)
    Rt = M.construction_specs()
    for k in range(M.NUM_SENSORS):
        w = unit(rng, 1)[0] * np.radians(rng.uniform(*deg))
        Rt[k][:3, :3] = M.exp_so3(w) @ Rt[k][:3, :3]
        Rt[k][:3, 3] += unit(rng, 1)[0] * rng.uniform(*cm) / 100
    return Rt


def pair_rows(rig, i, j, n, rng, noise=0.0, parallel=None):
    n_w = unit(rng, n) if parallel is None else np.tile(np.asarray(parallel, np.float64), (n, 1))
    D = rng.uniform(0.5, 4.0, n)
    rows = np.zeros((n, 10))
    for off, k in ((0, i), (4, j)):
        nk = n_w @ rig[k][:3, :3]          # rows of R_k^T n_w
        dk = D + n_w @ rig[k][:3, 3]
        if noise:
            nk = nk + rng.normal(scale=noise, size=nk.shape)
            nk /= np.linalg.norm(nk, axis=1, keepdims=True)
            dk = dk + rng.normal(scale=noise, size=n)
        rows[:, off:off + 3], rows[:, off + 3] = nk, dk
    rows[:, 8] = np.floor(rng.uniform(1000, 6000, n))
    rows[:, 9] = rng.uniform(50, 250, n)
    return rows


def make_rows(rig, counts, seed, noise=0.0, parallel=None):
    """{(i, j): rows} for counts {(i, j): n}, in pair order."""
    rng = np.random.default_rng(seed)
    return {p: pair_rows(rig, p[0], p[1], counts[p], rng, noise, parallel) for p in M.PAIRS if counts.get(p, 0) > 0}


def base_counts(extra=None, n=3):
    """The seven mandatory adjacent pairs at n rows, plus extra {(i, j): rows}."""
    c = {(k, k + 1): n for k in range(7)}
    c.update(extra or {})
    return c


def with_outliers(rows, frac, seed):
    """Replaces a fraction of the rows' second plane by a random one; returns (rows, planted mask)."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    k = int(round(frac * n))
    bad = np.zeros(n, bool)
    bad[rng.choice(n, k, replace=False)] = True
    out = rows.copy()
    out[bad, 4:7] = unit(rng, k)
    out[bad, 7] = rng.uniform(0.5, 4.0, k)
    return out, bad


def fixture_rows(adjacent_only=True):
    rows = golden_rows()
    if adjacent_only:
        rows = {p: r for p, r in rows.items() if p in ADJACENT}
    return rows


def relative_errors(Rt, truth):
    """Largest error of the relative rotations R_0^T R_k (rad) and of the relative translations R_0^T (t_k - t_0) (m)."""
    dr = dt = 0.0
    for k in range(1, M.NUM_SENSORS):
        A = Rt[0][:3, :3].T @ Rt[k][:3, :3]
        B = truth[0][:3, :3].T @ truth[k][:3, :3]
        E = A.T @ B
        s = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        dr = max(dr, float(np.arctan2(s, 0.5 * (np.trace(E) - 1.0))))
        ta = Rt[0][:3, :3].T @ (Rt[k][:3, 3] - Rt[0][:3, 3])
        tb = truth[0][:3, :3].T @ (truth[k][:3, 3] - truth[0][:3, 3])
        dt = max(dt, float(np.linalg.norm(ta - tb)))
    return dr, dt


def pose_diff(P, Q):
    """Largest rotation (rad) and translation (m) difference between two sets of eight poses."""
    dr = dt = 0.0
    for a, b in zip(P, Q):
        E = a[:3, :3].T @ b[:3, :3]
        s = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        dr = max(dr, float(np.arctan2(s, 0.5 * (np.trace(E) - 1.0))))
        dt = max(dt, float(np.linalg.norm(a[:3, 3] - b[:3, 3])))
    return dr, dt
