"""Rig extrinsic calibration from control planes, stated in numpy (float64 throughout): the oracle of r360_rigcal_*
(DESIGN.md §5e).

The reference's include/Calibration.h is stated by line:

  loadConstructionSpecs   :918-930   sensor 0 at z = 0.055, every next sensor turned 45 deg about X
  CalibrateRotation       :1026-1218 Gauss-Newton over the seven free rotations, 10 iterations, 1e-5 on |update|^2,
                                     1e-6 on the error decrease, then the turn that makes the mean X axis vertical
  CalibrateTranslation    :1222-1334 one linear solve, recentred
  calcConditioning        :1346-1352 sigma_max / sigma_min of the 21x21 matrix; threshold 8000 (Miscellaneous.h:76)

with its quirks kept (sensor 0's rows and cross block skipped, the lower cross block assigned as the transpose, the
accept test on the weighted error whatever the normal equations' weighting, a badly conditioned rotation system
breaks the loop but not the final alignment).  A correspondence row has ten columns: n_i (3), d_i, n_ii (3), d_ii in
the two sensors' own frames, the smaller inlier count (col 8) and the pixel-centre figure (col 9).

Deviations, all documented in DESIGN.md §5e: fp64 on the files' doubles where the reference holds floats; `weighted`
is a plain flag here (the reference also asks for 18 columns, which its own files never have); a missing adjacent
pair is an error code where the reference asserts; acos takes its argument clamped to [-1, 1]; the final alignment
is skipped when its 3x3 system is exactly singular (the untouched specs; the reference divides by zero there).

The outlier trimmer states the live form of the pair fit (Calibration/OnlinePairCalibrator.cpp:84-160) with
Calibration.h's thresholds (:193-225), since ControlPlanes::trimOutliersRANSAC applies its rotation the wrong way
round.  MRPT's random generator cannot be reproduced: the draw is a counter-based integer hash, stated in draw3().

Every 3-term product is written (a0 b0 + a1 b1) + a2 b2 as in tests/pgo_model.py; the kernels repeat it without
contraction, so the per-row terms are the same doubles on both sides and only the grouping of the sums differs.
"""
import math

import numpy as np

NUM_SENSORS = 8
PAIRS = [(i, j) for i in range(NUM_SENSORS) for j in range(i + 1, NUM_SENSORS)]   # 28, the reference's map order
MAX_ITERATIONS = 10
EPSILON_TRANSF = 1e-5
CONVERGENCE_ERROR = 1e-6
THRESHOLD_CONDITIONING = 8000.0
SMALL_ANGLE = 1e-4
STATUS_CONVERGED, STATUS_ITERATION_LIMIT, STATUS_BAD_CONDITIONED, STATUS_MISSING_PAIR = 0, 1, 2, 3
MODE_ROTATION, MODE_TRANSLATION = 0, 1


def construction_specs():
    """loadConstructionSpecs: [8][4][4]."""
    Rt = np.zeros((NUM_SENSORS, 4, 4))
    Rt[0] = np.eye(4)
    Rt[0, 2, 3] = 0.055
    c, s = math.cos(45 * math.pi / 180), math.sin(45 * math.pi / 180)
    turn = np.eye(4)
    turn[1, 1] = turn[2, 2] = c
    turn[1, 2] = -s
    turn[2, 1] = s
    for k in range(1, NUM_SENSORS):
        Rt[k] = turn @ Rt[k - 1]
    return Rt


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def mul3(A, B):
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    if B.ndim == 1:
        return (A[:, 0] * B[0] + A[:, 1] * B[1]) + A[:, 2] * B[2]
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def exp_so3(w):
    """Rodrigues, the form of tests/pgo_model.py."""
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


def rotate_rows(R, n):
    """R n for rows n [m][3]: (R0 x + R1 y) + R2 z per component."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)], axis=1)


def skew_rows(v):
    """[m][3][3] skew matrices of rows v."""
    m = len(v)
    K = np.zeros((m, 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -v[:, 2], v[:, 1]
    K[:, 1, 0], K[:, 1, 2] = v[:, 2], -v[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -v[:, 1], v[:, 0]
    return K


def atb_rows(A, B):
    """A^T B per row for [m][3][3] (B may be [m][3]): the fixed order over the summed index."""
    if B.ndim == 2:
        return (A[:, 0, :] * B[:, 0:1] + A[:, 1, :] * B[:, 1:2]) + A[:, 2, :] * B[:, 2:3]
    return (A[:, 0, :, None] * B[:, 0, None, :] + A[:, 1, :, None] * B[:, 1, None, :]) + A[:, 2, :, None] * B[:, 2, None, :]


def row_weight(rows):
    """calcCorrespRotErrorWeight's weight (:968): col 8 / (col 3 * col 9)."""
    return rows[:, 8] / (rows[:, 3] * rows[:, 9])


def missing_pair(rows):
    """The reference's assert (:1060, :1239): every adjacent pair (k, k+1), k = 0..6, has at least 3 rows."""
    for k in range(NUM_SENSORS - 1):
        r = rows.get((k, k + 1))
        if r is None or len(r) < 3:
            return True
    return False


def weighted_rot_error(rows, Rt):
    """calcCorrespRotErrorWeight (:958-980)."""
    acc = 0.0
    for (s1, s2) in PAIRS:
        r = rows.get((s1, s2))
        if r is None or len(r) == 0:
            continue
        e = rotate_rows(Rt[s1][:3, :3], r[:, 0:3]) - rotate_rows(Rt[s2][:3, :3], r[:, 4:7])
        acc += float(np.sum(row_weight(r) * ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])))
    return acc


def accumulate(rows, Rt, mode, weighted):
    """The 21x21 matrix, the 21-vector and the scalars of one linearisation, as the reference's loops build them.
    scalars: rotation (sum |r|^2, sum acos(n_i . n_ii), rows, weighted error); translation (sum r^2, 0, rows, 0)."""
    H = np.zeros((21, 21))
    g = np.zeros(21)
    sc = np.zeros(4)
    for (s1, s2) in PAIRS:
        r = rows.get((s1, s2))
        if r is None or len(r) == 0:
            continue
        a, b = 3 * (s1 - 1), 3 * (s2 - 1)
        n_i = rotate_rows(Rt[s1][:3, :3], r[:, 0:3])
        n_ii = rotate_rows(Rt[s2][:3, :3], r[:, 4:7])
        w = row_weight(r) if weighted else np.ones(len(r))
        if mode == MODE_ROTATION:
            Ji, Jii = skew_rows(-n_i), skew_rows(n_ii)
            e = n_i - n_ii
            e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            dot = (n_i[:, 0] * n_ii[:, 0] + n_i[:, 1] * n_ii[:, 1]) + n_i[:, 2] * n_ii[:, 2]
            sc += [np.sum(e2), np.sum(np.arccos(np.minimum(1.0, np.maximum(-1.0, dot)))), len(r), np.sum(row_weight(r) * e2)]
            Hii, Hij, Hjj = atb_rows(Ji, Ji), atb_rows(Ji, Jii), atb_rows(Jii, Jii)
            gi, gj = atb_rows(Ji, e), atb_rows(Jii, e)
        else:
            e = r[:, 3] - r[:, 7]
            sc += [np.sum(e * e), 0.0, len(r), 0.0]
            Hii = n_i[:, :, None] * n_i[:, None, :]
            Hij = -n_i[:, :, None] * n_ii[:, None, :]
            Hjj = n_ii[:, :, None] * n_ii[:, None, :]
            gi, gj = -n_i * e[:, None], n_ii * e[:, None]
        if s1 != 0:
            H[a:a + 3, a:a + 3] += np.sum(w[:, None, None] * Hii, axis=0)
            g[a:a + 3] += np.sum(w[:, None] * gi, axis=0)
            H[a:a + 3, b:b + 3] += np.sum(w[:, None, None] * Hij, axis=0)
        H[b:b + 3, b:b + 3] += np.sum(w[:, None, None] * Hjj, axis=0)
        g[b:b + 3] += np.sum(w[:, None] * gj, axis=0)
        if s1 != 0:
            H[b:b + 3, a:a + 3] = H[a:a + 3, b:b + 3].T
    return H, g, sc


def conditioning(H):
    s = np.linalg.svd(H, compute_uv=False)
    return float(s.max() / s.min()) if s.min() > 0 else float("inf")


def inv3_apply(A, b):
    """A^-1 b by cofactors; None when the determinant is exactly zero or not finite."""
    c00 = A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]
    c01 = A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2]
    c02 = A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]
    det = (A[0, 0] * c00 + A[0, 1] * c01) + A[0, 2] * c02
    if det == 0.0 or not np.isfinite(det):
        return None
    c10 = A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2]
    c11 = A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0]
    c12 = A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1]
    c20 = A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]
    c21 = A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]
    c22 = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    x0 = ((c00 * b[0] + c10 * b[1]) + c20 * b[2]) / det
    x1 = ((c01 * b[0] + c11 * b[1]) + c21 * b[2]) / det
    x2 = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det
    return np.array([x0, x1, x2])


def vertical_alignment(Rt):
    """:1176-1215: the turn (no component about X) that brings the mean X axis of the eight rotations to (1, 0, 0)."""
    X = np.array([1.0, 0.0, 0.0])
    Hr = np.zeros((3, 3))
    gr = np.zeros(3)
    for k in range(NUM_SENSORS):
        Xp = Rt[k][:3, 0]
        err = np.cross(X, Xp)
        J = -mul3(skew(X), skew(Xp))
        Hr += mul3(J.T, J)
        gr += mul3(J.T, err)
    m = inv3_apply(Hr, -gr)
    if m is None:
        return Rt
    rot = exp_so3([0.0, m[1], m[2]])
    out = Rt.copy()
    for k in range(NUM_SENSORS):
        out[k][:3, :3] = mul3(rot, Rt[k][:3, :3])
    return out


def calibrate_rotation(rows, Rt_init, weighted=False):
    """CalibrateRotation.  Returns (Rt, stats); stats: status, iterations (list of dicts: error = sum |r|^2, angle =
    sum of angles, cond, update2, werr0, werr1, accepted), rows."""
    st = {"status": STATUS_CONVERGED, "iterations": [], "rows": 0}
    Rt = np.array(Rt_init, np.float64).copy()
    if missing_pair(rows):
        st["status"] = STATUS_MISSING_PAIR
        return Rt, st
    increment = diff = 1000.0
    it = 0
    bad = False
    while it < MAX_ITERATIONS and increment > EPSILON_TRANSF and diff > CONVERGENCE_ERROR:
        H, g, sc = accumulate(rows, Rt, MODE_ROTATION, weighted)
        st["rows"] = int(sc[2])
        rec = {"error": sc[0], "angle": sc[1], "cond": conditioning(H), "update2": 0.0, "werr0": sc[3], "werr1": sc[3],
               "accepted": False}
        st["iterations"].append(rec)
        if rec["cond"] > THRESHOLD_CONDITIONING:
            bad = True
            break
        upd = -np.linalg.solve(H, g)
        Rtmp = Rt.copy()
        for k in range(1, NUM_SENSORS):
            Rtmp[k][:3, :3] = mul3(exp_so3(upd[3 * k - 3:3 * k]), Rt[k][:3, :3])
        e0 = sc[3]
        e1 = weighted_rot_error(rows, Rtmp)
        rec["werr1"] = e1
        if e1 < e0:
            Rt = Rtmp
            rec["accepted"] = True
        increment = float(upd @ upd)
        rec["update2"] = increment
        diff = e0 - e1
        it += 1
    if bad:
        st["status"] = STATUS_BAD_CONDITIONED
    elif it >= MAX_ITERATIONS and increment > EPSILON_TRANSF and diff > CONVERGENCE_ERROR:
        st["status"] = STATUS_ITERATION_LIMIT
    return vertical_alignment(Rt), st


def calibrate_translation(rows, Rt_in, weighted=False):
    """CalibrateTranslation on the rotations of Rt_in.  stats: status, error (sum r^2), cond, rows."""
    st = {"status": STATUS_CONVERGED, "error": 0.0, "cond": 0.0, "rows": 0}
    Rt = np.array(Rt_in, np.float64).copy()
    if missing_pair(rows):
        st["status"] = STATUS_MISSING_PAIR
        return Rt, st
    H, g, sc = accumulate(rows, Rt, MODE_TRANSLATION, weighted)
    st.update(error=sc[0], rows=int(sc[2]), cond=conditioning(H))
    if not st["cond"] < THRESHOLD_CONDITIONING:
        st["status"] = STATUS_BAD_CONDITIONED
        return Rt, st
    upd = -np.linalg.solve(H, g)
    center = np.zeros(3)
    for k in range(1, NUM_SENSORS):
        center = center + upd[3 * k - 3:3 * k]
    center = center / 8
    Rt[0][:3, 3] = -center
    for k in range(1, NUM_SENSORS):
        Rt[k][:3, 3] = upd[3 * k - 3:3 * k] - center
    return Rt, st


# ------------------------------------------------------------------ the outlier trimmer
TRIM_DIST = 0.2
TRIM_DEGENERATE = 0.3
TRIM_MAX_ITER = 5000
TRIM_PROB = 0.99
TRIM_MAX_REDRAWS = 100
FIT_RCOND = 1e-6            # a draw whose C has sigma_min <= FIT_RCOND sigma_max defines no rotation: the trial scores 0
M32 = 0xFFFFFFFF


def mix32(x):
    """A 32-bit integer finaliser (xorshift-multiply, twice)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def draw3(seed, trial, redraw, n):
    """Three distinct row indices below n (n >= 3) from (seed, trial, redraw)."""
    h = mix32(seed ^ mix32((trial * 0x9E3779B9 + mix32(redraw + 0x85EBCA6B)) & M32))
    i0 = mix32(h + 1) % n
    i1 = mix32(h + 2) % (n - 1)
    if i1 >= i0:
        i1 += 1
    i2 = mix32(h + 3) % (n - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


def degenerate(rows, idx, thr=TRIM_DEGENERATE):
    n1, n2, n3 = rows[idx[0], 0:3], rows[idx[1], 0:3], rows[idx[2], 0:3]
    c = np.array([n2[1] * n3[2] - n2[2] * n3[1], n2[2] * n3[0] - n2[0] * n3[2], n2[0] * n3[1] - n2[1] * n3[0]])
    return abs((n1[0] * c[0] + n1[1] * c[1]) + n1[2] * c[2]) < thr


def fit_pair(rows, idx):
    """The live getAlignment: R = V diag(1, 1, det) U^T of C = I00 + sum n_ii n_i^T, t = -(I00 + sum n_i n_i^T)^-1
    sum n_i (d_i - d_ii).  Returns (R, t, sigma_min / sigma_max); t is None when its system is singular."""
    C = np.zeros((3, 3))
    C[0, 0] = 1.0
    A = np.zeros((3, 3))
    A[0, 0] = 1.0
    b = np.zeros(3)
    for i in idx:
        n_i, n_ii = rows[i, 0:3], rows[i, 4:7]
        C += np.outer(n_ii, n_i)
        A += np.outer(n_i, n_i)
        b += n_i * (rows[i, 3] - rows[i, 7])
    U, S, Vt = np.linalg.svd(C)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        R = Vt.T @ np.diag([1.0, 1.0, -1.0]) @ U.T
    t = inv3_apply(A, b)
    return R, (None if t is None else -t), float(S[2] / S[0])


def score_trial(rows, seed, trial, dist=TRIM_DIST, degenerate_thr=TRIM_DEGENERATE, max_redraws=TRIM_MAX_REDRAWS, margin=1e-9):
    """One trial: (inlier count, has_model, mask, near) -- near: some row lies within `margin` of a threshold, or the
    fit's sigma_min / sigma_max lies within `margin` of FIT_RCOND.  A draw whose translation system is singular or
    whose C is rank-deficient (sigma_min <= FIT_RCOND sigma_max: the drawn n_ii coplanar) scores 0."""
    n = len(rows)
    idx = None
    for redraw in range(max_redraws):
        cand = draw3(seed, trial, redraw, n)
        if not degenerate(rows, cand, degenerate_thr):
            idx = cand
            break
    if idx is None:
        return 0, False, np.zeros(n, bool), False
    R, t, rcond = fit_pair(rows, idx)
    if t is None or not rcond > FIT_RCOND:
        return 0, True, np.zeros(n, bool), t is None or abs(rcond - FIT_RCOND) < margin
    n_i = rows[:, 0:3]
    Rn = rotate_rows(R, rows[:, 4:7])
    d_err = np.abs((rows[:, 7] - ((t[0] * n_i[:, 0] + t[1] * n_i[:, 1]) + t[2] * n_i[:, 2])) - rows[:, 3])
    cr = np.cross(n_i, Rn)
    a_err = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    mask = (d_err < dist) & (a_err < dist / 2)
    near = bool(np.any(np.abs(d_err - dist) < margin) or np.any(np.abs(a_err - dist / 2) < margin)
                or abs(rcond - FIT_RCOND) < margin)
    return int(mask.sum()), True, mask, near


def adaptive_trials(count, n_rows, prob=TRIM_PROB):
    """Hartley-Zisserman's bound as MRPT's RANSAC::execute applies it."""
    eps = np.finfo(np.float64).eps
    f = count / n_rows
    p_no = 1.0 - f * f * f
    p_no = min(1.0 - eps, max(eps, p_no))
    return math.log(1.0 - prob) / math.log(p_no)


def trim(rows, seed, dist=TRIM_DIST, degenerate_thr=TRIM_DEGENERATE, max_iter=TRIM_MAX_ITER, prob=TRIM_PROB,
         max_redraws=TRIM_MAX_REDRAWS):
    """trimOutliersRANSAC, sequential over the trial index.  Returns (rows kept, stats): stats = inliers, trials,
    winner, no_model, mask.  Row count <= 3 and no model leave the rows untouched."""
    n = len(rows)
    st = {"inliers": n, "trials": 0, "winner": -1, "no_model": False, "mask": np.ones(n, bool)}
    if n <= 3:
        return rows, st
    best, N, trial, best_mask = -1, float("inf"), 0, None
    while trial < N and trial < max_iter:
        c, has, mask, _ = score_trial(rows, seed, trial, dist, degenerate_thr, max_redraws)
        if has and c > best:
            best, best_mask = c, mask
            st["winner"] = trial
            N = adaptive_trials(c, n, prob)
        trial += 1
    st["trials"] = trial
    if best < 0:
        st["no_model"] = True
        return rows, st
    st["inliers"] = best
    st["mask"] = best_mask
    return rows[best_mask], st


# ------------------------------------------------------------------ the collector
COLLECT_MIN_INLIERS = 1000
COLLECT_MAX_ELONGATION = 5.0
COLLECT_MIN_DOT = 0.99
COLLECT_MAX_DIST = 0.2


def collect(local, labf, Rt, min_inliers=COLLECT_MIN_INLIERS, max_elongation=COLLECT_MAX_ELONGATION,
            min_dot=COLLECT_MIN_DOT, max_dist=COLLECT_MAX_DIST):
    """GetControlPlanes.cpp:358-469 on one frame.  local[s]: the sensor's planes in its own frame (dicts: normal, d,
    elongation, labels); labf [8][h][w]: the final label image; Rt [8][4][4]: the extrinsics the frame was built with.
    A plane's pixels are those of labf[s] that carry one of its labels; its rig-frame normal is R n and its rig-frame
    distance d - (R n) . t.  Returns ({(s1, s2): rows}, cov [8][3][3]): the rows in the reference's loop order, and
    the adjacent pairs' sums of n_i n_j^T (rig frame), the pair (0, 7) under 7 (:446-462)."""
    w = labf.shape[2]
    rig = []
    for s in range(NUM_SENSORS):
        R, t = np.asarray(Rt[s], np.float64)[:3, :3], np.asarray(Rt[s], np.float64)[:3, 3]
        idx = np.arange(labf[s].size)
        rc = idx // w + idx % w
        out = []
        for p in local[s]:
            n_s = np.asarray(p["normal"], np.float64)
            n = np.array([(R[r, 0] * n_s[0] + R[r, 1] * n_s[1]) + R[r, 2] * n_s[2] for r in range(3)])
            d = float(p["d"]) - ((n[0] * t[0] + n[1] * t[1]) + n[2] * t[2])
            m = np.isin(labf[s].ravel(), p["labels"])
            cnt = int(m.sum())
            out.append((n, d, cnt, (int(rc[m].sum()) / cnt) if cnt else 0.0))
        rig.append(out)
    rows, cov = {}, np.zeros((NUM_SENSORS, 3, 3))
    for (s1, s2) in PAIRS:
        for i, a in enumerate(rig[s1]):
            for j, b in enumerate(rig[s2]):
                pa, pb = local[s1][i], local[s2][j]
                if not (a[2] > min_inliers and b[2] > min_inliers and pa["elongation"] < max_elongation
                        and pb["elongation"] < max_elongation
                        and (a[0][0] * b[0][0] + a[0][1] * b[0][1]) + a[0][2] * b[0][2] > min_dot and abs(a[1] - b[1]) < max_dist):
                    continue
                row = [*np.asarray(pa["normal"], np.float64), float(pa["d"]), *np.asarray(pb["normal"], np.float64), float(pb["d"]),
                       float(min(a[2], b[2])), max(a[3], b[3])]
                rows.setdefault((s1, s2), []).append(row)
                k = s1 if s2 - s1 == 1 else (s2 if s2 - s1 == 7 else -1)
                if k >= 0:
                    cov[k] += np.outer(a[0], b[0])
    return {p: np.array(r) for p, r in rows.items()}, cov


def adjacent_conditioning(cov):
    out = np.ones(NUM_SENSORS)
    for k in range(NUM_SENSORS):
        if np.any(cov[k]):
            s = np.linalg.svd(cov[k], compute_uv=False)
            out[k] = s.max() / s.min() if s.min() > 0 else np.inf
    return out


# ------------------------------------------------------------------ files
def load_dir(path):
    """loadPlaneCorrespondences (:304-323): {(i, j): rows} of the correspondences_i_j.txt present."""
    import os
    out = {}
    for (i, j) in PAIRS:
        f = os.path.join(path, f"correspondences_{i}_{j}.txt")
        if os.path.exists(f):
            out[(i, j)] = np.loadtxt(f, dtype=np.float64, ndmin=2)
    return out
