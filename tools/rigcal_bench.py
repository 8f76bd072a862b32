#!/usr/bin/env python3
"""Times the rig calibration (r360_rigcal_rotation + r360_rigcal_translation) and the outlier trimmer on the largest
pair (r360_rigcal_trim) against the numpy statement tests/rigcal_model.py on the same rows, at three sizes: the
fixture's 1,090 rows (tests/golden/control_planes.npz, adjacent pairs), and those rows tiled with seeded noise (1e-3 on the
normals, renormalised, and on the distances) to 1e5 and 1e6 rows.  Wall time of the whole calls (host solves and read-backs included; the rows are on the device), the median of --reps after --warmup with min and max.  The model is timed once per size
(--no-model-above skips it above a row count).  No figure here is a pass / fail bar.

    python tools/rigcal_bench.py [--json profiles/rigcal/rigcal_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rgbd360_amd as R  # noqa: E402
import _rigcal_cases as Cs  # noqa: E402
import rigcal_model as M  # noqa: E402


def tiled(rows, target, seed):
    """The fixture's rows repeated with seeded noise until there are about `target` of them, pair shares kept."""
    total = sum(len(r) for r in rows.values())
    if target <= total:
        return rows
    rng = np.random.default_rng(seed)
    out = {}
    for p, r in rows.items():
        reps = int(np.ceil(target * len(r) / total / len(r)))
        t = np.tile(r, (reps, 1))
        for off in (0, 4):
            t[:, off:off + 3] += rng.normal(scale=1e-3, size=(len(t), 3))
            t[:, off:off + 3] /= np.linalg.norm(t[:, off:off + 3], axis=1, keepdims=True)
            t[:, off + 3] += rng.normal(scale=1e-3, size=len(t))
        out[p] = t
    return out


def timed(fn, warmup, reps):
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        res = fn()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1090, 100000, 1000000])
    ap.add_argument("--no-model-above", type=int, default=1 << 30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = R.Context(0)
    base = Cs.fixture_rows()
    S = M.construction_specs()
    res = {"reps": a.reps, "warmup": a.warmup, "cases": []}
    for size in a.sizes:
        rows = tiled(base, size, 360)
        n = sum(len(r) for r in rows.values())
        big = max(rows, key=lambda p: len(rows[p]))
        case = {"rows": n, "largest_pair": list(big), "largest_pair_rows": len(rows[big])}
        cal = R.RigCalibration(ctx)
        cal.setPairs(rows)
        cal.setInit(S)

        def solve():
            return cal.CalibrateRotation(), cal.CalibrateTranslation()
        case["gpu_solve"], (rs, ts) = timed(solve, a.warmup, a.reps)
        case["iterations"] = rs.iterations
        case["conditioning"] = [rs.conditioning[k] for k in range(rs.iterations)] + [ts.conditioning[0]]
        est = cal.estimate()

        # a trim replaces the pair's rows, so each repetition sets them again and uploads (one scored trial does it)
        # outside the timed region
        ms = []
        for k in range(a.warmup + a.reps):
            cal.setPair(*big, rows[big])
            cal.ransacEval(*big, 7, 0, 1)
            t0 = time.perf_counter()
            tst, _ = cal.trimOutliersRANSAC(*big, seed=7)
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        case["gpu_trim"] = {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}
        case["trim"] = {"inliers": tst.inliers, "trials": tst.trials, "winner": tst.winner}
        cal.close()
        if n <= a.no_model_above:
            t0 = time.perf_counter()
            mRt, mst = M.calibrate_rotation(rows, S)
            mRt, _ = M.calibrate_translation(rows, mRt)
            case["model_solve_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            _, mtr = M.trim(rows[big], 7)
            case["model_trim_ms"] = (time.perf_counter() - t0) * 1e3
            dr, dt = Cs.pose_diff(est, mRt)
            case["estimate_vs_model"] = {"rad": dr, "m": dt}
            case["trim_equal_to_model"] = bool((tst.inliers, tst.trials, tst.winner) == (mtr["inliers"], mtr["trials"], mtr["winner"]))
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
