#!/usr/bin/env python3
"""Times Generalized-ICP on the GPU (no pass bar: PCL cannot run here; figures for DESIGN.md §5c and
profiles/gicp/README.md).  GPU only: without a device the context cannot be created and the tool fails.

  voxel pair    the sphere clouds of two synthetic QVGA frames (r360_synth_frame, frames 0 and 3 of the benchmark's
                path), voxel-filtered with leaf 0.1 as RegisterPairRGBD360 does
  full pair     the same sphere clouds unfiltered (153,600 points each, non-finite rows included)

Per pair: set_source + set_target (intake, grid, kNN, covariances) and align from identity, each the median of --reps
calls after --warmup calls, timed with device events on the context's stream (the calls are synchronous, so the
events bracket the kernels, the copies and the host's part).  Beside them the wall time of the numpy statement
(tests/gicp_model.py, k-d tree queries on --workers threads) on the same inputs, and the pose difference.  Which
kernels dominate comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/gicp_bench.py --quick
--no-model` run (kernels k_gicp_*).

  python tools/gicp_bench.py [--reps 9] [--warmup 2] [--workers 16] [--quick] [--no-model] [--json out.json]"""
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
import gicp_model as GM  # noqa: E402

SEED = 360 << 16


def timed(stream, fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    out = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="few calls (for a kernel trace)")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gicp_bench: no GPU")
    GM.WORKERS = a.workers
    ctx = R.Context(0)
    res = {"reps": a.reps, "cases": []}
    cal = None
    frames = []
    try:
        stream = torch.cuda.ExternalStream(int(R.lib().r360_ctx_stream(ctx.h)))
        reps, warm = (2, 1) if a.quick else (a.reps, a.warmup)
        cal = R.Calib360(ctx, 240, 320)
        cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
        clouds = []
        for k in (0, 3):
            f = R.Frame360(cal)
            f.upload(*cal.synth_frame(SEED, R.synth_path_pose(SEED, k)))
            f.build(R.BUILD_UNDISTORT | R.BUILD_CLOUD)
            frames.append(f)
            clouds.append(f.sphereCloud()[0])
        voxel = [ctx.filter_voxel(c, None, 0.1)[0] for c in clouds]
        p = R.GicpParams.default()
        mp = GM.Params().as_float32()
        for name, (tgt, src) in (("voxel pair (leaf 0.1)", voxel), ("full pair", clouds)):
            def set_both():
                ctx.gicp_set_source(src, p)
                ctx.gicp_set_target(tgt, p)

            t_set = timed(stream, set_both, reps, warm)
            t_al = timed(stream, lambda: ctx.gicp_align(np.eye(4), p), reps, warm)
            pose, st, rc = t_al[3]
            row = {"case": name, "source_rows": int(len(src)), "target_rows": int(len(tgt)),
                   "source_kept": int(np.isfinite(src).all(1).sum()), "target_kept": int(np.isfinite(tgt).all(1).sum()),
                   "set_ms_median": t_set[0], "set_ms_min": t_set[1], "set_ms_max": t_set[2],
                   "align_ms_median": t_al[0], "align_ms_min": t_al[1], "align_ms_max": t_al[2], "status": rc,
                   "iterations": st.iterations, "inner_steps": st.inner_steps, "converged": st.converged,
                   "n_corr": st.n_corr, "fitness": st.fitness}
            if not a.no_model:
                t0 = time.perf_counter()
                ms_, mt_ = GM.Cloud(src, mp), GM.Cloud(tgt, mp)
                t1 = time.perf_counter()
                ref = GM.align(ms_, mt_, np.eye(4), mp)
                t2 = time.perf_counter()
                row.update({"model_set_ms": (t1 - t0) * 1e3, "model_align_ms": (t2 - t1) * 1e3,
                            "model_iterations": ref.iterations, "model_converged": ref.converged,
                            "drift_rad": GM.rot_angle(pose, ref.pose),
                            "drift_m": float(np.linalg.norm(pose[:3, 3] - ref.pose[:3, 3]))})
            print(json.dumps(row))
            res["cases"].append(row)
    finally:
        for f in frames:
            f.close()
        if cal is not None:
            cal.close()
        ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
