#!/usr/bin/env python3
"""Times the voxel grid and the context's global map on the GPU (no pass bar; figures for DESIGN.md §5b and
profiles/map/README.md).  GPU only: without a device the context cannot be created and the tool fails.

  filter_voxel      r360_cloud_filter_voxel on seeded clouds of 153,600 and 4 M points (host arrays in and out)
  map_add_frame     one keyframe (synthetic QVGA frame, 153,600 points) onto maps of about 0.25 M, 1 M and 4 M voxels
  host way          the same step as download, numpy Euclidean box + pose, upload + filter_voxel

Each figure is the median of --reps calls after --warmup calls, timed with device events on the context's stream (the
calls are synchronous, so the events bracket the kernels, the copies and the host decisions between them).  The
share of the HBM peak is algorithmic bytes (16 B per input point + 16 B per output point) over that time over
8.0 TB/s: a whole-call figure, not a kernel's.  Which passes dominate comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/map_bench.py --quick` run (kernels k_map_*).

  python tools/map_bench.py [--reps 9] [--warmup 2] [--quick] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgbd360_amd as R  # noqa: E402

HBM_PEAK = 8.0e12
LEAF = 0.05
SEED = 360 << 16


def room_cloud(rng, n, extent):
    """n points on the walls of a box of `extent` metres (surfaces, as a sphere cloud is), with random colours."""
    p = rng.uniform(-0.5, 0.5, (n, 3)) * extent
    ax = rng.integers(0, 3, n)
    p[np.arange(n), ax] = np.where(rng.random(n) < 0.5, -0.5, 0.5) * extent[ax] + rng.normal(0, 0.003, n)
    return p.astype(np.float32), rng.integers(0, 2 ** 24, n, dtype=np.uint32)


def timed(stream, fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
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
    ap.add_argument("--quick", action="store_true", help="small sizes and few calls (for a kernel trace)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("map_bench: no GPU")
    rng = np.random.default_rng(2016)
    ctx = R.Context(0)
    res = {"leaf": LEAF, "reps": a.reps, "hbm_peak_TBps": HBM_PEAK / 1e12, "filter_voxel": [], "map_add_frame": []}
    cal = frame = None
    try:
        stream = torch.cuda.ExternalStream(int(R.lib().r360_ctx_stream(ctx.h)))
        reps, warm = (3, 1) if a.quick else (a.reps, a.warmup)

        def row(name, n_in, n_out, t):
            med, lo, hi = t
            bytes_ = 16 * (n_in + n_out)
            r = {"case": name, "points_in": int(n_in), "points_out": int(n_out), "ms_median": med, "ms_min": lo, "ms_max": hi,
                 "algorithmic_GBps": bytes_ / med / 1e6, "share_of_hbm_peak": bytes_ / (med * 1e-3) / HBM_PEAK}
            print(json.dumps(r))
            return r

        for n in ((153600,) if a.quick else (153600, 4_000_000)):
            xyz, rgba = room_cloud(rng, n, np.array([8.0, 6.0, 3.0]))
            med, lo, hi, out = timed(stream, lambda: ctx.filter_voxel(xyz, rgba, LEAF), reps, warm)
            res["filter_voxel"].append(row(f"filter_voxel n={n}", n, len(out[0]), (med, lo, hi)))

        cal = R.Calib360(ctx, 240, 320)
        cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
        pose = R.synth_path_pose(SEED, 3)
        frame = R.Frame360(cal)
        frame.upload(*cal.synth_frame(SEED, pose))
        frame.build(R.BUILD_UNDISTORT | R.BUILD_CLOUD)
        n_frame = 153600
        for target, extent in ((250_000, 12.0),) if a.quick else ((250_000, 12.0), (1_000_000, 24.0), (4_000_000, 48.0)):
            # a base map of about `target` voxels: walls of a box sized so that they hold that many 5 cm cells
            bx, bc = room_cloud(rng, 4 * target, np.array([extent, extent, extent / 3]))
            ctx.map_reset()
            ctx.map_add_cloud(bx, bc, LEAF)
            base_x, base_c = ctx.map_download()
            m0 = len(base_x)

            def dev():
                ctx.map_reset()
                ctx.map_add_cloud(base_x, base_c, LEAF)
                return None

            # the timed call must start from the same map every time: restore it outside the events
            def step_device():
                ok = ctx.map_add_frame(frame, pose, LEAF)
                return ok

            def step_host():
                mx, mc = ctx.map_download()
                sx, sc, _, _ = frame.sphereCloud()
                keep = (np.isfinite(sx).all(1) & (sx[:, 0] >= -2) & (sx[:, 0] <= 1) & (np.abs(sx[:, 1:]) <= 4).all(1))
                p = sx[keep]
                T = pose.astype(np.float32)
                q = (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
                return ctx.filter_voxel(np.vstack([mx, q]), np.concatenate([mc, sc[keep]]), LEAF)

            for name, fn in (("map_add_frame", step_device), ("host way", step_host)):
                ms = []
                m1 = 0
                for i in range(warm + reps):
                    dev()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    out = fn()
                    e1.record(stream)
                    e1.synchronize()
                    if i >= warm:
                        ms.append(e0.elapsed_time(e1))
                    m1 = ctx.map_size() if name == "map_add_frame" else len(out[0])
                res["map_add_frame"].append(row(f"{name} onto {m0} voxels", m0 + n_frame, m1,
                                                (float(np.median(ms)), float(min(ms)), float(max(ms)))))
    finally:
        if frame is not None:
            frame.close()
        if cal is not None:
            cal.close()
        ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
