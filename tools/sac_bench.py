#!/usr/bin/env python3
"""Times the RANSAC plane segmentation on the context's global map on the GPU, next to the cluster extraction and the
normal estimation on the same map (no pass bar; figures for DESIGN.md §5b-5 and profiles/sac/README.md).
GPU only: without a device the context cannot be created and the tool fails.

  map_sac_planes         plain and gated (on the map's normals), at the default parameters unless given, on the map of
                         tools/cluster_bench.py: about 1.3 M voxels on the walls of a box of 24 m, 5 cm leaf
  map_filter_planes      the same segmentation, then the compaction of the map (the map is restored before the next call)
  map_cluster            plain, default parameters, and map_estimate_normals k = 20 within 0.25 m: the yardsticks, the
                         parent's own calls on the same map

Each figure is the median of --reps calls after --warmup calls, timed with device events on the context's stream around
the whole synchronous call; the calls alternate, so that drift of the shared host falls on all.  The map is restored
outside the events.  Per plane the records give the hypotheses evaluated, that is the rounds.  The per-kernel split comes
from a separate `rocprofv3 --kernel-trace --stats -- python tools/sac_bench.py --quick` run (kernels k_sac_*, k_out_scan_*).

  python tools/sac_bench.py [--distance 0.05] [--min-inliers 100] [--max-planes 8] [--reps 9] [--warmup 2] [--quick]
                            [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgbd360_amd as R  # noqa: E402
from tools.map_bench import room_cloud  # noqa: E402

LEAF = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distance", type=float, default=0.05)
    ap.add_argument("--min-inliers", type=int, default=100)
    ap.add_argument("--max-planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a map of about 0.33 M voxels and few calls (for a kernel trace)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sac_bench: no GPU")
    rng = np.random.default_rng(2016)
    ctx = R.Context(0)
    res = {"leaf": LEAF, "distance": a.distance, "min_inliers": a.min_inliers, "max_planes": a.max_planes,
           "round": R.SAC_ROUND, "rows": []}
    try:
        stream = torch.cuda.ExternalStream(int(R.lib().r360_ctx_stream(ctx.h)))
        reps, warm = (3, 1) if a.quick else (a.reps, a.warmup)
        target, extent = (250_000, 12.0) if a.quick else (1_000_000, 24.0)
        bx, bc = room_cloud(rng, 4 * target, np.array([extent, extent, extent / 3]))
        ctx.map_add_cloud(bx, bc, LEAF)
        base_x, base_c = ctx.map_download()
        m0 = len(base_x)
        lo, hi = base_x.min(0), base_x.max(0)
        views = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), (16, 3)).astype(np.float32)
        sprm = R.SacParams.make(distance_threshold=a.distance, min_inliers=a.min_inliers, max_planes=a.max_planes)
        cprm = R.ClusterParams.default()
        nprm = R.NormalParams.make(20, 0.25)

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            st = call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), st

        def restore():
            ctx.map_reset()
            ctx.map_add_cloud(base_x, base_c, LEAF)                  # a voxel grid of a voxel grid: the same map
            assert ctx.map_size() == m0

        names = ["normals", "cluster", "plain", "gated", "filter_plain", "filter_gated"]
        t = {k: [] for k in names}
        st, planes = {}, {}
        for i in range(warm + reps):
            restore()
            d = {}
            d["normals"], st["normals"] = timed(lambda: ctx.map_estimate_normals(views, nprm))
            d["cluster"], st["cluster"] = timed(lambda: ctx.map_cluster(cprm))
            d["plain"], st["plain"] = timed(lambda: ctx.map_sac_planes(sprm))
            planes["plain"] = ctx.map_planes()
            d["gated"], st["gated"] = timed(lambda: ctx.map_sac_planes(sprm, use_normals=True))
            planes["gated"] = ctx.map_planes()
            d["filter_gated"], st["filter_gated"] = timed(lambda: ctx.map_filter_planes(sprm, use_normals=True))
            restore()
            d["filter_plain"], st["filter_plain"] = timed(lambda: ctx.map_filter_planes(sprm))
            if i >= warm:
                for k in names:
                    t[k].append(d[k])
        med = {k: float(np.median(v)) for k, v in t.items()}

        def row(case, k, extra):
            return dict({"case": case, "points": m0, "ms_median": med[k], "ms_min": float(min(t[k])),
                         "ms_max": float(max(t[k])), "M_points_per_s": m0 / med[k] / 1e3}, **extra)

        def sst(s, pl=None):
            out = {"planes": int(s.n_planes), "in_planes": int(s.n_in_planes), "evaluated": int(s.n_evaluated),
                   "rounds": -(-int(s.n_evaluated) // R.SAC_ROUND)}
            if pl is not None:
                out["plane_sizes"] = [int(v) for v in pl["size"]]
                out["plane_rounds"] = [-(-int(v) // R.SAC_ROUND) for v in pl["evaluated"]]
            return out

        rows = [
            row(f"map_sac_planes plain dist={a.distance} min={a.min_inliers}", "plain", sst(st["plain"], planes["plain"])),
            row("map_sac_planes gated, on the map's normals", "gated", sst(st["gated"], planes["gated"])),
            row("map_filter_planes plain", "filter_plain", sst(st["filter_plain"])),
            row("map_filter_planes gated", "filter_gated", sst(st["filter_gated"])),
            row("map_cluster plain, defaults", "cluster", {"components": int(st["cluster"].n_components)}),
            row("map_estimate_normals k=20 bound=0.25", "normals", {"short": int(st["normals"].n_short)}),
            {"case": "ratios to map_estimate_normals (medians)", **{k: med[k] / med["normals"] for k in names if k != "normals"}},
        ]
        for r in rows:
            print(json.dumps(r), flush=True)
        res["rows"] = rows
    finally:
        ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
