#!/usr/bin/env python3
"""Times the Euclidean cluster extraction on the context's global map on the GPU, next to the normal estimation and the
statistical outlier filter on the same map (no pass bar; figures for DESIGN.md §5b-4 and profiles/clusters/README.md).
GPU only: without a device the context cannot be created and the tool fails.

  map_cluster            plain and conditional (on the map's normals), at the default parameters unless given, on the map
                         of tools/normals_bench.py: about 1.3 M voxels on the walls of a box of 24 m, 5 cm leaf.  The
                         walls meet, so the plain form finds one component of the whole map: the longest root chases
                         and the most contended root a map of this size can give
  map_filter_clusters    the same clustering, then the compaction of the map (the map is restored before the next call)
  map_estimate_normals   k = 20 within 0.25 m, and map_filter_outliers statistical (20, 1, 0.25): the yardsticks, the
                         parent's own calls on the same map, which share the grid build

Each figure is the median of --reps calls after --warmup calls, timed with device events on the context's stream around
the whole synchronous call; the calls alternate, so that drift of the shared host falls on all.  The map is restored
outside the events.  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py --quick` run (kernels k_clu_*, k_out_*).

  python tools/cluster_bench.py [--tolerance 0.1] [--min-size 100] [--eps-deg 10] [--reps 9] [--warmup 2] [--quick]
                                [--json out.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgbd360_amd as R  # noqa: E402
from tools.map_bench import room_cloud  # noqa: E402

LEAF = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerance", type=float, default=0.10)
    ap.add_argument("--min-size", type=int, default=100)
    ap.add_argument("--eps-deg", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a map of about 0.33 M voxels and few calls (for a kernel trace)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cluster_bench: no GPU")
    rng = np.random.default_rng(2016)
    ctx = R.Context(0)
    res = {"leaf": LEAF, "tolerance": a.tolerance, "min_size": a.min_size, "eps_deg": a.eps_deg, "ring": 1,
           "union_rounds": 1, "compress_rounds": 1, "rows": []}
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
        cprm = R.ClusterParams.make(a.tolerance, a.min_size, eps_angle=math.radians(a.eps_deg))
        nprm = R.NormalParams.make(20, 0.25)
        oprm = R.OutlierParams.statistical(20, 1.0, 0.25)

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

        names = ["normals", "plain", "conditional", "filter_clusters", "filter_outliers"]
        t = {k: [] for k in names}
        st = {}
        for i in range(warm + reps):
            restore()
            d = {}
            d["normals"], st["normals"] = timed(lambda: ctx.map_estimate_normals(views, nprm))
            d["plain"], st["plain"] = timed(lambda: ctx.map_cluster(cprm))
            d["conditional"], st["conditional"] = timed(lambda: ctx.map_cluster(cprm, use_normals=True))
            d["filter_clusters"], st["filter_clusters"] = timed(lambda: ctx.map_filter_clusters(cprm))
            restore()
            d["filter_outliers"], st["filter_outliers"] = timed(lambda: ctx.map_filter_outliers(oprm))
            if i >= warm:
                for k in names:
                    t[k].append(d[k])
        med = {k: float(np.median(v)) for k, v in t.items()}

        def row(case, k, extra):
            return dict({"case": case, "points": m0, "ms_median": med[k], "ms_min": float(min(t[k])),
                         "ms_max": float(max(t[k])), "M_points_per_s": m0 / med[k] / 1e3}, **extra)

        def cst(s):
            return {"components": int(s.n_components), "clusters": int(s.n_clusters), "clustered": int(s.n_clustered)}

        rows = [
            row(f"map_cluster plain tol={a.tolerance} min={a.min_size}", "plain", cst(st["plain"])),
            row(f"map_cluster conditional eps={a.eps_deg} deg", "conditional", cst(st["conditional"])),
            row("map_filter_clusters plain", "filter_clusters", cst(st["filter_clusters"])),
            row("map_estimate_normals k=20 bound=0.25", "normals", {"short": int(st["normals"].n_short)}),
            row("map_filter_outliers statistical (20, 1, 0.25)", "filter_outliers",
                {"points_out": m0 - int(st["filter_outliers"].n_removed)}),
            {"case": "ratios to map_estimate_normals (medians)", "plain": med["plain"] / med["normals"],
             "conditional": med["conditional"] / med["normals"], "filter_clusters": med["filter_clusters"] / med["normals"],
             "filter_outliers": med["filter_outliers"] / med["normals"]},
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
