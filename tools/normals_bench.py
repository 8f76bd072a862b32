#!/usr/bin/env python3
"""Times the normal estimation on the context's global map on the GPU, next to the statistical outlier filter on the same
map (no pass bar; figures for DESIGN.md §5b-3 and profiles/normals/README.md).  GPU only: without a device the context
cannot be created and the tool fails.

  map_estimate_normals   k = 20 within the bound, on a map of about 1 M voxels built as tools/map_bench.py builds them
                         (points on the walls of a box of 24 m, 5 cm leaf); the viewpoints are 16 points inside the box
  map_filter_outliers    statistical, the same k and the same bound: the same walk without indices, moments and
                         eigen-solve (it also compacts the map, so the map is restored before every call)

Each figure is the median of --reps calls after --warmup calls, timed with device events on the context's stream around
the whole synchronous call; the two calls alternate, so that drift of the shared host falls on both.  The map is
restored outside the events.  The LDS per workgroup is computed from k as the launchers compute it, and the waves per CU
it allows from the 160 KiB of a CU (one wave per workgroup); the per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/normals_bench.py --quick` run (kernels k_normals, k_nrm_init, k_out_*).

  python tools/normals_bench.py [--k 20] [--bound 0.25] [--reps 9] [--warmup 2] [--quick] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgbd360_amd as R  # noqa: E402
from tools.map_bench import room_cloud  # noqa: E402

LEAF = 0.05
LDS_PER_CU = 160 * 1024


def lds_figures(k):
    """Dynamic LDS per 64-lane workgroup of the two walks and the workgroups (= waves) per CU it allows."""
    normals, knn = 12 * 64 * k, 8 * 64 * k
    return {"k": k, "k_normals_lds_bytes": normals, "k_normals_waves_per_cu_by_lds": LDS_PER_CU // normals,
            "k_outlier_knn_lds_bytes": knn, "k_outlier_knn_waves_per_cu_by_lds": LDS_PER_CU // knn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--bound", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a map of about 0.33 M voxels and few calls (for a kernel trace)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("normals_bench: no GPU")
    rng = np.random.default_rng(2016)
    ctx = R.Context(0)
    res = {"leaf": LEAF, "k": a.k, "bound": a.bound, "lds": [lds_figures(a.k), lds_figures(64)], "rows": []}
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
        nprm = R.NormalParams.make(a.k, a.bound)
        oprm = R.OutlierParams.statistical(a.k, 1.0, a.bound)

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            st = call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), st

        t_n, t_o, nst, ost = [], [], None, None
        for i in range(warm + reps):
            ctx.map_reset()
            ctx.map_add_cloud(base_x, base_c, LEAF)                  # a voxel grid of a voxel grid: the same map
            assert ctx.map_size() == m0
            dn, nst = timed(lambda: ctx.map_estimate_normals(views, nprm))
            do, ost = timed(lambda: ctx.map_filter_outliers(oprm))
            if i >= warm:
                t_n.append(dn)
                t_o.append(do)
        mn, mo = float(np.median(t_n)), float(np.median(t_o))
        rows = [
            {"case": f"map_estimate_normals k={a.k} bound={a.bound}", "points": m0, "short": int(nst.n_short),
             "mean_neighbours": nst.sum_neighbors / max(nst.n_finite, 1), "ms_median": mn, "ms_min": float(min(t_n)),
             "ms_max": float(max(t_n)), "M_points_per_s": m0 / mn / 1e3},
            {"case": f"map_filter_outliers statistical ({a.k}, 1, {a.bound})", "points": m0, "short": int(ost.n_short),
             "points_out": m0 - int(ost.n_removed), "ms_median": mo, "ms_min": float(min(t_o)), "ms_max": float(max(t_o)),
             "M_points_per_s": m0 / mo / 1e3},
            {"case": "ratio normals / filter (medians)", "ratio": mn / mo},
        ]
        for row in rows + res["lds"]:
            print(json.dumps(row), flush=True)
        res["rows"] = rows
    finally:
        ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
