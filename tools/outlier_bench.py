#!/usr/bin/env python3
"""Times the outlier filters on the context's global map on the GPU (no pass bar; figures for DESIGN.md §5b-2 and
profiles/outliers/README.md).  GPU only: without a device the context cannot be created and the tool fails.

  map_filter_outliers   statistical (20, 1, 0.5) and radius (0.15, 5) on maps of about 0.33 M, 1.3 M and 5.2 M voxels,
                        built as tools/map_bench.py builds them (points on the walls of boxes of 12 / 24 / 48 m, 5 cm leaf)
  host way              smallest map only: download, the same filter over a host grid (numpy, one dense block of squared
                        distances per occupied cell against the 27 cells around it), upload as a new map

Each device figure is the median of --reps calls after --warmup calls, timed with device events on the context's stream
around the whole synchronous call; the map is restored before every call, outside the events.  "Candidates" is the
number of distance evaluations the walk would make if it pruned no cell and stopped no count early (every other point of
the (2 ring + 1)^3 cells around each point, ring 2 at edge max_dist / 2 for the statistical filter, ring 1 at edge radius
for the radius filter), computed on the host from the downloaded map: an upper bound of what the kernels evaluate, so
the rate printed from it is an upper bound too.  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/outlier_bench.py --quick` run (kernels k_outlier_*, k_out_*).

  python tools/outlier_bench.py [--reps 9] [--warmup 2] [--quick] [--no-host] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgbd360_amd as R  # noqa: E402
from tools.map_bench import room_cloud  # noqa: E402

LEAF = 0.05


def cell_keys(xyz, edge):
    c = np.floor(xyz.astype(np.float64) / edge).astype(np.int64)
    c -= c.min(0) - 2
    return c, (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def candidates(xyz, edge, ring):
    """Sum over the points of the other points in the (2 ring + 1)^3 cells around their own."""
    c, key = cell_keys(xyz, edge)
    uk, cnt = np.unique(key, return_counts=True)
    total = 0
    r = np.arange(-ring, ring + 1)
    for dz in r:
        for dy in r:
            for dx in r:
                nk = uk + (int(dz) << 42) + (int(dy) << 21) + int(dx)
                j = np.searchsorted(uk, nk)
                j[j == len(uk)] = 0
                hit = uk[j] == nk
                total += int((cnt[hit] * cnt[j[hit]]).sum())
    return total - len(xyz)


def host_filter(xyz, prm):
    """The model's rules over a host grid of edge = the search bound; returns the keep mask."""
    stat = prm.kind == R.OUTLIER_STATISTICAL
    lim = float(np.float32(prm.max_dist if stat else prm.radius))
    lim2, k = lim * lim, prm.mean_k
    c, key = cell_keys(xyz, lim * (1 + 2.0 ** -20))
    order = np.argsort(key, kind="stable")
    sk = key[order]
    uk, start = np.unique(sk, return_index=True)
    end = np.append(start[1:], len(sk))
    slot = {int(q): i for i, q in enumerate(uk)}
    p = xyz.astype(np.float64)[order]
    d = np.full(len(xyz), np.inf)
    cnt = np.zeros(len(xyz), np.int64)
    offs = [(dz << 42) + (dy << 21) + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    for i, q in enumerate(uk):
        s, e = start[i], end[i]
        parts, self_at = [], 0
        for o in offs:
            j = slot.get(int(q) + o)
            if j is None:
                continue
            if o == 0:
                self_at = sum(len(x) for x in parts)
            parts.append(p[start[j]:end[j]])
        cand = np.concatenate(parts)
        a = p[s:e]
        dx = cand[None, :, 0] - a[:, None, 0]
        dy = cand[None, :, 1] - a[:, None, 1]
        dz = cand[None, :, 2] - a[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(e - s), self_at + np.arange(e - s)] = np.inf     # the point itself
        if stat:
            if d2.shape[1] > k:
                near = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
                ok = near[:, k - 1] <= lim2
                d[order[s:e]] = np.where(ok, np.sqrt(near).sum(1) / k, np.inf)
        else:
            cnt[order[s:e]] = (d2 <= lim2).sum(1)
    if not stat:
        return cnt >= prm.min_neighbors
    good = np.isfinite(d)
    if not good.any():
        return good
    mean = d[good].mean()
    std = np.sqrt(((d[good] - mean) ** 2).sum() / (good.sum() - 1)) if good.sum() > 1 else 0.0
    return good & (d <= mean + float(np.float32(prm.stddev_mul)) * std)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="the smallest map and few calls (for a kernel trace)")
    ap.add_argument("--no-host", action="store_true", help="skip the host way")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("outlier_bench: no GPU")
    rng = np.random.default_rng(2016)
    ctx = R.Context(0)
    res = {"leaf": LEAF, "reps": a.reps, "rows": []}
    filters = (("statistical (20, 1, 0.5)", R.OutlierParams.statistical(20, 1.0, 0.5), 0.25, 2),
               ("radius (0.15, 5)", R.OutlierParams.radius_filter(0.15, 5), 0.15, 1))
    try:
        stream = torch.cuda.ExternalStream(int(R.lib().r360_ctx_stream(ctx.h)))
        reps, warm = (3, 1) if a.quick else (a.reps, a.warmup)
        sizes = ((250_000, 12.0),) if a.quick else ((250_000, 12.0), (1_000_000, 24.0), (4_000_000, 48.0))
        for idx, (target, extent) in enumerate(sizes):
            bx, bc = room_cloud(rng, 4 * target, np.array([extent, extent, extent / 3]))
            ctx.map_reset()
            ctx.map_add_cloud(bx, bc, LEAF)
            base_x, base_c = ctx.map_download()
            m0 = len(base_x)
            for name, prm, edge, ring in filters:
                ms, st = [], None
                for i in range(warm + reps):
                    ctx.map_reset()
                    ctx.map_add_cloud(base_x, base_c, LEAF)          # a voxel grid of a voxel grid: the same map
                    assert ctx.map_size() == m0
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    st = ctx.map_filter_outliers(prm)
                    e1.record(stream)
                    e1.synchronize()
                    if i >= warm:
                        ms.append(e0.elapsed_time(e1))
                cand = candidates(base_x, edge * (1 + 2.0 ** -20), ring)
                med = float(np.median(ms))
                row = {"case": f"map_filter_outliers {name}", "points_in": m0, "points_out": m0 - int(st.n_removed),
                       "short": int(st.n_short), "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                       "candidates_upper_bound": cand, "G_candidates_per_s_upper_bound": cand / med / 1e6}
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
                if idx == 0 and not a.no_host:
                    ctx.map_reset()
                    ctx.map_add_cloud(base_x, base_c, LEAF)
                    t0 = time.perf_counter()
                    mx, mc = ctx.map_download()                       # download, filter, upload as the new map
                    keep = host_filter(mx, prm)
                    ctx.map_reset()
                    ctx.map_add_cloud(mx[keep], mc[keep], LEAF)
                    dt = (time.perf_counter() - t0) * 1e3
                    row = {"case": f"host way {name} (one call, wall clock)", "points_in": m0,
                           "points_out": int(keep.sum()), "ms": dt, "same_count_as_device": int(keep.sum()) == m0 - int(st.n_removed)}
                    print(json.dumps(row), flush=True)
                    res["rows"].append(row)
    finally:
        ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
