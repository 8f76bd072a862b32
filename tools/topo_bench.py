#!/usr/bin/env python3
"""Times r360_topo_partition on the "rooms" graphs of tests/_topo_cases.py at n = 32, 100 and 256 nodes: a lone call
and a batch of 16 graphs (seeds 1 .. 16) in one r360_topo_partition_batch call, and the numpy model (tests/topo_model.py)
on the same inputs on the CPU.  Every call is synchronous (it reads back one integer per recursion level and the
labels at the end), so the host clock around a call measures all of it: upload, launches, read-backs, host numbering.
The median of --reps calls after --warmup, with min and max.  The parts are checked against the model's before a
case is timed.  There is no reference timing (MRPT is not part of the reference tree), so no figure here is a pass /
fail bar.

    python tools/topo_bench.py [--json out.json] [--markdown out.md]
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
import _topo_cases as Cs  # noqa: E402
import topo_model as M  # noqa: E402

SIZES = [(32, 3), (100, 6), (256, 12)]
BATCH = 16


def timed(fn, warmup, reps):
    ms = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if rep >= warmup:
            ms.append(dt)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("topo_bench: no GPU")
    ctx = R.Context(0)
    rows = []
    for n, rooms in SIZES:
        graphs = [Cs.rooms_graph(n, rooms, seed) for seed in range(1, BATCH + 1)]
        bis = [[] for _ in graphs]
        model = [M.part_of(M.partition(A, bisections=b), n) for A, b in zip(graphs, bis)]
        lone = R.topo_partition(ctx, graphs[0])
        batch = R.topo_partition_batch(ctx, graphs)
        # a part may differ from the model's where a Fiedler entry sits at the mean to rounding: counted, not hidden
        equal = sum(int(np.array_equal(g, m)) for g, m in zip(batch, model))
        assert np.array_equal(lone, batch[0])
        row = {"n": n, "rooms": rooms, "parts_lone": int(lone.max()) + 1, "bisections_lone": len(bis[0]),
               "bisections_batch": sum(len(b) for b in bis), "batch_equal_to_model": equal, "batch": BATCH}
        row["gpu_lone_ms"] = timed(lambda: R.topo_partition(ctx, graphs[0]), a.warmup, a.reps)
        row["gpu_batch_ms"] = timed(lambda: R.topo_partition_batch(ctx, graphs), a.warmup, a.reps)
        row["gpu_bisect_ms"] = timed(lambda: R.topo_bisect(ctx, graphs[0]), a.warmup, a.reps)
        row["model_lone_ms"] = timed(lambda: M.partition(graphs[0]), 1, a.reps)
        row["model_batch_ms"] = timed(lambda: [M.partition(A) for A in graphs], 1, max(3, a.reps // 3))
        row["sweeps_top"] = R.topo_bisect(ctx, graphs[0])["sweeps"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    res = {"reps": a.reps, "warmup": a.warmup, "cpu_threads": os.environ.get("OMP_NUM_THREADS"), "cases": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    if a.markdown:
        fmt = lambda t: f"{t[0]:.3g} ({t[1]:.3g} .. {t[2]:.3g})"
        lines = ["| n | parts, bisections (lone) | top bisection: sweeps, ms | GPU lone, ms (min .. max) | numpy lone, ms | "
                 "GPU batch of 16, ms | numpy 16 graphs, ms | batch parts equal to the model's |", "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['n']} | {r['parts_lone']}, {r['bisections_lone']} | {r['sweeps_top']}, {fmt(r['gpu_bisect_ms'])} | "
                         f"{fmt(r['gpu_lone_ms'])} | {fmt(r['model_lone_ms'])} | {fmt(r['gpu_batch_ms'])} | "
                         f"{fmt(r['model_batch_ms'])} | {r['batch_equal_to_model']} of {r['batch']} |")
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
