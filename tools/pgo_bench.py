#!/usr/bin/env python3
"""Times r360_graph_optimize on the shared 65-, 257- and 513-vertex pose graphs (tests/_pgo_cases.py) and on a
2049-vertex graph of the same recipe in the multi-launch form: device events on the context's stream around the whole
call (which includes its host decisions and read-backs), the median of --reps calls after --warmup, with min and max,
and the numpy model's wall time on the same inputs beside them.  At 257 vertices both CG forms are timed.  There is
no reference timing (g2o is not part of the reference tree), so no figure here is a pass / fail bar.  With
--robust-delta D one more row follows: the 257-vertex graph with a Huber kernel of width D on its loop edges.

    python tools/pgo_bench.py [--json out.json] [--robust-delta 1]
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
import _pgo_cases as Cs  # noqa: E402
import pgo_model as M  # noqa: E402

LOOPS_2049 = Cs.SIZED[513][1] + [(512, 1024), (0, 1024), (512, 1536), (1024, 1536), (0, 2048), (1024, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--robust-delta", type=float, default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pgo_bench: no GPU")
    ctx = R.Context(0)
    stream = torch.cuda.ExternalStream(int(R.lib().r360_ctx_stream(ctx.h)))
    res = {"reps": a.reps, "warmup": a.warmup, "cases": []}
    runs = [("n65", 0, None), ("n257", 1, None), ("n257", 2, None), ("n513", 0, None), ("n2049", 2, None)]
    if a.robust_delta is not None:
        runs.append(("n257", 1, a.robust_delta))
    model_s = {}
    for name, form, huber in runs:
        n = int(name[1:])
        if n in Cs.SIZED:
            g = Cs.build_sized(n, *Cs.SIZED[n])[0]
        else:
            g = Cs.build_sized(n, 1, LOOPS_2049)[0]
        pg = R.PoseGraph(ctx)
        for T in g.poses:
            pg.addVertex(T)
        for (i, j, Z, Om) in g.edges:
            pg.setRobustKernel(R.GRAPH_KERNEL_HUBER if huber and abs(i - j) != 1 else R.GRAPH_KERNEL_NONE, huber or 1.0)
            pg.addEdge(i, j, Z, Om)
        prm = R.GraphParams.default(cg_form=form)
        ms, st = [], None
        for rep in range(a.warmup + a.reps):
            for k, T in enumerate(g.poses):
                pg.setPose(k, T)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            st = pg.optimizeGraph(prm)
            e1.record(stream)
            e1.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        pg.close()
        if name not in model_s and not a.no_model and n <= 513:
            t0 = time.perf_counter()
            M.optimize(g)
            model_s[name] = time.perf_counter() - t0
        row = {"case": name if huber is None else f"{name} huber {huber:g} on the loop edges", "vertices": n,
               "edges": len(g.edges), "cg_form": st.cg_form, "status": st.status,
               "iterations": st.iterations, "trials": st.trials, "cg_iterations": st.cg_iterations,
               "cg_iterations_max": st.cg_iterations_max, "F_initial": st.F_initial, "F_final": st.F_final,
               "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
               "model_s": model_s.get(name) if huber is None else None}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
