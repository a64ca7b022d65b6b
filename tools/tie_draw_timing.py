#!/usr/bin/env python3
"""What the selectHost draw (yoda_set_tie_draw) adds to a step: the steady-state yoda_run with
the draw off and on, interleaved, per workload.  Run on a GPU box:
    python tools/tie_draw_timing.py > profiles/tiedraw/timing.txt
Workloads: the bench variants of yoda_amd.synth (c3, diskio, diskio_distinct, ...) and
`dense8`: make_nodes(N / 8, 3) repeated 8 times against make_pods(P, 5) -- every schedulable pod
ties over 8 nodes.  Each figure is the wall time of a window of steps ending in a synchronize,
per step; the windows alternate off / on, --reps times each.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,dense8,diskio,diskio_distinct")
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0, help="timed work per window")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "kubernetes-scheduler_amd"))
    import numpy as np
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_SCV, NodeSoA

    def workloads():
        for name in args.workloads.split(","):
            if name == "dense8":
                base = synth.make_nodes(args.nodes // 8, 3)
                nodes = NodeSoA(**{f: np.concatenate([getattr(base, f)] * 8, axis=0)
                                   for f in base.__dataclass_fields__}).normalized()
                yield name, nodes, synth.make_pods(args.pods, 5), MODE_SCV, {}
            else:
                yield from synth.variant_workloads([name])

    def window(y, mode, steps):
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            y.run(mode)
        y.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for name, nodes, pods, mode, kw in workloads():
        with Yoda(0) as y:
            y.upload_nodes(nodes, **kw)
            y.upload_pods(pods)
            res, steps = {}, {}
            for on in (False, True):  # warm both, size the windows
                y.set_tie_draw(args.seed if on else None)
                y.run(mode)
                one = window(y, mode, 2)
                steps[on] = max(3, min(200, math.ceil(args.window_ms / max(one, 1e-3))))
                res[on] = []
            r = y.download()
            tied = int(((r.status == 0) & (r.n_ties >= 2)).sum())
            for _ in range(args.reps):
                for on in (False, True):
                    y.set_tie_draw(args.seed if on else None)
                    res[on].append(window(y, mode, steps[on]))
            y.set_tie_draw(None)
            med = statistics.median
            out = {"workload": name, "pods": pods.n_pods, "nodes": nodes.n_nodes, "mode": mode,
                   "path": y.path, "tied_pods": tied, "max_ties": int(r.n_ties.max()),
                   "steps_per_window": {"off": steps[False], "on": steps[True]},
                   "off_ms": round(med(res[False]), 4), "on_ms": round(med(res[True]), 4),
                   "added_ms": round(med(res[True]) - med(res[False]), 4),
                   "off_all_ms": [round(t, 4) for t in res[False]],
                   "on_all_ms": [round(t, 4) for t in res[True]]}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
