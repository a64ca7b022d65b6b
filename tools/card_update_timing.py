#!/usr/bin/env python3
"""Wall time of keeping a snapshot current: yoda_upload_nodes + the first yoda_run after it,
against yoda_update_node_cards (1, 64, 1,024, 16,384 random nodes) + the first yoda_run after
it, each to completion, and the steady-state step beside both.  Medians of --reps repetitions,
interleaved (upload, then each list size, per repetition).  Run on a GPU box:
    python tools/card_update_timing.py > profiles/cardupdate/timing.txt
--pkg DIR times another build's package tree (a directory that holds yoda_amd/ with its
libyoda.so) and --upload-only skips the card updates: the parent commit's upload in the same
visit, which has no yoda_update_node_cards.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,mixed50")
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steady", type=int, default=20)
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    ap.add_argument("--upload-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import numpy as np
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_SCV

    sizes = [] if args.upload_only else [int(s) for s in args.sizes.split(",")]
    for name, nodes, pods, mode, kw in synth.variant_workloads(args.workloads.split(",")):
        assert mode == MODE_SCV
        rng = np.random.default_rng(99)
        real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[:, None]

        def draw(n):
            ids = rng.choice(nodes.n_nodes, n, replace=False).astype(np.uint32)
            total = nodes.card_total_memory[ids]
            free = np.minimum((rng.random(total.shape) * (total.astype(np.float64) + 1))
                              .astype(np.uint64), total)
            free = np.where(real[ids], free, 0).astype(np.uint64)
            healthy = ((nodes.card_healthy[ids] != 0) ^ (rng.random(total.shape) < 0.2)) & real[ids]
            return ids, free, healthy.astype(np.uint8), free.sum(axis=1, dtype=np.uint64)

        with Yoda(0) as y:
            y.upload_nodes(nodes, **kw)
            y.upload_pods(pods)
            for _ in range(3):
                y.run(mode)
            y.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steady):
                y.run(mode)
            y.synchronize()
            steady = (time.perf_counter() - t0) / args.steady * 1e3
            t_up, t_up_call = [], []
            t_upd = {s: [] for s in sizes}
            t_upd_call = {s: [] for s in sizes}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                y.upload_nodes(nodes, **kw)
                t1 = time.perf_counter()
                y.run(mode)
                y.synchronize()
                t2 = time.perf_counter()
                t_up.append((t2 - t0) * 1e3)
                t_up_call.append((t1 - t0) * 1e3)
                for s in sizes:
                    lst = draw(s)
                    y.synchronize()
                    t0 = time.perf_counter()
                    y.update_cards(*lst)
                    t1 = time.perf_counter()
                    y.run(mode)
                    y.synchronize()
                    t2 = time.perf_counter()
                    t_upd[s].append((t2 - t0) * 1e3)
                    t_upd_call[s].append((t1 - t0) * 1e3)
            med = statistics.median
            out = {"workload": name, "pods": pods.n_pods, "nodes": nodes.n_nodes,
                   "reps": args.reps, "pkg": os.path.relpath(os.path.abspath(args.pkg), REPO),
                   "steady_step_ms": round(steady, 3),
                   "upload_plus_run_ms": round(med(t_up), 3),
                   "upload_call_ms": round(med(t_up_call), 3),
                   "update_plus_run_ms": {str(s): round(med(t_upd[s]), 3) for s in sizes},
                   "update_call_ms": {str(s): round(med(t_upd_call[s]), 3) for s in sizes},
                   "upload_plus_run_all_ms": [round(t, 2) for t in t_up],
                   "update_plus_run_all_ms": {str(s): [round(t, 3) for t in t_upd[s]]
                                              for s in sizes}}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
