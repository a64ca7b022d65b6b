#!/usr/bin/env python3
"""Wall time of keeping a snapshot current through whole-record replacements and Mode B metric
updates, each call plus the first yoda_run after it, to completion:
  - yoda_replace_nodes of 1, 64, 1,024 and 16,384 random nodes (each takes another node's record)
    against yoda_update_node_cards of the SAME lists and against yoda_upload_nodes, on config 3
    and mixed50 (Mode A);
  - yoda_update_node_metrics, dense (every node) and sparse (1,024 nodes), against
    yoda_upload_nodes, on config 3 in Mode B.
Every repetition runs in a fresh process (this script with --one), the workloads interleaved per
repetition; the parent prints each child's line and the medians.  Run on a GPU box:
    python tools/replace_timing.py > profiles/replacenodes/timing.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "kubernetes-scheduler_amd")


def timed(y, mode, call):
    """(call ms, call + first run ms)."""
    y.synchronize()
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    y.run(mode)
    y.synchronize()
    t2 = time.perf_counter()
    return round((t1 - t0) * 1e3, 3), round((t2 - t0) * 1e3, 3)


def one(workload, sizes, steady_steps, seed):
    sys.path.insert(0, PKG)
    import numpy as np
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_DISKIO

    (name, nodes, pods, mode, kw), = synth.variant_workloads([workload])
    rng = np.random.default_rng(seed)
    n = nodes.n_nodes
    real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[:, None]
    out = {"workload": name, "pods": pods.n_pods, "nodes": n, "seed": seed}
    with Yoda(0) as y:
        y.upload_nodes(nodes, **kw)
        y.upload_pods(pods)
        for _ in range(3):
            y.run(mode)
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(steady_steps):
            y.run(mode)
        y.synchronize()
        out["steady_step_ms"] = round((time.perf_counter() - t0) / steady_steps * 1e3, 3)
        out["upload"] = timed(y, mode, lambda: y.upload_nodes(nodes, **kw))
        if mode == MODE_DISKIO:
            cpu, disk = rng.random(n) * 100.0, rng.random(n) * 100.0
            out["metrics_dense"] = timed(y, mode, lambda: y.update_node_metrics(None, cpu, disk))
            ids = rng.choice(n, 1024, replace=False).astype(np.uint32)
            out["metrics_sparse_1024"] = timed(
                y, mode, lambda: y.update_node_metrics(ids, cpu[:1024], disk[:1024]))
            return out
        out["cards"], out["replace"] = {}, {}
        for s in sizes:
            ids = rng.choice(n, s, replace=False).astype(np.uint32)
            total = nodes.card_total_memory[ids]
            free = np.minimum((rng.random(total.shape) * (total.astype(np.float64) + 1))
                              .astype(np.uint64), total)
            free = np.where(real[ids], free, 0).astype(np.uint64)
            healthy = (((nodes.card_healthy[ids] != 0) ^ (rng.random(total.shape) < 0.2))
                       & real[ids]).astype(np.uint8)
            fsum = free.sum(axis=1, dtype=np.uint64)
            out["cards"][str(s)] = timed(y, mode, lambda: y.update_cards(ids, free, healthy, fsum))
            recs = nodes.take((ids.astype(np.int64) + 1 + rng.integers(0, n - 1, s)) % n)
            # (NodeSoA.normalized, part of the Python wrapper, is inside the call's time)
            out["replace"][str(s)] = timed(y, mode, lambda: y.replace_nodes(ids, recs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,mixed50,diskio")
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steady", type=int, default=20)
    ap.add_argument("--one", default=None, help="(child) run one repetition of this workload")
    ap.add_argument("--seed", type=int, default=99)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.one:
        print(json.dumps(one(args.one, sizes, args.steady, args.seed)), flush=True)
        return
    rows = {}
    for rep in range(args.reps):
        for w in args.workloads.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", w, "--sizes",
                                args.sizes, "--steady", str(args.steady), "--seed",
                                str(args.seed + rep)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                sys.exit(r.returncode)
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.setdefault(w, []).append(json.loads(line))
    med = statistics.median

    def fold(vals):  # [(call, call + run)] -> medians
        return {"call_ms": round(med(v[0] for v in vals), 3),
                "call_plus_run_ms": round(med(v[1] for v in vals), 3)}

    for w, rs in rows.items():
        out = {"workload": w, "reps": len(rs), "median": True,
               "steady_step_ms": round(med(r["steady_step_ms"] for r in rs), 3),
               "upload": fold([r["upload"] for r in rs])}
        for key in ("metrics_dense", "metrics_sparse_1024"):
            if key in rs[0]:
                out[key] = fold([r[key] for r in rs])
        for key in ("cards", "replace"):
            if key in rs[0]:
                out[key] = {s: fold([r[key][s] for r in rs]) for s in rs[0][key]}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
