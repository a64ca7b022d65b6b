#!/usr/bin/env python3
"""Wall time of taking nodes out of a live snapshot, against the only other way: a re-upload of
the compacted snapshot.  Per workload and absent set (1, 64, 1,024, 16,384 nodes; scattered, or as
whole 64-node blocks where the size allows):
    present_call_ms        yoda_set_node_present(absent) alone
    present_plus_run_ms    ... plus the first yoda_run after it, to completion
    absent_step_ms         the steady step while they are absent
    return_call_ms         yoda_set_node_present(present) of the same list
    upload_call_ms         yoda_upload_nodes of the compacted snapshot (a second handle)
    upload_plus_run_ms     ... plus the first yoda_run after it
    compact_step_ms        the steady step of that fresh upload
and steady_step_ms, the step with every node present.  Medians of --reps repetitions,
interleaved.  Run on a GPU box:
    python tools/node_present_timing.py > profiles/nodepresent/timing.txt
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steady", type=int, default=10)
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import numpy as np
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_SCV

    med = statistics.median

    def steady(y, mode, k):
        for _ in range(2):
            y.run(mode)
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            y.run(mode)
        y.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    for name, nodes, pods, mode, kw in synth.variant_workloads(args.workloads.split(",")):
        assert mode == MODE_SCV
        n = nodes.n_nodes
        rng = np.random.default_rng(77)
        with Yoda(0) as y, Yoda(0) as y2:
            y.upload_nodes(nodes, **kw)
            y.upload_pods(pods)
            y2.upload_nodes(nodes, **kw)
            y2.upload_pods(pods)
            base = steady(y, mode, args.steady)
            print(json.dumps({"workload": name, "pods": pods.n_pods, "nodes": n,
                              "steady_step_ms": round(base, 3)}), flush=True)
            for size in (int(s) for s in args.sizes.split(",")):
                for pattern in ("scattered", "blocks"):
                    if pattern == "blocks" and size < 64:
                        continue
                    t = {k: [] for k in ("present_call_ms", "present_plus_run_ms",
                                         "absent_step_ms", "return_call_ms", "upload_call_ms",
                                         "upload_plus_run_ms", "compact_step_ms")}
                    for _ in range(args.reps):
                        if pattern == "scattered":
                            ids = rng.choice(n, size, replace=False)
                        else:
                            b = rng.choice(n // 64, size // 64, replace=False)
                            ids = (64 * b[:, None] + np.arange(64)[None, :]).ravel()
                        ids = np.sort(ids).astype(np.uint32)
                        keep = np.setdiff1d(np.arange(n), ids)
                        y.synchronize()
                        t0 = time.perf_counter()
                        y.set_node_present(ids, 0)
                        t1 = time.perf_counter()
                        y.run(mode)
                        y.synchronize()
                        t2 = time.perf_counter()
                        t["present_call_ms"].append((t1 - t0) * 1e3)
                        t["present_plus_run_ms"].append((t2 - t0) * 1e3)
                        t["absent_step_ms"].append(steady(y, mode, args.steady))
                        comp = nodes.take(keep)  # (the caller's compaction is not timed)
                        t0 = time.perf_counter()
                        y2.upload_nodes(comp, **kw)
                        t1 = time.perf_counter()
                        y2.run(mode)
                        y2.synchronize()
                        t2 = time.perf_counter()
                        t["upload_call_ms"].append((t1 - t0) * 1e3)
                        t["upload_plus_run_ms"].append((t2 - t0) * 1e3)
                        t["compact_step_ms"].append(steady(y2, mode, args.steady))
                        # both handles answer alike (picks of the compacted one mapped back)
                        a, c = y.download(), y2.download()
                        ok = c.pick >= 0
                        c.pick[ok] = keep[c.pick[ok]]
                        assert (a.pick == c.pick).all() and (a.n_feasible == c.n_feasible).all()
                        y.synchronize()
                        t0 = time.perf_counter()
                        y.set_node_present(ids, 1)
                        y.synchronize()
                        t["return_call_ms"].append((time.perf_counter() - t0) * 1e3)
                    out = {"workload": name, "absent": size, "pattern": pattern, "reps": args.reps}
                    out.update({k: round(med(v), 3) for k, v in t.items()})
                    out["absent_step_all_ms"] = [round(x, 3) for x in t["absent_step_ms"]]
                    out["compact_step_all_ms"] = [round(x, 3) for x in t["compact_step_ms"]]
                    print(json.dumps(out), flush=True)
            back = steady(y, mode, args.steady)
            print(json.dumps({"workload": name, "steady_step_after_ms": round(back, 3)}),
                  flush=True)


if __name__ == "__main__":
    main()
