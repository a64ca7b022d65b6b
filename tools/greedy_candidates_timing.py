#!/usr/bin/env python3
"""Wall time of yoda_greedy on config 5 with and without candidate classes
(yoda_greedy_candidates).  One process measures one case and prints one JSON line:

    --case steady           candidates never set (the path the setting does not touch); run it
                            from alternating processes against another build with --pkg
    --case share --share S  setting on, the recipe of tests/candidate_cases.py: 8 classes that
                            each lack a share S of the nodes, 64 nodes cordoned, pod classes
                            uniform over the classes and ANY

    seconds, pods_per_s     yoda_greedy of the whole batch (after a 4,096-pod warm-up)
    windows, restarts, fallbacks, refreshes    its work counters
    narrow_ms, narrow_share k_cand_narrow summed over the batch's windows (HIP events, a second
                            batch with the profile on) and its share of that batch's wall time

A time is printed only after the picks of the first --sample pods in queue order were compared
with tests/greedy_candidate_cases.reference (a queue prefix depends on no later pod).  Run on a
GPU box:
    python tools/greedy_candidates_timing.py --case share --share 0.01 --flags 1
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("steady", "share"), default="steady")
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--pods", type=int, default=None)
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests"), REPO]
    import numpy as np
    import candidate_cases as cc
    import greedy_candidate_cases as gc
    import oracle
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_SCV

    nodes, pods = synth.make_config(5, pods=args.pods, nodes=args.nodes)
    nodes, pods = nodes.normalized(), pods.normalized()
    P, n = pods.n_pods, nodes.n_nodes
    cand = args.case == "share"
    words = cls = None
    if cand:
        words, cls = cc.recipe(nodes, pods, seed=7, tenths=args.share)
    # the reference of a queue prefix (taken in queue order, the prefix is its own queue order)
    head = oracle.queue_order(pods)[:min(args.sample, P)]
    want = gc.reference(nodes, pods.take(head), words if cand else np.zeros(n, np.uint64),
                        cls[head] if cand else None, args.flags)

    out = {"case": args.case, "tag": args.tag, "flags": args.flags, "pods": P, "nodes": n,
           "sample": int(head.size)}
    if cand:
        out.update(classes=8, cordoned=64, missing_share=args.share)
    with Yoda(0) as y:
        y.upload_nodes(nodes)
        if cand:
            y.set_candidates(words, 8)
            y.greedy_candidates(True)
            y.set_pod_classes(cls[:min(P, 4096)])
        y.greedy(pods.slice(0, min(P, 4096)), MODE_SCV, args.flags)  # warm-up
        if cand:
            y.set_pod_classes(cls)
        t0 = time.perf_counter()
        picks = y.greedy(pods, MODE_SCV, args.flags)
        sec = time.perf_counter() - t0
        assert np.array_equal(picks[head], want), "picks differ from the reference"
        windows, fallbacks, times = y.greedy_stats(times=True)
        out.update(seconds=round(sec, 4), pods_per_s=round(P / sec), windows=windows,
                   restarts=y.greedy_restarts(), fallbacks=fallbacks,
                   refreshes=y.greedy_refreshes(),
                   **{k: round(v, 1) for k, v in times.items()})
        if cand and not args.no_profile:
            y.profile(True)
            y.profile_read()
            y.candidates_profile()
            t0 = time.perf_counter()
            again = y.greedy(pods, MODE_SCV, args.flags)
            sec2 = time.perf_counter() - t0
            k1, k2, _ = y.profile_read()
            nar = y.candidates_profile()
            y.profile(False)
            assert np.array_equal(again, picks), "the second batch's picks differ"
            out.update(profiled_seconds=round(sec2, 4), k1_ms=round(k1, 1), k2_ms=round(k2, 1),
                       narrow_ms=round(nar, 1), narrow_share=round(nar / (sec2 * 1e3), 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
