#!/usr/bin/env python3
"""Wall time of candidate classes (yoda_set_candidates) on a live snapshot.  Per workload:
    steady_step_ms          the step with candidates never set
    ones_step_ms            candidates on, all-ones words, one class: the pass skips every block;
                            what remains is its launch and the K2 pruning seeds it turns off
and per share of the nodes each of 8 classes lacks (the recipe of tests/candidate_cases.py, 64
nodes cordoned):
    set_call_ms             yoda_set_candidates of the whole table
    step_ms                 the steady step
    k1_ms, k2_ms, narrow_ms K1, K2 and k_cand_narrow alone per step (HIP events)
    update_N_call_ms        yoda_update_candidates of N nodes (1, 64, 1,024)
    update_N_plus_run_ms    ... plus the first yoda_run after it, to completion
Medians of --reps repetitions, interleaved.  Before a time is printed the handle's answers are
compared with candidate_cases.reference on a --sample pod sample.  Run on a GPU box:
    python tools/candidates_timing.py > profiles/candidates/timing.txt
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
    ap.add_argument("--shares", default="0.01,0.3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steady", type=int, default=10)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests"), REPO]
    import numpy as np
    import candidate_cases as cases
    from yoda_amd import synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_SCV

    med = statistics.median

    def steady(y, k):
        for _ in range(2):
            y.run(MODE_SCV)
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            y.run(MODE_SCV)
        y.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    def kernels(y, k):
        y.profile(True)
        y.profile_read()
        y.candidates_profile()
        for _ in range(k):
            y.run(MODE_SCV)
        k1, k2, n = y.profile_read()
        nar = y.candidates_profile()
        y.profile(False)
        return k1 / k, k2 / k, nar / k

    shares = [float(s) for s in args.shares.split(",")]
    for name, nodes, pods, mode, kw in synth.variant_workloads(args.workloads.split(",")):
        assert mode == MODE_SCV
        n, P = nodes.n_nodes, pods.n_pods
        rng = np.random.default_rng(77)
        sample = np.sort(rng.choice(P, min(args.sample, P), replace=False))
        sub = pods.take(sample)
        snap = cases.Snapshot(cases.Model(nodes), sub)  # the maxima and raw scores of the sample
        tables = {s: cases.recipe(nodes, pods, seed=7, tenths=s) for s in shares}

        def verify(y, words, n_classes, cls):
            m = cases.Model(nodes)
            m.apply(("cand", n_classes, words))
            m.apply(("classes", None if cls is None else cls[sample]))
            want, _ = cases.reference(snap, m)
            got = y.download()
            for f in ("pick", "status", "n_feasible"):
                assert (getattr(got, f)[sample] == getattr(want, f)).all(), (name, f)
            ok = want.status == 0
            assert (got.top_score[sample][ok] == want.top_score[ok]).all(), name
            assert (got.maxima[sample] == want.maxima).all(), name

        t = {"steady_step_ms": [], "ones_step_ms": []}
        per = {s: {} for s in shares}
        with Yoda(0) as y:
            y.upload_nodes(nodes, **kw)
            y.upload_pods(pods)
            for rep in range(args.reps):
                y.set_candidates(None, 0)
                t["steady_step_ms"].append(steady(y, args.steady))
                ones = np.ones(n, np.uint64)
                y.set_candidates(ones, 1)
                y.set_pod_classes(np.zeros(P, np.uint8))
                t["ones_step_ms"].append(steady(y, args.steady))
                if rep == 0:  # (the reference once per table: the later repetitions time only)
                    verify(y, ones, 1, np.zeros(P, np.uint8))
                for s in shares:
                    words, cls = tables[s]
                    d = per[s]
                    y.synchronize()
                    t0 = time.perf_counter()
                    y.set_candidates(words, 8)
                    d.setdefault("set_call_ms", []).append((time.perf_counter() - t0) * 1e3)
                    y.set_pod_classes(cls)
                    d.setdefault("step_ms", []).append(steady(y, args.steady))
                    if rep == 0:
                        verify(y, words, 8, cls)
                    k1, k2, nar = kernels(y, args.steady)
                    d.setdefault("k1_ms", []).append(k1)
                    d.setdefault("k2_ms", []).append(k2)
                    d.setdefault("narrow_ms", []).append(nar)
                    for size in (1, 64, 1024):
                        ids = np.sort(rng.choice(n, size, replace=False)).astype(np.uint32)
                        y.synchronize()
                        t0 = time.perf_counter()
                        y.update_candidates(ids, np.zeros(size, np.uint64))
                        t1 = time.perf_counter()
                        y.run(MODE_SCV)
                        y.synchronize()
                        t2 = time.perf_counter()
                        d.setdefault(f"update_{size}_call_ms", []).append((t1 - t0) * 1e3)
                        d.setdefault(f"update_{size}_plus_run_ms", []).append((t2 - t0) * 1e3)
                        y.update_candidates(ids, words[ids])
        out = {"workload": name, "pods": P, "nodes": n, "reps": args.reps, "sample": int(sample.size)}
        out.update({k: round(med(v), 3) for k, v in t.items()})
        out["steady_step_all_ms"] = [round(x, 3) for x in t["steady_step_ms"]]
        out["ones_step_all_ms"] = [round(x, 3) for x in t["ones_step_ms"]]
        print(json.dumps(out), flush=True)
        for s in shares:
            row = {"workload": name, "classes": 8, "cordoned": 64, "missing_share": s}
            row.update({k: round(med(v), 3) for k, v in per[s].items()})
            row["step_all_ms"] = [round(x, 3) for x in per[s]["step_ms"]]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
