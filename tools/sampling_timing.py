#!/usr/bin/env python3
"""Wall time of node sampling (yoda_set_node_sampling) on a live snapshot.  Per workload:
    steady_step_ms          the step with sampling never set (the block-grouped node order)
    upload_order_step_ms    sampling on with M = n_nodes: no pod is cut and every wave skips the
                            pass; what remains is the upload-order node tables, the K2 pruning
                            seeds that are off, and the pass's launches
and per (num_to_find, candidate classes) setting, with uniform random starts:
    set_call_ms             yoda_set_node_sampling of the whole start array
    step_ms                 the steady step
    k1_ms, k2_ms, pass_ms   K1, K2 and the sampling pass (count + scan + cut) per step (HIP events)
    narrow_ms               the candidates' narrowing pass, with 8 classes
Medians of --reps repetitions, interleaved.  Before a time is printed the handle's answers are
compared with sampling_cases.reference on a --sample pod sample.  Run on a GPU box:
    python tools/sampling_timing.py > profiles/sampling/timing.txt
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
    ap.add_argument("--workloads", default="c3")
    ap.add_argument("--pct", type=int, default=0, help="percentageOfNodesToScore (0: adaptive)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steady", type=int, default=10)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests"), REPO]
    import numpy as np
    import candidate_cases as cc
    import sampling_cases as cases
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
        y.sampling_profile()
        for _ in range(k):
            y.run(MODE_SCV)
        k1, k2, n = y.profile_read()
        nar, pas = y.candidates_profile(), y.sampling_profile()
        y.profile(False)
        return k1 / k, k2 / k, pas / k, nar / k

    for name, nodes, pods, mode, kw in synth.variant_workloads(args.workloads.split(",")):
        assert mode == MODE_SCV
        n, P = nodes.n_nodes, pods.n_pods
        m = Yoda.num_feasible_to_find(n, args.pct)
        rng = np.random.default_rng(77)
        sample = np.sort(rng.choice(P, min(args.sample, P), replace=False))
        sub = pods.take(sample)
        snap = cc.Snapshot(cc.Model(nodes), sub)  # the maxima and raw scores of the sample
        start = rng.integers(0, n, P).astype(np.uint32)
        words, cls = cc.recipe(nodes, pods, seed=7, tenths=0.01)

        def verify(y, with_classes):
            model = cc.Model(nodes)
            if with_classes:
                model.apply(("cand", 8, words))
                model.apply(("classes", cls[sample]))
            want, _, found, nxt, _ = cases.reference(snap, model, m, start[sample])
            got = y.download()
            for f in ("pick", "status", "n_feasible"):
                assert (getattr(got, f)[sample] == getattr(want, f)).all(), (name, f)
            ok = want.status == 0
            assert (got.top_score[sample][ok] == want.top_score[ok]).all(), name
            assert (got.maxima[sample] == want.maxima).all(), name
            f, x = y.download_sampling()
            assert (f[sample] == found).all() and (x[sample] == nxt).all(), name

        t = {"steady_step_ms": [], "upload_order_step_ms": []}
        per = {False: {}, True: {}}
        with Yoda(0) as y:
            y.upload_nodes(nodes, **kw)
            y.upload_pods(pods)
            for rep in range(args.reps):
                y.set_candidates(None, 0)
                y.set_node_sampling(0)
                t["steady_step_ms"].append(steady(y, args.steady))
                y.set_node_sampling(n, start)
                t["upload_order_step_ms"].append(steady(y, args.steady))
                for with_classes in (False, True):
                    d = per[with_classes]
                    if with_classes:
                        y.set_candidates(words, 8)
                        y.set_pod_classes(cls)
                    y.synchronize()
                    t0 = time.perf_counter()
                    y.set_node_sampling(m, start)
                    d.setdefault("set_call_ms", []).append((time.perf_counter() - t0) * 1e3)
                    d.setdefault("step_ms", []).append(steady(y, args.steady))
                    if rep == 0:  # (the reference once per setting: the later repetitions time only)
                        verify(y, with_classes)
                    k1, k2, pas, nar = kernels(y, args.steady)
                    d.setdefault("k1_ms", []).append(k1)
                    d.setdefault("k2_ms", []).append(k2)
                    d.setdefault("pass_ms", []).append(pas)
                    if with_classes:
                        d.setdefault("narrow_ms", []).append(nar)
        out = {"workload": name, "pods": P, "nodes": n, "reps": args.reps, "sample": int(sample.size)}
        out.update({k: round(med(v), 3) for k, v in t.items()})
        out["steady_step_all_ms"] = [round(x, 3) for x in t["steady_step_ms"]]
        out["upload_order_step_all_ms"] = [round(x, 3) for x in t["upload_order_step_ms"]]
        print(json.dumps(out), flush=True)
        for with_classes in (False, True):
            row = {"workload": name, "num_to_find": m, "starts": "uniform random",
                   "classes": 8 if with_classes else 0}
            row.update({k: round(med(v), 3) for k, v in per[with_classes].items()})
            row["step_all_ms"] = [round(x, 3) for x in per[with_classes]["step_ms"]]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
