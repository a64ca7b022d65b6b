#!/usr/bin/env python3
"""Wall time of the Mode B step with yoda_mode_b_follow, at 100k pods x 100k nodes (config 3).
Per workload (diskio: one pod spec; distinct: synth.distinct_diskio, a request per pod) and state:
    never       the setting never enabled (the step as it always was)
    full        enabled, nothing absent, candidates off: every E is the whole snapshot
    r01, r30    enabled, 8 candidate classes that each lack 1 % / 30 % of the nodes, the pod
                classes uniform over the 8 and ANY
    abs1024     enabled, 1,024 random nodes absent, candidates off
the steady step (yoda_run to completion, the pods uploaded once): the median of --reps
repetitions, the states interleaved within each repetition, and its ratio to `never`; the
effective classes and the launch form from yoda_mode_b_info.  Before a time is printed the
handle's answers are compared with mode_b_follow_cases.reference on a --sample pod sample.
--baseline: the library under YODA_LIB_PATH predates the setting; only `never` is measured.
Run on a GPU box:
    python tools/mode_b_follow_timing.py > profiles/modebfollow/timing.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="diskio,distinct")
    ap.add_argument("--states", default="never,full,r01,r30,abs1024")
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steady", type=int, default=50)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests"), REPO]
    import numpy as np
    import mode_b_follow_cases as cases
    from candidate_cases import Model
    from node_present_cases import _present
    from yoda_amd import capi, synth
    from yoda_amd.soa import MODE_DISKIO

    if args.baseline:
        for name in ("yoda_mode_b_follow", "yoda_mode_b_info"):
            capi._SIGS.pop(name, None)
    states = ["never"] if args.baseline else args.states.split(",")
    rng = np.random.default_rng(31)
    nodes, base_pods = synth.make_config(3, pods=args.pods, nodes=args.nodes)
    n, P = nodes.n_nodes, base_pods.n_pods

    def steps_of(state):
        if state in ("never", "full"):
            return []
        if state == "abs1024":
            return [_present(rng.choice(n, min(1024, n // 2), replace=False), 0)]
        share = {"r01": 0.01, "r30": 0.3}[state]
        words = np.full(n, np.uint64(0xFF), np.uint64)
        for c in range(8):
            words[rng.choice(n, int(n * share), replace=False)] &= ~np.uint64(1 << c)
        cls = rng.integers(0, 9, P).astype(np.uint8)
        cls[cls == 8] = cases.ANY
        return [("cand", 8, words), ("classes", cls)]

    def steady(y, k):
        for _ in range(2):
            y.run(MODE_DISKIO)
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            y.run(MODE_DISKIO)
        y.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    print(f"# mode_b_follow_timing {args.tag} lib={os.path.basename(capi.LIB_PATH)} "
          f"pods={P} nodes={n} reps={args.reps} steady={args.steady}", flush=True)
    for wl in args.workloads.split(","):
        pods = synth.distinct_diskio(base_pods) if wl == "distinct" else base_pods
        sample = np.sort(rng.choice(P, min(args.sample, P), replace=False))
        handles = []
        for st in states:
            model = Model(nodes)
            y = capi.Yoda(0)
            y.upload_nodes(nodes)
            if st != "never":
                y.mode_b_follow(True)
            for s in steps_of(st):
                model.apply(s)
                if s[0] == "cand":
                    y.set_candidates(s[2], s[1])
                elif s[0] == "classes":
                    y.set_pod_classes(s[1])
                else:
                    y.set_node_present(s[1], s[2])
            y.upload_pods(pods)
            y.run(MODE_DISKIO)
            if sample.size:  # the sample's pods, with their own class bytes, against the oracle
                got = y.download()
                sub = Model(nodes)
                sub.present, sub.n_classes, sub.words = model.present, model.n_classes, model.words
                sub.cls = None if model.cls is None else model.cls[sample]
                want = cases.reference(sub, pods.take(sample))
                for f in cases.FIELDS:
                    if not np.array_equal(getattr(got, f)[sample], getattr(want, f)):
                        raise SystemExit(f"{wl}/{st}: {f} differs from the reference")
            handles.append((st, y))
        times = {st: [] for st in states}
        for _ in range(args.reps):
            for st, y in handles:
                times[st].append(steady(y, args.steady))
        never = statistics.median(times["never"]) if "never" in times else None
        for st, y in handles:
            m = statistics.median(times[st])
            info = "" if args.baseline else " info=%s" % (y.mode_b_info(),)
            ratio = "" if never is None else f" x{m / never:.2f}"
            print(f"{wl:9s} {st:8s} step_ms {m:.4f}{ratio}  runs "
                  + " ".join(f"{t:.4f}" for t in times[st]) + info
                  + (f"  checked {sample.size} pods" if sample.size else ""), flush=True)
            y.close()


if __name__ == "__main__":
    main()
