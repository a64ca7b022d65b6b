#!/usr/bin/env python3
"""Wall time of the Mode B step under node sampling (yoda_mode_b_sampling), at 100k pods x 100k
nodes (config 3), M = yoda_num_feasible_to_find(N, 0), a uniform random start per pod.
Per workload (diskio: one pod spec; distinct: synth.distinct_diskio, a request per pod) and state:
    full        nothing absent, candidates off: every E is the whole snapshot
    abs1024     1,024 random nodes absent, candidates off
    r01, r30    8 candidate classes that each lack 1 % / 30 % of the nodes, the pod classes
                uniform over the 8 and ANY
and per draw setting (off, on) two steps on ONE handle for the same pods: `unsampled` (sampling
off: the step as it is without this setting) and `sampled`.  The steady step (yoda_run to
completion, the pods uploaded once): the median of --reps repetitions, every (state, step, draw)
interleaved within each repetition.  For the sampled step also the HIP-event times of the plan
kernel and of the sampled kernel (yoda_profile_read: the plan reports in K1's place); the draw
runs inside the sampled kernel, so its figure is the kernel's time with the draw on minus off.
Before a time is printed the sampled answers (draw off: every field, n_found, next_start; draw
on: the picks of one in forty of them) are compared with mode_b_sampling_cases.reference on a
--sample pod sample.
--baseline: the library under YODA_LIB_PATH predates the setting; only `never` (a handle that
never heard of the setting, sampling off, draw off) is measured, for the A/B of the unused path;
without --baseline `never` is measured too.
Run on a GPU box:
    python tools/mode_b_sampling_timing.py > profiles/modebsampling/timing.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xB10CFACE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="diskio,distinct")
    ap.add_argument("--states", default="full,abs1024,r01,r30")
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steady", type=int, default=20)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--never-only", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--pkg", default=os.path.join(REPO, "kubernetes-scheduler_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests"), REPO]
    import numpy as np
    from yoda_amd import capi, synth
    from yoda_amd.soa import MODE_DISKIO

    never_only = args.baseline or args.never_only
    if args.baseline:
        for name in ("yoda_mode_b_sampling", "yoda_mode_b_sampling_info"):
            capi._SIGS.pop(name, None)
    rng = np.random.default_rng(31)
    nodes, base_pods = synth.make_config(3, pods=args.pods, nodes=args.nodes)
    n, P = nodes.n_nodes, base_pods.n_pods

    def steady(y, k):
        for _ in range(2):
            y.run(MODE_DISKIO)
        y.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            y.run(MODE_DISKIO)
        y.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    print(f"# mode_b_sampling_timing {args.tag} lib={os.path.basename(capi.LIB_PATH)} "
          f"pods={P} nodes={n} reps={args.reps} steady={args.steady}", flush=True)
    if never_only:
        for wl in args.workloads.split(","):
            pods = synth.distinct_diskio(base_pods) if wl == "distinct" else base_pods
            with capi.Yoda(0) as y:
                y.upload_nodes(nodes)
                y.upload_pods(pods)
                runs = [steady(y, args.steady) for _ in range(args.reps)]
            print(f"{wl:9s} never    step_ms {statistics.median(runs):.4f}  runs "
                  + " ".join(f"{t:.4f}" for t in runs), flush=True)
        return

    import mode_b_sampling_cases as cases
    from candidate_cases import Model
    from node_present_cases import _present
    from tie_draw_cases import draw

    M = capi.Yoda.num_feasible_to_find(n, 0)
    start = rng.integers(0, n, P).astype(np.uint32)

    def steps_of(state):
        if state == "full":
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

    print(f"# M = {M}", flush=True)
    for wl in args.workloads.split(","):
        pods = synth.distinct_diskio(base_pods) if wl == "distinct" else base_pods
        sample = np.sort(rng.choice(P, min(args.sample, P), replace=False))
        handles = []
        for st in args.states.split(","):
            model = Model(nodes)
            y = capi.Yoda(0)
            y.upload_nodes(nodes)
            y.mode_b_follow(True)
            y.mode_b_sampling(True)
            for s in steps_of(st):
                model.apply(s)
                if s[0] == "cand":
                    y.set_candidates(s[2], s[1])
                elif s[0] == "classes":
                    y.set_pod_classes(s[1])
                else:
                    y.set_node_present(s[1], s[2])
            y.upload_pods(pods)
            if sample.size:  # the sample's pods against the oracle on their own S
                y.set_node_sampling(M, start)
                y.run(MODE_DISKIO)
                got = y.download()
                found, nxt = y.download_sampling()
                want, wf, wn = cases.reference(model, pods, M, start, sample=sample)
                for f in cases.FIELDS:
                    if not np.array_equal(getattr(got, f)[sample], getattr(want, f)[sample]):
                        raise SystemExit(f"{wl}/{st}: {f} differs from the reference")
                if not (np.array_equal(found[sample], wf[sample])
                        and np.array_equal(nxt[sample], wn[sample])):
                    raise SystemExit(f"{wl}/{st}: n_found / next_start differ from the reference")
                y.set_tie_draw(SEED)
                y.run(MODE_DISKIO)
                drawn = y.download()
                for p in sample[::40].tolist():
                    if want.status[p] == 0 and want.n_ties[p] >= 2:
                        ties = cases.detail(model, pods, p, start[p], M)["ties"]
                        if drawn.pick[p] != draw(SEED, p, ties):
                            raise SystemExit(f"{wl}/{st}: pod {p}'s draw differs")
                y.set_tie_draw(None)
            handles.append((st, y))
        keys = [(st, step, dr) for st, _ in handles for dr in ("off", "on")
                for step in ("unsampled", "sampled")]
        times = {k: [] for k in keys}
        plan = {k: [] for k in keys}
        kern = {k: [] for k in keys}
        never = []
        with capi.Yoda(0) as y0:
            y0.upload_nodes(nodes)
            y0.upload_pods(pods)
            for _ in range(args.reps):
                never.append(steady(y0, args.steady))
                for st, y in handles:
                    for dr in ("off", "on"):
                        y.set_tie_draw(SEED if dr == "on" else None)
                        for step in ("unsampled", "sampled"):
                            y.set_node_sampling(M if step == "sampled" else 0, start)
                            times[(st, step, dr)].append(steady(y, args.steady))
                            if step == "sampled":  # the kernels' own times, a separate pass
                                y.profile(True)
                                for _ in range(args.steady):
                                    y.run(MODE_DISKIO)
                                k1, k2, cnt = y.profile_read()
                                y.profile(False)
                                plan[(st, step, dr)].append(k1 / cnt)
                                kern[(st, step, dr)].append(k2 / cnt)
        med = statistics.median
        print(f"{wl:9s} never     step_ms {med(never):.4f}  runs "
              + " ".join(f"{t:.4f}" for t in never), flush=True)
        for st, y in handles:
            for dr in ("off", "on"):
                u, s = med(times[(st, "unsampled", dr)]), med(times[(st, "sampled", dr)])
                k = (st, "sampled", dr)
                extra = ""
                if dr == "on":
                    extra = f" draw_ms {med(kern[k]) - med(kern[(st, 'sampled', 'off')]):.4f}"
                print(f"{wl:9s} {st:8s} draw {dr:3s} unsampled_ms {u:.4f} sampled_ms {s:.4f} "
                      f"x{s / u:.2f}  plan_ms {med(plan[k]):.4f} kernel_ms {med(kern[k]):.4f}"
                      f"{extra}  runs " + " ".join(f"{t:.4f}" for t in times[k])
                      + f" info={y.mode_b_sampling_info()}"
                      + (f"  checked {sample.size} pods" if sample.size else ""), flush=True)
            y.close()


if __name__ == "__main__":
    main()
