#!/usr/bin/env python3
"""What the sharded selectHost draw (yoda_shard_tie_draw) adds to a yoda_comm_run_local step, and
whether the step with the draw OFF costs what it cost before the draw existed.  One process times
ONE build of libyoda; run the parent commit's build (this file copied into a built checkout of
it, or YODA_LIB_PATH) and this one in alternating processes on one GPU and compare the draw-off
figures:
    python <parent checkout>/tools/shard_draw_timing.py --parent
    python tools/shard_draw_timing.py --off-only
    python tools/shard_draw_timing.py            # what the draw adds
Workloads: c3 (config 3, Mode A) and b2 (config 2's generator, Mode B), both at --pods x --nodes,
over --world node shards on device 0.  Each figure is the wall time of a window of steps ending
in a synchronize, per step; off / on windows alternate, --reps times each.  --parent: a build
without the shard draw's entry points (draw-off windows only).  --off-only: draw-off windows
only on this build too -- the like-for-like figure against --parent (an off window that follows
an on window starts from other caches and clocks than one that follows an off window).
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
NEW = ("yoda_shard_tie_draw", "yoda_shard_draw_keys", "yoda_shard_draw_apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,b2")
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0, help="timed work per window")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "kubernetes-scheduler_amd"))
    import numpy as np
    from yoda_amd import capi, synth
    from yoda_amd.capi import Yoda
    from yoda_amd.soa import MODE_DISKIO, MODE_SCV

    if args.parent:
        for name in NEW:
            capi._SIGS.pop(name, None)

    def window(hs, mode, steps):
        hs[0].synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            capi.comm_run_local(hs, mode)  # (synchronizes the shared stream itself)
        return (time.perf_counter() - t0) / steps * 1e3

    def draw(hs, on):
        if args.parent:
            return
        for h in hs:
            h.set_tie_draw(args.seed if on else None)
            h.shard_tie_draw(on)

    for name in args.workloads.split(","):
        cfg, mode = {"c3": (3, MODE_SCV), "b2": (2, MODE_DISKIO)}[name]
        nodes, pods = synth.make_config(cfg, pods=args.pods, nodes=args.nodes)
        b = np.linspace(0, nodes.n_nodes, args.world + 1).astype(int)
        hs = [Yoda(0) for _ in range(args.world)]
        for r, h in enumerate(hs):
            h.upload_nodes(nodes.slice(b[r], b[r + 1]), node_offset=int(b[r]))
            h.upload_pods(pods)
        kinds = (False,) if args.parent or args.off_only else (False, True)
        res, steps = {}, {}
        for on in kinds:  # warm both, size the windows
            draw(hs, on)
            capi.comm_run_local(hs, mode)
            one = window(hs, mode, 2)
            steps[on] = max(3, min(200, math.ceil(args.window_ms / max(one, 1e-3))))
            res[on] = []
        r = hs[0].download()
        tied = int(((r.status == 0) & (r.n_ties >= 2)).sum())
        for _ in range(args.reps):
            for on in kinds:
                draw(hs, on)
                res[on].append(window(hs, mode, steps[on]))
        draw(hs, False)
        med = statistics.median
        build = "parent" if args.parent else "new_off_only" if args.off_only else "new"
        out = {"build": args.tag or build, "workload": name,
               "pods": pods.n_pods, "nodes": nodes.n_nodes, "world": args.world, "mode": mode,
               "path": hs[0].path, "tied_pods": tied, "tied_share": round(tied / pods.n_pods, 4),
               "max_ties": int(r.n_ties.max()),
               "off_ms": round(med(res[False]), 4),
               "off_all_ms": [round(t, 4) for t in res[False]]}
        if True in res:
            out.update(on_ms=round(med(res[True]), 4),
                       added_ms=round(med(res[True]) - med(res[False]), 4),
                       on_all_ms=[round(t, 4) for t in res[True]],
                       steps_per_window={"off": steps[False], "on": steps[True]})
        print(json.dumps(out), flush=True)
        for h in hs:
            h.close()


if __name__ == "__main__":
    main()
