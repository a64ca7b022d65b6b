#!/usr/bin/env python3
"""Fresh-upload table digests (tests/golden/upload_digests.json): for every shape of
tests/upload_cases.py the eight yoda_snapshot_check digests of a fresh handle, its record path
and whether the node order is grouped.

    python tests/golden/make_upload_digests.py        (on a GPU, after __graft_entry__.build())

The committed file was recorded at the last commit whose yoda_upload_nodes still built the block
summaries on the host, where mismatch == [0, 0, 0, 0] meant "host builder == k_bsum_build": its
digest 5 is that host builder's output, the independent witness of the kernel.  Digests 1-4, 6
and 7 pin the other base tables, the G table and the G maxima / reciprocals.  Regenerate only
when a table's layout or contents change on purpose, and say so in the commit.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "kubernetes-scheduler_amd"), os.path.join(REPO, "oracle"),
                os.path.dirname(HERE)]

import upload_cases  # noqa: E402
from yoda_amd.capi import Yoda  # noqa: E402


def main():
    fx = {"_about": "yoda_snapshot_check digests of fresh uploads (tests/upload_cases.py), "
                    "recorded by tests/golden/make_upload_digests.py"}
    for name in upload_cases.NAMES:
        with Yoda(0) as y:
            for nodes, kw in upload_cases.uploads(name):
                y.upload_nodes(nodes, **kw)
            d, m = y.snapshot_check()
            fx[name] = upload_cases.entry(y, d)
        assert m.tolist() == [0, 0, 0, 0], (name, m)
        print(name, fx[name], flush=True)
    with open(upload_cases.GOLDEN, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", upload_cases.GOLDEN)


if __name__ == "__main__":
    main()
