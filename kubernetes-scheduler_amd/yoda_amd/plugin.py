"""The reference's scheduler-framework plugin surface, backed by libyoda.

Mirrors pkg/yoda/scheduler.go (and sort.go) method for method — same names, argument
meaning and Status codes — so a caller of the reference plugin finds the same contract:

  PreFilter  scheduler.go:91-94    packs the pod, ONE libyoda call for the whole row
                                   (yoda_score_rows: Filter bits + raw Score of every node),
                                   kept in CycleState
  Filter     scheduler.go:96-99    lookup (the SCV predicates, filter.go:11-58)
  PreScore   scheduler.go:101-114  no-op: the inputs are the uploaded snapshot (the reference
                                   flushes Redis and queries Prometheus here — out of scope)
  Score      scheduler.go:116-156  lookup of the row (Uint64ToInt64 already applied)
  NormalizeScore scheduler.go:158-183  the reference algorithm, int64 wrap-around included
  PreBind    scheduler.go:189-196  node must exist in the snapshot
  Less       sort.go:8-10          scv/priority descending

`schedule_one` runs one kube-scheduler v1.22.3 cycle over these methods (Filter all nodes,
the single-feasible-node shortcut, PreScore, Score, NormalizeScore, range check, selectHost).
The Go drop-in has the same structure over cgo.
"""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .pack import pack_pods
from .soa import (MODE_SCV, REASON_ABSENT, REASON_CLOCK, REASON_MEMORY, REASON_NOT_CANDIDATE,
                  REASON_NUMBER, NodeSoA)

NAME = "yoda"
MAX_NODE_SCORE = 100
MIN_NODE_SCORE = 0

# k8s framework Code values
SUCCESS, ERROR, UNSCHEDULABLE = 0, 1, 2


@dataclass
class Status:
    code: int = SUCCESS
    message: str = ""

    def is_success(self) -> bool:
        return self.code == SUCCESS


class CycleState(dict):
    """framework.CycleState: per-pod scheduling-cycle storage."""

    def write(self, key, value):
        self[key] = value

    def read(self, key):
        if key not in self:
            raise KeyError(f"{key!r} not found in CycleState")
        return self[key]


@dataclass
class NodeScore:
    name: str
    score: int


# Filter's message when the backend cannot say why (no reason_rows), and per reason code
# (soa.REASON_*, include/yoda.h): kube-scheduler groups the nodes of a FitError event by message
FILTER_MESSAGE = "node(s) didn't match the scv card requirements"
REASON_MESSAGES = {
    REASON_NUMBER: "node(s) didn't have enough scv cards (scv/number)",
    REASON_MEMORY: "node(s) had too few healthy scv cards with the requested free memory "
                   "(scv/memory)",
    REASON_CLOCK: "node(s) had too few healthy scv cards at the requested clock (scv/clock)",
    REASON_NOT_CANDIDATE: "node(s) were rejected by another plugin or are not in the node set",
    REASON_ABSENT: "node(s) were rejected by another plugin or are not in the node set",
}


@dataclass
class _Row:
    feasible: np.ndarray  # bool [N]
    scores: np.ndarray    # int64 [N], -1 where infeasible
    reasons: Optional[np.ndarray] = None  # uint8 [N] soa.REASON_*, when the backend gives them


def _wrap_i64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _go_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


class YodaPlugin:
    """PreFilter/Filter/PreScore/Score/NormalizeScore/PreBind + Less, over a libyoda handle
    (or any backend with upload_pods(PodSoA) and score_rows(mode))."""

    def __init__(self, backend, node_names: Sequence[str], nodes: Optional[NodeSoA] = None,
                 mode: int = MODE_SCV):
        self.backend = backend
        self.node_names = list(node_names)
        self.index = {n: i for i, n in enumerate(self.node_names)}
        self.mode = mode
        # Mode A Score divides by TotalMemorySum (algorithm.go:294,309): Go panics on 0
        self.zero_total = (np.asarray(nodes.total_memory_sum) == 0) if nodes is not None \
            else np.zeros(len(self.node_names), bool)

    def name(self) -> str:
        return NAME

    # ---- the live snapshot ---------------------------------------------------------------
    def replace_nodes(self, ids, nodes: NodeSoA):
        """Whole new records for the nodes at positions `ids` of node_names (the backend's
        replace_nodes); Score's TotalMemorySum == 0 check follows the new records."""
        self.backend.replace_nodes(ids, nodes)
        self.zero_total[np.asarray(ids, np.int64)] = np.asarray(nodes.total_memory_sum) == 0

    def update_node_metrics(self, ids, cpu, disk_io):
        """Mode B's NodeInfo.Cpu / DiskIO of the nodes at positions `ids` (None: of every node,
        in node_names order), as the backend's update_node_metrics takes them."""
        self.backend.update_node_metrics(ids, cpu, disk_io)

    # ---- extension points ---------------------------------------------------------------
    def pre_filter(self, state: CycleState, pod: Mapping) -> Status:
        self.backend.upload_pods(pack_pods([pod]))
        # The reason row beside the score row (Mode A; Mode B has no Filter of its own).  It goes
        # first: yoda_reason_rows drops a pending run, yoda_score_rows leaves its own.  Every pod
        # gets it: kube-scheduler reads the per-node statuses whenever no node passes EVERY Filter
        # plugin, and this row knows nothing of the other plugins' verdicts.
        reasons = None
        if self.mode == MODE_SCV and hasattr(self.backend, "reason_rows"):
            reasons = self.backend.reason_rows()[0]
        feas, scores = self.backend.score_rows(self.mode)
        state.write(NAME + "/row", _Row(feas[0], scores[0], reasons))
        return Status()

    def filter(self, state: CycleState, pod: Mapping, node_name: str) -> Status:
        row: _Row = state.read(NAME + "/row")
        i = self.index[node_name]
        if row.feasible[i]:
            return Status()
        if row.reasons is None:
            return Status(UNSCHEDULABLE, FILTER_MESSAGE)
        return Status(UNSCHEDULABLE, REASON_MESSAGES.get(int(row.reasons[i]), FILTER_MESSAGE))

    def pre_score(self, state: CycleState, pod: Mapping, nodes: Sequence[str]) -> Status:
        return Status()

    def score(self, state: CycleState, pod: Mapping, node_name: str) -> Tuple[int, Status]:
        try:
            row: _Row = state.read(NAME + "/row")
        except KeyError as e:
            return 0, Status(ERROR, str(e))
        i = self.index[node_name]
        if self.mode == MODE_SCV and self.zero_total[i]:
            return 0, Status(ERROR, "runtime error: integer divide by zero")
        return int(row.scores[i]), Status()

    def score_extensions(self):
        return self

    def normalize_score(self, state: CycleState, pod: Mapping,
                        scores: List[NodeScore]) -> Status:
        """scheduler.go:158-183 verbatim (int64 arithmetic with Go wrap-around)."""
        highest, lowest = 0, scores[0].score
        for ns in scores:
            lowest = min(lowest, ns.score)
            highest = max(highest, ns.score)
        if highest == lowest:
            lowest -= 1
        for ns in scores:
            ns.score = _go_div(_wrap_i64((ns.score - lowest) * MAX_NODE_SCORE), highest - lowest)
        return Status()

    def pre_bind(self, state: CycleState, pod: Mapping, node_name: str) -> Status:
        if node_name not in self.index:
            return Status(ERROR, f"prebind get node info error: {node_name}")
        return Status()

    @staticmethod
    def less(pod_info1: Mapping, pod_info2: Mapping) -> bool:
        """sort.Less (sort.go:8-10)."""
        from .gostrconv import pod_priority

        def prio(p):
            labels = (p.get("metadata", {}) or {}).get("labels", {}) or {}
            return pod_priority(str(labels["scv/priority"])) if "scv/priority" in labels else 0
        return prio(pod_info1) > prio(pod_info2)


def select_host(scores: Sequence[NodeScore], rng: Optional[random.Random] = None) -> str:
    """k8s v1.22.3 selectHost: reservoir-sampled tie-break with rng; with rng=None the
    lowest-index member of the tie set (the build's deterministic rule)."""
    best = scores[0].score
    selected = scores[0].name
    cnt = 1
    for ns in scores[1:]:
        if ns.score > best:
            best, selected, cnt = ns.score, ns.name, 1
        elif ns.score == best:
            cnt += 1
            if rng is not None and rng.randrange(cnt) == 0:
                selected = ns.name
    return selected


def find_nodes_that_pass_filters(plugin: YodaPlugin, state: CycleState, pod: Mapping,
                                 num_to_find: int = 0, start: int = 0) -> Tuple[list, int]:
    """k8s v1.22.3 findNodesThatPassFilters at parallelism 1: walk the node list from index
    `start` (wrapping) and stop once `num_to_find` nodes have passed Filter; num_to_find 0: every
    node (percentageOfNodesToScore 100).  Returns (the feasible nodes in walk order, the index the
    next cycle's walk begins at: the node the walk stopped at, or `start` after a full circle) --
    what yoda_set_node_sampling / yoda_download_sampling compute for a batch."""
    names = plugin.node_names
    n = len(names)
    feasible = []
    for k in range(n):
        i = (start + k) % n
        if plugin.filter(state, pod, names[i]).is_success():
            if num_to_find and len(feasible) == num_to_find:
                return feasible, i
            feasible.append(names[i])
    return feasible, start


def schedule_one(plugin: YodaPlugin, pod: Mapping, rng: Optional[random.Random] = None,
                 weight: int = 1, num_to_find: int = 0,
                 start: int = 0) -> Tuple[Optional[str], Status]:
    """One scheduling cycle with yoda as the only Filter/Score plugin.  num_to_find 0:
    percentageOfNodesToScore 100; else only the first num_to_find feasible nodes of the walk that
    begins at node index `start` are scored (find_nodes_that_pass_filters).  Returns (node name or
    None, status)."""
    state = CycleState()
    st = plugin.pre_filter(state, pod)
    if not st.is_success():
        return None, st
    feasible, _ = find_nodes_that_pass_filters(plugin, state, pod, num_to_find, start)
    if num_to_find:  # (node-list order again: select_host's deterministic rule is the lowest node)
        feasible.sort(key=plugin.index.__getitem__)
    if not feasible:
        return None, Status(UNSCHEDULABLE, "0 nodes are available")
    if len(feasible) == 1:
        return feasible[0], Status()
    st = plugin.pre_score(state, pod, feasible)
    if not st.is_success():
        return None, st
    scores = []
    for n in feasible:
        s, st = plugin.score(state, pod, n)
        if not st.is_success():
            return None, st
        scores.append(NodeScore(n, s))
    plugin.score_extensions().normalize_score(state, pod, scores)
    for ns in scores:
        if ns.score > MAX_NODE_SCORE or ns.score < MIN_NODE_SCORE:
            return None, Status(ERROR, f"plugin yoda returns an invalid score {ns.score}")
        ns.score *= weight
    return select_host(scores, rng), Status()
