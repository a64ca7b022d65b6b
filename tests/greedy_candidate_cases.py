"""Greedy batches with candidate classes (yoda_greedy_candidates) as plain data (no fixtures): the
workloads and their reference.  tests/test_greedy_candidate_cases.py checks with the oracle and the
host session alone that the cases would fail a handle that ignored the words, narrowed the maxima
or counted a non-candidate as lost from the feasible set; tests/test_gpu_greedy_candidates.py runs
them on libyoda.

The reference needs no oracle of its own: it is the sequential loop of oracle.greedy restated.  For
each pod in oracle.queue_order, oracle.pod_detail on the CURRENT node state gives Yoda's
feasibility and the raw scores under the maxima of every node that passes Yoda's Filter now
(CollectMaxValues never sees another plugin's Filter); the pod's class bit is applied to the
feasibility; the cycle's tail (none, one node without scoring, DIV_ZERO, NormalizeScore, the
lowest node among the top-scored) is candidate_cases.detail's; the assume is oracle_greedy's
(alloc += scv/memory, with the capacity flag a saturating CardNumber decrement)."""
import functools

import numpy as np

import candidate_cases as cc
import oracle
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, PICK_ERROR, PICK_NONE

ANY = cc.ANY
CAPACITY = 1  # YODA_GREEDY_CARD_CAPACITY


def reference(nodes, pods, words, cls, flags, present=None):
    """pick [P] in input order (ids of `nodes`).  words: one uint64 per node; cls: one class byte
    per pod or None (every pod ANY); present: bool per node, None: every node (an absent node is
    in no feasible set and feeds no maximum: the loop runs on the snapshot without them)."""
    nodes, pods = nodes.normalized(), pods.normalized()
    keep = np.arange(nodes.n_nodes) if present is None else np.flatnonzero(present)
    cur = nodes.take(keep).normalized()
    cur.alloc_memory = np.array(cur.alloc_memory, np.uint64)
    cur.card_number = np.array(cur.card_number, np.uint64)
    w = np.asarray(words, np.uint64)[keep]
    zero = cur.total_memory_sum == 0
    P = pods.n_pods
    pick = np.full(P, PICK_NONE, np.int32)
    for p in oracle.queue_order(pods).tolist():
        _, feas, raw, _ = oracle.pod_detail(cur, pods, p, MODE_SCV)
        c = ANY if cls is None else int(cls[p])
        if c != ANY:
            feas = feas & ((w >> np.uint64(c)) & np.uint64(1)).astype(bool)
        idx = np.flatnonzero(feas)
        if idx.size == 0:
            continue
        if idx.size == 1:  # returned without scoring
            n = int(idx[0])
        elif zero[idx].any():
            pick[p] = PICK_ERROR
            continue
        else:
            norm = cc._normalize(raw[idx])
            if norm is None:  # SCORE_RANGE
                pick[p] = PICK_ERROR
                continue
            n = int(idx[np.flatnonzero(norm == norm.max())[0]])
        pick[p] = keep[n]
        with np.errstate(over="ignore"):
            if pods.has_memory[p]:
                cur.alloc_memory[n] += np.uint64(pods.memory[p])  # uint64 wrap
            if flags & CAPACITY:
                num = int(pods.number[p]) if pods.has_number[p] else 1
                cur.card_number[n] = np.uint64(max(int(cur.card_number[n]) - num, 0))
    return pick


def as_absent(nodes, pods, words, cls, flags):
    """The per-class absent-node reading of the same state: class by class the blind greedy on the
    snapshot without the class's non-candidates, so that its maxima narrow with it.  (Each class a
    batch of its own: what a caller gets who marks non-candidates absent.)"""
    pick = np.full(pods.n_pods, PICK_NONE, np.int32)
    for c in np.unique(cls).tolist():
        sel = np.flatnonzero(cls == c)
        keep = (np.arange(nodes.n_nodes) if c == ANY else
                np.flatnonzero((words >> np.uint64(c)) & np.uint64(1)))
        if keep.size == 0:
            continue
        r = oracle.greedy(nodes.take(keep), pods.take(sel), MODE_SCV, flags)[0]
        pick[sel] = np.where(r >= 0, keep[np.maximum(r, 0)], r)
    return pick


def single_and_none(nodes, pods, words, cls, flags):
    """(pods whose F' held one node, pods whose F' was empty) along the reference's sequence."""
    ref = reference(nodes, pods, words, cls, flags)
    nodes, pods = nodes.normalized(), pods.normalized()
    cur = nodes.take(np.arange(nodes.n_nodes)).normalized()
    cur.alloc_memory = np.array(cur.alloc_memory, np.uint64)
    cur.card_number = np.array(cur.card_number, np.uint64)
    one = none = 0
    for p in oracle.queue_order(pods).tolist():
        _, feas, _, _ = oracle.pod_detail(cur, pods, p, MODE_SCV)
        if int(cls[p]) != ANY:
            feas = feas & ((words >> np.uint64(int(cls[p]))) & np.uint64(1)).astype(bool)
        one += int(feas.sum() == 1)
        none += int(feas.sum() == 0)
        n = int(ref[p])
        if n < 0:
            continue
        with np.errstate(over="ignore"):
            if pods.has_memory[p]:
                cur.alloc_memory[n] += np.uint64(pods.memory[p])
            if flags & CAPACITY:
                num = int(pods.number[p]) if pods.has_number[p] else 1
                cur.card_number[n] = np.uint64(max(int(cur.card_number[n]) - num, 0))
    return one, none


@functools.lru_cache(maxsize=None)
def workload(pods=2500, nodes=600, mixed=False):
    """The config-5 generator with the recipe classes (8 classes + ANY, 8 cordoned nodes).
    mixed: half the nodes hold cards of several models (the dense-mask witness kernel).
    Cached: do not write to the arrays."""
    nd, pd = synth.make_config(5, pods=pods, nodes=nodes)
    if mixed:
        nd = synth.mixed_models(nd, 0.5)
    nd, pd = nd.normalized(), pd.normalized()
    words, cls = cc.recipe(nd, pd, seed=3, cordoned=8)
    return nd, pd, words, cls


@functools.lru_cache(maxsize=None)
def want(pods=2500, nodes=600, mixed=False, flags=0):
    """reference() of workload(), computed once."""
    nd, pd, words, cls = workload(pods, nodes, mixed)
    return reference(nd, pd, words, cls, flags)


# ---- the session KAT: F' and F told apart in scan_lost ------------------------------------
# Five nodes with one identical card each, K = 1 lists, three pods in queue order:
#   pod 0  takes X's last two cards;
#   pod 1  takes A with enough scv/memory that A's Allocate score (300 -> 120) falls below pod
#          2's list threshold, so pod 2's list no longer certifies A by score;
#   pod 2  (class 0, two cards) is the pod under test: its list holds A alone.
# base         F'(2) = {A, B}, counts 2.  X passed Yoda's Filter for pod 2 but is not its
#              candidate: F' lost nothing, two nodes remain, and B -- unlisted -- may now outscore
#              A, so resolve() stops at pod 2.  A session that counts X as lost from the feasible
#              set sees one node left and returns A without scoring.
# mirror       X IS a candidate and B is not: F'(2) = {A, X}, counts 2; X is lost, one node is
#              left, and it is A: certified.
# zero         X and Z have TotalMemorySum 0; Z is a candidate of class 0, X is not: F'(2) =
#              {A, B, Z}, counts 3 with one zero-total node.  Losing X leaves Z in F': DIV_ZERO
#              (YODA_PICK_ERROR), certified.  A session that counts X in lz believes the
#              zero-total node gone and goes on to the list, where it stops.  (Pods 0 and 1 carry
#              classes of their own here, {X} and {A, Y}, so that no zero-total node is in THEIR
#              feasible sets.)
KAT_A, KAT_B, KAT_X, KAT_Y, KAT_Z = 0, 1, 2, 3, 4
KAT_VARIANTS = ("base", "mirror", "zero")
# variant -> (window index resolve() must return, pod 2's pick when it is resolved)
KAT_WANT = {"base": (2, None), "mirror": (3, KAT_A), "zero": (3, PICK_ERROR)}


def kat_nodes(variant):
    from yoda_amd.soa import NodeSoA
    n = 5
    one = np.ones((n, 1), np.uint64)
    total = np.full(n, 1000, np.uint64)
    if variant == "zero":
        total[[KAT_X, KAT_Z]] = 0
    return NodeSoA(card_number=np.array([4, 4, 2, 4, 4], np.uint64),
                   free_memory_sum=np.full(n, 500, np.uint64), total_memory_sum=total,
                   alloc_memory=np.zeros(n, np.uint64), card_count=np.ones(n, np.uint32),
                   card_healthy=np.ones((n, 1), np.uint8), card_free_memory=500 * one,
                   card_clock=1500 * one, card_total_memory=1000 * one, card_bandwidth=100 * one,
                   card_core=64 * one, card_power=300 * one, cpu=np.zeros(n),
                   disk_io=np.zeros(n)).normalized()


def kat_pods():
    from yoda_amd.soa import PodSoA
    # queue order = input order (equal priorities)
    return PodSoA(has_number=np.array([1, 1, 1], np.uint8), number=np.array([2, 1, 2], np.uint64),
                  has_memory=np.array([0, 1, 0], np.uint8), memory=np.array([0, 600, 0], np.uint64),
                  has_clock=np.zeros(3, np.uint8), clock=np.zeros(3, np.uint64),
                  priority=np.zeros(3, np.int64), rio=np.zeros(3),
                  rcpu=np.zeros(3, np.int64)).normalized()


def kat_window(variant):
    """The hand-built window [0, 3): dict(n_classes, words, cls, counts [2][3], top_score [1][3],
    top_node [1][3], maxima [6][3], wit_count [6][3], wit_node [6][3]).  Every node scores 600 at
    the window start (ties go to the lowest node, which each list holds); every maximum has all
    five nodes as witnesses, so the maxima certificate is never the obstacle."""
    A, B, X, Y, Z = KAT_A, KAT_B, KAT_X, KAT_Y, KAT_Z
    words = np.zeros(5, np.uint64)
    if variant == "base":
        words[[A, B]] = 1
        cls = [ANY, ANY, 0]
        counts = [[5, 5, 2], [0, 0, 0]]
    elif variant == "mirror":
        words[[A, X]] = 1
        cls = [ANY, ANY, 0]
        counts = [[5, 5, 2], [0, 0, 0]]
    else:
        words[[A, B, Z]] |= np.uint64(1)   # class 0: pod 2
        words[X] |= np.uint64(2)           # class 1: pod 0
        words[[A, Y]] |= np.uint64(4)      # class 2: pod 1
        cls = [1, 2, 0]
        counts = [[1, 2, 3], [1, 0, 1]]
    return dict(n_classes=3, words=words, cls=np.array(cls, np.uint8),
                counts=np.array(counts, np.uint32), top_score=np.full((1, 3), 600.0),
                top_node=np.array([[X, A, A]], np.uint32),
                maxima=np.array([[100] * 3, [1500] * 3, [64] * 3, [500] * 3, [300] * 3,
                                 [1000] * 3], np.uint64),
                wit_count=np.full((6, 3), 5, np.uint32), wit_node=np.zeros((6, 3), np.uint32))


def kat_run(variant, with_candidates=True):
    """Drive a capacity GreedySession through the window: (resolve()'s window index, picks)."""
    from yoda_amd.capi import GreedySession
    w = kat_window(variant)
    g = GreedySession(kat_nodes(variant), kat_pods(), CAPACITY)
    try:
        if with_candidates:
            g.set_candidates(w["words"], w["n_classes"], w["cls"])
        g.begin_window(0, 1, w["counts"], w["top_score"], w["top_node"])
        g.set_witness(w["maxima"], w["wit_count"], w["wit_node"])
        nxt = g.resolve()
        return nxt, g.picks()[0].copy()
    finally:
        g.close()
