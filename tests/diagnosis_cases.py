"""Filter-diagnosis scenarios as plain data (no fixtures), and the reference: why Filter rejected
a (pod, node) pair (include/yoda.h YODA_REASON_*).  tests/test_diagnosis_cases.py checks the
reference against the two oracles and that no scenario passes vacuously;
tests/test_gpu_diagnosis.py replays the scenarios on libyoda (yoda_diagnose, yoda_reason_rows).

Each scenario is (nodes, pods, steps) in the style of tests/candidate_cases.py, whose steps and
Model (presence, candidate words, pod classes, pushed CardNumber, card updates) are reused.

The reference is a vectorised numpy restatement of the three predicates of
pkg/yoda/filter/filter.go:11-58 over the model's CURRENT node values, with the precedence
absent > not a candidate > number > memory > clock.  Pods with the same labels and class share one
evaluation."""
import functools

import numpy as np

import candidate_cases as cc
import card_update_cases as cu
import node_present_cases as npc
from yoda_amd import synth
from yoda_amd.soa import (REASON_ABSENT, REASON_CLOCK, REASON_MEMORY, REASON_NONE,
                          REASON_NOT_CANDIDATE, REASON_NUMBER)

ANY = cc.ANY
UNSELECTED = 0xFFFFFFFF
# the order of the four counted reasons in yoda_download_diagnosis
COUNTED = (REASON_NOT_CANDIDATE, REASON_NUMBER, REASON_MEMORY, REASON_CLOCK)
WALK_SHAPES = ("small", "c4", "ranks", "mixed", "f64", "u64")
MIXED_PODS = 300  # (the mixed shape's batch: few pods, the upload order of the nodes)


def _spec_codes(nd, present, words, n_classes, spec):
    """uint8 [N]: the code of every node for one pod spec (has_number, number, has_memory,
    memory, has_clock, clock, class)."""
    hn, num, hm, mem, hc, clk, cls = spec
    k = nd.max_cards
    real = np.arange(k)[None, :] < nd.card_count[:, None]
    healthy = (nd.card_healthy != 0) & real          # Card.Health == "Healthy" of a listed card
    number = np.uint64(num) if hn else np.uint64(1)  # filter.go:12-15
    fits_number = number <= nd.card_number
    fits_memory = np.ones(nd.n_nodes, bool)
    if hm:  # filter.go:19-30, CardFitsMemory :52-54
        cards = ((nd.card_free_memory >= np.uint64(mem)) & healthy).sum(axis=1).astype(np.uint64)
        fits_memory = cards >= number
    fits_clock = np.ones(nd.n_nodes, bool)
    if hc:  # filter.go:36-47, CardFitsClock :56-58
        cards = ((nd.card_clock == np.uint64(clk)) & healthy).sum(axis=1).astype(np.uint64)
        fits_clock = cards >= number
    cand = np.ones(nd.n_nodes, bool)
    if n_classes and cls != ANY:
        cand = ((words >> np.uint64(cls)) & np.uint64(1)).astype(bool)
    code = np.where(fits_clock, REASON_NONE, REASON_CLOCK)
    code = np.where(fits_memory, code, REASON_MEMORY)
    code = np.where(fits_number, code, REASON_NUMBER)
    code = np.where(cand, code, REASON_NOT_CANDIDATE)
    return np.where(present, code, REASON_ABSENT).astype(np.uint8)


class Reference:
    """The codes and counts of every pod in one state of a candidate_cases.Model."""

    def __init__(self, model, pods):
        self.nd = model.nodes()
        self.present = model.present.copy()
        self.words = model.words.copy()
        self.n_classes = model.n_classes
        P = pods.n_pods
        cls = np.full(P, ANY, np.uint64) if model.cls is None or not model.n_classes \
            else model.cls.astype(np.uint64)
        key = np.stack([pods.has_number.astype(np.uint64), pods.number,
                        pods.has_memory.astype(np.uint64), pods.memory,
                        pods.has_clock.astype(np.uint64), pods.clock, cls], axis=1)
        # (a label that is absent carries no value)
        key[:, 1] *= key[:, 0]
        key[:, 3] *= key[:, 2]
        key[:, 5] *= key[:, 4]
        self.specs, self.spec_of = np.unique(key, axis=0, return_inverse=True)
        self.spec_of = self.spec_of.reshape(-1)
        self._codes = {}
        hist = np.zeros((len(self.specs), 6), np.int64)
        for s in range(len(self.specs)):
            hist[s] = np.bincount(self.spec_codes(s), minlength=6)
        self.hist = hist[self.spec_of]                 # [P, 6] nodes per code
        self.all_counts = self.hist[:, list(COUNTED)].astype(np.uint32)
        self.n_feasible = self.hist[:, REASON_NONE].astype(np.uint32)

    def spec_codes(self, s):
        if s not in self._codes:
            if len(self._codes) > 64:
                self._codes.clear()
            self._codes[s] = _spec_codes(self.nd, self.present, self.words, self.n_classes,
                                         [int(v) for v in self.specs[s]])
        return self._codes[s]

    def codes(self, p):
        """uint8 [N]: the reason row of pod p."""
        return self.spec_codes(int(self.spec_of[p]))

    def selected(self):
        return self.n_feasible == 0

    def counts(self, all=False):
        """What yoda_diagnose + yoda_download_diagnosis answer: uint32 [P, 4]."""
        out = self.all_counts.copy()
        if not all:
            out[~self.selected()] = UNSELECTED
        return out


def oracle_feasible(model, pods, idx):
    """{pod: bool [n_nodes]} for the pods `idx`: the C oracle's Filter (oracle.pod_detail) on the
    snapshot WITHOUT the absent nodes, narrowed by the pod's class bit -- F' of include/yoda.h,
    with no word of this file's predicates in it."""
    import oracle
    from yoda_amd.soa import MODE_SCV
    keep, out = model.keep(), {}
    idx = np.asarray(idx, np.int64)
    comp, sub = (model.compact(), pods.take(idx)) if keep.size else (None, None)
    for q, p in enumerate(idx.tolist()):
        bits = np.zeros(model.base.n_nodes, bool)
        if keep.size:
            feas = np.asarray(oracle.pod_detail(comp, sub, q, MODE_SCV)[1], bool)
            bits[keep[feas & model.candidates(p)[keep]]] = True
        out[p] = bits
    return out


def references(nodes, pods, steps):
    """[(tag, Reference, Model copy)] of every check, in order."""
    return [(tag, Reference(m, pods), m) for tag, m in cc.states(nodes, steps)]


def _push_numbers(rng, nd, share=0.5, top=3):
    """CardNumber of a share of the nodes down to 0 .. top - 1; the allocation stays."""
    ids = np.sort(rng.choice(nd.n_nodes, max(1, int(nd.n_nodes * share)), replace=False))
    cn = rng.integers(0, top, ids.size).astype(np.uint64)
    return ("push", ids.astype(np.uint32), nd.alloc_memory[ids].copy(), cn)


def _classes(rng, n, P, n_classes, lack=0.3):
    """(words, cls): every class lacks a share `lack` of the nodes; the pods are spread over the
    classes and ANY."""
    words = np.full(n, np.uint64((1 << n_classes) - 1), np.uint64)
    for c in range(n_classes):
        words[rng.choice(n, max(1, int(n * lack)), replace=False)] &= ~np.uint64(1 << c)
    cls = rng.integers(0, n_classes + 1, P).astype(np.uint8)
    cls[cls == n_classes] = ANY
    return words, cls


WALK = ("number pushed", "cards updated", "nodes out", "classes", "half back", "words updated",
        "classes off")


@functools.lru_cache(maxsize=None)
def walk(shape, seed=5):
    """A seeded walk on a shape of card_update_cases.shape_workload: CardNumber pushed down (the
    config-3 shapes have no number failure as uploaded), card FreeMemory / Health updated, nodes
    taken out and half of them back, 3-8 classes with ANY pods mixed in, a sparse word update,
    candidates off; a check after each.  Cached: do not write to the arrays."""
    nd, pd = cu.shape_workload(shape, MIXED_PODS)
    rng = np.random.default_rng(seed + WALK_SHAPES.index(shape))
    n, P = nd.n_nodes, pd.n_pods
    m = cc.Model(nd)
    steps = []

    def add(tag, *ss):
        for s in ss:
            m.apply(s)
        steps.extend(list(ss) + [("check", tag)])

    add(WALK[0], _push_numbers(rng, nd))
    ids = np.sort(rng.choice(n, n // 4, replace=False))
    pool = cu._free_pool(nd) if shape == "ranks" else None
    add(WALK[1], cu._cards(ids, *cu._draw(rng, m, ids, pool, flip=0.4)))
    gone = rng.choice(n, n // 8, replace=False)
    add(WALK[2], npc._present(gone, 0))
    n_classes = 3 + (seed + WALK_SHAPES.index(shape)) % 6
    words, cls = _classes(rng, n, P, n_classes)
    add(WALK[3], ("cand", n_classes, words), ("classes", cls))
    add(WALK[4], npc._present(gone[: gone.size // 2], 1))
    upd = rng.choice(n, 40, replace=False).astype(np.uint32)
    add(WALK[5], ("update", upd, np.where(rng.random(40) < 0.5, 0, (1 << n_classes) - 1)
                  .astype(np.uint64)))
    add(WALK[6], ("cand", 0, None))
    return nd, pd, steps


def _fleet(n_nodes, n_pods, seed=9, cfg=3, n_classes=4):
    """A fleet as uploaded, then CardNumber pushed down, then classes: three checks."""
    nd, pd = synth.make_config(cfg, pods=n_pods, nodes=n_nodes)
    rng = np.random.default_rng(seed + n_nodes + n_pods)
    words, cls = _classes(rng, n_nodes, n_pods, n_classes)
    steps = [("check", "as uploaded"), _push_numbers(rng, nd), ("check", "number pushed"),
             ("cand", n_classes, words), ("classes", cls), ("check", "classes")]
    return nd, pd, steps


TINY_FLEETS = (1, 63, 64, 65, 193)     # nodes; 193 spans four 64-node blocks and ends mid-block
BATCHES = (1, 64, 65, 130)             # pods
MAX_CARDS = (1, 2, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def tiny_fleet(n_nodes):
    return _fleet(n_nodes, 130)


@functools.lru_cache(maxsize=None)
def batch(n_pods):
    return _fleet(193, n_pods)


@functools.lru_cache(maxsize=None)
def ordered_batch():
    """More than 128 pods: the batch is sorted on the device (and padded to waves) unless
    yoda_set_pod_order(h, 0); the GPU test runs it both ways."""
    return _fleet(1500, 700)


@functools.lru_cache(maxsize=None)
def cards(k):
    """A fleet whose card arrays are k wide (the kernels' K): config 3 cut to its first k cards,
    or at 16 config 4 (empty CardLists, CardNumber != len(CardList))."""
    if k == 16:
        return _fleet(700, 130, cfg=4)
    nd, pd, steps = _fleet(700, 130)
    nd = nd.slice(0, nd.n_nodes)
    for f in ("card_free_memory", "card_total_memory", "card_clock", "card_bandwidth", "card_core",
              "card_power", "card_healthy"):
        setattr(nd, f, np.ascontiguousarray(getattr(nd, f)[:, :k]))
    nd.card_count = np.minimum(nd.card_count, k).astype(nd.card_count.dtype)
    nd.free_memory_sum = nd.card_free_memory.sum(axis=1, dtype=np.uint64)
    nd.total_memory_sum = nd.card_total_memory.sum(axis=1, dtype=np.uint64)
    nd.alloc_memory = np.minimum(nd.alloc_memory, nd.total_memory_sum)
    nd = nd.normalized()
    assert nd.max_cards == k
    steps = [s if s[0] != "push" else (s[0], s[1], nd.alloc_memory[s[1]].copy(), s[3])
             for s in steps]
    return nd, pd, steps


# Long chunks.  The sweep cuts the nodes into about 32768 / (selected pod waves) chunks of whole
# 64-node blocks: with 1032 selected waves (YODA_DIAG_ALL over 66,000 pods) that is 31 chunks, so
# the 34 blocks of 2150 nodes make 17 chunks of two blocks, the last of them 102 nodes long (it
# ends mid-block).  The default selection of the same batch takes one-block chunks.
LONG_PODS, LONG_NODES = 66000, 2150


@functools.lru_cache(maxsize=None)
def long_chunks():
    """(600 distinct pods, repeated: the reference evaluates each distinct (labels, class) once)"""
    nd, pd, steps = _fleet(LONG_NODES, LONG_PODS)
    return nd, pd.take(np.arange(LONG_PODS) % 600), steps


@functools.lru_cache(maxsize=None)
def number_labels():
    """Pods with scv/number "0" (passes every present node's PodFitsNumber, needs no card),
    absent (CardNumber > 0, one card) and a wrapped negative (strconv.Atoi("-3") as uint: above
    every CardNumber and every card count), on a fleet with CardNumber 0 nodes."""
    nd, pd, steps = _fleet(193, 130)
    pd = pd.slice(0, pd.n_pods)
    for i, (has, num) in enumerate([(1, 0), (0, 0), (1, 2 ** 64 - 3)] * 4):
        pd.has_number[i], pd.number[i] = has, num
    return nd, pd.normalized(), steps


@functools.lru_cache(maxsize=None)
def none_selected():
    """Every pod has a feasible node: the default selection is empty."""
    nd, pd = synth.make_config(3, pods=130, nodes=900)
    ok = Reference(cc.Model(nd), pd).n_feasible > 0
    pd = pd.take(np.flatnonzero(ok)[:100])
    return nd, pd, [("check", "as uploaded")]


def scenarios():
    """{name: (nodes, pods, steps)} of every scenario but the walks' (walk(shape))."""
    out = {f"fleet {n}": tiny_fleet(n) for n in TINY_FLEETS}
    out.update({f"batch {p}": batch(p) for p in BATCHES})
    out.update({f"cards {k}": cards(k) for k in MAX_CARDS})
    out["ordered batch"] = ordered_batch()
    out["number labels"] = number_labels()
    out["none selected"] = none_selected()
    out["long chunks"] = long_chunks()
    return out
