"""Stream-contract scenarios as plain data (no fixtures): the inputs of tests/test_gpu_streams.py,
which queues libyoda calls behind a busy caller stream (include/yoda.h: yoda_set_stream, "work
already queued on the previous stream is ordered before the new stream's next work"; yoda_run
"asynchronous on the handle's stream").  A wrong ordering there is silent -- the previous batch's
pods, the previous node state, the other snapshot's table -- so every scenario comes with the
answer a wrong ordering would give, and tests/test_stream_cases.py shows with the oracle alone that
it differs from the right one.  The generators are the suite's own (batch_2085 of
tests/test_gpu_step_kernels.py, synth.make_config, the *_cases walks); nothing here runs libyoda.

    mode_b_batch()     scenario 2: a batch whose Mode B answers differ pod by pod
    batch_pair(name)   scenario 3: one snapshot and the two batches A, B of a size sequence
    burst()            scenario 4: five live-snapshot updates whose last writer decides
    ranks_pair()       scenario 7: two memory-ranks snapshots, as many distinct memory values each
    state_pair()       scenario 7 with a node-state push in place of the re-upload"""
import functools

import numpy as np

import oracle
import replace_cases as rc
from test_gpu_step_kernels import batch_2085
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, NodeSoA

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
MAX_FREE, MAX_TOTAL = 3, 5  # columns of EvalResult.maxima: FreeMemory, TotalMemory (kMaxFree, kMaxTotal)


def schedule(nodes, pods):
    return oracle.schedule(nodes, pods, MODE_SCV, threads=8)


def copy_nodes(nd):
    return NodeSoA(**{f: np.array(getattr(nd, f)) for f in nd.__dataclass_fields__})


# ---- scenario 2: Mode B after Mode A ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mode_b_batch():
    """(nodes, pods): batch_2085 with a distinct Mode B request per pod.  Cached: do not write."""
    nodes, pods = _big()
    return nodes, synth.distinct_diskio(pods).normalized()


# ---- scenario 3: back-to-back batches of changing size ----------------------------------------
SIZE_SEQUENCES = ("big_small", "small_big", "big_reversed")


@functools.lru_cache(maxsize=None)
def _big():
    return batch_2085()


@functools.lru_cache(maxsize=None)
def _small_pods():
    # the 300-pod batch of the 300x130 shape (two pod blocks, no probe), on the big snapshot
    return synth.make_config(3, pods=300, nodes=130)[1].normalized()


def batch_pair(name):
    """(nodes, A, B): 2,085 pods then 300, 300 then 2,085, 2,085 then the same pods reversed.
    Cached arrays: do not write to them."""
    nodes, big = _big()
    if name == "big_small":
        return nodes, big, _small_pods()
    if name == "small_big":
        return nodes, _small_pods(), big
    if name == "big_reversed":
        return nodes, big, big.take(np.arange(big.n_pods)[::-1])
    raise ValueError(name)


def disagreement(ra, rb):
    """(share of the compared pod positions -- the first min(P_A, P_B) -- where A and B differ in
    n_feasible or a maximum, share where they differ in the pick)."""
    n = min(ra.pick.size, rb.pick.size)
    state = (ra.n_feasible[:n] != rb.n_feasible[:n]) | (ra.maxima[:n] != rb.maxima[:n]).any(axis=1)
    return float(state.mean()), float((ra.pick[:n] != rb.pick[:n]).mean())


# ---- scenario 4: the hand-written burst -------------------------------------------------------
class Model(rc.Model):
    """replace_cases.Model (every field of every node, who is present) that also takes the node-state
    push and the card update of tests/card_update_cases.py."""

    def apply(self, step):
        n, k = self.base.n_nodes, self.base.max_cards
        if step[0] == "push":
            _, ids, alloc, cn = step
            for i, a, c in zip(ids.tolist(), alloc.tolist(), cn.tolist()):
                if i < n:
                    self.cur.alloc_memory[i], self.cur.card_number[i] = a, c
        elif step[0] == "cards":
            _, ids, free, healthy, fsum = step
            free, healthy = np.asarray(free).reshape(-1, k), np.asarray(healthy).reshape(-1, k)
            for t, i in enumerate(np.asarray(ids).tolist()):
                if i < n:
                    real = np.arange(k) < self.cur.card_count[i]
                    self.cur.card_free_memory[i] = np.where(real, free[t], 0)
                    self.cur.card_healthy[i] = np.where(real, healthy[t] != 0, 0)
                    self.cur.free_memory_sum[i] = fsum[t]
        else:
            super().apply(step)


BURST_CALLS = ("push full", "push empty", "cards", "present", "replace")
# the calls that write what another call of the burst writes: moving one of them across that call
# changes the state.  set_node_present commutes with the other four by contract (an update that
# names an absent node applies and leaves it absent): dropping it is what shows.
BURST_ORDERED = ((0, 1), (1, 4), (2, 4))  # (earlier, later): swapping the pair changes the answer


@functools.lru_cache(maxsize=None)
def burst():
    """(nodes, pods, five steps): 700 pods x 900 nodes (card_update_cases' "small" shape).  With
    `top` the nodes most pods pick, most first:
      0  set_node_state  top[0:40]   fully allocated
      1  set_node_state  top[20:60]  nothing allocated, CardNumber 1   (top[20:40]: the last writer)
      2  update_cards    top[30:70]  half the free memory a card
      3  set_node_present top[60:90] absent
      4  replace_nodes   top[35]     the record of the node fewest pods fit, nothing allocated
    Cached arrays: do not write to them."""
    nd, pd = synth.make_config(3, pods=700, nodes=900)
    nd, pd = nd.normalized(), pd.normalized()
    r = schedule(nd, pd)
    ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
    top = ids[np.argsort(-cnt, kind="stable")]
    rest = np.setdiff1d(np.arange(nd.n_nodes), top)
    top = np.concatenate([top, rest])[:90].astype(np.uint32)
    a, b, c, d = top[0:40], top[20:60], top[30:70], top[60:90]
    x = top[35:36]
    free = nd.card_free_memory[c] // np.uint64(2)
    src = int(rest[-1])
    rec = nd.take(np.array([src]))
    rec.alloc_memory = np.zeros(1, np.uint64)
    steps = (
        ("push", a, nd.total_memory_sum[a].copy(), nd.card_number[a].copy()),
        ("push", b, np.zeros(b.size, np.uint64), np.ones(b.size, np.uint64)),
        ("cards", c, free, nd.card_healthy[c].copy(), free.sum(axis=1, dtype=np.uint64)),
        ("present", d, np.zeros(d.size, np.uint8)),
        ("replace", x, rec),
    )
    return nd, pd, steps


def after(nodes, steps):
    m = Model(nodes)
    for s in steps:
        m.apply(s)
    return m


def burst_variants():
    """{name: steps}: the burst with one call dropped, and with each ordered pair swapped."""
    _, _, steps = burst()
    out = {}
    for k, name in enumerate(BURST_CALLS):
        out[f"without {name}"] = steps[:k] + steps[k + 1:]
    for i, j in BURST_ORDERED:
        s = list(steps)
        s[i], s[j] = s[j], s[i]
        out[f"{BURST_CALLS[j]} before {BURST_CALLS[i]}"] = tuple(s)
    return out


# ---- scenario 7: a re-upload with a step in flight --------------------------------------------
RANK_FIELDS = ("card_free_memory", "card_total_memory", "free_memory_sum", "total_memory_sum",
               "alloc_memory")


RANK_SHAPES = {"1300": (600, 1300), "64": (300, 64)}  # name: (pods, nodes)


@functools.lru_cache(maxsize=None)
def ranks_pair(shape="1300"):
    """(first, second, pods) for upload_nodes(mem_ranks=True): 600 pods x 1,300 nodes, or 300 x 64
    -- a snapshot whose every upload copy is a few KB, which a HIP runtime takes from pageable
    memory without waiting for the stream.  The second snapshot holds every memory quantity three
    times the first's -- as many distinct values, every one another -- so a step of the first that
    read the second's value table reports other FreeMemory and TotalMemory maxima.  Cached arrays:
    do not write to them."""
    n_pods, n_nodes = RANK_SHAPES[shape]
    nd, pd = synth.make_config(3, pods=n_pods, nodes=n_nodes)
    first = nd.normalized()
    second = copy_nodes(first)
    for f in RANK_FIELDS:
        setattr(second, f, getattr(first, f) * np.uint64(3))
    return first, second.normalized(), pd.normalized()


@functools.lru_cache(maxsize=None)
def state_pair():
    """(nodes, pods, push, nodes after the push): the same shape without ranks; the push takes
    CardNumber to 0 on every second node and allocates the others' memory in full."""
    nd, pd = synth.make_config(3, pods=600, nodes=1300)
    nd, pd = nd.normalized(), pd.normalized()
    ids = np.arange(nd.n_nodes, dtype=np.uint32)
    cn = np.where(ids % 2 == 0, 0, nd.card_number).astype(np.uint64)
    alloc = np.where(ids % 2 == 0, nd.alloc_memory, nd.total_memory_sum).astype(np.uint64)
    moved = copy_nodes(nd)
    moved.card_number, moved.alloc_memory = cn.copy(), alloc.copy()
    return nd, pd, ("push", ids, alloc, cn), moved.normalized()
