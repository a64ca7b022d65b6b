"""Whole-record replacement and Mode B metric scenarios as plain data (no fixtures): the snapshot
as uploaded, the pods, and the steps a long-lived handle would see between uploads.
tests/test_replace_cases.py checks with the oracle alone that every scenario moves enough picks,
feasible counts or PreScore maxima to fail a wrong handle; tests/test_gpu_replace_nodes.py and
tests/test_gpu_node_metrics.py replay them on libyoda.

Each scenario returns (nodes, pods, steps); a step is one of
    ("replace", ids u32, recs NodeSoA)              yoda_replace_nodes of that list (GLOBAL ids)
    ("metrics", ids u32 or None, cpu, disk_io)      yoda_update_node_metrics (None: dense)
    ("present", ids u32, flags u8)                  yoda_set_node_present
    ("check", tag)                                  compare the handle with the model here
Model applies a step to ALL node fields and returns the NodeSoA a fresh upload of that state
would get."""
import functools

import numpy as np

from card_update_cases import BASE_NODES, BASE_PODS, SHAPES, UPLOAD_KW, shape_workload  # noqa: F401
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, NodeSoA

FIELDS = tuple(NodeSoA.__dataclass_fields__)
CARD_FIELDS = tuple(f for f in FIELDS if f.startswith("card_") and f not in ("card_number",
                                                                             "card_count"))
# PreScore's MaxValue fields in the order of EvalResult.maxima's columns' sources
MAX_FIELDS = ("card_bandwidth", "card_clock", "card_core", "card_free_memory", "card_power",
              "card_total_memory")


def copy_nodes(nd):
    return NodeSoA(**{f: np.array(getattr(nd, f)) for f in FIELDS})


class Model:
    """The state a handle holds after the steps applied so far: every field of every node, and
    who is present.  A replacement of an absent node applies and leaves it absent."""

    def __init__(self, nodes):
        self.base = nodes
        self.cur = copy_nodes(nodes)
        self.present = np.ones(nodes.n_nodes, bool)

    def apply(self, step):
        n, k = self.base.n_nodes, self.base.max_cards
        if step[0] == "replace":
            _, ids, recs = step
            recs = recs.normalized()
            kr = recs.max_cards
            # ids outside the snapshot are ignored by contract; a repeated id keeps its last entry
            for t, i in enumerate(np.asarray(ids).tolist()):
                if i >= n:
                    continue
                for f in FIELDS:
                    v = getattr(recs, f)[t]
                    if f in CARD_FIELDS:
                        assert not v[k:].any(), "the record's cards fit the snapshot's stride"
                        row = np.zeros(k, v.dtype)
                        row[:min(k, kr)] = v[:k]
                        v = row
                    getattr(self.cur, f)[i] = v
        elif step[0] == "metrics":
            _, ids, cpu, disk = step
            if ids is None:
                self.cur.cpu[:], self.cur.disk_io[:] = cpu, disk
            else:
                for t, i in enumerate(np.asarray(ids).tolist()):
                    if i < n:
                        self.cur.cpu[i], self.cur.disk_io[i] = cpu[t], disk[t]
        elif step[0] == "present":
            _, ids, flags = step
            for i, f in zip(np.asarray(ids).tolist(), np.asarray(flags).tolist()):
                if i < n:
                    self.present[i] = f != 0
        elif step[0] != "check":
            raise ValueError(step[0])

    def nodes(self):
        return copy_nodes(self.cur)

    def keep(self):
        """Ids of the present nodes, ascending: position in the compacted snapshot -> id."""
        return np.flatnonzero(self.present)

    def absent(self):
        return np.flatnonzero(~self.present)

    def compact(self):
        return self.nodes().take(self.keep())


def states(nodes, steps):
    """[(tag, Model copy)] of every check, in order."""
    import copy
    m, out = Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], copy.deepcopy(m)))
    return out


def reference(model, pods, threads=8):
    """What every Mode A evaluation must answer in this state: the oracle on the snapshot
    without the absent nodes, picks as ids of the full one."""
    import oracle
    keep = model.keep()
    res = oracle.schedule(model.compact(), pods, MODE_SCV, threads=threads)
    ok = res.pick >= 0
    res.pick[ok] = keep[res.pick[ok]].astype(res.pick.dtype)
    return res


def _replace(ids, recs):
    return ("replace", np.asarray(ids, np.uint32), recs)


def _present(ids, flags):
    ids = np.asarray(ids, np.uint32)
    return ("present", ids, np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8),
                                                                 ids.shape)))


def _most_picked(nd, pd):
    """Node ids by how many pods pick them in this state, most first."""
    import oracle
    r = oracle.schedule(nd, pd, MODE_SCV, threads=8)
    ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
    return ids[np.argsort(-cnt, kind="stable")]


def _real(nd, ids):
    return np.arange(nd.max_cards)[None, :] < nd.card_count[ids][:, None]


def _sums(rec):
    """The record's memory sums and CardNumber recomputed from its cards."""
    rec.free_memory_sum = rec.card_free_memory.sum(axis=1, dtype=np.uint64)
    rec.total_memory_sum = rec.card_total_memory.sum(axis=1, dtype=np.uint64)
    return rec


WALK_SIZES = (64, 1, 700, 0, 7, 64)
WALK_EMPTY = 3     # index of the check after the count == 0 list
WALK_OUTSIDE = 5   # this list also holds ids at or beyond n_nodes and repeated ids
OUTSIDE = (0, 5, 100000)  # + n_nodes; and 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def walk(shape="base", seed=23, mixed_pods=32768 + 37):
    """(a) A seeded walk of replacements of 64, 1, 700, 0 and 7 nodes and one list with ids
    outside the snapshot and 40 repeated ids whose real entry is last.  Each replaced node takes
    the record of another node of the snapshot as uploaded -- in-format by construction, the rank
    tables included -- with another card count where the shape has differing counts.  Half of
    every list (at least one node) are the nodes most pods pick when the list is made.  Cached:
    the arrays are shared, do not write to them."""
    nd, pd = shape_workload(shape, mixed_pods)
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    sample = pd.slice(0, min(pd.n_pods, 3000))
    m = Model(nd)
    counts_differ = np.unique(nd.card_count).size > 1
    steps = []

    def choose(size):
        ids = _most_picked(m.nodes(), sample)[:(size + 1) // 2] if size else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(n), ids)
        return rng.permutation(np.concatenate([ids, rng.choice(rest, size - ids.size,
                                                               replace=False)]))

    def sources(ids):
        src = rng.integers(0, n, ids.size)
        for _ in range(40):
            bad = src == ids
            if counts_differ:
                bad |= nd.card_count[src] == nd.card_count[ids]
            if not bad.any():
                break
            src[bad] = rng.integers(0, n, int(bad.sum()))
        assert (src != ids).all()
        return src

    for k, size in enumerate(WALK_SIZES):
        ids = choose(size)
        src = sources(ids)
        if k == WALK_OUTSIDE:
            # ignored by contract: n_nodes, beyond it, and u32 max (with some node's record); and
            # 40 ids listed twice, first with the record of yet another node, their real entry last
            out = np.array([n + o for o in OUTSIDE] + [0xFFFFFFFF], np.int64)
            at = rng.choice(ids.size, out.size, replace=False)
            ids2 = np.insert(ids, at, out)
            src2 = np.insert(src, at, rng.integers(0, n, out.size))
            rep = rng.choice(ids.size, 40, replace=False)
            ids = np.concatenate([ids[rep], ids2])
            src = np.concatenate([(src[rep] + 1) % n, src2])
        step = _replace(ids, nd.take(src))
        m.apply(step)
        steps += [step, ("check", f"walk {k}")]
    return nd, pd, steps


# (b) what each MaxValue field rises by: new values no model of the snapshot holds, inside every
# format the shapes use (small fields <= 55738, memory <= 0xFFFFFFFE)
RAISE = {"card_bandwidth": 100, "card_clock": 45, "card_core": 12, "card_free_memory": 1000,
         "card_power": 50, "card_total_memory": 1024}


def new_model(nodes=BASE_NODES, pods=BASE_PODS):
    """(b) The node most pods pick becomes a GPU model the snapshot did not hold: for each of the
    six MaxValue fields one replacement lifts that field above the fleet's maximum (every card
    of the node for the model fields and TotalMemory, one healthy card for FreeMemory), a second
    returns the node's own record: the G maxima go up and back, six times."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    i = int(_most_picked(nd, pd)[0])
    own = nd.take([i])
    steps = [("check", "as uploaded")]
    for f in MAX_FIELDS:
        rec = copy_nodes(own)
        top = getattr(nd, f).max() + np.uint64(RAISE[f])
        if f == "card_free_memory":
            rec.card_free_memory[0, int(np.argmax(rec.card_healthy[0] != 0))] = top
        else:
            getattr(rec, f)[0, :int(rec.card_count[0])] = top
        steps += [_replace([i], _sums(rec)), ("check", f"{f} raised"),
                  _replace([i], own), ("check", f"{f} restored")]
    return nd, pd, steps


def block_clocks(nodes=BASE_NODES, pods=BASE_PODS):
    """(c) Every node of the 64-node blocks with block % 3 == 1 gets another clock of the fleet's
    three (a model of its own: the clock of one GPU model with the rest of another), then its own
    back.  Half the pods carry a clock label: whole blocks change sides for them."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    assert pd.has_clock.mean() > 0.3
    ids = np.flatnonzero((np.arange(nd.n_nodes) // 64) % 3 == 1)
    own = nd.take(ids)
    rec = copy_nodes(own)
    at = np.searchsorted(synth.CLOCKS, own.card_clock)
    rec.card_clock = np.where(_real(nd, ids), synth.CLOCKS[(at + 1) % 3], 0).astype(np.uint64)
    steps = [("check", "as uploaded"), _replace(ids, rec), ("check", "other clocks"),
             _replace(ids, own), ("check", "own clocks")]
    return nd, pd, steps


def mixed_and_back(nodes=BASE_NODES, pods=BASE_PODS):
    """(d) Ten nodes of an all-one-model snapshot -- the five most picked and five more -- become
    mixed-model nodes (their odd cards take the next GPU model's clock, bandwidth, cores and
    power), then revert: all_one_model flips both ways."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    top = _most_picked(nd, pd)[:5]
    rest = np.setdiff1d(np.arange(nd.n_nodes), top)
    ids = np.concatenate([top, np.random.default_rng(41).choice(rest, 5, replace=False)])
    own = nd.take(ids)
    rec = copy_nodes(own)
    at = (np.searchsorted(synth.CLOCKS, own.card_clock) + 1) % 3
    odd = _real(nd, ids) & (np.arange(nd.max_cards)[None, :] % 2 == 1)
    for f, table in (("card_clock", synth.CLOCKS), ("card_bandwidth", synth.BANDWIDTHS),
                     ("card_core", synth.CORES), ("card_power", synth.POWERS)):
        setattr(rec, f, np.where(odd, table[at], getattr(own, f)).astype(np.uint64))
    steps = [("check", "one model each"), _replace(ids, rec), ("check", "ten mixed"),
             _replace(ids, own), ("check", "one model again")]
    return nd, pd, steps


SPARE, JOIN = 128, 64


def spare_slots(nodes=BASE_NODES, pods=BASE_PODS):
    """(e) Scale-up through spare slots: 128 scattered nodes of the upload are placeholders (card
    count 0, every field 0) and are taken out.  64 of them get real records while absent -- the
    records of the nodes most pods pick, so that a slot that counted would take picks -- and stay
    out; then they are put back.  Returns the slots too."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    rng = np.random.default_rng(43)
    slots = np.sort(rng.choice(nd.n_nodes, SPARE, replace=False))
    top = _most_picked(nd, pd)
    top = top[~np.isin(top, slots)][:JOIN]
    rest = np.setdiff1d(np.arange(nd.n_nodes), np.concatenate([top, slots]))
    src = np.concatenate([top, rng.choice(rest, JOIN - top.size, replace=False)])
    recs = nd.take(src)
    up = copy_nodes(nd)
    for f in FIELDS:
        getattr(up, f)[slots] = 0
    join = slots[rng.permutation(SPARE)[:JOIN]]
    steps = [_present(slots, 0), ("check", "slots out"),
             _replace(join, recs), ("check", "records while absent"),
             _present(join, 1), ("check", "joined")]
    return up.normalized(), pd, steps, slots, join


def card_counts(nodes=900, pods=700):
    """(f) 32 nodes, half of them the most picked, go from 8 cards to their first 2, to none and
    back to their own 8 (CardNumber and the sums follow).  Then the most picked node gets a clock
    no other node has and TotalMemorySum 0: pods it stays feasible for among others end in
    YODA_STATUS_DIV_ZERO, and the last pod, labelled with that clock, finds it alone feasible --
    the single-feasible-node rule scores nothing and picks it."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    lone = int(synth.CLOCKS.max()) + 45
    pd = copy_pods_with_clock(pd, lone)
    top = _most_picked(nd, pd)[:16]
    rest = np.setdiff1d(np.arange(nd.n_nodes), top)
    ids = np.concatenate([top, np.random.default_rng(47).choice(rest, 16, replace=False)])
    own = nd.take(ids)

    def cut(cnt):
        rec = copy_nodes(own)
        rec.card_count[:] = cnt
        rec.card_number[:] = cnt
        return _sums(rec.normalized())

    z = nd.take(top[:1])
    z.card_clock = np.where(z.card_clock != 0, np.uint64(lone), 0).astype(np.uint64)
    z.total_memory_sum = np.zeros(1, np.uint64)
    steps = [("check", "8 cards"), _replace(ids, cut(2)), ("check", "2 cards"),
             _replace(ids, cut(0)), ("check", "no cards"), _replace(ids, own),
             ("check", "8 cards again"), _replace(top[:1], z), ("check", "zero total")]
    return nd, pd, steps


def copy_pods_with_clock(pd, clock):
    """The batch with its last pod asking for one card at `clock` and nothing else."""
    p = type(pd)(**{f: np.array(getattr(pd, f)) for f in pd.__dataclass_fields__})
    p.has_number[-1], p.number[-1] = 1, 1
    p.has_memory[-1], p.memory[-1] = 0, 0
    p.has_clock[-1], p.clock[-1] = 1, clock
    return p.normalized()


# ---- (g) the range rules: (name, shape, what the offending record changes) ----
def _small():
    return synth.make_config(3, pods=300, nodes=900)


def range_shape(shape):
    """(nodes, pods, upload kwargs) of a range-rule shape."""
    nd, pd = _small()
    kw = {}
    if shape == "ranks":
        nd, pd = synth.memory_in_bytes(nd, pd)
    elif shape == "wide":  # bandwidth beyond 16 bits: unpacked K1 partials, f64 quotients
        nd = synth.wide_fields(nd, ("bandwidth",), 1000)
    elif shape in ("f64", "u64"):
        kw = UPLOAD_KW[shape]
    elif shape != "small":
        raise ValueError(shape)
    return nd, pd, kw


def _set_all(field, value):
    def f(rec):
        a = getattr(rec, field)
        a[0, :int(rec.card_count[0])] = value
    return f


def _wide_record(rec):
    k = 16
    out = NodeSoA(**{f: (np.pad(getattr(rec, f), ((0, 0), (0, k - rec.max_cards)))
                         if f in CARD_FIELDS else np.array(getattr(rec, f))) for f in FIELDS})
    for f in CARD_FIELDS:
        getattr(out, f)[0, 8] = getattr(out, f)[0, 0]
    out.card_count[0] = 9
    return out


def _mixed(rec):
    rec.card_clock[0, 1] = rec.card_clock[0, 0] + np.uint64(1)


def _fast_clock(rec):  # 100 * clock / bandwidth of 6e8: 8 * (800 + that) leaves 32 bits
    rec.card_clock[0, :int(rec.card_count[0])] = 6_000_000
    rec.card_bandwidth[0, :int(rec.card_count[0])] = 1


def _alien(field):
    def f(rec):
        a = getattr(rec, field)
        a[0, 0] = a[0, 0] + np.uint64(1)   # bytes: every uploaded value is a multiple of 2^20
    return f


def _static(rec):  # Actual = FreeMemorySum * 100 / TotalMemorySum * 2
    rec.free_memory_sum[0] = 1 << 45
    rec.total_memory_sum[0] = 1


RANGE_RULES = (
    ("card count above K", "small", _wide_record),
    ("small field above 0xFFFFFFFE", "wide", _set_all("card_bandwidth", 0xFFFFFFFF)),
    ("small field above 16 bits", "small", _set_all("card_power", 0x10000)),
    ("small field above the f32 quotients", "small", _set_all("card_core", 55739)),
    ("mixed-model node without f32 quotients", "wide", _mixed),
    ("clock quotient", "wide", _fast_clock),
    ("memory above 0xFFFFFFFE", "small", _set_all("card_total_memory", 0xFFFFFFFF)),
    ("FreeMemory outside the rank table", "ranks", _alien("card_free_memory")),
    ("TotalMemory outside the rank table", "ranks", _alien("card_total_memory")),
    ("f64 field above 2^44", "f64", _set_all("card_free_memory", (1 << 44) + 1)),
    ("static score n32", "small", _static),
    ("static score f64", "f64", _static),
    ("node score f64", "f64", _set_all("card_clock", 1 << 43)),
    ("card count above K f64", "f64", _wide_record),
    ("card count above K u64", "u64", _wide_record),
)
RANGE_IDS = (5, 70, 300, 640, 899)


def range_rule(k):
    """(nodes, pods, kw, good step, bad step) of rule k: a five-node list of records of other
    nodes; the bad step's LAST record breaks the rule, the good step is the list without it."""
    name, shape, change = RANGE_RULES[k]
    nd, pd, kw = range_shape(shape)
    ids = np.array(RANGE_IDS, np.uint32)
    recs = nd.take((ids.astype(np.int64) + 17) % nd.n_nodes)
    last = copy_nodes(recs.take([4]))
    out = change(last)
    last = last if out is None else out
    kb = last.max_cards
    bad = NodeSoA(**{f: np.concatenate([
        np.pad(getattr(recs, f)[:4], ((0, 0), (0, kb - recs.max_cards)))
        if f in CARD_FIELDS else getattr(recs, f)[:4], getattr(last, f)]) for f in FIELDS})
    return nd, pd, kw, _replace(ids[:4], recs.take(np.arange(4))), _replace(ids, bad)


# ---- (i) Mode B ----
METRIC_NODES, METRIC_PODS = 1500, 400
METRIC_SIZES = (1, 64, 700, None)


def metrics_walk(seed=29):
    """(i) 1500 nodes, one pod spec and a distinct request per pod (two batches); sparse lists
    of 1, 64 and 700 nodes and the dense form.  The single node is the one most pods pick; every
    list also holds an id outside the snapshot and a repeated id whose real entry is last."""
    import oracle
    from yoda_amd.soa import MODE_DISKIO
    nd, pd = synth.make_config(3, pods=METRIC_PODS, nodes=METRIC_NODES)
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    m = Model(nd)
    steps = [("check", "as uploaded")]
    for size in METRIC_SIZES:
        if size is None:
            step = ("metrics", None, rng.random(n) * 100.0, rng.random(n) * 100.0)
        else:
            r = oracle.schedule(m.nodes(), synth.distinct_diskio(pd), MODE_DISKIO, threads=8)
            top, cnt = np.unique(r.pick[r.pick >= 0], return_counts=True)
            top = top[np.argsort(-cnt, kind="stable")][:(size + 1) // 2]
            rest = np.setdiff1d(np.arange(n), top)
            ids = np.concatenate([top, rng.choice(rest, size - top.size, replace=False)])
            cpu, disk = rng.random(size) * 100.0, rng.random(size) * 100.0
            # first a wrong entry for ids[0], an id outside, then the real entries
            ids = np.concatenate([[ids[0], n + 7], ids]).astype(np.uint32)
            cpu = np.concatenate([[0.0, 1.0], cpu])
            disk = np.concatenate([[99.0, 1.0], disk])
            step = ("metrics", ids, cpu, disk)
        m.apply(step)
        steps += [step, ("check", f"metrics {size}")]
    return nd, pd, steps
