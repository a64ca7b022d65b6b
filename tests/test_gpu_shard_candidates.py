"""Node shards honour candidate classes in the evaluation step (include/yoda.h
yoda_shard_candidates): a snapshot split over several shard handles, each holding its own nodes'
candidate words and the whole batch's class array, gives on EVERY shard what one handle holding the
whole snapshot gives from yoda_run -- the maxima over F, the counts, the single-node rule, DIV_ZERO,
NormalizeScore's bounds, ties, picks and the seeded draw over the global F'.

Every check compares three things: candidate_cases.reference (the oracle's feasibility, raw scores
and maxima, narrowed on the host), every shard's download after the sharded step, and the
download of a single handle that was told the same steps -- the last two bit for bit.  Scenarios and
splits: tests/shard_candidate_cases.py; tests/test_shard_candidate_cases.py shows with the oracle
alone that each of them straddles the cuts.  All shards run on device 0, through
yoda_comm_run_local, dist.ShardExchange.local or a one-rank RCCL communicator."""
import numpy as np
import pytest

import candidate_cases as cases
import shard_candidate_cases as sc
from test_gpu_parity import assert_same
from tie_draw_cases import draw
from yoda_amd import capi
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
_REFS = {}


def reference(key, model, pods, fresh):
    """candidate_cases.reference of a scenario's check, computed once per (scenario, check tag)
    and shared by the splits and drivers; the Snapshot is shared until node values change."""
    if key not in _REFS:
        snap = None if fresh else _REFS.get(("snap", key[0]))
        if snap is None:
            snap = cases.Snapshot(model, pods)
        _REFS["snap", key[0]] = snap
        _REFS[key] = cases.reference(snap, model)
    return _REFS[key]


def same(a, b, what):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{what}: {f}")


class Fleet:
    """One handle per shard of the split, one handle holding the whole snapshot, and the model of
    what all of them were told."""

    def __init__(self, s, b, setting=True):
        self.s, self.b = s, tuple(b)
        self.model = cases.Model(s.nodes)
        self.hs, self.one = [], None
        try:
            for lo, hi in self.ranges():
                y = Yoda(0)
                self.hs.append(y)
                y.upload_nodes(s.nodes.slice(lo, hi), node_offset=lo, **s.kw)
                if setting:
                    y.shard_candidates(True)
            self.one = Yoda(0)
            self.one.upload_nodes(s.nodes, **s.kw)
            assert len({h.path for h in self.hs + [self.one] if h.n_nodes}) == 1
        except Exception:
            self.close()
            raise

    def ranges(self):
        return list(zip(self.b[:-1], self.b[1:]))

    def words(self, step):
        """A "cand" step's words per shard."""
        return sc.split_words(self.b, step[2])

    def apply(self, step):
        self.model.apply(step)
        n = self.s.nodes.n_nodes
        for y, (lo, hi) in zip(self.hs + [self.one], self.ranges() + [(0, n)]):
            if step[0] == "cand":
                y.set_candidates(None if step[2] is None else step[2][lo:hi], step[1])
            elif step[0] == "update":  # global ids: one list for every shard
                y.update_candidates(step[1], step[2])
            elif step[0] == "classes":
                y.set_pod_classes(step[1])
            elif step[0] == "present":
                y.set_node_present(step[1], step[2])
            elif step[0] == "cards":
                y.update_cards(*step[1:])
            elif step[0] == "push":
                y.set_node_state(*step[1:])
            else:
                raise ValueError(step[0])

    def step(self, run=None):
        """One sharded step (yoda_comm_run_local, or `run`); every shard's download identical."""
        for h in self.hs:
            h.upload_pods(self.s.pods)
        if run is None:
            capi.comm_run_local(self.hs, MODE_SCV)
        else:
            run()
        res = [h.download() for h in self.hs]
        for k, r in enumerate(res[1:]):
            same(r, res[0], f"shard {k + 1} against shard 0")
        return res[0]

    def whole(self):
        return self.one.eval(self.s.pods, MODE_SCV)

    def close(self):
        for y in self.hs + ([self.one] if self.one else []):
            y.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def replay(name, fl, steps=None, run=None):
    """The scenario's steps on the fleet; at every check the sharded step against the reference
    and, bit for bit, against the single handle.  Returns the sharded results of the checks."""
    out, fresh = [], False
    for step in (fl.s.steps if steps is None else steps):
        if step[0] != "check":
            fl.apply(step)
            fresh = fresh or step[0] in ("present", "cards", "push")
            continue
        want, _ = reference((name, step[1]), fl.model, fl.s.pods, fresh)
        fresh = False
        got = fl.step(run)
        assert_same(got, want)
        same(got, fl.whole(), f"{name} / {step[1]}: shards against the single handle")
        out.append(got)
    return out


# ---- 1. the walk's states, every record path, both worlds -----------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape", sc.WALK_SHAPES)
def test_walk(shape, world):
    """small: below the grouped node order; base: N32 with it; f64 / u64: the per-node K1's dense
    masks, u64 the record merge.  Updates go to every shard as ONE list of global ids."""
    s = sc.walk(shape)
    with Fleet(s, s.splits[world - 2]) as fl:
        assert fl.one.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert len(replay("walk " + shape, fl)) == len(cases.WALK)
        assert all(h.candidates_info()[0] == 0 for h in fl.hs)


# ---- 2. the raw protocol through the Python driver -------------------------------------------------
def exchange(fl, cand_step, cls, **kw):
    import torch
    from yoda_amd.dist import ShardExchange
    for h in fl.hs:
        h.upload_pods(fl.s.pods)
    shards = [fl.s.nodes.slice(lo, hi) for lo, hi in fl.ranges()]
    return ShardExchange.local(fl.hs, torch.device("cuda:0"), shards, list(fl.b[:-1]),
                               candidates=(cand_step[1], fl.words(cand_step), cls), **kw)


@pytest.mark.parametrize("caller_order", [True, False])
@pytest.mark.parametrize("compact", [True, False])
def test_shard_exchange_driver(compact, caller_order):
    """dist.ShardExchange.local with candidates on base at world 3: the packed-key and the
    three-reduce merges, the caller-order and the shared radix-order exchange buffers; then the
    walk's live updates between two steps of the same exchange."""
    s = sc.walk("base")
    with Fleet(s, s.splits[1], setting=False) as fl:
        cand, classes = s.steps[0], s.steps[1]
        fl.model.apply(cand)
        fl.model.apply(classes)
        fl.one.set_candidates(cand[2], cand[1])
        fl.one.set_pod_classes(classes[1])
        ex = exchange(fl, cand, classes[1], compact=compact, caller_order=caller_order)
        assert (ex.ib is not None) == compact
        run = lambda: ex.step(MODE_SCV)
        assert len(replay("walk base", fl, s.steps[2:3], run)) == 1
        k = [t[0] == "update" for t in s.steps].index(True)  # uncordon half: global ids
        fl.apply(s.steps[k])
        # (the recipe and this update: the state of the walk's check of that name)
        assert s.steps[k + 1] == ("check", "uncordon half")
        want, _ = reference(("walk base", "uncordon half"), fl.model, s.pods, False)
        got = fl.step(run)
        assert_same(got, want)
        same(got, fl.whole(), "after the update")


# ---- 3. the cross-shard rules -----------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
def test_cross_shard_rules(split):
    """Maxima from shards that hold no candidate of the pod's class, a class nowhere, a shard of
    non-candidates, one-candidate pods beyond shard 0; split 1 adds an empty shard."""
    s, holders, ones = sc.rules()
    with Fleet(s, s.splits[split]) as fl:
        (got,) = replay("rules", fl)
        assert (got.n_feasible[ones] == 1).all() and (got.status[ones] == 0).all()
        assert (got.pick[ones] >= fl.b[1]).all()
        rest = np.setdiff1d(np.flatnonzero((fl.model.cls != sc.ANY) & (got.pick >= 0)), ones)
        assert rest.size >= 500 and not np.isin(got.pick[rest], holders).any()
        assert (got.status[fl.model.cls == 2] == 1).all()


def test_zero_total_split():
    """DIV_ZERO by a zero-total count that another shard holds, the zero node hidden, then the
    zero node as the one survivor: each decided by sums over the shards."""
    s, z, p = sc.zero_split()
    with Fleet(s, s.splits[0]) as fl:
        got = replay("zero", fl)
        assert [int(r.status[p]) for r in got] == [2, 0, 0, 2]
        assert (got[2].pick[p], got[2].n_feasible[p], got[2].n_ties[p]) == (z, 1, 1)


# ---- 4. the exact-normalize exchange ----------------------------------------------------------------
@pytest.mark.parametrize("driver", ["comm_run_local", "shard_exchange"])
def test_overflow_world2(driver):
    s = sc.overflow()
    with Fleet(s, s.splits[0], setting=driver == "comm_run_local") as fl:
        assert fl.one.path == "u64"
        if driver == "comm_run_local":
            assert len(replay("overflow", fl)) == 2
        else:
            cand, classes = s.steps[1], s.steps[2]
            fl.model.apply(cand)
            fl.model.apply(classes)
            fl.one.set_candidates(cand[2], cand[1])
            fl.one.set_pod_classes(classes[1])
            ex = exchange(fl, cand, classes[1])
            assert len(replay("overflow", fl, s.steps[3:], lambda: ex.step(MODE_SCV))) == 1
        assert fl.hs[0].shard_overflow_count() > 0  # the step went through the exact merge


# ---- 5. the draw ------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_draw_over_the_global_tie_set(world):
    """Each tied pod's pick is the argmin of (yoda_tie_hash << 32) | node over the REFERENCE's tie
    set and equals the single handle's draw; nothing else moves."""
    s = sc.dense()
    with Fleet(s, s.splits[world - 2]) as fl:
        (off,) = replay("dense", fl)
        want, ties = _REFS["dense", "dense"]
        tied = np.flatnonzero((want.status == 0) & (want.n_ties >= 2))
        on = want.pick.copy()
        for p in tied.tolist():
            on[p] = draw(sc.SEED, p, ties[p])
        assert (on != want.pick).sum() >= 50
        for h in fl.hs:
            h.set_tie_draw(sc.SEED)
            h.shard_tie_draw(True)
        fl.one.set_tie_draw(sc.SEED)
        got = fl.step()
        np.testing.assert_array_equal(got.pick, on)
        for f in FIELDS[1:]:
            np.testing.assert_array_equal(getattr(got, f), getattr(off, f), err_msg=f)
        same(got, fl.whole(), "the draw: shards against the single handle")


# ---- 6. live state ----------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_with_absent_nodes_and_updates(world):
    s = sc.with_absent()
    with Fleet(s, s.splits[world - 2]) as fl:
        assert len(replay("absent", fl)) == 3


# ---- 7. RCCL ----------------------------------------------------------------------------------------
def test_rccl_world1():
    """yoda_comm_run over a one-rank RCCL communicator with candidates on: the agreement words
    through ncclAllReduce itself (more ranks need more GPUs than a test has)."""
    s = sc.walk("small")
    n = s.nodes.n_nodes
    with Fleet(s, (0, n)) as fl:
        (y,) = fl.hs
        y.comm_init(capi.comm_unique_id(), 0, 1)
        got = replay("walk small", fl, s.steps[:5], lambda: y.comm_run(MODE_SCV))
        assert len(got) == 2


# ---- 8. state ---------------------------------------------------------------------------------------
def raises_state(word="candidate"):
    return pytest.raises(YodaError, match=f"YODA_ERR_STATE.*{word}")


def test_setting_off_keeps_the_refusals():
    import torch
    from yoda_amd.dist import ShardBuffers
    s = sc.walk("small")
    with Fleet(s, s.splits[0], setting=False) as fl:
        for st in s.steps[:2]:
            fl.apply(st)
        b = ShardBuffers(s.pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        for h in fl.hs:
            h.upload_pods(s.pods)
        with raises_state():
            capi.comm_run_local(fl.hs, MODE_SCV)
        with raises_state():
            fl.hs[0].shard_phase1(MODE_SCV, p(b.maxima), p(b.counts))
        # on for one shard only: the other still refuses, and says so
        fl.hs[0].shard_candidates(True)
        with raises_state():
            capi.comm_run_local(fl.hs, MODE_SCV)
        fl.hs[0].shard_candidates(False)
        fl.apply(("cand", 0, None))
        assert_same(fl.step(), fl.whole())


def test_setting_on_without_candidates_changes_nothing():
    s = sc.walk("base")
    with Fleet(s, s.splits[1], setting=False) as fl:
        off = fl.step()
        for h in fl.hs:
            h.shard_candidates(True)
        same(fl.step(), off, "setting on, candidates never set")
        same(off, fl.whole(), "no candidates")


def test_shards_must_agree():
    """Shards that differ in the class array, n_classes or the setting all fail with
    YODA_ERR_STATE; the next agreed step is right."""
    s = sc.walk("small")
    with Fleet(s, s.splits[1]) as fl:
        for st in s.steps[:2]:
            fl.apply(st)
        want, _ = reference(("walk small", cases.WALK[0]), fl.model, s.pods, False)
        words, cls = s.steps[0][2], s.steps[1][1]
        other = cls.copy()
        other[5] = (other[5] + 1) % 8
        lo, hi = fl.ranges()[1]
        for h in fl.hs:
            h.upload_pods(s.pods)

        def disagree(word):
            with raises_state(word):
                capi.comm_run_local(fl.hs, MODE_SCV)
            for h in fl.hs:  # every shard carries the message
                assert word.encode() in capi.lib().yoda_last_error(h._h)

        fl.hs[1].set_pod_classes(other)            # another class array of the same length
        disagree("disagree on the candidate")
        fl.hs[1].set_pod_classes(None)             # no class array
        disagree("disagree on the candidate")
        fl.hs[1].set_pod_classes(cls)
        fl.hs[1].set_candidates(words[lo:hi], 9)   # another n_classes
        disagree("disagree on the candidate")
        fl.hs[1].set_candidates(None, 0)           # candidates off on one shard
        disagree("disagree on the candidate")
        fl.hs[1].set_candidates(words[lo:hi], 8)
        fl.hs[1].shard_candidates(False)           # the setting
        with raises_state():
            capi.comm_run_local(fl.hs, MODE_SCV)
        fl.hs[1].shard_candidates(True)
        got = fl.step()
        assert_same(got, want)
        same(got, fl.whole(), "after the disagreements")


def test_wrong_class_array_length():
    import torch
    from yoda_amd.dist import ShardBuffers
    s = sc.walk("small")
    with Fleet(s, s.splits[0]) as fl:
        for st in s.steps[:2]:
            fl.apply(st)
        want, _ = reference(("walk small", cases.WALK[0]), fl.model, s.pods, False)
        b = ShardBuffers(300, torch.device("cuda:0"))
        for h in fl.hs:
            h.upload_pods(s.pods.slice(0, 300))
        with raises_state("length"):
            capi.comm_run_local(fl.hs, MODE_SCV)
        with raises_state("length"):
            fl.hs[1].shard_phase1(MODE_SCV, b.maxima.data_ptr(), b.counts.data_ptr())
        assert_same(fl.step(), want)


def test_greedy_windows_and_mode_b_still_refuse():
    """With the setting on: the greedy-window shard calls, Mode B on shards, yoda_comm_greedy_local
    and dist.sharded_greedy return YODA_ERR_STATE, and the evaluation step still answers right."""
    import torch
    from yoda_amd.dist import HandleShard, Reducer, ShardBuffers, sharded_greedy
    s = sc.walk("small")
    with Fleet(s, s.splits[0]) as fl:
        for st in s.steps[:2]:
            fl.apply(st)
        want, _ = reference(("walk small", cases.WALK[0]), fl.model, s.pods, False)
        assert_same(fl.step(), want)
        dev = torch.device("cuda:0")
        b = ShardBuffers(s.pods.n_pods, dev)
        b.ensure_witness()
        p = ShardBuffers.ptr
        h = fl.hs[0]
        few = s.pods.slice(0, 50)
        calls = (lambda: h.shard_topk(p(b.maxima), p(b.counts), capi.topk_k()),
                 lambda: h.shard_topk(p(b.maxima), p(b.counts), capi.topk_k_capacity(),
                                      capi.greedy_cap_depth()),
                 lambda: h.shard_best_one(0),
                 lambda: h.shard_phase1_witness(p(b.maxima), p(b.counts), p(b.wit)),
                 lambda: h.shard_witness_prepare(p(b.maxima), p(b.maxima_local), p(b.wit)),
                 lambda: h.shard_witness_download(p(b.maxima), p(b.wit)),
                 lambda: capi.comm_greedy_local(fl.hs, s.nodes, few, MODE_SCV, 0),
                 lambda: capi.comm_greedy_local(fl.hs, s.nodes, few, MODE_SCV, 1),
                 lambda: sharded_greedy([HandleShard(x, dev) for x in fl.hs], Reducer(local=True),
                                        s.nodes, few),
                 lambda: capi.comm_run_local(fl.hs, MODE_DISKIO),
                 lambda: h.shard_phase1(MODE_DISKIO, p(b.maxima), p(b.counts)))
        for k, call in enumerate(calls):
            with raises_state():
                call()
        assert_same(fl.step(), want)
