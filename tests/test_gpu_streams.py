"""The stream contract of include/yoda.h on a BUSY caller stream: yoda_set_stream launches all of a
handle's work on the caller's stream, yoda_run is asynchronous on it, and work queued on the
previous stream is ordered before the new stream's next work by an event wait on the device.
Every other GPU test runs on the handle's own idle stream, where each kernel and copy finishes
microseconds after it is queued and a missing event wait, a staging buffer rewritten too early or
a copy on the wrong stream still gives the right answer.

The method, for every scenario:
  1. the caller's stream is made busy with a timed spin (torch.cuda._sleep, calibrated once per
     module with two events on an idle stream); the spin ends by itself;
  2. the library calls are queued behind it; an event recorded directly after the spin tells
     whether it is still running when a call returns;
  3. the sequence first runs once on the idle stream: that pass sizes every buffer and gives the
     wall time T of the calls; the spin lasts max(SPIN_FLOOR_MS, SPIN_MULT * T), at most
     SPIN_CAP_MS.  The floor covers a host thread that loses its CPU for a few scheduler slices
     on a shared machine, the multiple a sequence whose calls are slower than that;
  4. yoda_run and dist.ShardExchange.step -- the two calls documented as returning without a host
     wait -- must return while the spin runs on the N32 path; for every other call the test
     prints whether it did (the line that starts with "STREAMS|");
  5. one synchronisation, then every comparison is exact: the six outputs byte for byte against a
     second handle that replays the same calls on its own idle stream with synchronize() after
     each, and against the C oracle (or the scenario module's reference) on the state the sequence
     ends in;
  6. where updates were made, yoda_snapshot_check's mismatch words are zero.
Between the warm-up pass and the busy pass the handle is put back to the scenario's start with
another batch uploaded and run (the pods reversed), so what a lost call would leave behind is never
the right answer.  tests/test_stream_cases.py shows without a GPU that each scenario's wrong
outcome differs from the right one.

SPIN_FLOOR_MS = 40, SPIN_MULT = 4, SPIN_CAP_MS = 500; a spin that ran longer than 1 s fails its
test.  T measured on an MI355X (warm-up pass, host wall time of the whole sequence, its downloads
included): a step 0.24 - 0.80 ms; Mode B after Mode A 0.41 - 0.49 ms; the rows after a lazy upload
0.99 ms; back-to-back batches 0.43 - 0.79 ms; a walk's group of steps with its run 0.69 - 1.81 ms;
the burst 1.35 ms; the stream switches 1.55 ms; a shard exchange step with its uploads 0.64 -
2.22 ms; comm_run_local over three handles 0.93 ms; yoda_greedy of 600 pods with the run after it
8.0 - 8.9 ms; the re-upload 0.71 - 2.26 ms; the node-state variant 0.96 ms.  4 T stays below the
floor everywhere, so every spin is 40 ms (measured 39.9 - 40.0 ms; one of 87 ran 61 ms).

Which calls returned while the spin was running, on that machine (printed, not asserted, but for
yoda_run and ShardExchange.step on N32):
  during: upload_pods (the first of a sequence), yoda_run in Mode A, shard_phase1, set_stream,
          set_node_state (1 - 700 nodes), set_node_present of 1 - 128 nodes, update_cards of
          1 - 64 nodes (but for the list that follows a push of the same nodes), update_candidates,
          the dense update_node_metrics, set_candidates(off), an empty list of any call,
          ShardExchange.step on N32 and F64;
  after:  every download, score_rows, diagnose, snapshot_check; a second upload_pods (it waits for
          its staging pages); an update queued right behind another (the burst, a push after a card
          list: the update staging pages); update_alloc; set_node_present and update_cards of 700
          nodes; replace_nodes of any length; set_candidates and set_pod_classes (pageable sources);
          yoda_run in Mode B; upload_nodes; the U64 exchange step (it reads its overflow count);
          comm_run_local (it ends in a synchronisation); yoda_greedy."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import candidate_cases as cc
import card_update_cases as cuc
import diagnosis_cases as dc
import node_present_cases as npc
import node_state_cases as nsc
import oracle
import replace_cases as rc
import stream_cases as cases
from test_gpu_greedy_single import wrap_case  # noqa: F401  (fixture: 600 x 300 of config 5)
from test_gpu_parity import assert_same
from test_gpu_step_kernels import batch_2085
from yoda_amd import capi, dist, synth
from yoda_amd.capi import Yoda, lib
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

SPIN_FLOOR_MS, SPIN_MULT, SPIN_CAP_MS = 40.0, 4.0, 500.0
SPIN_LIMIT_MS = 1000.0  # no spin may last longer, as measured
B_FIELDS = ("status", "pick", "n_feasible", "n_ties", "top_score")
ZERO = [0, 0, 0, 0]
SEED = 0x5EEDFACE
DEVICE = torch.device("cuda", 0)


# ---- the spin -------------------------------------------------------------------------------
class Spin:
    def __init__(self, begin, done, asked_ms):
        self.begin, self.done, self.asked_ms = begin, done, asked_ms

    def running(self):
        return not self.done.query()

    def measured_ms(self):
        self.done.synchronize()
        return self.begin.elapsed_time(self.done)


class Spinner:
    """torch.cuda._sleep(cycles) with the cycles of a millisecond measured once."""

    def __init__(self):
        s = torch.cuda.Stream(DEVICE)
        cycles = 1_000_000
        self._time(s, cycles)  # (loads the kernel)
        for _ in range(6):
            ms = self._time(s, cycles)
            if ms >= 4.0:
                break
            cycles = int(cycles * min(10.0, 8.0 / max(ms, 0.01)))
        assert 4.0 <= ms <= 100.0, f"spin calibration: {cycles} cycles took {ms} ms"
        self.cycles_per_ms = cycles / ms

    @staticmethod
    def _time(s, cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def start(self, stream, t_ms):
        """A spin of max(floor, multiple of t_ms) on `stream`, with the event after it."""
        ms = min(SPIN_CAP_MS, max(SPIN_FLOOR_MS, SPIN_MULT * t_ms))
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            begin.record()
            torch.cuda._sleep(max(1, int(ms * self.cycles_per_ms)))
            done.record()
        return Spin(begin, done, ms)


@pytest.fixture(scope="module")
def spinner():
    return Spinner()


@pytest.fixture(scope="module")
def streams():
    return [torch.cuda.Stream(DEVICE) for _ in range(3)]


@pytest.fixture
def pair():
    """(the handle that goes behind the spin, the handle that replays on its own idle stream)"""
    busy, idle = Yoda(0), Yoda(0)
    busy.follows, idle.follows = True, False
    yield busy, idle
    torch.cuda.synchronize()
    busy.close()
    idle.close()


def on_busy(fn):
    """A call only the busy handle makes (its stream switches): the idle handle stays where it is."""
    return lambda h: fn(h) if h.follows else None


# ---- playing a sequence -----------------------------------------------------------------------
class Watch:
    """The spin the calls of a busy pass are measured against (a sequence may start another)."""

    def __init__(self, spin):
        self.spin = spin
        self.spins = [spin]
        self.table = []

    def again(self, spin):
        self.spin = spin
        self.spins.append(spin)


def play(h, ops, watch=None, sync_each=False):
    """ops: [(name, fn(h))]; returns {name: what fn returned, when not None}."""
    out = {}
    for name, fn in ops:
        r = fn(h)
        if watch is not None:
            watch.table.append((name, watch.spin.running()))
        if r is not None:
            out[name] = r
        if sync_each:
            h.synchronize()
            torch.cuda.synchronize()
    return out


def settle(h):
    h.synchronize()
    torch.cuda.synchronize()


def report(tag, t_ms, watch, must):
    spins = " + ".join(f"{s.asked_ms:.0f} ms (ran {s.measured_ms():.1f} ms)" for s in watch.spins)
    calls = " ".join(f"{n}={'during' if r else 'AFTER'}" for n, r in watch.table)
    print(f"STREAMS| {tag} | T {t_ms:.2f} ms | spin {spins} | {calls}")
    for s in watch.spins:
        assert s.measured_ms() <= SPIN_LIMIT_MS, tag
    late = [n for n, r in watch.table if n in must and not r]
    assert not late, f"{tag}: returned only after the spin had ended: {late}"


def behind_spin(tag, spinner, busy, idle, reset, ops, stream, must=(), ctx=None):
    """The method of the module docstring for one sequence; returns (busy's results, idle's).
    reset: the calls that bring a handle to the scenario's start (run with a synchronisation
    after each); ctx: a dict the sequence's own calls may read (ctx["watch"], ctx["t_ms"])."""
    play(idle, reset, sync_each=True)
    ref = play(idle, ops, sync_each=True)
    play(busy, reset, sync_each=True)
    t0 = time.perf_counter()
    play(busy, ops)
    settle(busy)
    t_ms = (time.perf_counter() - t0) * 1e3
    play(busy, reset, sync_each=True)
    watch = Watch(spinner.start(stream, t_ms))
    if ctx is not None:
        ctx.update(watch=watch, t_ms=t_ms)
    got = play(busy, ops, watch=watch)
    settle(busy)
    report(tag, t_ms, watch, must)
    return got, ref


def same_bytes(got, ref, what, fields=cases.FIELDS):
    for f in fields:
        assert getattr(got, f).tobytes() == getattr(ref, f).tobytes(), f"{what}: {f}"


def same_b(got, want, what):
    for f in B_FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f"{what}: {f}")


def reverse(pods):
    return pods.take(np.arange(pods.n_pods)[::-1])


def decoy(pods, mode=MODE_SCV):
    """Another batch uploaded and run: what is on the device before a pass is never its answer."""
    other = reverse(pods)

    def fn(h):
        h.upload_pods(other)
        h.run(mode)
    return ("decoy batch", fn)


_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def want_scv(key, nodes, pods):
    return memo(("scv", key), lambda: oracle.schedule(nodes, pods, MODE_SCV, threads=8))


def new_bufs(h, n_pods):
    h.bufs = dist.ShardBuffers(n_pods, DEVICE)
    return h.bufs


def clear_bufs(h):
    h.bufs.maxima.zero_()
    h.bufs.counts.zero_()
    torch.cuda.synchronize()


def phase1(h):
    h.shard_phase1(MODE_SCV, h.bufs.maxima.data_ptr(), h.bufs.counts.data_ptr())


def phase1_results(h):
    """(maxima u64 [P, 6], n_feasible u32 [P]) of the handle's exchange buffers, caller order."""
    P = h.bufs.n_pods
    mx = h.bufs.maxima.cpu().numpy().view(np.uint64).reshape(6, P).T
    cnt = h.bufs.counts.cpu().numpy().view(np.uint32).reshape(2, P)[0]
    return mx, cnt


def assert_phase1(h, want, what):
    mx, cnt = phase1_results(h)
    np.testing.assert_array_equal(cnt, want.n_feasible, err_msg=f"{what}: counts")
    np.testing.assert_array_equal(mx, want.maxima, err_msg=f"{what}: maxima")


# ---- 1. a step behind a spin ------------------------------------------------------------------
def step_shape(shape):
    if shape == "2085x1000":
        return batch_2085()
    nodes, pods = synth.make_config(3, pods=300, nodes=130)
    return nodes.normalized(), pods.normalized()


@pytest.mark.parametrize("shape", ["2085x1000", "300x130_unordered"])
@pytest.mark.parametrize("where", ["side", "null", "switched"])
def test_step_behind_a_spin(spinner, streams, pair, where, shape):
    """upload_pods, run, download behind a spin on a torch side stream, on the HIP null stream
    (the spin on torch's default stream) and on a second side stream the handle switches to with
    the spin already on it.  2,085 x 1,000: N32, the counting order, the probe and the pod-block
    order, so the run takes the deferred pod copy on the copy stream; 300 x 130 with
    set_pod_order(False) takes none."""
    busy, idle = pair
    ordered = shape == "2085x1000"
    nodes, pods = memo(("shape", shape), lambda: step_shape(shape))
    want = want_scv(shape, nodes, pods)
    s1, s2, _ = streams
    null = torch.cuda.default_stream(DEVICE)
    assert null.cuda_stream == 0
    start, spin_on = {"side": (s1, s1), "null": (null, null), "switched": (s1, s2)}[where]
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("pod order", lambda h: h.set_pod_order(ordered)),
             ("start stream", on_busy(lambda h: h.set_stream(start.cuda_stream))),
             decoy(pods)]
    ops = [("upload_pods", lambda h: h.upload_pods(pods)),
           ("run", lambda h: h.run(MODE_SCV)),
           ("download", lambda h: h.download())]
    if where == "switched":
        ops.insert(0, ("set_stream", on_busy(lambda h: h.set_stream(s2.cuda_stream))))
    got, ref = behind_spin(f"1 step {where} {shape}", spinner, busy, idle, reset, ops, spin_on,
                           must=("run",))
    assert busy.path == "n32"
    assert busy.order_info()["kind"] == (2 if ordered else 0)
    same_bytes(got["download"], ref["download"], "busy against idle")
    assert_same(got["download"], want)


# ---- 2. the deferred pod arrays reach their readers ---------------------------------------------
def upload_without_mode_b(h, pods):
    """yoda_upload_pods with rio / rcpu NULL: the f64 thresholds and the Mode B weights are packed
    on the host later (the lazy part of the upload)."""
    p = pods.normalized()
    cp = p.c()
    cp.rio, cp.rcpu = None, None
    h._pods = p
    h._check(lib().yoda_upload_pods(h._h, C.byref(cp)), "yoda_upload_pods")
    h.n_pods = p.n_pods


@pytest.mark.parametrize("f64", [False, True], ids=["n32", "f64"])
def test_mode_b_after_mode_a_behind_one_spin(spinner, streams, pair, f64):
    """(a) A batch with rio / rcpu, run(MODE_SCV), run(MODE_DISKIO): the Mode B run reads the
    weights the Mode A run left to the copy stream.  f64: the first run's kernels read the f64
    pod arrays themselves."""
    busy, idle = pair
    nodes, pods = cases.mode_b_batch()
    want = memo("mode b", lambda: oracle.schedule(nodes, pods, MODE_DISKIO, threads=8))
    s1 = streams[0]
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes, force_f64=f64)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods, MODE_DISKIO)]
    ops = [("upload_pods", lambda h: h.upload_pods(pods)),
           ("run", lambda h: h.run(MODE_SCV)),
           ("run mode b", lambda h: h.run(MODE_DISKIO)),
           ("download", lambda h: h.download())]
    got, ref = behind_spin(f"2a mode b {'f64' if f64 else 'n32'}", spinner, busy, idle, reset, ops,
                           s1, must=() if f64 else ("run",))
    assert busy.path == ("f64" if f64 else "n32")
    same_bytes(got["download"], ref["download"], "busy against idle", B_FIELDS)
    same_b(got["download"], want, "Mode B against the oracle")


@pytest.mark.parametrize("switch", [False, True], ids=["same_stream", "switched"])
def test_rows_after_a_lazy_upload(spinner, streams, pair, switch):
    """(b) A batch without Mode B inputs, run(MODE_SCV), then the raw and the normalized score rows
    of a 24-pod slice; (c) with set_stream(other) between the run and the row calls."""
    busy, idle = pair
    nodes, pods = memo(("shape", "2085x1000"), lambda: step_shape("2085x1000"))
    want = want_scv("2085x1000", nodes, pods)
    sub = pods.take(np.arange(176, 200))  # two-node pods, then the generator's own
    s1, s2, _ = streams
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods)]
    ops = [("upload_pods lazy", lambda h: upload_without_mode_b(h, pods)),
           ("run", lambda h: h.run(MODE_SCV)),
           ("download", lambda h: h.download()),
           ("upload_pods lazy 24", lambda h: upload_without_mode_b(h, sub)),
           ("score_rows", lambda h: h.score_rows(MODE_SCV)),
           ("score_rows norm", lambda h: h.score_rows(MODE_SCV, norm=True)),
           ("download 24", lambda h: h.download())]
    if switch:
        ops.insert(2, ("set_stream", on_busy(lambda h: h.set_stream(s2.cuda_stream))))
    got, ref = behind_spin(f"2{'c' if switch else 'b'} rows", spinner, busy, idle, reset, ops, s1,
                           must=("run",))
    same_bytes(got["download"], ref["download"], "busy against idle")
    assert_same(got["download"], want)
    for name in ("score_rows", "score_rows norm"):
        for a, b in zip(got[name], ref[name]):
            np.testing.assert_array_equal(a, b, err_msg=name)
    feas, raw, norm = got["score_rows norm"]
    for p in (0, 9, 23):
        _, f, r, nrm = oracle.pod_detail(nodes, sub, p, MODE_SCV)
        np.testing.assert_array_equal(feas[p], f, err_msg=f"row bits {p}")
        np.testing.assert_array_equal(raw[p][f], r[f], err_msg=f"raw row {p}")
    assert_same(got["download 24"], oracle.schedule(nodes, sub, MODE_SCV, threads=8))


# ---- 3. back-to-back batches of changing size ---------------------------------------------------
@pytest.mark.parametrize("name", cases.SIZE_SEQUENCES)
def test_back_to_back_batches(spinner, streams, pair, name):
    """upload_pods(A), shard_phase1 into torch buffers (caller order), upload_pods(B), run,
    download, all behind one spin: the buffers hold A's maxima and counts, the download B's six
    outputs.  (The second upload waits for the first one's staging pages.)"""
    busy, idle = pair
    nodes, a, b = cases.batch_pair(name)
    want_a, want_b = want_scv((name, "a"), nodes, a), want_scv((name, "b"), nodes, b)
    s1 = streams[0]
    for h in pair:
        new_bufs(h, a.n_pods)
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("caller order", lambda h: h.shard_exchange_order(True)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(b), ("clear", clear_bufs)]
    ops = [("upload_pods A", lambda h: h.upload_pods(a)),
           ("shard_phase1 A", phase1),
           ("upload_pods B", lambda h: h.upload_pods(b)),
           ("run B", lambda h: h.run(MODE_SCV)),
           ("download B", lambda h: h.download())]
    got, ref = behind_spin(f"3 batches {name}", spinner, busy, idle, reset, ops, s1)
    assert_phase1(idle, want_a, "idle handle, A")
    assert_phase1(busy, want_a, "busy handle, A")
    same_bytes(got["download B"], ref["download B"], "busy against idle")
    assert_same(got["download B"], want_b)


# ---- 4. live-snapshot updates queued behind a spin ----------------------------------------------
def apply_step(h, step):
    k = step[0]
    if k == "push":
        h.set_node_state(*step[1:])
    elif k == "update_alloc":
        h.update_alloc(step[1])
    elif k == "cards":
        h.update_cards(*step[1:])
    elif k == "present":
        h.set_node_present(step[1], step[2])
    elif k == "replace":
        h.replace_nodes(step[1], step[2])
    elif k == "metrics":
        h.update_node_metrics(*step[1:])
    elif k == "cand":
        h.set_candidates(step[2], step[1])
    elif k == "update":
        h.update_candidates(step[1], step[2])
    elif k == "classes":
        h.set_pod_classes(step[1])
    else:
        raise ValueError(k)


def groups_of(steps):
    """[(tag, the steps since the check before)]"""
    out, cur = [], []
    for s in steps:
        if s[0] == "check":
            out.append((s[1], cur))
            cur = []
        else:
            cur.append(s)
    return out


def _replace_walk():
    nodes, pods, steps = rc.walk("small")
    rng = np.random.default_rng(41)
    n = nodes.n_nodes
    steps = list(steps) + [("metrics", None, rng.random(n) * 100.0, rng.random(n) * 100.0),
                           ("check", "dense metrics")]
    return nodes, synth.distinct_diskio(pods).normalized(), steps


def _cand_reference(model, pods):
    sample = np.arange(0, pods.n_pods, 4)
    return cc.reference(cc.Snapshot(model, pods), model, sample)[0], sample


# name -> (scenario, model class, reference(model, pods) -> (EvalResult, sample or None))
WALKS = {
    "node_state": (lambda: nsc.walk(pods=700, nodes=900), nsc.Model,
                   lambda m, pods: (oracle.schedule(m.nodes(), pods, MODE_SCV, threads=8), None)),
    "card_update": (lambda: cuc.walk("small"), cuc.Model,
                    lambda m, pods: (oracle.schedule(m.nodes(), pods, MODE_SCV, threads=8), None)),
    "node_present": (lambda: npc.walk("small"), npc.Model,
                     lambda m, pods: (npc.reference(m, pods), None)),
    "replace": (_replace_walk, rc.Model, lambda m, pods: (rc.reference(m, pods), None)),
    "candidates": (lambda: cc.walk("small"), cc.Model, _cand_reference),
    "diagnosis": (lambda: dc.walk("small"), cc.Model, None),
}


def walk_pass(h, nodes, pods, groups, name, spinner=None, stream=None, times=None):
    """Upload, then every group of steps followed by upload_pods, run, download (and Mode B on the
    replace walk, the diagnosis on its walk).  With a spinner: each group behind a spin sized from
    times[k].  Returns ([per check: dict of results], [T per group])."""
    h.upload_nodes(nodes)
    h.set_pod_classes(None)
    if h.follows:
        h.set_stream(stream.cuda_stream)
    decoy(pods)[1](h)
    settle(h)
    results, took = [], []
    for k, (tag, steps) in enumerate(groups):
        ops = [(f"{s[0]}", (lambda st: lambda hh: apply_step(hh, st))(s)) for s in steps]
        ops += [("upload_pods", lambda hh: hh.upload_pods(pods)),
                ("run", lambda hh: hh.run(MODE_SCV)),
                ("download", lambda hh: hh.download())]
        if name == "replace":
            ops += [("run mode b", lambda hh: hh.run(MODE_DISKIO)),
                    ("download b", lambda hh: hh.download())]
        if name == "diagnosis":
            ops += [("diagnose", lambda hh: hh.diagnose())]
        ops += [("snapshot_check", lambda hh: hh.snapshot_check()[1].tolist())]
        watch = None
        if spinner is not None:
            watch = Watch(spinner.start(stream, times[k]))
        t0 = time.perf_counter()
        out = play(h, ops, watch=watch, sync_each=spinner is None and not h.follows)
        settle(h)
        took.append((time.perf_counter() - t0) * 1e3)
        if watch is not None:
            report(f"4 walk {name} / {tag}", times[k], watch, ())
        results.append(out)
    return results, took


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_behind_spins(spinner, streams, pair, name):
    """One walk of each live-update module on a handle that sits on a torch side stream, a spin
    before every group of steps between two checks; each module's own model and reference.  The
    whole walk first runs on the idle stream (buffer sizes, T per group); the snapshot is then
    uploaded again, so the busy pass starts from the state as uploaded."""
    busy, idle = pair
    scenario, model_cls, reference = WALKS[name]
    nodes, pods, steps = memo(("walk", name), scenario)
    groups = groups_of(steps)
    s1 = streams[0]
    refs, _ = walk_pass(idle, nodes, pods, groups, name)
    _, times = walk_pass(busy, nodes, pods, groups, name, stream=s1)
    gots, _ = walk_pass(busy, nodes, pods, groups, name, spinner=spinner, stream=s1, times=times)
    model = model_cls(nodes)
    for (tag, group), got, ref in zip(groups, gots, refs):
        for s in group:
            model.apply(s)
        what = f"{name} / {tag}"
        same_bytes(got["download"], ref["download"], what)
        assert got["snapshot_check"] == ZERO and ref["snapshot_check"] == ZERO, what
        if name == "diagnosis":
            r = dc.Reference(model, pods)
            np.testing.assert_array_equal(got["download"].n_feasible, r.n_feasible, err_msg=what)
            np.testing.assert_array_equal(got["diagnose"], r.counts(), err_msg=what)
            np.testing.assert_array_equal(got["diagnose"], ref["diagnose"], err_msg=what)
            continue
        want, sample = reference(model, pods)
        assert_same(got["download"], want, pods=sample)
        if name == "replace":
            same_bytes(got["download b"], ref["download b"], what + " (Mode B)", B_FIELDS)
            same_b(got["download b"], oracle.schedule(model.nodes(), pods, MODE_DISKIO, threads=8),
                   what + " (Mode B)")


def test_burst_behind_one_spin(spinner, streams, pair):
    """Two set_node_state calls on overlapping lists with different values, an update_cards, a
    set_node_present, a replace_nodes of a node the first three name, then the run, all behind one
    spin: the result is the last writer's."""
    busy, idle = pair
    nodes, pods, steps = cases.burst()
    model = cases.after(nodes, steps)
    want = memo("burst", lambda: rc.reference(model, pods))
    s1 = streams[0]
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods)]
    ops = [(name, (lambda st: lambda h: apply_step(h, st))(s))
           for name, s in zip(cases.BURST_CALLS, steps)]
    ops += [("upload_pods", lambda h: h.upload_pods(pods)),
            ("run", lambda h: h.run(MODE_SCV)),
            ("download", lambda h: h.download()),
            ("snapshot_check", lambda h: h.snapshot_check()[1].tolist())]
    got, ref = behind_spin("4 burst", spinner, busy, idle, reset, ops, s1)
    same_bytes(got["download"], ref["download"], "busy against idle")
    assert_same(got["download"], want)
    assert got["snapshot_check"] == ZERO and ref["snapshot_check"] == ZERO
    assert busy.nodes_absent == 30


# ---- 5. stream switches ---------------------------------------------------------------------------
def test_stream_switches(spinner, streams, pair):
    """upload_pods and set_node_state on a busy stream S1; set_stream(S2), S2 idle: the run sees
    both.  use_own_stream and a second run: the same answer.  Back to S1 with a new spin on it and
    a fresh update: the run sees that.  set_stream of the current stream changes nothing."""
    busy, idle = pair
    nodes, pods, push, moved = cases.state_pair()
    ids = push[1]
    back = ("push", ids, nodes.alloc_memory.copy(), nodes.card_number.copy())
    want_moved = want_scv("state moved", moved, pods)
    want_base = want_scv("state base", nodes, pods)
    s1, s2, _ = streams
    ctx = {}

    def spin_again(h):
        if "watch" in ctx:  # (the busy pass; the warm-up pass has no spin)
            ctx["watch"].again(spinner.start(s1, ctx["t_ms"]))

    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods)]
    ops = [("upload_pods", lambda h: h.upload_pods(pods)),
           ("set_node_state", lambda h: apply_step(h, push)),
           ("set_stream S2", on_busy(lambda h: h.set_stream(s2.cuda_stream))),
           ("set_stream S2 again", on_busy(lambda h: h.set_stream(s2.cuda_stream))),
           ("run", lambda h: h.run(MODE_SCV)),
           ("download", lambda h: h.download()),
           ("use_own_stream", on_busy(lambda h: h.use_own_stream())),
           ("run own", lambda h: h.run(MODE_SCV)),
           ("download own", lambda h: h.download()),
           ("set_stream S1", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
           ("second spin", on_busy(spin_again)),
           ("set_node_state back", lambda h: apply_step(h, back)),
           ("set_stream S1 again", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
           ("run S1", lambda h: h.run(MODE_SCV)),
           ("download S1", lambda h: h.download()),
           ("snapshot_check", lambda h: h.snapshot_check()[1].tolist())]
    got, ref = behind_spin("5 switches", spinner, busy, idle, reset, ops, s1, ctx=ctx)
    for name, want in (("download", want_moved), ("download own", want_moved),
                       ("download S1", want_base)):
        same_bytes(got[name], ref[name], name)
        assert_same(got[name], want)
    assert got["snapshot_check"] == ZERO
    assert lib().yoda_set_stream(None, None) == -1       # YODA_ERR_INVALID_ARG
    assert lib().yoda_use_own_stream(None) == -1


# ---- 6. several handles -----------------------------------------------------------------------
def shard_fleet(nodes, world, **kw):
    n = nodes.n_nodes
    b = [0] + [int(c * n) for c in npc.SHARD_CUTS[world]] + [n]
    hs, shards = [], []
    for r in range(world):
        h = Yoda(0)
        shards.append(nodes.slice(b[r], b[r + 1]))
        h.upload_nodes(shards[-1], node_offset=b[r], **kw)
        hs.append(h)
    return b, hs, shards


EXCHANGE = {
    "n32_packed": ({}, False),
    "n32_draw_candidates": ({}, True),
    "f64": ({"force_f64": True}, False),
    "u64": ({"force_generic": True}, False),
}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("variant", list(EXCHANGE))
def test_shard_exchange_behind_a_spin(spinner, streams, variant, world):
    """(a) dist.ShardExchange.local inside `with torch.cuda.stream(S)`, S busy: the pod uploads and
    one step with no synchronisation inside, then every shard's download equals one handle's that
    holds the whole snapshot.  The U64 step reads its overflow count back: recorded only."""
    kw, extras = EXCHANGE[variant]
    nodes, pods = memo("small", lambda: tuple(x.normalized()
                                              for x in synth.make_config(3, pods=700, nodes=900)))
    s1 = streams[0]
    words, cls = memo("recipe", lambda: cc.recipe(nodes, pods))
    with Yoda(0) as whole:
        whole.upload_nodes(nodes, **kw)
        if extras:
            whole.set_candidates(words, 8)
            whole.set_pod_classes(cls)
            whole.set_tie_draw(SEED, 0)
        want = whole.eval(pods, MODE_SCV)
    if not extras:
        assert_same(want, want_scv("small", nodes, pods))
    b, hs, shards = shard_fleet(nodes, world, **kw)
    try:
        for h in hs:
            h.upload_pods(reverse(pods))
        with torch.cuda.stream(s1):
            ex = dist.ShardExchange.local(
                hs, DEVICE, shards, b[:-1], tie_draw=(SEED, 0) if extras else None,
                candidates=(8, [words[b[r]:b[r + 1]] for r in range(world)], cls)
                if extras else None)
            if variant == "n32_packed":
                assert ex.ib is not None and ex.narrow
            assert hs[0].path == {"f64": "f64", "u64": "u64"}.get(variant, "n32")

            def one(watch=None):
                ops = [(f"upload_pods {r}", (lambda h: lambda _: h.upload_pods(pods))(h))
                       for r, h in enumerate(hs)]
                ops += [("step", lambda _: ex.step(MODE_SCV))]
                play(None, ops, watch=watch)

            ex.step(MODE_SCV)  # (the decoy batch's step)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one()
            torch.cuda.synchronize()
            t_ms = (time.perf_counter() - t0) * 1e3
            for h in hs:
                h.upload_pods(reverse(pods))
            ex.step(MODE_SCV)
            torch.cuda.synchronize()
            watch = Watch(spinner.start(s1, t_ms))
            one(watch)
            torch.cuda.synchronize()
        report(f"6a exchange {variant} world {world}", t_ms, watch,
               ("step",) if variant.startswith("n32") else ())
        res = [h.download() for h in hs]
        for r in res:
            same_bytes(r, res[0], f"{variant} world {world}: shard against shard")
            assert_same(r, want)
    finally:
        torch.cuda.synchronize()
        for h in hs:
            h.close()


def test_comm_run_local_over_three_streams(spinner, streams):
    """(b) Three shard handles on three streams (two torch side streams, one handle's own); the two
    side streams are busy when the pods are uploaded and a node-state push is queued on every
    handle; yoda_comm_run_local folds them onto one stream and back.  The result is one handle's;
    afterwards each handle runs correctly alone on the stream it was on."""
    nodes, pods, push, moved = cases.state_pair()
    want = want_scv("state moved", moved, pods)
    b, hs, _ = shard_fleet(nodes, 3)
    s1, s2, _ = streams
    try:
        hs[0].set_stream(s1.cuda_stream)
        hs[1].set_stream(s2.cuda_stream)

        def one(watch=None):
            ops = []
            for r, h in enumerate(hs):
                ops += [(f"upload_pods {r}", (lambda h: lambda _: h.upload_pods(pods))(h)),
                        (f"set_node_state {r}", (lambda h: lambda _: apply_step(h, push))(h))]
            ops += [("comm_run_local", lambda _: capi.comm_run_local(hs, MODE_SCV))]
            play(None, ops, watch=watch)

        def start():
            for h, shard_lo, shard_hi in zip(hs, b[:-1], b[1:]):
                h.upload_nodes(nodes.slice(shard_lo, shard_hi), node_offset=shard_lo)
                h.upload_pods(reverse(pods))
                h.run(MODE_SCV)
            torch.cuda.synchronize()
            for h in hs:
                h.synchronize()

        start()
        t0 = time.perf_counter()
        one()
        for h in hs:
            h.synchronize()
        t_ms = (time.perf_counter() - t0) * 1e3
        start()
        watch = Watch(spinner.start(s1, t_ms))
        watch.spins.append(spinner.start(s2, t_ms))
        one(watch)
        for h in hs:
            h.synchronize()
        report("6b comm_run_local", t_ms, watch, ())
        res = [h.download() for h in hs]
        for r in res:
            same_bytes(r, res[0], "comm_run_local: shard against shard")
            assert_same(r, want)
        for r, h in enumerate(hs):  # alone, on its saved stream (a spin on the torch ones)
            lo, hi = b[r], b[r + 1]
            alone = oracle.schedule(moved.slice(lo, hi), pods, MODE_SCV, threads=8)
            alone.pick = np.where(alone.pick >= 0, alone.pick + lo, alone.pick).astype(np.int32)
            w = Watch(spinner.start((s1, s2)[r], 0.0)) if r < 2 else None
            out = play(h, [("upload_pods", lambda hh: hh.upload_pods(pods)),
                           ("run", lambda hh: hh.run(MODE_SCV)),
                           ("download", lambda hh: hh.download())], watch=w)
            if w is not None:
                report(f"6b alone {r}", 0.0, w, ("run",))
            assert_same(out["download"], alone)
    finally:
        torch.cuda.synchronize()
        for h in hs:
            h.close()


@pytest.mark.parametrize("flags", [0, 1])
def test_greedy_behind_a_spin(spinner, streams, pair, wrap_case, flags):
    """(c) yoda_greedy on a busy side stream: its pushes go through the mapped staging pages its
    kernels read from host memory, and its host polls coherent memory.  The picks are the
    sequential oracle's and the snapshot is as uploaded afterwards."""
    busy, idle = pair
    nodes, pods, want, sub, sub_want = wrap_case
    s1 = streams[0]
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(sub)]
    ops = [("greedy", lambda h: h.greedy(pods, MODE_SCV, flags)),
           ("eval after", lambda h: h.eval(sub, MODE_SCV)),
           ("snapshot_check", lambda h: h.snapshot_check()[1].tolist())]
    got, ref = behind_spin(f"6c greedy flags {flags}", spinner, busy, idle, reset, ops, s1)
    np.testing.assert_array_equal(got["greedy"], want[flags])
    np.testing.assert_array_equal(ref["greedy"], want[flags])
    same_bytes(got["eval after"], ref["eval after"], "after greedy")
    assert_same(got["eval after"], sub_want)
    assert got["snapshot_check"] == ZERO


# ---- 7. a re-upload with a step in flight -------------------------------------------------------
@pytest.mark.parametrize("shape", list(cases.RANK_SHAPES))
def test_reupload_with_a_step_in_flight(spinner, streams, pair, shape):
    """A memory-ranks snapshot; behind a spin: upload_pods, shard_phase1 into a torch buffer, then
    upload_nodes of a second memory-ranks snapshot with as many distinct memory values, every one
    another, then upload_pods, run, download.  The buffer holds the FIRST snapshot's maxima and
    counts -- the queued phase 1 must not read the second's value table -- the download the
    second's.  1,300 nodes: the re-upload's first copy (260 KB of records from pageable memory) is
    one the runtime waits for the stream with; 64 nodes: every copy of the re-upload is a few KB,
    taken without a wait, so the value table's own copy decides."""
    busy, idle = pair
    first, second, pods = cases.ranks_pair(shape)
    want_1 = want_scv(("ranks 1", shape), first, pods)
    want_2 = want_scv(("ranks 2", shape), second, pods)
    s1 = streams[0]
    for h in pair:
        new_bufs(h, pods.n_pods)
    reset = [("upload_nodes", lambda h: h.upload_nodes(first, mem_ranks=True)),
             ("caller order", lambda h: h.shard_exchange_order(True)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods), ("clear", clear_bufs)]
    ops = [("upload_pods", lambda h: h.upload_pods(pods)),
           ("shard_phase1", phase1),
           ("upload_nodes second", lambda h: h.upload_nodes(second, mem_ranks=True)),
           ("upload_pods again", lambda h: h.upload_pods(pods)),
           ("run", lambda h: h.run(MODE_SCV)),
           ("download", lambda h: h.download())]
    got, ref = behind_spin(f"7 re-upload, ranks, {shape} nodes", spinner, busy, idle, reset, ops, s1)
    assert busy.memory_ranks and busy.path == "n32"
    assert_phase1(idle, want_1, "idle handle, first snapshot")
    assert_phase1(busy, want_1, "busy handle, first snapshot")
    same_bytes(got["download"], ref["download"], "busy against idle")
    assert_same(got["download"], want_2)


def test_node_state_with_a_step_in_flight(spinner, streams, pair):
    """The same with set_node_state in place of the re-upload, on a snapshot without ranks."""
    busy, idle = pair
    nodes, pods, push, moved = cases.state_pair()
    want_1, want_2 = want_scv("state base", nodes, pods), want_scv("state moved", moved, pods)
    s1 = streams[0]
    for h in pair:
        new_bufs(h, pods.n_pods)
    reset = [("upload_nodes", lambda h: h.upload_nodes(nodes)),
             ("caller order", lambda h: h.shard_exchange_order(True)),
             ("start stream", on_busy(lambda h: h.set_stream(s1.cuda_stream))),
             decoy(pods), ("clear", clear_bufs)]
    ops = [("upload_pods", lambda h: h.upload_pods(pods)),
           ("shard_phase1", phase1),
           ("set_node_state", lambda h: apply_step(h, push)),
           ("upload_pods again", lambda h: h.upload_pods(pods)),
           ("run", lambda h: h.run(MODE_SCV)),
           ("download", lambda h: h.download()),
           ("snapshot_check", lambda h: h.snapshot_check()[1].tolist())]
    got, ref = behind_spin("7 node state", spinner, busy, idle, reset, ops, s1)
    assert not busy.memory_ranks
    assert_phase1(idle, want_1, "idle handle, the state as uploaded")
    assert_phase1(busy, want_1, "busy handle, the state as uploaded")
    same_bytes(got["download"], ref["download"], "busy against idle")
    assert_same(got["download"], want_2)
    assert got["snapshot_check"] == ZERO
