"""The node-presence scenarios of tests/node_present_cases.py can fail: with the oracle alone, every
state with an absent node differs from the full snapshot's in the picks or the feasible counts of
a large share of the pods, so a handle that ignored yoda_set_node_present, kept an absent node in
a maximum, or lost a returned one cannot pass tests/test_gpu_node_present.py.  These are
conditions on the inputs, not on libyoda -- except the three tests at the end: the entry point's
binding, pack_node's presence bits (a host program, as tests/test_node_pack.py) and NodeSoA.take."""
import os
import subprocess

import numpy as np
import pytest

import node_present_cases as cases
import oracle
import pyoracle as po
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, PICK_ERROR, STATUS_DIV_ZERO, STATUS_OK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _full(model, pods):
    return oracle.schedule(model.nodes(), pods, MODE_SCV, threads=8)


def _moved(a, b):
    """Share of the pods whose pick or feasible count differs."""
    return float(((a.pick != b.pick) | (a.n_feasible != b.n_feasible)).mean())


def _pick_share(a, b):
    feas = (a.status == 0) | (b.status == 0)
    assert feas.sum() > 100
    return float((a.pick != b.pick)[feas].mean())


def test_model_applies_presence_steps():
    nodes, _ = cases.shape_workload("small")
    n = nodes.n_nodes
    m = cases.Model(nodes)
    m.apply(("present", np.array([3, n, 5, 3, 0xFFFFFFFF, 7, 7], np.uint32),
             np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)))
    assert m.absent().tolist() == [5, 7]  # 3: the last entry returns it; 7: the last takes it out
    assert m.keep().size == n - 2 and m.compact().n_nodes == n - 2
    # an update of an absent node is applied and leaves it absent
    k = nodes.max_cards
    free = np.full((1, k), 11, np.uint64)
    m.apply(("cards", np.array([5], np.uint32), free, np.ones((1, k), np.uint8),
             np.array([11 * k], np.uint64)))
    m.apply(("push", np.array([5], np.uint32), np.array([1], np.uint64), np.array([2], np.uint64)))
    assert m.absent().tolist() == [5, 7]
    m.apply(("present", np.array([5], np.uint32), np.array([1], np.uint8)))
    got = m.compact()
    at = int(np.searchsorted(m.keep(), 5))
    assert got.free_memory_sum[at] == 11 * k and got.card_number[at] == 2 and got.alloc_memory[at] == 1
    np.testing.assert_array_equal(cases.remap(np.array([-1, 0, at, -2], np.int32), m.keep()),
                                  [-1, 0, 5, -2])


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_walk_moves_picks(shape):
    nodes, pods, steps = cases.walk(shape, mixed_pods=3000)
    n = nodes.n_nodes
    lists = [s for s in steps if s[0] == "present"]
    assert lists[cases.WALK_EMPTY][1].size == 0
    out = lists[cases.WALK_OUTSIDE][1]
    assert (out >= n).sum() == 4
    ids, cnt = np.unique(out[out < n], return_counts=True)
    assert (cnt == 2).all() and ids.size >= 60  # every real id twice, with conflicting flags
    states = cases.states(nodes, steps)
    assert [t for t, _ in states] == list(cases.WALK)
    sizes = [m.absent().size for _, m in states]
    assert sizes[0] == 1 and sizes[1] == 65 and sizes[cases.WALK_NONE] == n and sizes[-1] == 0
    assert sizes[3] - sizes[2] == min(700, n - sizes[2] - 100)
    two = np.setdiff1d(states[2][1].absent(), states[1][1].absent())
    blocks = np.unique(states[2][1].absent() // 64, return_counts=True)
    assert two.size > 64 and (blocks[1] == 64).sum() == 2   # two whole 64-aligned blocks
    assert sizes[cases.WALK_OUTSIDE] == sizes[cases.WALK_EMPTY] + 20   # only the last entries count
    assert sizes[cases.WALK_UPDATES] == sizes[cases.WALK_UPDATES - 1]  # updates leave presence
    # the update named absent nodes, and their new values differ from the uploaded ones
    upd = [s for s in steps if s[0] == "cards"][0][1]
    named = np.intersect1d(upd, states[cases.WALK_UPDATES][1].absent())
    assert named.size >= 20
    after = states[cases.WALK_UPDATES][1].nodes()
    assert (after.free_memory_sum[named] != nodes.free_memory_sum[named]).any()
    best = 0.0
    prev = None
    for k, (tag, m) in enumerate(states):
        ref, full = cases.reference(m, pods), _full(m, pods)
        assert (ref.pick < n).all()
        if m.absent().size:
            assert not np.isin(ref.pick[ref.pick >= 0], m.absent()).any(), tag
            share, picks = _moved(ref, full), _pick_share(ref, full)
            print(shape, tag, "absent", m.absent().size, "moved", round(share, 3), "picks",
                  round(picks, 3))
            assert share >= 0.10, tag
            best = max(best, picks)
        else:
            np.testing.assert_array_equal(ref.pick, full.pick)
        if k == cases.WALK_EMPTY:
            np.testing.assert_array_equal(ref.pick, prev.pick)
        prev = ref
    assert best >= 0.25
    none = cases.reference(states[cases.WALK_NONE][1], pods)
    assert (none.n_feasible == 0).all() and (none.pick == -1).all() and (none.maxima == 1).all()


def test_pyoracle_agrees_on_the_compacted_snapshot():
    nodes, pods, steps = cases.walk("small")
    tag, m = cases.states(nodes, steps)[2]
    sample = pods.slice(0, 12)
    want = cases.reference(m, sample)
    scvs, plist = oracle.to_py(m.compact(), sample)
    keep = m.keep()
    for p, pod in enumerate(plist):
        r = po.schedule_one(pod, scvs, MODE_SCV)
        assert r.status == want.status[p] and r.n_feasible == want.n_feasible[p], (tag, p)
        assert (keep[r.pick] if r.pick >= 0 else r.pick) == want.pick[p], (tag, p)
        assert r.maxima == want.maxima[p].tolist(), (tag, p)


def test_single_survivor_is_picked_without_scoring():
    nodes, pods, steps, s, p = cases.single_survivor()
    assert nodes.total_memory_sum[s] == 0
    (_, a), (_, b), (_, c) = cases.states(nodes, steps)
    up, one, back = (cases.reference(m, pods) for m in (a, b, c))
    assert up.status[p] == STATUS_DIV_ZERO and up.pick[p] == PICK_ERROR
    assert one.status[p] == STATUS_OK and one.pick[p] == s and one.n_feasible[p] == 1
    single = one.n_feasible == 1
    flipped = (up.status == STATUS_DIV_ZERO) & single
    print("pods with one feasible node", int(single.sum()), "of them DIV_ZERO before",
          int(flipped.sum()))
    assert 2 <= single.sum() and flipped.sum() >= 2
    assert (one.pick[flipped] == s).all() and (one.status[flipped] == STATUS_OK).all()
    # the pods that still pass the survivor and another node keep DIV_ZERO
    assert ((one.status == STATUS_DIV_ZERO) & (one.n_feasible >= 2)).any()
    np.testing.assert_array_equal(back.pick, up.pick)


def test_max_holders_move_the_maxima():
    nodes, pods, steps = cases.max_holders()
    (_, a), (_, b), (_, c) = cases.states(nodes, steps)
    up, gone, back = (cases.reference(m, pods) for m in (a, b, c))
    assert 0 < b.absent().size < nodes.n_nodes
    left = b.compact()
    assert left.card_bandwidth.max() < nodes.card_bandwidth.max()  # the G maxima move too
    share = float((gone.maxima != up.maxima).any(axis=1).mean())
    print("maxima moved for", round(share, 3), "of the pods; picks", round(_pick_share(gone, up), 3))
    assert share >= 0.25 and _moved(gone, up) >= 0.10
    np.testing.assert_array_equal(back.maxima, up.maxima)
    np.testing.assert_array_equal(back.pick, up.pick)


def test_shard_absent_covers_whole_shards():
    nodes, pods, steps = cases.shard_absent()
    n = nodes.n_nodes
    (_, a), (_, b), (_, c) = cases.states(nodes, steps)
    lo, hi = (int(x * n) for x in cases.SHARD_CUTS[3])
    assert a.absent().tolist() == list(range(lo, hi))
    assert b.absent().tolist() == list(range(0, int(cases.SHARD_CUTS[2][0] * n)))
    assert c.absent().size == 0
    for m in (a, b):
        assert _moved(cases.reference(m, pods), _full(m, pods)) >= 0.10


def test_binding_declares_the_entry_points():
    """libyoda exports yoda_set_node_present / yoda_nodes_absent and yoda_amd.capi binds them
    (capi.lib() resolves every declared entry point when it loads the library)."""
    from yoda_amd import capi
    lib = capi.lib()
    assert lib.yoda_set_node_present.argtypes is not None and len(lib.yoda_set_node_present.argtypes) == 4
    assert lib.yoda_nodes_absent.restype is not None
    assert callable(capi.Yoda.set_node_present) and isinstance(capi.Yoda.nodes_absent, property)
    with open(os.path.join(REPO, "include", "yoda.h")) as f:
        header = f.read()
    assert "int yoda_set_node_present(yoda_t* h, uint32_t count, const uint32_t* nodes," in header
    assert "int yoda_nodes_absent(const yoda_t* h, uint32_t* n_absent);" in header
    assert "#define YODA_ABI_VERSION 1" in header


def test_pack_node_presence_bits(tmp_path):
    """tools/check_node_absent.cpp, built with AddressSanitizer and UBSan as an ordinary
    executable: absent and present packs differ in kNodeAbsent / kSumAbsent alone."""
    exe = str(tmp_path / "check_node_absent")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_node_absent.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_node_absent ok" in out.stdout, out.stdout


def test_node_soa_take():
    nodes = synth.make_nodes(300, 9, cards=4)
    idx = np.array([299, 0, 17, 17, 128])
    got = nodes.take(idx)
    assert got.n_nodes == 5 and got.max_cards == nodes.max_cards
    for f in nodes.__dataclass_fields__:
        a = getattr(got, f)
        np.testing.assert_array_equal(a, getattr(nodes, f)[idx], err_msg=f)
        assert a.flags["C_CONTIGUOUS"] and a.dtype == getattr(nodes, f).dtype
    mask = np.zeros(300, bool)
    mask[[4, 250]] = True
    np.testing.assert_array_equal(nodes.take(mask).card_free_memory, nodes.card_free_memory[[4, 250]])
    assert nodes.take(np.zeros(0, np.int64)).n_nodes == 0
    got.card_number[0] = 12345  # a copy: the source is untouched
    assert nodes.card_number[299] != 12345
    # the oracle takes the compacted snapshot as it is, and the survivors' results are those of
    # the same nodes in the full one where no pick depends on the others
    pods = synth.make_pods(40, 3)
    keep = np.setdiff1d(np.arange(300), [7, 8, 9])
    a = oracle.schedule(nodes.take(keep), pods, MODE_SCV, threads=2)
    b = oracle.schedule(nodes, pods, MODE_SCV, threads=2)
    assert (a.n_feasible <= b.n_feasible).all()
