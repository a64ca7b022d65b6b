"""The Filter-diagnosis scenarios of tests/diagnosis_cases.py without a GPU: the reference is right
where it can be checked against an independent statement (oracle/pyoracle.py's three predicates
node by node, the C oracle's feasibility narrowed by the candidates), its counts add up, every
scenario exercises what it is there for, and the plugin turns a reason row into messages."""
import numpy as np
import pytest

import diagnosis_cases as cases
import oracle
import pyoracle
from yoda_amd import plugin as plug
from yoda_amd import synth
from yoda_amd.pack import pods_to_dicts
from yoda_amd.soa import (REASON_ABSENT, REASON_CLOCK, REASON_MEMORY, REASON_NONE,
                          REASON_NOT_CANDIDATE, REASON_NUMBER)

ORACLE_PODS = 120  # pods per check that go through oracle.pod_detail (unschedulable ones first)


def _named():
    out = {f"walk {s}": (lambda s=s: cases.walk(s)) for s in cases.WALK_SHAPES}
    for name in cases.scenarios():
        out[name] = (lambda name=name: cases.scenarios()[name])
    return out


NAMED = _named()


@pytest.fixture(scope="module")
def refs():
    out = {}

    def get(name):
        if name not in out:
            nd, pd, steps = NAMED[name]()
            out[name] = (nd, pd, cases.references(nd, pd, steps))
        return out[name]
    return get


def test_reference_equals_pyoracle_node_by_node():
    """A tiny fleet with CardNumber pushed down, absent nodes and classes: the first predicate of
    pod_fits_number / _memory / _clock that fails, in the call order of collection.go:41-44."""
    nd, pd, steps = cases.tiny_fleet(65)
    steps = list(steps) + [cases.npc._present(np.array([3, 40, 64]), 0), ("check", "absent")]
    seen = set()
    for tag, ref, m in cases.references(nd, pd, steps):
        scvs, plist = oracle.to_py(m.nodes(), pd)
        for p, pod in enumerate(plist):
            cand, row = m.candidates(p), ref.codes(p)
            for i, s in enumerate(scvs):
                ok_n, number = pyoracle.pod_fits_number(pod, s)
                if not m.present[i]:
                    want = REASON_ABSENT
                elif not cand[i]:
                    want = REASON_NOT_CANDIDATE
                elif not ok_n:
                    want = REASON_NUMBER
                elif not pyoracle.pod_fits_memory(number, pod, s)[0]:
                    want = REASON_MEMORY
                elif not pyoracle.pod_fits_clock(number, pod, s)[0]:
                    want = REASON_CLOCK
                else:
                    want = REASON_NONE
                assert row[i] == want, (tag, p, i)
                seen.add(want)
    assert seen == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_code_zero_is_the_c_oracle_feasibility(refs, name):
    """Code 0 <=> oracle.pod_detail's feasibility on the present nodes, narrowed by the class bit
    (diagnosis_cases.oracle_feasible).  A SAMPLE of every check of every scenario, for run time:
    up to ORACLE_PODS pods, the first 60 without a feasible node and an even spread of the rest
    (every pod where the batch is smaller).  The reference evaluates a pod through its (labels,
    class) alone, so a sampled pod stands for every pod of the check with the same ones."""
    nd, pd, checks = refs(name)
    for tag, ref, m in checks:
        sel = np.flatnonzero(ref.selected())
        rest = np.flatnonzero(~ref.selected())
        some = np.concatenate([sel[:ORACLE_PODS // 2],
                               rest[:: max(1, rest.size // (ORACLE_PODS // 2))]])[:ORACLE_PODS]
        for p, bits in cases.oracle_feasible(m, pd, some).items():
            np.testing.assert_array_equal(ref.codes(p) == 0, bits, err_msg=f"{name} {tag} pod {p}")


@pytest.mark.parametrize("name", sorted(NAMED))
def test_counts_add_up(refs, name):
    """counts.sum() + n_feasible == n_nodes - n_absent for every pod, and the default selection
    is the pods without a feasible node."""
    nd, pd, checks = refs(name)
    for tag, ref, m in checks:
        total = ref.all_counts.sum(axis=1, dtype=np.int64) + ref.n_feasible
        assert (total == nd.n_nodes - m.absent().size).all(), (name, tag)
        got = ref.counts()
        assert (got[~ref.selected()] == cases.UNSELECTED).all()
        np.testing.assert_array_equal(got[ref.selected()], ref.all_counts[ref.selected()])
        if not m.n_classes:
            assert (ref.all_counts[:, 0] == 0).all(), (name, tag)
        elif m.cls is not None:
            assert (ref.all_counts[m.cls == cases.ANY, 0] == 0).all(), (name, tag)


@pytest.mark.parametrize("shape", cases.WALK_SHAPES)
def test_walks_are_not_vacuous(refs, shape):
    """At some check at least 10 unschedulable pods; over the checks each of the four counted
    reasons non-zero for some SELECTED pod; some selected pod with two different reasons."""
    _, _, checks = refs(f"walk {shape}")
    assert [t for t, _, _ in checks] == list(cases.WALK)
    assert max(int(ref.selected().sum()) for _, ref, _ in checks) >= 10
    seen, two = np.zeros(4, bool), False
    for _, ref, _ in checks:
        c = ref.all_counts[ref.selected()]
        seen |= (c > 0).any(axis=0)
        two |= bool(((c > 0).sum(axis=1) >= 2).any())
    assert seen.all(), seen
    assert two


def test_scenarios_hold_what_they_are_for(refs):
    """The shapes the kernel can go wrong at are really there."""
    # fleets of 1, 63, 64, 65 and 193 nodes; batches of 1, 64, 65 and 130 pods; K of 1 .. 16
    assert [refs(f"fleet {n}")[0].n_nodes for n in cases.TINY_FLEETS] == list(cases.TINY_FLEETS)
    assert [refs(f"batch {p}")[1].n_pods for p in cases.BATCHES] == list(cases.BATCHES)
    assert [refs(f"cards {k}")[0].max_cards for k in cases.MAX_CARDS] == list(cases.MAX_CARDS)
    nd16 = refs("cards 16")[0]
    assert (nd16.card_count == 0).any() and (nd16.card_number != nd16.card_count).any()
    # the sorted batch is above 128 pods and has unschedulable pods in the middle of the order
    nd, pd, checks = refs("ordered batch")
    assert pd.n_pods > 128 and all(ref.selected().sum() >= 10 for _, ref, _ in checks[1:])
    # a selection that ends in a partly filled wave, at the sizes the issue measured (31 of 130)
    n_sel = [int(ref.selected().sum()) for _, ref, _ in refs("fleet 193")[2]]
    assert any(0 < n % 64 for n in n_sel), n_sel
    assert n_sel[0] >= 10
    # a selection of zero pods
    (_, ref, _), = refs("none selected")[2]
    assert ref.selected().sum() == 0 and refs("none selected")[1].n_pods == 100
    # scv/number "0", absent and a wrapped negative
    nd, pd, checks = refs("number labels")
    assert pd.has_number[:3].tolist() == [1, 0, 1] and pd.number[0] == 0 and pd.number[2] > 2 ** 63
    _, ref, m = checks[1]  # (CardNumber pushed down: some nodes hold 0 cards)
    assert (m.card_number == 0).any()
    assert (ref.codes(0) != REASON_NUMBER).all()            # 0 <= every CardNumber
    assert ((ref.codes(1) == REASON_NUMBER) == (m.card_number == 0)).all()
    assert (ref.codes(2) == REASON_NUMBER).all()
    # long chunks: with every pod selected the sweep takes two-block chunks, the last mid-block
    nd, pd, checks = refs("long chunks")
    waves = (pd.n_pods + 63) // 64
    blocks = (nd.n_nodes + 63) // 64
    want = max(1, min(blocks, 32768 // waves))
    per = (blocks + want - 1) // want
    assert per == 2 and (blocks + per - 1) // per >= 2 and nd.n_nodes % (64 * per) % 64 != 0
    assert all(0 < ref.selected().sum() for _, ref, _ in checks)


class _Rows:
    """A row backend that knows no reasons: today's sentence."""

    def __init__(self, ref):
        self.ref = ref

    def upload_pods(self, pods):
        self.pods = pods

    def score_rows(self, mode):
        codes = self.ref.codes(self.p)[None, :]
        return codes == 0, np.where(codes == 0, 7, -1).astype(np.int64)


class _ReasonRows(_Rows):
    def reason_rows(self):
        return self.ref.codes(self.p)[None, :]


def test_plugin_messages_follow_the_reason_row():
    """YodaPlugin.filter names the predicate when the backend has reason_rows (three distinct
    sentences for number / memory / clock, one for a node rejected elsewhere or absent) and keeps
    the single sentence when it has not."""
    nd, pd, steps = cases.tiny_fleet(193)
    steps = list(steps) + [cases.npc._present(np.arange(0, 193, 7), 0), ("check", "absent")]
    _, ref, _ = cases.references(nd, pd, steps)[-1]
    names = [f"node-{i}" for i in range(nd.n_nodes)]
    dicts = pods_to_dicts(pd)
    msgs = plug.REASON_MESSAGES
    assert len({msgs[REASON_NUMBER], msgs[REASON_MEMORY], msgs[REASON_CLOCK],
                msgs[REASON_NOT_CANDIDATE]}) == 4
    assert msgs[REASON_NOT_CANDIDATE] == msgs[REASON_ABSENT]
    assert plug.FILTER_MESSAGE not in msgs.values()
    seen = set()
    for p in np.flatnonzero(ref.selected()).tolist():
        for backend, told in ((_ReasonRows(ref), True), (_Rows(ref), False)):
            backend.p = p
            pl = plug.YodaPlugin(backend, names, nd)
            state = plug.CycleState()
            assert pl.pre_filter(state, dicts[p]).is_success()
            for i, code in enumerate(ref.codes(p).tolist()):
                st = pl.filter(state, dicts[p], names[i])
                assert st.code == plug.UNSCHEDULABLE and code != 0
                assert st.message == (msgs[code] if told else plug.FILTER_MESSAGE), (p, i, code)
                seen.add(code)
    assert seen == {1, 2, 3, 4, 5}
    # pods WITH a feasible node (another plugin may still reject it, and kube-scheduler then
    # reads every status): the nodes Yoda rejects are named all the same
    seen = set()
    for p in np.flatnonzero(~ref.selected())[:20].tolist():
        for backend, told in ((_ReasonRows(ref), True), (_Rows(ref), False)):
            backend.p = p
            pl = plug.YodaPlugin(backend, names, nd)
            state = plug.CycleState()
            assert pl.pre_filter(state, dicts[p]).is_success()
            codes = ref.codes(p)
            assert (codes == 0).any() and (codes != 0).any(), p
            for i, code in enumerate(codes.tolist()):
                st = pl.filter(state, dicts[p], names[i])
                assert st.is_success() == (code == 0), (p, i)
                if code:
                    assert st.message == (msgs[code] if told else plug.FILTER_MESSAGE), (p, i, code)
                    seen.add(code)
    assert {REASON_MEMORY, REASON_CLOCK, REASON_ABSENT} <= seen, seen
    # Mode B has no Filter of its own: the reason row is not asked for
    backend = _ReasonRows(ref)
    backend.p = p
    backend.reason_rows = None  # (a call would raise)
    pl = plug.YodaPlugin(backend, names, nd, mode=1)
    assert pl.pre_filter(plug.CycleState(), dicts[p]).is_success()


def test_reason_constants_match_the_header():
    import re
    from yoda_amd import capi, soa
    text = open(capi.HEADER_PATH).read()
    for name in ("NONE", "NUMBER", "MEMORY", "CLOCK", "NOT_CANDIDATE", "ABSENT"):
        m = re.search(r"#define YODA_REASON_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(soa, "REASON_" + name)
    assert int(re.search(r"#define YODA_DIAG_ALL (\d+)u", text).group(1)) == soa.DIAG_ALL
