"""yoda_amd.soa.card_delta: the list a plugin hands to Yoda.update_cards between two snapshots,
or None when only a re-upload will do."""
import os
import re

import numpy as np

import card_update_cases as cases
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import card_delta

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fleet(n=40):
    return synth.make_config(4, pods=1, nodes=n)[0].normalized()


def _copy(nd):
    return synth._copy(nd)  # (NodeSoA.slice returns views)


def _node_with_cards(nd, k=2):
    return int(np.flatnonzero(nd.card_count >= k)[0])


def test_no_change_is_an_empty_list():
    nd = _fleet()
    ids, free, healthy, fsum = card_delta(nd, _copy(nd))
    assert ids.size == 0 and ids.dtype == np.uint32
    assert free.shape == (0, nd.max_cards) and healthy.shape == (0, nd.max_cards)
    assert fsum.size == 0


def test_free_health_and_sum_each_list_their_node():
    nd = _fleet()
    a, j, c = _node_with_cards(nd), _node_with_cards(nd, 1), 7
    new = _copy(nd)
    new.card_free_memory[a, 0] += 5            # free only
    new2 = _copy(nd)
    new2.card_healthy[j, 0] ^= 1               # health only
    new3 = _copy(nd)
    new3.free_memory_sum[c] += 9               # sum only
    for new_nd, node in ((new, a), (new2, j), (new3, c)):
        ids, free, healthy, fsum = card_delta(nd, new_nd)
        assert ids.tolist() == [node]
        np.testing.assert_array_equal(free[0], new_nd.card_free_memory[node])
        np.testing.assert_array_equal(healthy[0], new_nd.card_healthy[node])
        assert fsum[0] == new_nd.free_memory_sum[node]


def test_static_changes_need_an_upload():
    nd = _fleet()
    i = _node_with_cards(nd)
    for field in ("card_total_memory", "card_clock", "card_bandwidth", "card_core", "card_power"):
        new = _copy(nd)
        getattr(new, field)[i, 0] += 1
        assert card_delta(nd, new) is None, field
    new = _copy(nd)
    new.total_memory_sum[i] += 1
    assert card_delta(nd, new) is None
    new = _copy(nd)
    new.card_count[i] -= 1                      # a card left the node
    assert card_delta(nd, new) is None
    assert card_delta(nd, nd.slice(0, nd.n_nodes - 1)) is None


def test_alloc_and_card_number_are_not_its_business():
    nd = _fleet()
    new = _copy(nd)
    new.alloc_memory[3] += 100
    new.card_number[5] += 1
    assert card_delta(nd, new)[0].size == 0
    new.card_free_memory[_node_with_cards(nd), 0] += 1
    assert card_delta(nd, new)[0].tolist() == [_node_with_cards(nd)]


def test_model_reproduces_the_new_snapshot():
    nd = synth.make_config(4, pods=1, nodes=300)[0].normalized()
    m = cases.Model(nd)
    rng = np.random.default_rng(4)
    ids = rng.choice(nd.n_nodes, 120, replace=False)
    free, healthy, fsum = cases._draw(rng, m, ids)
    m.apply(("cards", ids.astype(np.uint32), free, healthy, fsum))
    new = m.nodes()
    delta = card_delta(nd, new)
    assert 0 < delta[0].size <= 120
    again = cases.Model(nd)
    again.apply(("cards",) + delta)
    got = again.nodes()
    for f in nd.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(got, f), getattr(new, f), err_msg=f)


def test_prototype_and_wrappers_exist():
    with open(os.path.join(REPO, "include", "yoda.h")) as fh:
        text = fh.read()
    proto = re.search(r"int yoda_update_node_cards\(([^;]*)\);", text)
    assert proto, "yoda_update_node_cards is not declared in include/yoda.h"
    args = " ".join(proto.group(1).split())
    assert args == ("yoda_t* h, uint32_t count, const uint32_t* nodes, uint32_t max_cards, "
                    "const uint64_t* card_free_memory, const uint8_t* card_healthy, "
                    "const uint64_t* free_memory_sum")
    assert re.search(r"int yoda_snapshot_check\(yoda_t\* h, uint64_t\* digest, uint32_t\* mismatch\);",
                     text)
    assert callable(getattr(Yoda, "update_cards", None))
    assert callable(getattr(Yoda, "snapshot_check", None))
