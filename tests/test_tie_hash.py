"""The selectHost draw word (include/yoda.h yoda_tie_hash; host only): equal to the header's
formula restated in numpy, a bijection of the node ids for one pod, and uniform over a tie set
whatever the ids' pattern.  Every input is fixed, so nothing here can flake."""
import numpy as np
import pytest

from yoda_amd import capi

from tie_draw_cases import tie_hash

U64_MAX = 2**64 - 1


def test_matches_the_formula_on_a_grid():
    seeds = [0, 1, 12345, 0x9E3779B97F4A7C15, U64_MAX]
    pods = [0, 1, 63, 64, 99999, 2**32 - 1, 2**32, 2**32 + 7, 2**40 + 3, U64_MAX]
    nodes = [0, 1, 2, 63, 64, 4095, 70000, 2**31 - 1, 2**31, 0xFFFFFFFE, 0xFFFFFFFF]
    for s in seeds:
        for p in pods:
            want = tie_hash(s, p, np.array(nodes, np.uint32))
            got = [capi.tie_hash(s, p, n) for n in nodes]
            assert got == [int(w) for w in want], (s, p)


def test_null_handle_is_rejected():
    assert capi.lib().yoda_set_tie_draw(None, 1, 0, 0) == -1


@pytest.mark.parametrize("seed,pod", [(0, 0), (12345, 2**32 + 5), (U64_MAX, 77)])
def test_words_of_one_pod_are_distinct(seed, pod):
    words = tie_hash(seed, pod, np.arange(1 << 22, dtype=np.uint32))
    assert np.unique(words).size == words.size
    # the library agrees on a sample of them
    for n in (0, 1, 4097, (1 << 22) - 1):
        assert capi.tie_hash(seed, pod, n) == int(words[n])


PATTERNS = {
    "pair": np.array([0, 1]),
    "three": np.array([1000, 1001, 1002]),
    "stride64": np.arange(17) * 64,
    "run1000": np.arange(1000) + 3,
    "stride12500": np.arange(8) * 12500,
}
N_PODS = 200000


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_draw_is_uniform_over_a_tie_set(seed, name):
    """chi-square z-score (chi2 - dof) / sqrt(2 dof) within +-4 and the fraction of consecutive
    pods drawing the same member within 0.005 of 1 / |set| (measured with these inputs: worst
    |z| 2.25, worst fraction off by 0.0014)."""
    ids = PATTERNS[name].astype(np.uint64)
    k = ids.size
    winner = np.empty(N_PODS, np.int64)
    step = 20000 if k <= 32 else 2000  # pods per broadcast: bounded memory
    for p0 in range(0, N_PODS, step):
        pods = np.arange(p0, p0 + step, dtype=np.uint64)[:, None]
        key = (tie_hash(seed, pods, ids.astype(np.uint32)[None, :]).astype(np.uint64)
               << np.uint64(32)) | ids[None, :]
        winner[p0:p0 + step] = np.argmin(key, axis=1)
    counts = np.bincount(winner, minlength=k).astype(np.float64)
    e = N_PODS / k
    chi2 = ((counts - e) ** 2 / e).sum()
    dof = k - 1
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    same = float((winner[1:] == winner[:-1]).mean())
    print(f"{name} seed {seed}: z {z:+.3f}, same-as-previous {same:.5f} (1/k {1.0 / k:.5f})")
    assert abs(z) <= 4.0, z
    assert abs(same - 1.0 / k) <= 0.005, same
