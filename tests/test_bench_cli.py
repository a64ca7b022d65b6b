"""bench.py's command line: a plain run is the headline only, --full adds the rest, and
--dump-outputs writes the last timed step's outputs for build-to-build comparison."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, EvalResult

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
FULL_ONLY = ("e2e_ms", "status_counts", "extra", "cpu_baseline")


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    res = EvalResult.empty(5)
    res.pick[:] = [3, -1, 0, 2047, 7]
    res.top_score[:] = [-1, 0, 1 << 40, 5, 6]
    res.maxima[:] = np.arange(30, dtype=np.uint64).reshape(5, 6)
    shapes = bench.dump_outputs(res, str(tmp_path / "d"), 0, 1)
    assert sorted(shapes) == sorted(FIELDS)
    for f in FIELDS:
        a = np.load(tmp_path / "d" / f"{f}.npy")
        assert a.dtype == np.float64 and list(a.shape) == shapes[f]
        assert np.array_equal(a, getattr(res, f).astype(np.float64))
    bench.dump_outputs(res, str(tmp_path / "d"), 1, 2)
    assert (tmp_path / "d" / "pick.rank1.npy").exists()


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--pods", "256", "--nodes", "2048", *argv],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["value"] == pytest.approx(256 * 2048 / (d["ms_per_step"] / 1e3))
    assert not [k for k in FULL_ONLY if k in d]
    nodes, pods = synth.make_config(3, pods=256, nodes=2048)
    want = oracle.schedule(nodes, pods, MODE_SCV, threads=4)
    ok = want.status == 0  # ties and top scores are defined for scheduled pods
    assert ok.any()
    for f in FIELDS:
        a = np.load(tmp_path / f"{f}.npy")
        assert a.dtype == np.float64
        sel = ok if f in ("n_ties", "top_score") else slice(None)
        assert np.array_equal(a[sel], getattr(want, f).astype(np.float64)[sel]), f


@pytest.mark.gpu
def test_full_run_keeps_the_other_figures():
    # the disclosure runs of `extra` are full-size workloads: trimmed here with --no-extras
    d = _bench("--steps", "2", "--warmup", "1", "--full", "--no-extras", "--cpu-seconds", "0.5")
    for k in ("e2e_ms", "status_counts", "cpu_baseline"):
        assert k in d
    assert d["cpu_baseline"]["sample_picks_match_gpu"] is True
    assert sum(d["status_counts"].values()) == 256
