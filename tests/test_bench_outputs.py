"""bench.py's one-GPU run: --steps is the number of timed iterations, --dump-outputs writes what the timed solve computed (the
same bits run after run, and those of the CPU oracle with exact inner products), and the figures that take passes of their own
come only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*extra, timeout=300):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", *extra], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_is_refused_for_more_than_one_gpu(tmp_path):
    """Not a GPU test: the refusal comes from the argument check, before anything is imported or started."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--dump-outputs" in out.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_a_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    from oracle import oracle
    n, k = 256, 30
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        j = _bench("--steps", str(k), "--warmup", "5", "--grid", str(n), "--dump-outputs", str(d))
        assert (j["metric"], j["unit"], j["higher_is_better"], j["dtype"]) == ("cg_iters_per_sec", "iters/s", True, "f64")
        assert j["steps"] == k and j["repeats"] == 1 and j["ms_per_step"] > 0
        assert j["value"] == pytest.approx(1e3 / j["ms_per_step"], rel=1e-3)
        assert j["roofline"] is None and "cpu_baseline" not in j and "repeat_spread" not in j      # --full only
        x, rec = np.load(d / "x.npy"), np.load(d / "results.npy")
        assert x.dtype == rec.dtype == np.float64
        runs.append((x, rec))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    og = oracle.OracleGrid(n, n)
    with oracle.exact_dots():
        ex = og.mf_solve(eps=0.0, max_iterations=k)
    x, rec = runs[0]
    assert ex.iterations == k == rec[0]
    assert (rec[1], rec[2]) == (ex.r_norm, ex.initial_r_norm)
    assert np.array_equal(x, ex.x)


@pytest.mark.gpu
def test_a_full_run_adds_the_roofline_and_the_spread():
    j = _bench("--steps", "40", "--warmup", "5", "--grid", "512", "--full", "--cpu-iters", "0")
    assert j["steps"] == 40 and j["repeats"] == 1
    assert j["roofline"]["kernel"] in ("k_stencil", "k_update_st") and j["roofline"]["achieved"] > 0
    assert j["repeat_spread"]["solves"] == 11 and j["repeat_spread"]["median_iters_per_sec"] > 0
