"""bench.py command line: the result line, --dump-outputs and --full.
Runs the cartpole preset so a step is fast; the argument handling, timing
and dump code are the ones the flagship run uses."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--batches", "2", "--preset", "cartpole", *extra],
        cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Two runs with the same arguments, each dumping its outputs, plus their
    result lines.  The second adds --full, which must leave the headline
    path and its outputs as they are."""
    dirs = [str(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]
    recs = [_bench("--dump-outputs", dirs[0]),
            _bench("--dump-outputs", dirs[1], "--full")]
    return dirs, recs


def test_result_line_fields(dumped):
    _, recs = dumped
    for rec in recs:
        _check_result_line(rec)


def _check_result_line(rec):
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in rec, key
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    c_batch = rec["config"]["global_batch"]
    assert rec["value"] == pytest.approx(
        c_batch / (rec["ms_per_step"] / 1000.0), rel=1e-2)


def test_dump_outputs_written_and_repeatable(dumped):
    dirs, recs = dumped
    B = recs[0]["config"]["global_batch"]
    arrays = []
    for d in dirs:
        assert sorted(os.listdir(d)) == ["loss.npy", "priorities.npy"]
        loss = np.load(os.path.join(d, "loss.npy"))
        prio = np.load(os.path.join(d, "priorities.npy"))
        assert loss.dtype == np.float32 and loss.shape == (1,)
        assert prio.dtype == np.float32 and prio.shape == (B,)
        assert np.isfinite(loss).all() and np.isfinite(prio).all()
        assert (prio >= 0).all()
        arrays.append((loss, prio))
    # same arguments -> same inputs -> same outputs (fp32 reduction order is
    # the only freedom between two runs)
    np.testing.assert_allclose(arrays[0][0], arrays[1][0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(arrays[0][1], arrays[1][1], rtol=1e-4, atol=1e-6)

