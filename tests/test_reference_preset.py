"""The single-frame `mspacman_reference` preset: it applies and validates,
the five BASELINE presets are untouched, the HIP gating admits the shape,
and bench.py runs it to a result line (eager on a machine without a GPU)."""

import json
import os
import subprocess
import sys

from r2d2_amd import config as cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the five BASELINE presets as they stood before the reference preset
BASELINE_PRESETS = {
    "cartpole": dict(
        game_name="CartPole", env_type="cartpole", obs_shape=(4,),
        action_dim=2, encoder="mlp", hidden_dim=128, mlp_hidden=128,
        device="cpu", dtype="fp32", use_hip_kernels=False, gpu_replay=False,
        buffer_capacity=40_000, learning_starts=2_000, block_length=40,
        burn_in_steps=8, learning_steps=8, forward_steps=3,
        training_steps=2_000, num_actors=2, amp=False,
    ),
    "mspacman": dict(
        game_name="MsPacman", env_type="synthetic", obs_shape=(4, 84, 84),
        action_dim=9, encoder="nature", gpu_replay=False,
    ),
    "mspacman_gpu_replay": dict(
        game_name="MsPacman", env_type="synthetic", obs_shape=(4, 84, 84),
        action_dim=9, encoder="nature", gpu_replay=True, num_actors=256,
        buffer_capacity=4_000_000, vector_actors=True, actor_device="cuda",
    ),
    "mspacman_dp": dict(
        game_name="MsPacman", env_type="synthetic", obs_shape=(4, 84, 84),
        action_dim=9, encoder="nature", gpu_replay=True, num_actors=256,
        buffer_capacity=4_000_000, vector_actors=True, actor_device="cuda",
    ),
    "seaquest_impala": dict(
        game_name="Seaquest", env_type="synthetic", obs_shape=(4, 84, 84),
        action_dim=18, encoder="impala",
    ),
}


def test_baseline_presets_unchanged_and_first():
    names = list(cfg.PRESETS)
    assert names[:5] == list(BASELINE_PRESETS)
    for name, want in BASELINE_PRESETS.items():
        assert cfg.PRESETS[name] == want, name


def test_reference_preset_applies():
    base = cfg.apply("mspacman")
    c = cfg.apply("mspacman_reference")
    assert tuple(c.obs_shape) == (1, 84, 84) and cfg.obs_shape == (1, 84, 84)
    assert c.encoder == "nature" and c.hidden_dim == 512
    assert c.loss_fn == "huber"          # project default; reference: mse
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    assert diff == {"obs_shape"}, diff
    # overrides still validate
    assert cfg.apply("mspacman_reference", loss_fn="mse").loss_fn == "mse"


def test_reference_gpu_replay_preset_applies():
    base = cfg.apply("mspacman_gpu_replay")
    c = cfg.apply("mspacman_reference_gpu_replay")
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    assert diff == {"obs_shape"}, diff
    assert tuple(c.obs_shape) == (1, 84, 84)


def test_hip_gate_channels():
    from r2d2_amd.ops.engine import conv1_channels
    assert conv1_channels("nature") == (1, 4)
    assert conv1_channels("impala") == (4,)   # IMPALA stays 4-channel


def test_bench_cli_runs_reference_preset():
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--batches", "1", "--preset", "mspacman_reference"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["config"]["obs"] == [1, 84, 84]
    assert rec["metric"] == \
        "learner seq-samples/sec (mspacman_reference preset)"
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
