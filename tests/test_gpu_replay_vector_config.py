"""The `cartpole_hip_gpu_replay` preset: it exists, validates, is
`cartpole_hip` in the learner-owns-the-replay topology and nothing else, and
leaves `cartpole_hip` as it was."""

import pytest

from r2d2_amd import config as cfg

NAME = "cartpole_hip_gpu_replay"

TOPOLOGY = dict(gpu_replay=True, vector_actors=True, actor_device="cuda",
                num_actors=16)


@pytest.fixture(autouse=True)
def _restore_config():
    yield
    cfg.apply("mspacman")


def test_preset_exists_and_validates():
    assert NAME in cfg.PRESETS
    c = cfg.apply(NAME)
    assert cfg.get() is c
    assert c.obs_shape == (4,) and c.encoder == "mlp"
    assert c.hidden_dim == 512 and c.mlp_hidden == 512
    assert c.device == "cuda" and c.use_hip_kernels
    for k, v in TOPOLOGY.items():
        assert getattr(c, k) == v, k
    assert cfg.gpu_replay is True and cfg.num_actors == 16


def test_preset_is_cartpole_hip_in_the_gpu_replay_topology():
    base = cfg.apply("cartpole_hip")
    c = cfg.apply(NAME)
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    assert diff == set(TOPOLOGY), diff
    assert c.seq_len == base.seq_len == 19
    assert c.seq_per_block == base.seq_per_block == 5
    assert c.num_blocks == base.num_blocks == 1000
    # the fused actor step stays at the dataclass default
    assert "fused_actor_step" not in cfg.PRESETS[NAME]
    assert c.fused_actor_step is cfg.Config().fused_actor_step


def test_frame_dedup_on_a_vector_preset_raises():
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        cfg.apply(NAME, replay_frame_dedup=True)


def test_other_mlp_widths_validate():
    c = cfg.apply(NAME, hidden_dim=128, mlp_hidden=128)
    assert c.gpu_replay and c.hidden_dim == 128 and c.mlp_hidden == 128


def test_cartpole_hip_is_unchanged():
    assert cfg.PRESETS["cartpole_hip"] == dict(
        game_name="CartPole", env_type="cartpole", obs_shape=(4,),
        action_dim=2, encoder="mlp", hidden_dim=512, mlp_hidden=512,
        device="cuda", dtype="bf16", use_hip_kernels=True, gpu_replay=False,
        buffer_capacity=40_000, learning_starts=2_000, block_length=40,
        burn_in_steps=8, learning_steps=8, forward_steps=3,
        training_steps=2_000, num_actors=2, amp=True)
    c = cfg.apply("cartpole_hip")
    assert c.gpu_replay is False and c.vector_actors is False
    assert c.actor_device == "cpu" and c.num_actors == 2
