"""The fused_actor_step config field (CPU): default off, accepted by apply,
carried through the asdict snapshot that train() hands to spawned actors,
and ignored by a VectorActor that has no K15 path."""

import queue
from dataclasses import asdict

from r2d2_amd import config as cfg


def test_default_is_off():
    assert cfg.Config().fused_actor_step is False
    for name in cfg.PRESETS:
        assert "fused_actor_step" not in cfg.PRESETS[name], name


def test_apply_accepts_and_survives_the_spawn_snapshot():
    try:
        c = cfg.apply("mspacman_gpu_replay", fused_actor_step=True)
        assert c.fused_actor_step is True and cfg.fused_actor_step is True
        d = asdict(c)
        cfg.apply("mspacman")                  # a spawned child's start state
        assert cfg.get().fused_actor_step is False
        c2 = cfg.apply(**d)
        assert c2.fused_actor_step is True
        assert asdict(c2) == d
    finally:
        cfg.apply("mspacman")


def test_cpu_vector_actor_ignores_the_field():
    from r2d2_amd.models.network import Network
    from r2d2_amd.train import epsilon_ladder
    from r2d2_amd.worker import VectorActor

    def run(fused):
        c = cfg.apply("cartpole", num_actors=2, vector_actors=True,
                      actor_device="cpu", fused_actor_step=fused)
        import torch
        torch.manual_seed(0)
        model = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                        encoder=c.encoder, forward_steps=c.forward_steps,
                        mlp_hidden=c.mlp_hidden)
        sq = queue.Queue()
        va = VectorActor(epsilon_ladder(2), model, [sq], device="cpu", seed=1)
        assert va.hip_inf is None
        assert va.run(stop_after_steps=60) >= 60
        out = []
        while not sq.empty():
            block, prio, _ = sq.get()
            out.append((block.action.tobytes(), block.hidden.tobytes()))
        return out

    try:
        off, on = run(False), run(True)
        assert len(off) >= 1 and off == on
    finally:
        cfg.apply("mspacman")
