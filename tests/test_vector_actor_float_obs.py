"""VectorActor hands 1-D (vector) observations to the policy as the float32
env states they are; 3-D frame stacks stay uint8."""

import queue

import numpy as np
import torch

from r2d2_amd import config as cfg
from r2d2_amd.models.network import Network
from r2d2_amd.train import epsilon_ladder
from r2d2_amd.worker import VectorActor


class _Recorder(torch.nn.Module):
    """Stands in for VectorActor.model: keeps a copy of state.obs per tick
    and answers like the real network."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.seen = []

    def forward(self, state):
        self.seen.append(state.obs.clone())
        return self.net(state)


def test_policy_input_is_the_float32_env_state():
    try:
        c = cfg.apply("cartpole", hidden_dim=32, mlp_hidden=32, num_actors=3,
                      max_episode_steps=50, actor_update_interval=10_000)
        torch.manual_seed(0)
        model = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                        encoder="mlp", forward_steps=c.forward_steps,
                        mlp_hidden=c.mlp_hidden)
        E = 3
        sq = queue.Queue()
        va = VectorActor(epsilon_ladder(E), model, [sq], device="cpu", seed=5)
        assert va.obs_t.dtype == torch.float32
        assert va._obs_host.dtype == np.float32
        rec = _Recorder(va.model)
        va.model = rec

        # the env states as the envs hand them out, in tick order
        states = [[] for _ in range(E)]
        for i, env in enumerate(va.envs):
            reset, step = env.reset, env.step

            def spy_reset(_r=reset, _i=i):
                obs = _r()
                states[_i].append(obs.copy())
                return obs

            def spy_step(a, _s=step, _i=i):
                out = _s(a)
                states[_i].append(out[0].copy())
                return out

            env.reset, env.step = spy_reset, spy_step

        assert va.run(stop_after_steps=120) >= 120
        assert len(rec.seen) >= 40
        # tick t's policy input for env i is the latest state env i produced
        # before that tick; an env that ended an episode is reset in the same
        # tick, so its last two states (terminal, reset) arrive together and
        # the policy sees the reset one.  Every captured row must therefore be
        # one of the env's recorded states, bit for bit.
        allowed = [{s.tobytes() for s in states[i]} for i in range(E)]
        frac = neg = 0
        for obs in rec.seen:
            assert obs.dtype == torch.float32 and obs.shape == (E, 4)
            for i in range(E):
                row = obs[i].numpy()
                assert row.tobytes() in allowed[i], (i, row)
                frac += bool((row != np.round(row)).any())
                neg += bool((row < 0).any())
        assert frac > 0 and neg > 0, "fractional and negative values reach " \
                                     "the policy"
        # first tick: exactly the reset states
        for i in range(E):
            assert rec.seen[0][i].numpy().tobytes() == states[i][0].tobytes()
        # and the data LocalBuffer stores is the same floats
        block, _, _ = sq.get_nowait()
        assert block.obs.dtype == np.float32
    finally:
        cfg.apply("mspacman")


def test_frame_stack_buffers_stay_uint8():
    try:
        c = cfg.apply("mspacman", num_actors=2, hidden_dim=32,
                      device="cpu", use_hip_kernels=False, gpu_replay=False)
        torch.manual_seed(0)
        model = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                        encoder="nature", forward_steps=c.forward_steps)
        va = VectorActor(epsilon_ladder(2), model, [queue.Queue()],
                         device="cpu", seed=1)
        assert va.obs_t.dtype == torch.uint8
        assert va._obs_host.dtype == np.uint8
        assert va.obs_t.shape == (2, 4, 84, 84)
    finally:
        cfg.apply("mspacman")
