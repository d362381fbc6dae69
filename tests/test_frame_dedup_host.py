"""Host side of the frame-once GPU replay store (replay_frame_dedup): the
numpy helpers, the frame-stacking synthetic env, the invariant on real
LocalBuffer blocks, AtariEnv's stacking, and the config fields."""

from dataclasses import asdict

import numpy as np
import pytest

from r2d2_amd import config as cfg
from r2d2_amd.envs.synthetic import SyntheticAtariEnv
from r2d2_amd.replay.frame_dedup import (frames_from_stacked, is_frame_stack,
                                         stacked_from_frames)


def make_stacked(rows, C, hw=(5, 7), seed=0):
    """(rows, C, H, W) rolling stack of rows + C - 1 random frames."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(rows + C - 1,) + hw, dtype=np.uint8)
    x = np.stack([frames[r:r + C] for r in range(rows)])
    return frames, x


@pytest.mark.parametrize("C", [2, 3, 4])
def test_round_trip_and_invariant(C):
    for rows in (1, 2, C, 50):      # rows = 1: all lead-in plus one frame
        frames, x = make_stacked(rows, C, seed=rows)
        assert x.shape == (rows, C, 5, 7)
        got = frames_from_stacked(x)
        assert got.shape == (rows + C - 1, 5, 7) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, frames)
        back = stacked_from_frames(got, C)
        np.testing.assert_array_equal(back, x)
        assert is_frame_stack(x)
        # writing into a caller's buffer (the pinned staging path)
        out = np.zeros_like(frames)
        assert frames_from_stacked(x, out=out) is out
        np.testing.assert_array_equal(out, frames)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_is_frame_stack_sees_one_changed_byte(C):
    _, x = make_stacked(50, C)
    assert is_frame_stack(x)
    x[3, 1, 2, 4] ^= 1
    assert not is_frame_stack(x)


def test_frames_from_stacked_is_defined_for_any_input():
    """Not a stack: the first C - 1 channels of row 0, then the last channel
    of every row — what a verify-off ingest stores."""
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, size=(6, 4, 3, 3), dtype=np.uint8)
    assert not is_frame_stack(x)
    f = frames_from_stacked(x)
    np.testing.assert_array_equal(f[:3], x[0, :3])
    np.testing.assert_array_equal(f[3:], x[:, 3])


# ---------------------------------------------------------------------------
# SyntheticAtariEnv(frame_stack=True)
# ---------------------------------------------------------------------------

def test_synthetic_frame_stack_rolls_one_frame_per_step():
    env = SyntheticAtariEnv(obs_shape=(4, 20, 20), seed=3, frame_stack=True)
    obs = env.reset()
    assert obs.shape == (4, 20, 20) and obs.dtype == np.uint8
    for c in range(1, 4):           # reset: C copies of one frame
        np.testing.assert_array_equal(obs[c], obs[0])
    seen = [obs]
    for t in range(12):
        nxt, r, done, _ = env.step(t % 9)
        assert nxt.shape == (4, 20, 20) and nxt.dtype == np.uint8
        np.testing.assert_array_equal(nxt[:-1], seen[-1][1:])
        seen.append(nxt)
    assert is_frame_stack(np.stack(seen))
    # the blob moves, so consecutive frames differ: the stack is not trivial
    assert not np.array_equal(seen[-1][-1], seen[-1][0])
    # the returned stack is a copy, not the env's live state
    seen[-1][:] = 0
    nxt, *_ = env.step(0)
    assert nxt[:-1].any()
    # a new episode starts from one repeated frame again
    obs = env.reset()
    for c in range(1, 4):
        np.testing.assert_array_equal(obs[c], obs[0])


def test_synthetic_default_mode_is_unchanged():
    """Flag off: the observations for a fixed seed equal the generator's
    arithmetic as it was before the flag existed (copied here)."""
    shape, seed = (4, 20, 24), 11
    env = SyntheticAtariEnv(obs_shape=shape, seed=seed)
    assert env.frame_stack is False
    rng = np.random.default_rng(seed)
    c, h, w = shape
    base = rng.integers(0, 64, size=(c, h, w)).astype(np.uint8)
    pos = np.array([h // 2, w // 2], dtype=np.int64)

    def frame():
        f = base.copy()
        y, x = int(pos[0]) % (h - 8), int(pos[1]) % (w - 8)
        f[:, y:y + 8, x:x + 8] = 255
        return f

    np.testing.assert_array_equal(env.reset(), frame())
    moves = [(-2, 0), (2, 0), (0, -2), (0, 2)]
    for a in (0, 3, 5, 2, 8, 1):
        obs, reward, done, _ = env.step(a)
        pos += moves[a % 4]
        assert reward == float(rng.random() < 0.05) * 10.0
        assert done == bool(rng.random() < 1.0 / 600)
        np.testing.assert_array_equal(obs, frame())


def test_create_env_passes_the_config_field():
    from r2d2_amd.envs import create_env
    cfg.apply("mspacman")
    assert create_env(seed=0).frame_stack is False
    cfg.apply("mspacman", synthetic_frame_stack=True)
    env = create_env(seed=0)
    assert env.frame_stack is True
    obs = env.reset()
    np.testing.assert_array_equal(obs[0], obs[3])


def test_local_buffer_blocks_are_frame_stacks():
    """An episode pushed through a real LocalBuffer: every block satisfies
    the invariant — the second block of the episode too, whose rows start
    with the carried burn-in prefix — and so does the first block of the
    next episode."""
    from r2d2_amd.worker import LocalBuffer
    c = cfg.apply("mspacman", obs_shape=(4, 20, 20), block_length=20,
                  learning_steps=10, burn_in_steps=6, forward_steps=3,
                  hidden_dim=8)
    env = SyntheticAtariEnv(obs_shape=c.obs_shape, seed=5, frame_stack=True)
    lb = LocalBuffer(c.action_dim)
    q = np.zeros(c.action_dim, dtype=np.float32)
    hid = np.zeros((2, c.hidden_dim), dtype=np.float32)
    blocks = []

    def run_episode(steps):
        lb.reset(env.reset())
        for t in range(steps):
            obs, r, _, _ = env.step(t % c.action_dim)
            lb.add(t % c.action_dim, r, obs, q, hid)
            last = t == steps - 1
            if len(lb) == c.block_length or last:
                blocks.append(lb.finish(None if last else q)[0])

    run_episode(20 + 20 + 7)        # full, full continuation, short tail
    run_episode(1)                  # a one-step episode
    assert [b.obs.shape[0] for b in blocks] == [21, 27, 14, 2]
    assert [int(b.burn_in_steps[0]) for b in blocks] == [0, 6, 6, 0]
    for b in blocks:
        assert is_frame_stack(b.obs)
        np.testing.assert_array_equal(
            stacked_from_frames(frames_from_stacked(b.obs), 4), b.obs)
    # the continuation block's first row is a mid-episode stack (its lead-in
    # frames are real earlier frames, not copies of one)
    assert not np.array_equal(blocks[1].obs[0, 0], blocks[1].obs[0, 3])
    # across an episode boundary the invariant does NOT hold — blocks never
    # span one, which is why the store can keep frames once per block
    joined = np.concatenate([blocks[2].obs, blocks[3].obs])
    assert not is_frame_stack(joined)


def test_atari_env_stacking_satisfies_the_invariant():
    """AtariEnv's stacking (_warp) without ALE: fake frames through an
    instance built without gymnasium."""
    from r2d2_amd.envs.atari import AtariEnv
    env = AtariEnv.__new__(AtariEnv)
    env.obs_shape = (4, 84, 84)
    env._stack = None
    rng = np.random.default_rng(0)
    obs = [env._warp(rng.integers(0, 256, size=(210, 160)).astype(np.uint8))
           for _ in range(7)]
    for c in range(1, 4):           # first observation: one frame repeated
        np.testing.assert_array_equal(obs[0][c], obs[0][0])
    assert is_frame_stack(np.stack(obs))
    env._stack = None               # what reset() does
    first = env._warp(np.full((210, 160), 9, dtype=np.uint8))
    assert (first == 9).all()


# ---------------------------------------------------------------------------
# config
# ---------------------------------------------------------------------------

def test_defaults_are_off():
    c = cfg.apply("mspacman")
    assert c.replay_frame_dedup is False
    assert c.replay_dedup_verify is True
    assert c.synthetic_frame_stack is False
    assert cfg.replay_frame_dedup is False
    for name in ("mspacman_gpu_replay", "mspacman_dp", "cartpole"):
        assert cfg.apply(name).replay_frame_dedup is False


def test_dedup_flag_validation():
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        cfg.apply("mspacman_gpu_replay", replay_frame_dedup=True,
                  obs_shape=(1, 84, 84))
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        cfg.apply("cartpole", replay_frame_dedup=True, gpu_replay=True)
    assert cfg.PRESETS["cartpole"]["obs_shape"] == (4,)
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        cfg.apply("mspacman_gpu_replay", replay_frame_dedup=True,
                  gpu_replay=False)
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        cfg.apply("mspacman", replay_frame_dedup=True)   # host replay preset
    c = cfg.apply("mspacman_gpu_replay", replay_frame_dedup=True)
    assert c.replay_frame_dedup and cfg.replay_frame_dedup is True
    assert cfg.apply("mspacman", replay_frame_dedup=True, gpu_replay=True,
                     obs_shape=(2, 84, 84)).replay_frame_dedup


def test_dedup_presets_resolve():
    base = cfg.apply("mspacman")
    c = cfg.apply("mspacman_dedup")
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    # gpu_replay=True is what the flag's validation demands
    assert diff == {"replay_frame_dedup", "replay_dedup_verify",
                    "gpu_replay"}, diff
    assert c.replay_frame_dedup and not c.replay_dedup_verify

    base = cfg.apply("mspacman_gpu_replay")
    c = cfg.apply("mspacman_gpu_replay_dedup")
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    assert diff == {"replay_frame_dedup", "synthetic_frame_stack"}, diff
    assert c.replay_frame_dedup and c.replay_dedup_verify
    assert c.synthetic_frame_stack
    # appended after the presets other tests pin by position
    assert list(cfg.PRESETS)[-2:] == ["mspacman_dedup",
                                      "mspacman_gpu_replay_dedup"]


def test_fields_survive_the_spawn_snapshot():
    """Spawned actor/learner processes start from the default config and
    re-apply asdict(c) (train.py)."""
    c = cfg.apply("mspacman_gpu_replay_dedup", replay_dedup_verify=False)
    snap = asdict(c)
    assert snap["replay_frame_dedup"] is True
    cfg.apply("mspacman")
    assert cfg.get().replay_frame_dedup is False
    c2 = cfg.apply(**snap)
    assert c2 == c
    assert c2.replay_frame_dedup and c2.synthetic_frame_stack
    assert c2.replay_dedup_verify is False
