"""GPU tests of the frame-once replay store (config.replay_frame_dedup): the
dedup gather against the plain store and against numpy, ring overwrite, the
direct kernel binding at C = 2, 3, 4, the ingest check, the argument checks,
and a train step on a dedup-sampled batch.

Both storage modes only move bytes, so every comparison is exact."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.ops import hip_ops
    from r2d2_amd.replay.frame_dedup import (frames_from_stacked,
                                             is_frame_stack,
                                             stacked_from_frames)

# smallest layout with two+ sequences per block and burn-in shorter than a
# block: 4 sequences of 20 per 80-step block, T = 10 + 20 + 5 = 35, 8 slots
SMALL = dict(block_length=80, learning_steps=20, burn_in_steps=10,
             forward_steps=5, buffer_capacity=8 * 80, batch_size=16)

# episode lengths -> blocks (steps, burn_in[0]):
#   173 -> (80, 0) full first-of-episode, (80, 10) full continuation with the
#          whole prefix, (13, 10) shorter than learning_steps
#   1   -> (1, 0) a block of one step
#   125 -> (80, 0), (45, 10);  30 -> (30, 0);  80 -> (80, 0)
EPISODES_8 = (173, 1, 125, 30, 80)
# 2 * 8 + 3 = 19 blocks: eight full ones, then short ones landing in every
# slot that held a full one (slot 2: 80 -> 30 -> 2 steps), then three more
EPISODES_19 = (640, 1, 13, 30, 85, 45, 7, 80, 25, 82)


def small_cfg(dedup, **kw):
    over = dict(SMALL)
    over.update(kw)
    if dedup:
        over.update(gpu_replay=True, replay_frame_dedup=True)
    return cfg.apply("mspacman", **over)


@functools.lru_cache(maxsize=None)
def make_blocks(episodes, seed=0):
    """[(Block, priorities)] from SyntheticAtariEnv(frame_stack=True) through
    a real LocalBuffer, episode ends forced at the given lengths.  Built
    once per argument set and never modified."""
    from r2d2_amd.envs.synthetic import SyntheticAtariEnv
    from r2d2_amd.worker import LocalBuffer
    from dataclasses import asdict
    prev = asdict(cfg.get())
    c = small_cfg(False)
    rng = np.random.default_rng(seed)
    env = SyntheticAtariEnv(obs_shape=c.obs_shape, seed=seed,
                            frame_stack=True)
    lb = LocalBuffer(c.action_dim)       # reads the layout from the config
    cfg.apply(**prev)
    out = []
    for steps in episodes:
        lb.reset(env.reset())
        for t in range(steps):
            a = int(rng.integers(c.action_dim))
            obs, r, _, _ = env.step(a)
            lb.add(a, r + float(rng.normal()),
                   obs, rng.normal(size=c.action_dim).astype(np.float32),
                   rng.normal(size=(2, c.hidden_dim)).astype(np.float32))
            last = t == steps - 1
            if len(lb) == c.block_length or last:
                q = None if last else rng.normal(
                    size=c.action_dim).astype(np.float32)
                block, prio, _ = lb.finish(q)
                assert is_frame_stack(block.obs)
                out.append((block, prio))
    return tuple(out)


def build_pair(blocks, **kw):
    """One buffer per storage mode, fed the same blocks and priorities."""
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    small_cfg(False, **kw)
    plain = GpuReplayBuffer(device="cuda")
    small_cfg(True, **kw)
    dedup = GpuReplayBuffer(device="cuda")
    assert dedup.frame_dedup and not plain.frame_dedup
    C, hw = 4, 84 * 84
    assert plain.obs_store.shape == (8, 91, C * hw)
    assert dedup.obs_store.shape == (8, 91 + C - 1, hw)
    assert dedup._pin_obs[0].shape == (91 + C - 1, hw)
    for block, prio in blocks:
        plain.ingest(block, prio)
        dedup.ingest(block, prio)
    torch.cuda.synchronize()
    assert torch.equal(plain.tree, dedup.tree)
    assert plain.block_ptr == dedup.block_ptr and len(plain) == len(dedup)
    return plain, dedup


BATCH_FIELDS = ("obs", "last_action", "last_reward", "action",
                "n_step_reward", "gamma", "is_weights", "hidden",
                "burn_in_steps", "learning_steps", "forward_steps",
                "meta_dev", "seg_dev")


def assert_batches_equal(bp, bd):
    assert torch.equal(bp.idxes, bd.idxes)
    for f in BATCH_FIELDS:
        a, b = getattr(bp, f), getattr(bd, f)
        assert a.shape == b.shape and a.dtype == b.dtype, f
        assert torch.equal(a, b), f


def check_against_blocks(batch, slot_blocks, replay, obs_of=lambda b: b.obs):
    """Independent of the plain gather: every sampled row is the HWC
    transpose of the source block's obs row, rows past the sequence zero."""
    c = replay.cfg
    obs = batch.obs.cpu().numpy()
    idx = batch.idxes.cpu().numpy()
    assert obs.shape == (len(idx), c.seq_len, 84, 84, 4)
    for i, s in enumerate(idx):
        blk = slot_blocks[s // replay.spb]
        si = s % replay.spb
        assert si < blk.num_sequences
        burn = int(batch.burn_in_steps[i])
        L = burn + int(batch.learning_steps[i]) + int(batch.forward_steps[i])
        assert burn == int(blk.burn_in_steps[si])
        start = (int(blk.burn_in_steps[0])
                 + int(blk.learning_steps[:si].astype(np.int64).sum()) - burn)
        want = obs_of(blk)[start:start + L].transpose(0, 2, 3, 1)
        np.testing.assert_array_equal(obs[i, :L], want)
        assert not obs[i, L:].any()


def sample_pairs(plain, dedup, seeds):
    out = []
    for k in seeds:
        torch.manual_seed(k)
        bp = plain.sample(16)
        torch.manual_seed(k)
        bd = dedup.sample(16)
        torch.cuda.synchronize()
        out.append((bp, bd))
    return out


def run_equality(blocks):
    plain, dedup = build_pair(blocks)
    nb = plain.num_blocks
    slot_blocks = {}
    for i, (block, _) in enumerate(blocks):
        slot_blocks[i % nb] = block
    T = plain.T
    seen_padded = seen_partial_burn = False
    for bp, bd in sample_pairs(plain, dedup, range(5)):
        assert_batches_equal(bp, bd)
        check_against_blocks(bd, slot_blocks, dedup)
        valid = bd.burn_in_steps + bd.learning_steps + bd.forward_steps
        seen_padded |= bool((valid < T).any())
        seen_partial_burn |= bool((bd.burn_in_steps
                                   < dedup.cfg.burn_in_steps).any())
    # the draws must have exercised padding (t >= valid rows) and a sequence
    # whose burn-in is cut short by the episode start
    assert seen_padded and seen_partial_burn


def test_block_set_has_every_kind():
    c = small_cfg(False)
    blocks = [b for b, _ in make_blocks(EPISODES_8)]
    kinds = [(b.action.shape[0], int(b.burn_in_steps[0])) for b in blocks]
    assert kinds == [(80, 0), (80, 10), (13, 10), (1, 0), (80, 0), (45, 10),
                     (30, 0), (80, 0)]
    assert 13 < c.learning_steps and c.seq_per_block == 4


def test_dedup_equals_plain_store():
    run_equality(make_blocks(EPISODES_8))


def test_ring_overwrite():
    blocks = make_blocks(EPISODES_19, seed=1)
    assert len(blocks) == 2 * 8 + 3
    steps = [b.action.shape[0] for b, _ in blocks]
    assert steps[:8] == [80] * 8
    # slot 2: 80 -> 30 -> 2 steps; slot 0: 80 -> 1 -> 25; slot 4: 80 -> 5
    assert (steps[2], steps[10], steps[18]) == (80, 30, 2)
    assert (steps[0], steps[8], steps[16]) == (80, 1, 25)
    assert (steps[4], steps[12]) == (80, 5)
    run_equality(blocks)


# ---------------------------------------------------------------------------
# the kernel through its binding, hand-built stores
# ---------------------------------------------------------------------------

def hand_store(C, hw=256, H=4):
    """2 slots, obs_rows = 6 (burn 1 + block 4 + 1), spb = 2, T = 5.
    Frame f of the store holds (f * 251 + pixel) % 256, so a wrong frame,
    pixel or channel order shows."""
    obs_rows, block_len, nb = 6, 4, 2
    nfr = obs_rows + C - 1
    f = np.arange(nb * nfr, dtype=np.int64)[:, None]
    p = np.arange(hw, dtype=np.int64)[None, :]
    frames = ((f * 251 + p) % 256).astype(np.uint8).reshape(nb, nfr, hw)
    rng = np.random.default_rng(C)
    st = dict(
        obs=frames,
        la=rng.integers(0, 5, size=(nb, obs_rows)).astype(np.uint8),
        lr=rng.normal(size=(nb, obs_rows)).astype(np.float32),
        act=rng.integers(0, 5, size=(nb, block_len)).astype(np.uint8),
        nsr=rng.normal(size=(nb, block_len)).astype(np.float32),
        gam=rng.random(size=(nb, block_len)).astype(np.float32),
        hid=rng.normal(size=(nb * 2, 2 * H)).astype(np.float32),
    )
    # sample b: (slot, seq, burn, learn, fwd, learn_off)
    samples = [(0, 0, 1, 2, 2, 0),    # g = 0..4: fills T, slot 0 from row 0
               (1, 1, 1, 2, 1, 2),    # g = 8..11: last row of the last slot
               (1, 0, 0, 1, 1, 0)]    # g = 6, 7: slot 1 from its row 0
    meta = np.zeros((5, 3), dtype=np.int32)
    idx = np.zeros(3, dtype=np.int64)
    for b, (slot, seq, burn, learn, fwd, off) in enumerate(samples):
        meta[:, b] = (burn, learn, fwd, slot * obs_rows + 1 + off, off)
        idx[b] = slot * 2 + seq
    # first-of-episode slot 1 seq 0 has burn_in[0] = 0 in this layout
    meta[3, 2] = 1 * obs_rows + 0
    seg = np.concatenate([[0], np.cumsum(meta[1])]).astype(np.int32)
    w = np.array([0.5, 1.0, 0.25], dtype=np.float32)
    return st, samples, meta, idx, seg, w


def call_dedup(st, meta, idx, seg, w, C, A=5, T=5, H=4, **replace):
    dev = "cuda"
    t = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    t.update(replace)
    return hip_ops.ext().replay_gather_batch_dedup(
        t["obs"], t["la"], t["lr"], t["act"], t["nsr"], t["gam"], t["hid"],
        torch.from_numpy(idx).to(dev), torch.from_numpy(meta).to(dev),
        torch.from_numpy(seg).to(dev), torch.from_numpy(w).to(dev),
        T, A, 2, H, 2, C)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_kernel_on_hand_built_store(C):
    """C = 4 is the register-transpose path, 2 and 3 the byte-wise one."""
    st, samples, meta, idx, seg, w = hand_store(C)
    A, T, H, hw = 5, 5, 4, 256
    outs = call_dedup(st, meta, idx, seg, w, C)
    torch.cuda.synchronize()
    obs, la, lr, act, nsr, gam, w_rep, hid = [o.cpu().numpy() for o in outs]
    assert obs.shape == (3, T, hw * C) and obs.dtype == np.uint8
    stacks = [stacked_from_frames(st["obs"][s], C) for s in range(2)]
    R = 0
    for b, (slot, seq, burn, learn, fwd, off) in enumerate(samples):
        valid = burn + learn + fwd
        r0 = int(meta[3, b]) - slot * 6 - burn
        for t in range(T):
            if t < valid:
                want = stacks[slot][r0 + t].T          # (hw, C)
                np.testing.assert_array_equal(
                    obs[b, t].reshape(hw, C), want, err_msg=f"b={b} t={t}")
                onehot = np.zeros(A, dtype=np.float32)
                onehot[st["la"][slot, r0 + t]] = 1
                np.testing.assert_array_equal(la[b, t], onehot)
                assert lr[b, t] == st["lr"][slot, r0 + t]
            else:
                assert not obs[b, t].any()
                assert not la[b, t].any() and lr[b, t] == 0
        np.testing.assert_array_equal(
            act[R:R + learn], st["act"][slot, off:off + learn])
        np.testing.assert_array_equal(
            nsr[R:R + learn], st["nsr"][slot, off:off + learn])
        np.testing.assert_array_equal(
            gam[R:R + learn], st["gam"][slot, off:off + learn])
        assert (w_rep[R:R + learn] == w[b]).all()
        np.testing.assert_array_equal(
            hid[:, b], st["hid"][slot * 2 + seq].reshape(2, H))
        R += learn


def test_argument_checks_raise_before_launch():
    C = 4
    st, _, meta, idx, seg, w = hand_store(C)
    obs = torch.from_numpy(st["obs"]).cuda()
    ok = call_dedup(st, meta, idx, seg, w, C, obs=obs)
    assert ok[0].shape == (3, 5, 256 * C)
    with pytest.raises(RuntimeError, match="uint8"):
        call_dedup(st, meta, idx, seg, w, C, obs=obs.to(torch.int32))
    wide = torch.zeros(2, 9, 512, dtype=torch.uint8, device="cuda")
    assert wide[:, :, :256].shape == obs.shape
    with pytest.raises(RuntimeError, match="contiguous"):
        call_dedup(st, meta, idx, seg, w, C, obs=wide[:, :, :256])
    with pytest.raises(RuntimeError, match="GPU"):
        call_dedup(st, meta, idx, seg, w, C, obs=obs.cpu())
    # a store with obs_rows + C frames per slot, or a plain-layout store
    tall = torch.zeros(2, 10, 256, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="obs_rows \\+ C - 1"):
        call_dedup(st, meta, idx, seg, w, C, obs=tall)
    with pytest.raises(RuntimeError, match="obs_rows \\+ C - 1"):
        call_dedup(st, meta, idx, seg, w, C, obs=obs[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="obs_rows \\+ C - 1"):
        call_dedup(st, meta, idx, seg, w, 3, obs=obs)
    with pytest.raises(RuntimeError, match="C must be"):
        call_dedup(st, meta, idx, seg, w, 1, obs=obs[:, :6].contiguous())
    # C = 4 vector path needs H*W % 16 == 0
    odd = torch.zeros(2, 9, 250, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="% 16"):
        call_dedup(st, meta, idx, seg, w, C, obs=odd)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# ingest check
# ---------------------------------------------------------------------------

def test_verify_rejects_a_non_stack_block_and_leaves_the_store():
    from bench import build_synthetic_block
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    c = small_cfg(True)
    assert c.replay_dedup_verify
    replay = GpuReplayBuffer(device="cuda")
    good, prio = make_blocks(EPISODES_8)[0]
    replay.ingest(good, prio)
    torch.cuda.synchronize()
    store0, tree0 = replay.obs_store.clone(), replay.tree.clone()
    ptr0, size0 = replay.block_ptr, len(replay)
    bad = build_synthetic_block(c, np.random.default_rng(0))
    assert not is_frame_stack(bad.obs)
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        replay.ingest(bad, np.ones(replay.spb, dtype=np.float32))
    torch.cuda.synchronize()
    assert torch.equal(replay.obs_store, store0)
    assert torch.equal(replay.tree, tree0)
    assert replay.block_ptr == ptr0 and len(replay) == size0
    # and the buffer still works
    replay.ingest(good, prio)
    assert replay.block_ptr == ptr0 + 1


def test_verify_off_stores_first_stack_and_newest_frames():
    from bench import build_synthetic_block
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    c = small_cfg(True, replay_dedup_verify=False)
    replay = GpuReplayBuffer(device="cuda")
    rng = np.random.default_rng(3)
    slot_blocks = {}
    for s in range(replay.num_blocks):
        blk = build_synthetic_block(c, rng)
        slot_blocks[s] = blk
        replay.ingest(blk, rng.random(replay.spb).astype(np.float32) + 0.5)
    torch.manual_seed(0)
    batch = replay.sample(16)
    torch.cuda.synchronize()
    check_against_blocks(
        batch, slot_blocks, replay,
        obs_of=lambda b: stacked_from_frames(frames_from_stacked(b.obs), 4))


# ---------------------------------------------------------------------------
# train step
# ---------------------------------------------------------------------------

def test_train_step_on_dedup_batches():
    """Three sample -> Learner.train_step -> update_priorities rounds in
    dedup mode (as test_gpu_replay_train_integration).  Loss and priorities
    of the FIRST step equal those of a plain-mode buffer fed the same blocks
    and seed, computed by the same engine before any update (the forward
    and the loss do not depend on the atomically accumulated gradients of
    their own step; later steps differ through the optimiser)."""
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner
    plain, dedup = build_pair(make_blocks(EPISODES_8), batch_size=8)
    c = cfg.get()
    assert c.replay_frame_dedup and c.batch_size == 8
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                    forward_steps=c.forward_steps)
    learner = Learner(None, None, model)
    learner.enable_hip_engine()

    torch.manual_seed(100)
    ref_batch = plain.sample(8)
    ref_loss, ref_prio = learner.engine.train_step(ref_batch)   # no update
    ref_loss, ref_prio = ref_loss.clone(), ref_prio.clone()

    total0 = dedup.total_priority
    for k in range(3):
        torch.manual_seed(100 + k)
        batch = dedup.sample(8)
        if k == 0:
            assert_batches_equal(ref_batch, batch)
        loss, prio = learner.train_step(batch)
        assert torch.isfinite(loss)
        assert torch.isfinite(prio).all()
        if k == 0:
            assert torch.equal(loss, ref_loss)
            assert torch.equal(prio, ref_prio)
        dedup.update_priorities(batch.idxes, prio, batch.old_ptr)
    torch.cuda.synchronize()
    assert dedup.total_priority != total0
    assert np.isfinite(dedup.total_priority)
