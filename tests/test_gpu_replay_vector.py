"""GPU tests of the float row store of the GPU replay (vector observations,
1-D obs_shape): ingest -> sample round trip against numpy slices of the host
blocks, gather_rows_f32_kernel through its binding on hand-built stores, ring
overwrite, ingest dtypes, the wrapper's argument checks, a train step on the
HIP engine and the eager path, and the in-process actor -> replay -> learner
loop on native CartPole.

Everything the gather produces is a copy, so every comparison of gathered
data is exact."""

import functools
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.ops import hip_ops

PRESET = "cartpole_hip_gpu_replay"
# block 40 = 5 sequences of 8, burn-in 8, forward 3: T = 19, obs_rows = 49
SMALL = dict(block_length=40, burn_in_steps=8, learning_steps=8,
             forward_steps=3, buffer_capacity=800, batch_size=16)
T_SEQ, SPB, OBS_ROWS = 19, 5, 49

# episode lengths -> blocks (steps, burn_in[0]):
#   93 -> (40, 0) first of an episode, (40, 8) continuation, (13, 8) truncated:
#         two sequences of 8 and 5 steps
#   1  -> (1, 0);  45 -> (40, 0), (5, 8);  30 -> (30, 0): last sequence 6 steps
#   40 -> (40, 0);  7 -> (7, 0): one sequence shorter than learning_steps
EPISODES = (93, 1, 45, 30, 40, 7)
KINDS = [(40, 0), (40, 8), (13, 8), (1, 0), (40, 0), (5, 8), (30, 0),
         (40, 0), (7, 0)]


def vec_cfg(D=4, A=2, **kw):
    over = dict(SMALL)
    over.update(obs_shape=(D,), action_dim=A)
    over.update(kw)
    return cfg.apply(PRESET, **over)


def fill_obs(block, k):
    """Distinct float32 contents per block, row and column."""
    rows, D = block.obs.shape
    block.obs = (k * 1000.0 + np.arange(rows, dtype=np.float32)[:, None]
                 + np.arange(D, dtype=np.float32)[None, :] / 32.0)
    assert block.obs.dtype == np.float32


@functools.lru_cache(maxsize=None)
def make_blocks(D, A, H=512, episodes=EPISODES, seed=0):
    """((Block, priorities), ...) cut by a real LocalBuffer from episodes of
    the given lengths; built once per argument set and never modified."""
    from dataclasses import asdict
    from r2d2_amd.worker import LocalBuffer
    prev = asdict(cfg.get())
    c = vec_cfg(D, A, hidden_dim=H, mlp_hidden=H)
    lb = LocalBuffer(A)
    cfg.apply(**prev)
    rng = np.random.default_rng(seed)
    out = []
    for steps in episodes:
        lb.reset(rng.normal(size=D).astype(np.float32))
        for t in range(steps):
            a = int(rng.integers(A))
            lb.add(a, 1.0 + 0.1 * float(rng.normal()),
                   rng.normal(size=D).astype(np.float32),
                   rng.normal(size=A).astype(np.float32),
                   (rng.normal(size=(2, H)) * 0.05).astype(np.float32))
            last = t == steps - 1
            if len(lb) == c.block_length or last:
                q = None if last else rng.normal(size=A).astype(np.float32)
                block, prio, _ = lb.finish(q)
                fill_obs(block, len(out) + 1)
                # unused sequence slots keep priority zero
                prio[:block.num_sequences] += 0.05
                out.append((block, prio))
    return tuple(out)


def full_block(c, k, rng):
    """A full block (as bench.build_synthetic_block) with float contents."""
    from bench import build_synthetic_block
    block = build_synthetic_block(c, rng)
    fill_obs(block, k)
    return block


def new_replay(**kw):
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    return GpuReplayBuffer(device="cuda", **kw)


def expected_sample(blk, si):
    """What one sampled sequence must hold, from the host block in numpy."""
    burn = int(blk.burn_in_steps[si])
    learn = int(blk.learning_steps[si])
    fwd = int(blk.forward_steps[si])
    ls = int(blk.learning_steps[:si].astype(np.int64).sum())
    start = int(blk.burn_in_steps[0]) + ls - burn
    L = burn + learn + fwd
    return dict(
        burn=burn, learn=learn, fwd=fwd, L=L,
        obs=blk.obs[start:start + L].astype(np.float32),
        la=blk.last_action[start:start + L].astype(np.float32),
        lr=blk.last_reward[start:start + L],
        action=blk.action[ls:ls + learn].astype(np.int64),
        nsr=blk.n_step_reward[ls:ls + learn],
        gamma=blk.gamma[ls:ls + learn],
        hidden=blk.hidden[si])


def sample_seeded(replay, B, seed):
    """replay.sample(B) with the descent's jitter known: the per-sample
    (idx, weight) the sampler must have drawn, recomputed by the same
    kernel on the same tree."""
    torch.manual_seed(seed)
    jitter = torch.rand(B, device="cuda")
    torch.manual_seed(seed)
    batch = replay.sample(B)
    torch.cuda.synchronize()
    max_leaf = min(replay.blocks_written * replay.spb,
                   replay.num_sequences) - 1
    idx, _, weight = hip_ops.ext().sumtree_sample(
        replay.tree, replay.leaf_offset, replay.num_levels, jitter, B,
        replay.beta, max_leaf)
    torch.cuda.synchronize()
    assert torch.equal(batch.idxes, idx)
    return batch, weight.cpu().numpy()


def check_batch(batch, weight, slot_blocks, replay, D, A):
    """Every field of a sampled batch against the host blocks."""
    B = len(batch.idxes)
    T = replay.T
    assert batch.obs.shape == (B, T, D) and batch.obs.dtype == torch.float32
    assert batch.last_action.shape == (B, T, A)
    assert batch.last_reward.shape == (B, T)
    assert batch.hidden.shape == (2, B, replay.H)
    assert batch.meta_dev is not None and batch.seg_dev is not None
    obs = batch.obs.cpu().numpy()
    la = batch.last_action.cpu().numpy()
    lr = batch.last_reward.cpu().numpy()
    hid = batch.hidden.cpu().numpy()
    act = batch.action.cpu().numpy()
    nsr = batch.n_step_reward.cpu().numpy()
    gam = batch.gamma.cpu().numpy()
    isw = batch.is_weights.cpu().numpy()
    R = int(batch.learning_steps.sum())
    assert act.shape == (R, 1) and nsr.shape == gam.shape == isw.shape == (R,)
    np.testing.assert_array_equal(
        batch.seg_dev.cpu().numpy(),
        np.concatenate([[0], np.cumsum(batch.learning_steps.numpy())]))
    r0 = 0
    for i, s in enumerate(batch.idxes.cpu().numpy()):
        blk = slot_blocks[s // replay.spb]
        si = int(s % replay.spb)
        assert si < blk.num_sequences
        want = expected_sample(blk, si)
        assert int(batch.burn_in_steps[i]) == want["burn"]
        assert int(batch.learning_steps[i]) == want["learn"]
        assert int(batch.forward_steps[i]) == want["fwd"]
        L, learn = want["L"], want["learn"]
        np.testing.assert_array_equal(obs[i, :L], want["obs"])
        np.testing.assert_array_equal(la[i, :L], want["la"])
        np.testing.assert_array_equal(lr[i, :L], want["lr"])
        # rows past the sequence are exactly zero
        assert not obs[i, L:].any() and not la[i, L:].any()
        assert not lr[i, L:].any()
        np.testing.assert_array_equal(act[r0:r0 + learn, 0], want["action"])
        np.testing.assert_array_equal(nsr[r0:r0 + learn], want["nsr"])
        np.testing.assert_array_equal(gam[r0:r0 + learn], want["gamma"])
        np.testing.assert_array_equal(hid[:, i], want["hidden"])
        assert (isw[r0:r0 + learn] == weight[i]).all()
        r0 += learn
    assert r0 == R


# ---------------------------------------------------------------------------
# ingest -> sample round trip
# ---------------------------------------------------------------------------

def test_block_set_has_every_kind():
    blocks = [b for b, _ in make_blocks(4, 2)]
    assert [(b.action.shape[0], int(b.burn_in_steps[0]))
            for b in blocks] == KINDS
    assert blocks[2].num_sequences == 2 < SPB
    assert list(blocks[2].learning_steps) == [8, 5]
    assert list(blocks[6].learning_steps) == [8, 8, 8, 6]


@pytest.mark.parametrize("D,A", [(1, 2), (4, 2), (4, 3), (5, 3), (16, 2),
                                 (17, 3)])
def test_roundtrip(D, A):
    vec_cfg(D, A)
    replay = new_replay()
    assert replay.vector_obs and not replay.frame_dedup
    assert replay.obs_store.shape == (20, OBS_ROWS, D)
    assert replay.obs_store.dtype == torch.float32
    assert replay._pin_obs[0].shape == (OBS_ROWS, D)
    assert replay._pin_obs[0].dtype == torch.float32
    assert (replay.T, replay.spb) == (T_SEQ, SPB)
    slot_blocks = {}
    for k, (block, prio) in enumerate(make_blocks(D, A)):
        slot_blocks[k] = block
        replay.ingest(block, prio)
    torch.cuda.synchronize()
    assert len(replay) == sum(s for s, _ in KINDS)
    seen_padded = seen_partial_burn = seen_short = False
    for seed in range(4):
        batch, weight = sample_seeded(replay, 16, seed)
        check_batch(batch, weight, slot_blocks, replay, D, A)
        valid = (batch.burn_in_steps + batch.learning_steps
                 + batch.forward_steps)
        seen_padded |= bool((valid < T_SEQ).any())
        seen_partial_burn |= bool((batch.burn_in_steps < 8).any())
        seen_short |= bool((batch.learning_steps < 8).any())
    assert seen_padded and seen_partial_burn and seen_short


# ---------------------------------------------------------------------------
# the kernel through its binding, hand-built stores
# ---------------------------------------------------------------------------

NB, HH, AA = 3, 4, 3      # slots, hidden width, actions of the hand store
PAT_F, PAT_I = -7.25, -77


def hand_store(T, D, seed=0):
    """NB slots of T + 3 rows; block_len = T; spb = 2.  Row g of the store
    holds g * 64 + d (exact in float32), so a wrong row or column shows."""
    obs_rows, block_len = T + 3, T
    rng = np.random.default_rng(seed)
    g = np.arange(NB * obs_rows, dtype=np.float32)[:, None]
    obs = (g * 64.0 + np.arange(D, dtype=np.float32)[None, :]).reshape(
        NB, obs_rows, D)
    return dict(
        obs=obs,
        la=rng.integers(0, AA, size=(NB, obs_rows)).astype(np.uint8),
        lr=rng.normal(size=(NB, obs_rows)).astype(np.float32),
        act=rng.integers(0, AA, size=(NB, block_len)).astype(np.uint8),
        nsr=rng.normal(size=(NB, block_len)).astype(np.float32),
        gam=rng.random(size=(NB, block_len)).astype(np.float32),
        hid=rng.normal(size=(NB * 2, 2 * HH)).astype(np.float32))


def hand_samples(B, T, mode, seed=0):
    """meta (5, B), idx, seg, weights.  mode: 'full' every sample T rows,
    'one' every sample one row, 'mixed' lengths 1..T."""
    rng = np.random.default_rng(seed + 17)
    obs_rows = T + 3
    meta = np.zeros((5, B), dtype=np.int32)
    idx = np.zeros(B, dtype=np.int64)
    for b in range(B):
        valid = {"full": T, "one": 1}.get(mode) or int(rng.integers(1, T + 1))
        burn = int(rng.integers(0, valid))            # learn >= 1
        fwd = int(rng.integers(0, valid - burn))
        learn = valid - burn - fwd
        slot = int(rng.integers(NB))
        row0 = int(rng.integers(0, obs_rows - valid + 1))
        off = int(rng.integers(0, T - learn + 1))
        meta[:, b] = (burn, learn, fwd, slot * obs_rows + row0 + burn, off)
        idx[b] = slot * 2 + int(rng.integers(2))
    seg = np.concatenate([[0], np.cumsum(meta[1])]).astype(np.int32)
    w = (rng.random(B) + 0.25).astype(np.float32)
    return meta, idx, seg, w


def out_buffers(B, T, D, A=AA, H=HH, pad=64):
    """The eight outputs as views `pad` elements inside pattern-filled
    backing tensors.  pad = 64 keeps the views 256-byte aligned."""
    shapes = [(B, T, D), (B, T, A), (B, T), (B * T,), (B * T,), (B * T,),
              (B * T,), (2, B, H)]
    backs, views = [], []
    for k, shp in enumerate(shapes):
        n = int(np.prod(shp))
        if k == 3:
            back = torch.full((n + 2 * pad,), PAT_I, dtype=torch.int64,
                              device="cuda")
        else:
            back = torch.full((n + 2 * pad,), PAT_F, dtype=torch.float32,
                              device="cuda")
        backs.append(back)
        views.append(back[pad:pad + n].view(shp))
    return backs, views


def guards_intact(backs, pad=64):
    for k, back in enumerate(backs):
        pat = PAT_I if k == 3 else PAT_F
        if not (bool((back[:pad] == pat).all())
                and bool((back[-pad:] == pat).all())):
            return False
    return True


def untouched(backs):
    return all(bool((back == (PAT_I if k == 3 else PAT_F)).all())
               for k, back in enumerate(backs))


def call_vec(st, meta, idx, seg, w, T, A=AA, H=HH, max_learn=None, out=None,
             **replace):
    t = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    t.update(idx=torch.from_numpy(idx).cuda(),
             meta=torch.from_numpy(meta).cuda(),
             seg=torch.from_numpy(seg).cuda(), w=torch.from_numpy(w).cuda())
    t.update(replace)
    return hip_ops.ext().replay_gather_batch_vec(
        t["obs"], t["la"], t["lr"], t["act"], t["nsr"], t["gam"], t["hid"],
        t["idx"], t["meta"], t["seg"], t["w"], T, A,
        T if max_learn is None else max_learn, H, 2, out=out)


def expected_outputs(st, meta, idx, seg, w, T, D, dead=()):
    """numpy reference of the eight outputs; samples in `dead` pad as if
    valid = 0 (obs / la / lr only: the flat arrays do not read obs_start)."""
    B = meta.shape[1]
    obs_rows = T + 3
    obs = np.zeros((B, T, D), np.float32)
    la = np.zeros((B, T, AA), np.float32)
    lr = np.zeros((B, T), np.float32)
    R = int(seg[-1])
    act = np.zeros(R, np.int64)
    nsr, gam, wr = (np.zeros(R, np.float32) for _ in range(3))
    hid = np.zeros((2, B, HH), np.float32)
    flat = {k: st[k].reshape(-1) for k in ("la", "lr")}
    rows = st["obs"].reshape(-1, D)
    for b in range(B):
        burn, learn, fwd, start, off = (int(v) for v in meta[:, b])
        valid = burn + learn + fwd
        if b not in dead:
            g0 = start - burn
            obs[b, :valid] = rows[g0:g0 + valid]
            la[b, np.arange(valid), flat["la"][g0:g0 + valid]] = 1.0
            lr[b, :valid] = flat["lr"][g0:g0 + valid]
        slot = int(idx[b]) // 2
        s0 = int(seg[b])
        act[s0:s0 + learn] = st["act"][slot, off:off + learn]
        nsr[s0:s0 + learn] = st["nsr"][slot, off:off + learn]
        gam[s0:s0 + learn] = st["gam"][slot, off:off + learn]
        wr[s0:s0 + learn] = w[b]
        hid[:, b] = st["hid"][int(idx[b])].reshape(2, HH)
    assert obs_rows * NB == rows.shape[0]
    return obs, la, lr, act, nsr, gam, wr, hid


def assert_outputs(outs, want, R):
    got = [o.cpu().numpy() for o in outs]
    names = ("obs", "la", "lr", "act", "nsr", "gam", "w", "hid")
    for k, (g, e) in enumerate(zip(got, want)):
        if 3 <= k <= 6:
            g = g[:R]          # the flat arrays are written up to seg[B]
        assert g.shape == e.shape and g.dtype == e.dtype, names[k]
        np.testing.assert_array_equal(g, e, err_msg=names[k])


@pytest.mark.parametrize("T", [1, 2, 19])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_kernel_on_hand_built_store(B, T):
    """D = 4 takes the 16-byte path, D = 5 the 4-byte one; D = 4 written
    through a view 4 bytes off a 16-byte boundary takes the 4-byte one too."""
    for D in (4, 5):
        st = hand_store(T, D)
        for mode in ("full", "one", "mixed"):
            meta, idx, seg, w = hand_samples(B, T, mode, seed=B * 31 + T)
            R = int(seg[-1])
            want = expected_outputs(st, meta, idx, seg, w, T, D)
            pads = (64, 1) if D == 4 else (64,)
            for pad in pads:
                backs, views = out_buffers(B, T, D, pad=pad)
                outs = call_vec(st, meta, idx, seg, w, T, out=views)
                torch.cuda.synchronize()
                for o, v in zip(outs, views):
                    assert o.data_ptr() == v.data_ptr() and o.shape == v.shape
                assert_outputs(outs, want, R)
                assert guards_intact(backs, pad), (D, mode, pad)
                # the flat arrays past seg[B] are not written either
                for k in (3, 4, 5, 6):
                    pat = PAT_I if k == 3 else PAT_F
                    assert bool((views[k][R:] == pat).all())
            # and with outputs the wrapper allocates itself
            outs = call_vec(st, meta, idx, seg, w, T)
            torch.cuda.synchronize()
            assert outs[0].shape == (B, T, D)
            assert outs[0].dtype == torch.float32
            assert_outputs(outs, want, R)


@pytest.mark.parametrize("D", [4, 5])
def test_metadata_outside_the_store_pads_that_sample(D):
    """obs_start before row 0 or past the last row is an ordinary input:
    that sample's obs / last_action / last_reward are zero, its neighbours
    and everything outside the views intact."""
    B, T = 5, 19
    st = hand_store(T, D)
    total_rows = NB * (T + 3)
    meta, idx, seg, w = hand_samples(B, T, "mixed", seed=3)
    R = int(seg[-1])
    for b, start in ((0, None), (2, "before"), (4, "past"), (1, "min"),
                     (3, "max")):
        m = meta.copy()
        burn = int(m[0, b])
        valid = int(m[0, b] + m[1, b] + m[2, b])
        m[3, b] = {None: m[3, b], "before": burn - 1,
                   "past": total_rows - valid + 1 + burn,
                   "min": -2 ** 31, "max": 2 ** 31 - 1}[start]
        dead = () if start is None else (b,)
        want = expected_outputs(st, m, idx, seg, w, T, D, dead=dead)
        if dead:
            assert not want[0][b].any() and want[0][(b + 1) % B].any()
        backs, views = out_buffers(B, T, D)
        outs = call_vec(st, m, idx, seg, w, T, out=views)
        torch.cuda.synchronize()
        assert_outputs(outs, want, R)
        assert guards_intact(backs)
    # the last row of the store itself is still inside
    m = meta.copy()
    m[:, 0] = (0, 1, 0, total_rows - 1, 0)
    seg1 = np.concatenate([[0], np.cumsum(m[1])]).astype(np.int32)
    outs = call_vec(st, m, idx, seg1, w, T)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs[0][0, 0].cpu().numpy(),
                                  st["obs"].reshape(-1, D)[-1])


def test_vector_and_scalar_paths_agree():
    """The same logical data at D = 4 (16-byte moves) and at D = 5 with a
    dummy fifth column (4-byte moves)."""
    B, T = 64, 19
    st4 = hand_store(T, 4)
    st5 = dict(st4)
    st5["obs"] = np.concatenate(
        [st4["obs"], np.full(st4["obs"].shape[:2] + (1,), 0.5, np.float32)],
        axis=2)
    meta, idx, seg, w = hand_samples(B, T, "mixed", seed=9)
    o4 = call_vec(st4, meta, idx, seg, w, T)
    o5 = call_vec(st5, meta, idx, seg, w, T)
    torch.cuda.synchronize()
    assert torch.equal(o5[0][..., :4], o4[0])
    valid = torch.from_numpy(meta[:3].sum(0)).cuda()
    inside = torch.arange(T, device="cuda")[None, :] < valid[:, None]
    assert torch.equal(o5[0][..., 4], inside.float() * 0.5)
    for a, b in zip(o4[1:], o5[1:]):
        assert torch.equal(a[:int(seg[-1])] if a.dim() == 1 else a,
                           b[:int(seg[-1])] if b.dim() == 1 else b)


# ---------------------------------------------------------------------------
# ring overwrite
# ---------------------------------------------------------------------------

def test_ring_overwrite_and_stale_priorities():
    c = vec_cfg(4, 2)
    replay = new_replay()
    nb = replay.num_blocks
    assert nb == 20
    rng = np.random.default_rng(5)
    slot_blocks = {}

    def ingest(k):
        block = full_block(c, k + 1, rng)
        slot_blocks[k % nb] = block
        replay.ingest(block, rng.random(SPB).astype(np.float32) + 0.5)

    for k in range(nb - 2):
        ingest(k)
    old_ptr = replay.block_ptr
    assert old_ptr == nb - 2
    for k in range(nb - 2, nb + 3):
        ingest(k)
    torch.cuda.synchronize()
    assert replay.block_ptr == 3 and len(replay) == replay.capacity
    # samples never show overwritten rows: every row is the slot's current
    # block (the contents carry the block number)
    for seed in range(4):
        batch, weight = sample_seeded(replay, 16, seed)
        check_batch(batch, weight, slot_blocks, replay, 4, 2)
    # priorities computed on a batch sampled at old_ptr: slots nb-2, nb-1, 0,
    # 1, 2 were overwritten since and keep their leaves
    lo = replay.leaf_offset
    before = replay.tree[lo:lo + replay.num_sequences].clone()
    idxes = torch.arange(replay.num_sequences, device="cuda")
    replay.update_priorities(idxes, torch.full((replay.num_sequences,), 9.0,
                                               device="cuda"), old_ptr)
    torch.cuda.synchronize()
    after = replay.tree[lo:lo + replay.num_sequences]
    slot = idxes // SPB
    stale = (slot >= old_ptr) | (slot < replay.block_ptr)
    assert int(stale.sum()) == 5 * SPB
    assert torch.equal(after[stale], before[stale])
    fresh = after[~stale]
    assert bool((fresh == fresh[0]).all()) and float(fresh[0]) > 5.0
    assert not bool((before[~stale] == fresh[0]).any())
    assert np.isfinite(replay.total_priority)


# ---------------------------------------------------------------------------
# ingest dtypes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_ingest_casts_to_float32(dtype):
    from bench import build_synthetic_block
    c = vec_cfg(4, 2)
    replay = new_replay()
    rng = np.random.default_rng(0)
    block = build_synthetic_block(c, rng)
    assert block.obs.dtype == np.uint8 and block.obs.shape == (OBS_ROWS, 4)
    if dtype is np.float64:
        block.obs = block.obs.astype(np.float64) / 7.0
    replay.ingest(block, np.ones(SPB, dtype=np.float32))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(replay.obs_store[0].cpu().numpy(),
                                  block.obs.astype(np.float32))
    batch, weight = sample_seeded(replay, 8, 0)
    block.obs = block.obs.astype(np.float32)
    check_batch(batch, weight, {0: block}, replay, 4, 2)


def test_wrong_width_raises_before_the_store_is_touched():
    c = vec_cfg(4, 2)
    replay = new_replay()
    rng = np.random.default_rng(0)
    replay.ingest(full_block(c, 1, rng), np.ones(SPB, dtype=np.float32))
    torch.cuda.synchronize()
    store0, tree0 = replay.obs_store.clone(), replay.tree.clone()
    state0 = (replay.block_ptr, len(replay), replay._pin_cursor,
              list(replay._pin_used))
    bad = full_block(c, 2, rng)
    bad.obs = np.zeros((OBS_ROWS, 5), dtype=np.float32)
    with pytest.raises(AssertionError):
        replay.ingest(bad, np.ones(SPB, dtype=np.float32))
    torch.cuda.synchronize()
    assert torch.equal(replay.obs_store, store0)
    assert torch.equal(replay.tree, tree0)
    assert (replay.block_ptr, len(replay), replay._pin_cursor,
            list(replay._pin_used)) == state0


def test_frame_dedup_with_vector_observations_raises():
    with pytest.raises(ValueError, match="replay_frame_dedup"):
        vec_cfg(4, 2, replay_frame_dedup=True)


# ---------------------------------------------------------------------------
# the wrapper's argument checks
# ---------------------------------------------------------------------------

def test_wrapper_rejections_leave_the_outputs_untouched():
    B, T, D = 5, 19, 4
    st = hand_store(T, D)
    meta, idx, seg, w = hand_samples(B, T, "mixed", seed=1)
    backs, views = out_buffers(B, T, D)
    obs = torch.from_numpy(st["obs"]).cuda()

    def rejected(match, samples=(meta, idx, seg, w), **kw):
        with pytest.raises(RuntimeError, match=match):
            call_vec(st, *samples, T, out=views, **kw)
        torch.cuda.synchronize()
        assert untouched(backs), match

    rejected("float32", obs=obs.double())
    rejected("GPU", obs=obs.cpu())
    wide = torch.zeros(NB, T + 3, 2 * D, device="cuda")
    assert wide[:, :, :D].shape == obs.shape
    rejected("contiguous", obs=wide[:, :, :D])

    def sized(n):
        return (np.zeros((5, n), np.int32), np.zeros(n, np.int64),
                np.zeros(n + 1, np.int32), np.ones(n, np.float32))

    rejected("B must be", samples=sized(0))
    rejected("B must be", samples=sized(1025))
    rejected("A must be", A=257)
    # outputs of another shape are rejected too, before any launch
    with pytest.raises(RuntimeError, match="out\\["):
        call_vec(st, meta, idx, seg, w, T, out=views, A=AA + 1)
    torch.cuda.synchronize()
    assert untouched(backs)
    # the same arguments without the fault run
    outs = call_vec(st, meta, idx, seg, w, T, out=views)
    torch.cuda.synchronize()
    assert_outputs(outs, expected_outputs(st, meta, idx, seg, w, T, D),
                   int(seg[-1]))


# ---------------------------------------------------------------------------
# engine integration
# ---------------------------------------------------------------------------

def filled_replay(B, H=512, **kw):
    c = vec_cfg(4, 2, batch_size=B, hidden_dim=H, mlp_hidden=H, **kw)
    replay = new_replay()
    slot_blocks = {}
    for k, (block, prio) in enumerate(make_blocks(4, 2, H)):
        slot_blocks[k] = block
        replay.ingest(block, prio)
    torch.cuda.synchronize()
    return c, replay, slot_blocks


def make_learner(c, seed=0):
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner
    torch.manual_seed(seed)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="mlp",
                    forward_steps=c.forward_steps, mlp_hidden=c.mlp_hidden)
    learner = Learner(None, None, model)
    learner.enable_hip_engine()
    return learner


def host_batch(batch, weight, slot_blocks, replay):
    """The sampled batch rebuilt on the host from the blocks."""
    from r2d2_amd.worker import TrainingBatch
    B, T = len(batch.idxes), replay.T
    D, A, H = replay.obs_shape[0], replay.A, replay.H
    obs = np.zeros((B, T, D), np.float32)
    la = np.zeros((B, T, A), np.float32)
    lr = np.zeros((B, T), np.float32)
    hid = np.zeros((2, B, H), np.float32)
    act, nsr, gam, isw, burn, learn, fwd = ([] for _ in range(7))
    for i, s in enumerate(batch.idxes.cpu().numpy()):
        e = expected_sample(slot_blocks[s // replay.spb], int(s % replay.spb))
        L = e["L"]
        obs[i, :L], la[i, :L], lr[i, :L] = e["obs"], e["la"], e["lr"]
        hid[:, i] = e["hidden"]
        act.append(e["action"]); nsr.append(e["nsr"]); gam.append(e["gamma"])
        isw.append(np.full(e["learn"], weight[i], np.float32))
        burn.append(e["burn"]); learn.append(e["learn"]); fwd.append(e["fwd"])
    cat = lambda xs: torch.from_numpy(np.concatenate(xs))
    return TrainingBatch(
        obs=torch.from_numpy(obs), last_action=torch.from_numpy(la),
        last_reward=torch.from_numpy(lr), hidden=torch.from_numpy(hid),
        action=cat(act).unsqueeze(1), n_step_reward=cat(nsr), gamma=cat(gam),
        burn_in_steps=torch.tensor(burn), learning_steps=torch.tensor(learn),
        forward_steps=torch.tensor(fwd), idxes=batch.idxes.cpu().numpy(),
        is_weights=cat(isw), old_ptr=batch.old_ptr, env_steps=batch.env_steps)


def test_engine_step_equals_the_host_built_batch():
    """Loss and priorities of the sampled batch (positions built on the
    device from meta_dev) against the same batch rebuilt on the host from
    the blocks and moved with TrainingBatch.to.  The difference is bounded by
    two runs of the host-built batch against each other, which is zero where
    the engine is run-to-run reproducible: bit equality."""
    B = 8
    c, replay, slot_blocks = filled_replay(B)
    learner = make_learner(c)
    assert learner.engine is not None and learner.engine.mlp
    batch, weight = sample_seeded(replay, B, 0)
    assert batch.meta_dev is not None
    assert batch.obs.shape == (B, T_SEQ, 4)
    loss_d, prio_d = (t.clone() for t in learner.engine.train_step(batch))
    runs = []
    for _ in range(2):
        hb = host_batch(batch, weight, slot_blocks, replay).to(
            torch.device("cuda"), non_blocking=False)
        assert getattr(hb, "meta_dev", None) is None
        loss_h, prio_h = learner.engine.train_step(hb)
        runs.append((loss_h.clone(), prio_h.clone()))
    (l1, p1), (l2, p2) = runs
    dl = float((loss_d - l1).abs())
    dp = float((prio_d - p1).abs().max())
    bl = float((l1 - l2).abs())
    bp = float((p1 - p2).abs().max())
    print(f"loss device {float(loss_d):.9g} host {float(l1):.9g} "
          f"|diff| {dl:.3e} (host run-to-run {bl:.3e}); priorities max |diff| "
          f"{dp:.3e} (host run-to-run {bp:.3e})")
    assert torch.isfinite(loss_d) and prio_d.shape == (B,)
    assert dl <= bl and dp <= bp, (dl, bl, dp, bp)


def test_twenty_updates_reduce_the_loss_on_a_fixed_replay():
    """The loss of one held batch before and after 20 sample -> train ->
    update-priorities rounds on a replay that no longer changes."""
    B = 8
    c, replay, _ = filled_replay(B, lr=1e-3)
    learner = make_learner(c)
    held, _ = sample_seeded(replay, B, 123)
    before = float(learner.engine.train_step(held)[0])
    total0 = replay.total_priority
    for k in range(20):
        torch.manual_seed(k)
        batch = replay.sample(B)
        loss, prio = learner.train_step(batch)
        assert torch.isfinite(loss) and torch.isfinite(prio).all()
        replay.update_priorities(batch.idxes, prio, batch.old_ptr)
    after = float(learner.engine.train_step(held)[0])
    torch.cuda.synchronize()
    print(f"held-batch loss before {before:.6f} after 20 updates {after:.6f}")
    assert after < before, (before, after)
    assert np.isfinite(replay.total_priority)
    assert replay.total_priority != total0


def test_eager_step_at_width_128():
    """Widths the engine does not serve sample from the vector store and
    train through the eager train_step with the fused loss kernels."""
    B = 8
    c, replay, slot_blocks = filled_replay(B, H=128)
    assert replay.hid_store.shape == (20 * SPB, 256)
    learner = make_learner(c)
    assert learner.engine is None and learner.hip_engine
    batch, weight = sample_seeded(replay, B, 0)
    check_batch(batch, weight, slot_blocks, replay, 4, 2)
    loss, prio = learner.train_step(batch)
    assert torch.is_tensor(prio) and prio.is_cuda and prio.shape == (B,)
    assert torch.isfinite(loss) and torch.isfinite(prio).all()
    replay.update_priorities(batch.idxes, prio, batch.old_ptr)
    torch.cuda.synchronize()
    assert np.isfinite(replay.total_priority)


# ---------------------------------------------------------------------------
# actor -> replay -> learner in one process
# ---------------------------------------------------------------------------

def test_in_process_topology_on_cartpole():
    from r2d2_amd.train import epsilon_ladder
    from r2d2_amd.worker import VectorActor
    B, E = 8, 4
    c = cfg.apply(PRESET, num_actors=E, batch_size=B, buffer_capacity=2000)
    assert c.gpu_replay and c.vector_actors and c.obs_shape == (4,)
    learner = make_learner(c)
    assert learner.engine is not None and learner.weight_bus is not None
    sq = queue.Queue()
    actor = VectorActor(epsilon_ladder(E), learner.shared_model, [sq],
                        device="cuda", seed=3,
                        weight_bus=learner.weight_bus)
    assert actor.hip_inf is not None
    assert actor.run(stop_after_steps=400) >= 400
    replay = new_replay()
    assert replay.vector_obs
    n = 0
    while not sq.empty():
        block, prio, _ = sq.get()
        assert block.obs.dtype == np.float32 and block.obs.shape[1:] == (4,)
        replay.ingest(block, prio)
        n += 1
    torch.cuda.synchronize()
    assert n >= 4 and len(replay) >= 8 * B
    totals = [replay.total_priority]
    for _ in range(3):
        batch = replay.sample(B)
        assert batch.obs.shape == (B, c.seq_len, 4)
        assert bool((batch.obs != batch.obs.round()).any())
        loss, prio = learner.train_step(batch)
        assert torch.isfinite(loss) and torch.isfinite(prio).all()
        replay.update_priorities(batch.idxes, prio, batch.old_ptr)
        torch.cuda.synchronize()
        totals.append(replay.total_priority)
    assert np.isfinite(totals).all()
    assert len(set(totals)) > 1, totals


# ---------------------------------------------------------------------------
# the frame gather is as it was
# ---------------------------------------------------------------------------

def test_frame_gather_regression_guard():
    """replay_gather_batch on a (4, 84, 84) store against numpy."""
    FB, obs_rows, T, A, H = 4 * 84 * 84, 6, 5, 5, 4
    rng = np.random.default_rng(0)
    st = dict(
        obs=rng.integers(0, 256, size=(2, obs_rows, FB)).astype(np.uint8),
        la=rng.integers(0, A, size=(2, obs_rows)).astype(np.uint8),
        lr=rng.normal(size=(2, obs_rows)).astype(np.float32),
        act=rng.integers(0, A, size=(2, 4)).astype(np.uint8),
        nsr=rng.normal(size=(2, 4)).astype(np.float32),
        gam=rng.random(size=(2, 4)).astype(np.float32),
        hid=rng.normal(size=(4, 2 * H)).astype(np.float32))
    # (slot, seq, burn, learn, fwd, learn_off)
    samples = [(0, 0, 1, 2, 2, 0), (1, 1, 1, 2, 1, 2), (1, 0, 0, 1, 1, 0)]
    meta = np.zeros((5, 3), dtype=np.int32)
    idx = np.zeros(3, dtype=np.int64)
    for b, (slot, seq, burn, learn, fwd, off) in enumerate(samples):
        meta[:, b] = (burn, learn, fwd, slot * obs_rows + burn + off, off)
        idx[b] = slot * 2 + seq
    seg = np.concatenate([[0], np.cumsum(meta[1])]).astype(np.int32)
    w = np.array([0.5, 1.0, 0.25], dtype=np.float32)
    t = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    outs = hip_ops.ext().replay_gather_batch(
        t["obs"], t["la"], t["lr"], t["act"], t["nsr"], t["gam"], t["hid"],
        torch.from_numpy(idx).cuda(), torch.from_numpy(meta).cuda(),
        torch.from_numpy(seg).cuda(), torch.from_numpy(w).cuda(),
        T, A, 2, H, 2)
    torch.cuda.synchronize()
    obs, la, lr, act, nsr, gam, w_rep, hid = [o.cpu().numpy() for o in outs]
    assert obs.shape == (3, T, FB) and obs.dtype == np.uint8
    rows = st["obs"].reshape(-1, FB)
    r0 = 0
    for b, (slot, seq, burn, learn, fwd, off) in enumerate(samples):
        valid = burn + learn + fwd
        g0 = int(meta[3, b]) - burn
        np.testing.assert_array_equal(obs[b, :valid], rows[g0:g0 + valid])
        assert not obs[b, valid:].any()
        onehot = np.zeros((valid, A), np.float32)
        onehot[np.arange(valid), st["la"].reshape(-1)[g0:g0 + valid]] = 1
        np.testing.assert_array_equal(la[b, :valid], onehot)
        np.testing.assert_array_equal(lr[b, :valid],
                                      st["lr"].reshape(-1)[g0:g0 + valid])
        assert not la[b, valid:].any() and not lr[b, valid:].any()
        np.testing.assert_array_equal(act[r0:r0 + learn],
                                      st["act"][slot, off:off + learn])
        np.testing.assert_array_equal(nsr[r0:r0 + learn],
                                      st["nsr"][slot, off:off + learn])
        np.testing.assert_array_equal(gam[r0:r0 + learn],
                                      st["gam"][slot, off:off + learn])
        assert (w_rep[r0:r0 + learn] == w[b]).all()
        np.testing.assert_array_equal(hid[:, b],
                                      st["hid"][slot * 2 + seq].reshape(2, H))
        r0 += learn
