"""GPU end-to-end at the reference's observation shape, ONE 84x84 frame per
step (preset mspacman_reference): the HIP engine vs the eager fp32 golden
learner, the gather-kernel repack, K15 inference, the WeightBus, the GPU
replay loop and the VectorActor fast path — test_hip_engine.py's checks and
thresholds at one input channel."""

import copy
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner

SMALL = dict(batch_size=8, burn_in_steps=8, learning_steps=8, forward_steps=3,
             amp=False, dtype="fp32")


def make_learners(seed=0, **kw):
    c = cfg.apply("mspacman_reference", **{**SMALL, **kw})
    assert tuple(c.obs_shape) == (1, 84, 84)
    torch.manual_seed(seed)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                    forward_steps=c.forward_steps)
    eager = Learner(None, None, model)
    hip = Learner(None, None, model)
    hip.enable_hip_engine()
    return c, eager, hip


def cos(a, b):
    a, b = a.flatten().float(), b.flatten().float()
    denom = a.norm() * b.norm()
    if denom == 0:
        return 1.0
    return float((a @ b) / denom)


def test_engine_is_built_for_single_frame():
    c, eager, hip = make_learners()
    assert hip.engine is not None
    assert hip.engine.C == 1
    assert hip.engine.online.enc_pack.w1t.shape == (32, 64)
    assert eager.engine is None


def test_engine_matches_eager_loss_and_grads():
    c, eager, hip = make_learners()
    from bench import build_batch
    dev = torch.device("cuda")
    batch_a = build_batch(c, dev, seed=5)
    assert batch_a.obs.shape[2:] == (1, 84, 84)
    batch_b = copy.deepcopy(batch_a)
    # the same frames channels-innermost, as the GPU replay hands them over
    # (same seed -> same byte stream; with one channel CHW and HWC frames
    # are the same bytes)
    batch_c = build_batch(c, dev, seed=5, hwc=True)
    assert batch_c.obs.shape[2:] == (84, 84, 1)
    assert torch.equal(batch_c.obs.permute(0, 1, 4, 2, 3), batch_a.obs)

    loss_e, prio_e = eager.train_step(batch_a)
    grads_e = {n: p.grad.clone() for n, p in eager.online_net.named_parameters()}

    # engine-only call (no optimizer step) so grads compare at equal weights
    loss_h, prio_h = hip.engine.train_step(batch_b)
    grads_h = {n: p.grad.clone() for n, p in hip.online_net.named_parameters()}

    lf_e, lf_h = float(loss_e), float(loss_h)
    assert abs(lf_e - lf_h) < 0.05 * max(1.0, abs(lf_e)), (lf_e, lf_h)

    pe = prio_e if isinstance(prio_e, np.ndarray) else prio_e.cpu().numpy()
    np.testing.assert_allclose(prio_h.cpu().numpy(), pe, rtol=0.1, atol=0.05)

    assert "encoder.conv1.weight" in grads_e and "encoder.conv1.bias" in grads_e
    assert grads_h["encoder.conv1.weight"].shape == (32, 1, 8, 8)
    bad = []
    for n, ge in grads_e.items():
        gh = grads_h[n]
        cs = cos(ge, gh)
        rel = float((gh.float() - ge.float()).norm() / (ge.float().norm() + 1e-8))
        if cs < 0.98 and rel > 0.1:
            bad.append((n, cs, rel))
    assert not bad, bad
    for n in ("encoder.conv1.weight", "encoder.conv1.bias"):
        assert float(grads_e[n].norm()) > 0, n

    # NCHW and HWC deliveries of the same frames are the same forward (the
    # forward has no atomics, so the loss is reproduced exactly)
    loss_hwc, prio_hwc = hip.engine.train_step(batch_c)
    assert torch.equal(loss_hwc, loss_h), (float(loss_hwc), lf_h)
    assert torch.equal(prio_hwc, prio_h)


def test_fast_refresh_matches_python_repack():
    from r2d2_amd.ops.engine import _NetPack, _pack_items, _item_get

    c, eager, hip = make_learners(seed=7)
    engine = hip.engine
    with torch.no_grad():
        engine.flat_param.add_(
            torch.randn_like(engine.flat_param) * 0.01)
    engine.refresh_online()   # fast path (maps)
    ref = _NetPack(engine.online_net, engine.device, engine.A,
                   with_bwd=True)   # python repack of the same weights
    fast_items = {n: _item_get(h, a, k)
                  for n, h, a, k in _pack_items(engine.online)}
    ref_items = {n: _item_get(h, a, k)
                 for n, h, a, k in _pack_items(ref)}
    assert set(fast_items) == set(ref_items)
    assert fast_items["enc_pack.w1t"].shape == (32, 64)
    for n, t in fast_items.items():
        assert torch.equal(t, ref_items[n].view(t.shape)), n


def test_hip_inference_matches_eager():
    """K15 single-step inference vs the eager Network.forward; E = 5 gives
    M = 2000 conv1 rows, a partial last tile."""
    from r2d2_amd.models.network import AgentState
    from r2d2_amd.ops.engine import HipInference

    c = cfg.apply("mspacman_reference")
    torch.manual_seed(3)
    net = Network(c.action_dim, c.obs_shape, 512, encoder="nature",
                  forward_steps=c.forward_steps).cuda().eval()
    E = 5
    obs = torch.randint(0, 256, (E, 1, 84, 84), device="cuda",
                        dtype=torch.uint8)
    la = torch.zeros(E, c.action_dim, device="cuda")
    la[torch.arange(E), torch.randint(0, c.action_dim, (E,))] = 1.0
    lr = torch.randn(E, 1, device="cuda") * 0.1
    h = torch.randn(1, E, 512, device="cuda") * 0.1
    ccell = torch.randn(1, E, 512, device="cuda") * 0.1

    inf = HipInference(net, "cuda")
    q, (h1, c1) = inf.forward(obs, la, lr, (h, ccell))

    state = AgentState.__new__(AgentState)
    state.obs = obs
    state.action_dim = c.action_dim
    state.last_action = la
    state.last_reward = lr
    state.hidden_state = (h, ccell)
    with torch.no_grad():
        q_ref, (h_ref, c_ref) = net(state)

    scale = float(q_ref.abs().max())
    assert torch.allclose(q.float(), q_ref, atol=0.05 * max(1.0, scale)), \
        float((q.float() - q_ref).abs().max())
    assert torch.allclose(h1, h_ref, atol=0.03), \
        float((h1 - h_ref).abs().max())


def test_weight_bus_roundtrip():
    from r2d2_amd.parallel.weight_bus import WeightBus, pack_tensors
    from r2d2_amd.ops.engine import HipInference

    c, eager, hip = make_learners(seed=3)
    engine = hip.engine
    assert hip.weight_bus is not None
    bus = WeightBus(pack_tensors(engine.target), "cuda")

    torch.manual_seed(99)
    other = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                    encoder=c.encoder, forward_steps=c.forward_steps,
                    mlp_hidden=c.mlp_hidden).cuda()
    inf = HipInference(other, torch.device("cuda"), c)
    assert inf.pack.enc_pack.w1t.shape == (32, 64)

    before = {n: t.clone() for n, t in pack_tensors(inf.pack).items()}
    bus.publish(engine.online)
    ver = bus.pull_into(inf.pack, 0)
    assert ver == 2   # seqlock: odd while publishing, even when stable

    src = pack_tensors(engine.online)
    dst = pack_tensors(inf.pack)
    changed = 0
    for name, t in dst.items():
        assert torch.equal(t, src[name].view(t.shape)), name
        if not torch.equal(t, before[name]):
            changed += 1
    assert changed > 0
    assert bus.pull_into(inf.pack, ver) == ver


def test_gpu_replay_loop_single_frame():
    """Ingest -> sample -> HIP train_step -> on-device priority update with
    7056-byte frames; gathered frames are the source rows byte for byte."""
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    from bench import build_synthetic_block

    c, eager, hip = make_learners(seed=0, block_length=40,
                                  buffer_capacity=8 * 40)
    rng = np.random.default_rng(2)
    replay = GpuReplayBuffer(device="cuda", capacity=8 * 40)
    assert replay.num_blocks == 8 and replay.frame_bytes == 84 * 84
    blocks = []
    for _ in range(replay.num_blocks):
        blk = build_synthetic_block(c, rng)
        blocks.append(blk)
        replay.ingest(blk, rng.random(replay.spb).astype(np.float32) + 0.5)
    batch = replay.sample()
    torch.cuda.synchronize()
    B, T = 8, c.seq_len
    assert batch.obs.shape == (B, T, 84, 84, 1) and batch.obs.dtype == torch.uint8
    idx = batch.idxes.cpu().numpy()
    for i in range(B):
        bi, si = idx[i] // replay.spb, idx[i] % replay.spb
        blk = blocks[bi]
        burn, learn, fwd = (int(batch.burn_in_steps[i]),
                            int(batch.learning_steps[i]),
                            int(batch.forward_steps[i]))
        L = burn + learn + fwd
        ls = int(blk.learning_steps[:si].sum())
        r0 = int(blk.burn_in_steps[0]) + ls - burn
        got = batch.obs[i].cpu().numpy().reshape(T, -1)
        want = blk.obs[r0:r0 + L].reshape(L, -1)   # C = 1: CHW bytes == HWC
        np.testing.assert_array_equal(got[:L], want)
        assert (got[L:] == 0).all()

    total0 = replay.total_priority
    loss, prio = hip.train_step(batch)
    assert torch.isfinite(loss)
    replay.update_priorities(batch.idxes, prio, batch.old_ptr)
    torch.cuda.synchronize()
    assert np.isfinite(replay.total_priority)
    assert replay.total_priority != total0


def test_vector_actor_gpu_hip_inference_single_frame():
    from r2d2_amd.train import epsilon_ladder
    from r2d2_amd.worker import VectorActor

    # episodes capped at 20 steps so every env finishes a block within the
    # 30 ticks that 120 env steps over 4 envs give
    c = cfg.apply("mspacman_reference", num_actors=4, block_length=40,
                  burn_in_steps=8, learning_steps=8, forward_steps=3,
                  actor_update_interval=64, max_episode_steps=20)
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                    forward_steps=c.forward_steps)
    sq = queue.Queue()
    va = VectorActor(epsilon_ladder(4), model, [sq], device="cuda", seed=4)
    assert va.hip_inf is not None, "K15 path must be active on GPU"
    total = va.run(stop_after_steps=120)
    assert total >= 120
    n = 0
    while not sq.empty():
        block, prio, reward = sq.get()
        assert np.isfinite(prio).all()
        assert block.obs.dtype == np.uint8
        assert block.obs.shape[1:] == (1, 84, 84)
        n += 1
    assert n >= 1
