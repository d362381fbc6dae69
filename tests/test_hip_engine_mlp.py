"""GPU end-to-end: vector observations through the HIP engine (MLP encoder:
mlp_in_fwd + the fc2 GEMMs, manual backward) against the eager fp32 learner
on identical weights and batch, and HipInference on the same encoder.

Bounds against the eager learner are those of tests/test_hip_engine.py: loss
within 5 % of max(1, |eager|), priorities rtol 0.1 / atol 0.05, and for every
parameter cosine >= 0.98 or relative norm error <= 0.1.
"""

import queue

import numpy as np
import pytest
import torch

from test_hip_lstm_layouts import FACTOR, bits_equal, rel_err
from test_hip_actor_step import FLOOR, _Spy, assert_bound, pack_exact

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner, TrainingBatch

T_FULL = 19          # burn-in 8 + learning 8 + forward 3


@pytest.fixture(autouse=True)
def _restore_config():
    yield
    if torch.cuda.is_available():
        cfg.apply("mspacman")


def apply_cfg(B=8, D=4, A=2, **over):
    kw = dict(batch_size=B, obs_shape=(D,), action_dim=A, amp=False,
              dtype="fp32")
    kw.update(over)
    return cfg.apply("cartpole_hip", **kw)


def make_net(c, seed):
    torch.manual_seed(seed)
    return Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="mlp",
                   forward_steps=c.forward_steps, mlp_hidden=c.mlp_hidden)


def make_learners(B=8, D=4, A=2, seed=0):
    c = apply_cfg(B, D, A)
    model = make_net(c, seed)
    eager = Learner(None, None, model)
    hip = Learner(None, None, model)
    hip.enable_hip_engine()
    assert hip.engine is not None
    return c, eager, hip


def cos(a, b):
    a, b = a.flatten().float(), b.flatten().float()
    denom = a.norm() * b.norm()
    if denom == 0:
        return 1.0
    return float((a @ b) / denom)


def build_ragged_batch(c, device, seed):
    """Per-sample burn-in / learning / forward variation; sample 0 keeps the
    full 8 + 8 + 3 layout so T = 19.  Observations are float32 states at
    CartPole's scale."""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, A, D = c.batch_size, c.action_dim, c.obs_shape[0]
    burn = rng.integers(0, c.burn_in_steps + 1, B)
    learn = rng.integers(1, c.learning_steps + 1, B)
    fwd = rng.integers(1, c.forward_steps + 1, B)
    burn[0], learn[0], fwd[0] = (c.burn_in_steps, c.learning_steps,
                                 c.forward_steps)
    burn, learn, fwd = (torch.from_numpy(v).long() for v in (burn, learn, fwd))
    T = int((burn + learn + fwd).max())
    assert T == T_FULL
    R = int(learn.sum())
    scale = torch.tensor([2.4, 3.0, 0.21, 3.0]).repeat(4)[:D]
    obs = torch.randn(B, T, D, generator=g) * scale
    la = torch.zeros(B, T, A)
    la[torch.arange(B)[:, None], torch.arange(T)[None, :],
       torch.randint(0, A, (B, T), generator=g)] = 1.0
    lr = torch.randn(B, T, generator=g) * 0.1
    hidden = torch.randn(2, B, c.hidden_dim, generator=g) * 0.05
    batch = TrainingBatch(
        obs=obs, last_action=la, last_reward=lr, hidden=hidden,
        action=torch.randint(0, A, (R, 1), generator=g),
        n_step_reward=torch.randn(R, generator=g).abs(),
        gamma=torch.full((R,), c.gamma ** c.forward_steps),
        burn_in_steps=burn, learning_steps=learn, forward_steps=fwd,
        idxes=np.arange(B), is_weights=torch.rand(R, generator=g) * 0.5 + 0.5,
        old_ptr=0, env_steps=0)
    return batch.to(device, non_blocking=False)


# ---------------------------------------------------------------------------
# Engine against the eager fp32 learner
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,A", [(8, 4, 2), (16, 4, 2), (8, 5, 3),
                                   (16, 16, 9)],
                         ids=["B8-D4-A2", "B16-D4-A2", "B8-D5-A3",
                              "B16-D16-A9"])
def test_engine_matches_eager_on_ragged_layouts(B, D, A):
    c, eager, hip = make_learners(B, D, A, seed=11 + B)
    dev = torch.device("cuda")
    batch_a = build_ragged_batch(c, dev, seed=50 + B + D)
    batch_b = build_ragged_batch(c, dev, seed=50 + B + D)
    assert batch_b.obs.dtype == torch.float32

    loss_e, prio_e = eager.train_step(batch_a)
    grads_e = {n: p.grad.clone()
               for n, p in eager.online_net.named_parameters()}
    loss_h, prio_h = hip.engine.train_step(batch_b)
    grads_h = {n: p.grad.clone()
               for n, p in hip.online_net.named_parameters()}

    lf_e, lf_h = float(loss_e), float(loss_h)
    print(f"loss eager {lf_e:.6f} engine {lf_h:.6f}")
    assert abs(lf_e - lf_h) < 0.05 * max(1.0, abs(lf_e)), (lf_e, lf_h)
    pe = prio_e if isinstance(prio_e, np.ndarray) else prio_e.cpu().numpy()
    np.testing.assert_allclose(prio_h.cpu().numpy(), pe, rtol=0.1, atol=0.05)

    bad, enc = [], []
    for n, ge in grads_e.items():
        gh = grads_h[n]
        cs = cos(ge, gh)
        rel = float((gh.float() - ge.float()).norm()
                    / (ge.float().norm() + 1e-8))
        if n.startswith("encoder."):
            # cos() answers 1.0 for a zero vector: an engine gradient that
            # was never written must not pass as "parallel"
            assert float(ge.norm()) > 0 and float(gh.norm()) > 0, n
            enc.append((n, round(cs, 5), round(rel, 5)))
        if cs < 0.98 and rel > 0.1:
            bad.append((n, cs, rel))
    print("encoder grads (name, cosine, rel):", enc)
    assert {n for n, _, _ in enc} == {
        "encoder.fc1.weight", "encoder.fc1.bias",
        "encoder.fc2.weight", "encoder.fc2.bias"}
    assert not bad, (f"gradients off (encoder.fc1.* / encoder.fc2.* figures: "
                     f"{enc}): {bad}")


def test_engine_training_reduces_loss():
    c, eager, hip = make_learners(8, 4, 2, seed=1)
    batch = build_ragged_batch(c, torch.device("cuda"), seed=9)
    first = last = None
    for i in range(20):
        loss, _ = hip.train_step(batch)
        if i == 0:
            first = float(loss)
        last = float(loss)
    assert np.isfinite(last)
    assert last < first, (first, last)


def test_engine_rejects_uint8_observations():
    c, eager, hip = make_learners(8, 4, 2, seed=2)
    batch = build_ragged_batch(c, torch.device("cuda"), seed=3)
    batch.obs = batch.obs.to(torch.uint8)
    with pytest.raises(TypeError):
        hip.engine.train_step(batch)


def test_fast_refresh_matches_python_repack():
    from r2d2_amd.ops.engine import _NetPack, _pack_items, _item_get

    c, eager, hip = make_learners(8, 4, 2, seed=7)
    engine = hip.engine
    batch = build_ragged_batch(c, torch.device("cuda"), seed=4)
    hip.train_step(batch)         # an optimizer step, then the fast refresh
    with torch.no_grad():
        engine.flat_param.add_(torch.randn_like(engine.flat_param) * 0.01)
    engine.refresh_online()
    ref = _NetPack(engine.online_net, engine.device, engine.A, with_bwd=True)
    fast_items = {n: _item_get(h, a, k)
                  for n, h, a, k in _pack_items(engine.online)}
    ref_items = {n: _item_get(h, a, k) for n, h, a, k in _pack_items(ref)}
    assert set(fast_items) == set(ref_items)
    assert {"enc_pack.mw1", "enc_pack.mb1", "enc_pack.mw2t", "enc_pack.mb2",
            "enc_pack.mw2_kn"} <= set(fast_items)
    for n, t in fast_items.items():
        assert torch.equal(t, ref_items[n].view(t.shape)), n
    assert fast_items["enc_pack.mw1"].dtype == torch.float32
    assert bits_equal(fast_items["enc_pack.mw1"],
                      engine.online_net.encoder.fc1.weight.detach())


def test_weight_bus_roundtrip():
    from r2d2_amd.parallel.weight_bus import WeightBus, pack_tensors
    from r2d2_amd.ops.engine import HipInference

    c, eager, hip = make_learners(8, 4, 2, seed=3)
    engine = hip.engine
    bus = WeightBus(pack_tensors(engine.target), "cuda")
    other = make_net(c, 99).cuda()
    inf = HipInference(other, torch.device("cuda"), c)
    before = {n: t.clone() for n, t in pack_tensors(inf.pack).items()}
    assert {"enc_pack.mw1", "enc_pack.mb1", "enc_pack.mw2t",
            "enc_pack.mb2"} <= set(before)
    bus.publish(engine.online)
    ver = bus.pull_into(inf.pack, 0)
    assert ver == 2
    src = pack_tensors(engine.online)
    dst = pack_tensors(inf.pack)
    assert set(dst) == set(pack_tensors(engine.target))
    for name, t in dst.items():
        assert bits_equal(t, src[name].view(t.shape)), name
    for name in ("enc_pack.mw1", "enc_pack.mb1", "enc_pack.mw2t",
                 "enc_pack.mb2"):
        assert not torch.equal(dst[name], before[name]), name


# ---------------------------------------------------------------------------
# Admission
# ---------------------------------------------------------------------------

def test_learner_builds_engine_under_cartpole_hip():
    c = cfg.apply("cartpole_hip")
    assert c.gpu_replay is False and c.use_hip_kernels
    learner = Learner(None, None, make_net(c, 0))
    learner.enable_hip_engine()
    assert learner.engine is not None and learner.engine.mlp
    assert learner.weight_bus is not None


def test_other_mlp_widths_keep_the_eager_path():
    c = cfg.apply("cartpole_hip", mlp_hidden=128)
    learner = Learner(None, None, make_net(c, 0))
    learner.enable_hip_engine()
    assert learner.engine is None and learner.hip_engine


@pytest.mark.parametrize("over,word", [
    (dict(mlp_hidden=128), "mlp_hidden"),
    (dict(hidden_dim=128), "hidden_dim"),
    (dict(obs_shape=(17,)), "width"),
], ids=["mlp_hidden128", "hidden128", "D17"])
def test_engine_constructor_raises_on_unsupported_mlp(over, word):
    from r2d2_amd.ops.engine import HipInference, HipNetworkEngine
    c = cfg.apply("cartpole_hip", **over)
    on, tg = make_net(c, 0).cuda(), make_net(c, 0).cuda()
    with pytest.raises(ValueError, match=word):
        HipNetworkEngine(on, tg, torch.device("cuda"), c)
    with pytest.raises(ValueError, match=word):
        HipInference(on, torch.device("cuda"), c)


# ---------------------------------------------------------------------------
# HipInference
# ---------------------------------------------------------------------------

def make_inference(D=4, A=2):
    from r2d2_amd.ops.engine import HipInference
    c = apply_cfg(8, D, A)
    net = make_net(c, 3).cuda().eval()
    inf = HipInference(net, "cuda")
    inf.m = _Spy(inf.m)
    return c, net, inf


def tick_inputs(c, E, seed, scale=0.3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, A = c.obs_shape[0], c.action_dim
    sc = torch.tensor([2.4, 3.0, 0.21, 3.0], device="cuda").repeat(4)[:D]
    obs = torch.randn(E, D, device="cuda", generator=g) * sc
    la = torch.zeros(E, A, device="cuda")
    idx = torch.randint(0, A, (E,), device="cuda", generator=g)
    la[torch.arange(E, device="cuda"), idx] = 1.0
    lr = torch.randn(E, 1, device="cuda", generator=g) * 0.3
    h = torch.randn(1, E, 512, device="cuda", generator=g) * scale
    cc = torch.randn(1, E, 512, device="cuda", generator=g) * scale
    return obs, la, lr, h, cc


@pytest.mark.parametrize("E", [5, 64])
def test_inference_matches_network_forward(E):
    """forward and step against Network.forward in fp32.

    Latent: float64 of the pack's operands (f32 fc1, bf16 fc2), yardstick the
    f32 torch model that rounds A1 and the latent to bf16, bound 4x.  After
    the latent: the calibrated method of
    test_hip_actor_step.test_step_matches_forward.  Against the fp32 network
    itself the bound on q is 2^-5 of max|q|: the path rounds ten times to
    bf16 (A1; fc2's weights and output; W_ih, W_hh and the h operand; the
    LSTM output; the head hidden weights and output; the head output
    weights), each at most 2^-9 relative, and no stage has a gain above one
    (ReLU, sigmoid and tanh slopes <= 1), so the roundings add to at most
    10 * 2^-9 < 2^-5."""
    c, net, inf = make_inference()
    A = c.action_dim
    obs, la, lr, h, cc = tick_inputs(c, E, 5)
    h_in, c_in = h.clone(), cc.clone()
    qf, (hf, cf) = inf.forward(obs, la, lr, (h, cc))
    q, greedy, (h1, c1) = inf.step(obs, la, lr, (h, cc))
    assert bits_equal(h, h_in) and bits_equal(cc, c_in)
    assert q.shape == qf.shape == (E, A)
    lat_f, = inf.m.latents["assemble_rin"]
    lat_s, = inf.m.latents["lstm_cell_step"]
    assert bits_equal(lat_f, lat_s), "same encoder calls, same latent"

    p, e = inf.pack, inf.pack.enc_pack
    a1_64 = torch.relu(obs.double() @ e.mw1.double().t() + e.mb1.double())
    a1_32 = torch.relu(obs @ e.mw1.t() + e.mb1).bfloat16()
    lat_64 = torch.relu(a1_64 @ e.mw2t.double().t() + e.mb2.double())
    lat_32 = torch.relu(a1_32.float() @ e.mw2t.float().t()
                        + e.mb2).bfloat16()
    ek, em = rel_err(lat_s, lat_64), rel_err(lat_32, lat_64)
    print(f"CALIB latent E{E}: kernel {ek:.3e} yardstick {em:.3e}")
    assert ek <= FACTOR * em, (ek, em)

    qe, he, ce = pack_exact(p, lat_s, la, lr, h[0].double(), cc[0].double(),
                            A)
    assert_bound(f"mlp step h1 E{E}", h1[0], hf[0], he, FLOOR)
    assert_bound(f"mlp step c1 E{E}", c1[0], cf[0], ce, FLOOR)
    assert_bound(f"mlp step q E{E}", q, qf, qe)
    assert torch.equal(greedy.long(), q.argmax(1))

    from r2d2_amd.models.network import AgentState
    st = AgentState.__new__(AgentState)
    st.obs, st.last_action, st.last_reward = obs, la, lr
    st.hidden_state = (h, cc)
    with torch.no_grad():
        qn, (hn, cn) = net(st)
    scale = float(qn.abs().max())
    for name, got in (("forward", qf), ("step", q)):
        err = float((got - qn).abs().max()) / scale
        print(f"q {name} vs Network.forward fp32 E{E}: {err:.3e} of max|q|")
        assert err <= 2.0 ** -5, (name, err)
    for name, got, want in (("h", h1, hn), ("c", c1, cn)):
        err = rel_err(got, want)
        print(f"{name} step vs Network.forward fp32 E{E}: {err:.3e}")
        assert err <= 2.0 ** -5, (name, err)


def test_vector_actor_on_gpu_ticks_through_hip_inference():
    from r2d2_amd.train import epsilon_ladder
    from r2d2_amd.worker import VectorActor

    for fused in (True, False):
        c = cfg.apply("cartpole_hip", num_actors=4, block_length=8,
                      burn_in_steps=4, learning_steps=4, forward_steps=2,
                      actor_update_interval=64, max_episode_steps=12,
                      fused_actor_step=fused)
        model = make_net(c, 0)
        sq = queue.Queue()
        va = VectorActor(epsilon_ladder(4), model, [sq], device="cuda",
                         seed=4)
        assert va.hip_inf is not None, "K15 path must be active on GPU"
        assert va.obs_t.dtype == torch.float32
        seen = []
        name = "step" if fused else "forward"
        inner = getattr(va.hip_inf, name)

        def spy(obs, *a, _inner=inner):
            seen.append(obs.clone())
            return _inner(obs, *a)

        setattr(va.hip_inf, name, spy)
        assert va.run(stop_after_steps=80) >= 80
        assert len(seen) >= 20
        assert all(o.dtype == torch.float32 and o.shape == (4, 4)
                   for o in seen)
        frac = torch.stack(seen)
        assert (frac != frac.round()).any() and (frac < 0).any()
        n = 0
        while not sq.empty():
            block, prio, _ = sq.get()
            assert block.obs.dtype == np.float32 and np.isfinite(prio).all()
            n += 1
        assert n >= 4
