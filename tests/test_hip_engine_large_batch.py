"""GPU end-to-end above 64 sequences per batch: the HIP engine, with the
multi-pass persistent LSTM under it, against the eager fp32 golden learner on
identical weights — test_hip_engine.py's construction and thresholds (loss
within 5 %, priorities rtol 0.1 / atol 0.05, per-parameter cosine >= 0.98 or
relative error <= 0.1) at batch sizes that leave a partial last 64-row
chunk."""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner, TrainingBatch

SMALL = dict(burn_in_steps=8, learning_steps=8, forward_steps=3, amp=False,
             dtype="fp32")


def make_learners(preset, batch_size, seed=0, eager=True, **kw):
    c = cfg.apply(preset, batch_size=batch_size, **{**SMALL, **kw})
    torch.manual_seed(seed)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                    encoder=c.encoder, forward_steps=c.forward_steps)
    eager_l = Learner(None, None, model) if eager else None
    hip = Learner(None, None, model)
    hip.enable_hip_engine()
    assert hip.engine is not None
    return c, eager_l, hip


def cos(a, b):
    a, b = a.flatten().float(), b.flatten().float()
    denom = a.norm() * b.norm()
    if denom == 0:
        return 1.0
    return float((a @ b) / denom)


class CountingExt:
    """The extension module behind a call counter: engine.m is swapped for
    this, so the test sees which LSTM entry points a step went through."""

    def __init__(self, m):
        self._m = m
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._m, name)
        if not name.startswith("lstm_"):
            return fn

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return counted


def assert_not_poisoned(engine):
    torch.cuda.synchronize()
    assert int(engine.bar[256].item()) == 0
    assert not bool(engine._poison_pin.any())


def check_engine_matches_eager(preset, batch_size):
    from bench import build_batch
    c, eager, hip = make_learners(preset, batch_size)
    dev = torch.device("cuda")
    batch_a = build_batch(c, dev, seed=5)
    assert batch_a.obs.shape[0] == batch_size
    batch_b = copy.deepcopy(batch_a)

    loss_e, prio_e = eager.train_step(batch_a)
    grads_e = {n: p.grad.clone()
               for n, p in eager.online_net.named_parameters()}

    # engine-only call (no optimizer step) so grads compare at equal weights
    counter = hip.engine.m = CountingExt(hip.engine.m)
    loss_h, prio_h = hip.engine.train_step(batch_b)
    grads_h = {n: p.grad.clone() for n, p in hip.online_net.named_parameters()}
    assert_not_poisoned(hip.engine)
    assert counter.calls == {"lstm_fwd_multi": 1, "lstm_bwd_multi": 1}

    lf_e, lf_h = float(loss_e), float(loss_h)
    print(f"B={batch_size} loss eager {lf_e:.6f} engine {lf_h:.6f}")
    assert abs(lf_e - lf_h) < 0.05 * max(1.0, abs(lf_e)), (lf_e, lf_h)

    pe = prio_e if isinstance(prio_e, np.ndarray) else prio_e.cpu().numpy()
    ph = prio_h.cpu().numpy()
    assert ph.shape == (batch_size,)
    np.testing.assert_allclose(ph, pe, rtol=0.1, atol=0.05)

    bad = []
    for n, ge in grads_e.items():
        gh = grads_h[n]
        cs = cos(ge, gh)
        rel = float((gh.float() - ge.float()).norm()
                    / (ge.float().norm() + 1e-8))
        if cs < 0.98 and rel > 0.1:
            bad.append((n, cs, rel))
    assert not bad, bad
    return c, hip


@pytest.mark.parametrize("batch_size", [72, 130])
def test_nature_four_channels_matches_eager(batch_size):
    check_engine_matches_eager("mspacman", batch_size)


def test_nature_single_frame_matches_eager():
    c, hip = check_engine_matches_eager("mspacman_reference", 72)
    assert tuple(c.obs_shape) == (1, 84, 84) and hip.engine.C == 1


def test_impala_engine_train_step():
    """As tests/test_hip_impala.py::test_impala_engine_train_step, at 72."""
    from bench import build_batch
    c = cfg.apply("seaquest_impala", batch_size=72, burn_in_steps=8,
                  learning_steps=8, forward_steps=3)
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="impala",
                    forward_steps=c.forward_steps)
    learner = Learner(None, None, model)
    learner.enable_hip_engine()
    assert learner.engine is not None and learner.engine.impala
    batch = build_batch(c, torch.device("cuda:0"), seed=11)
    losses = []
    for _ in range(12):
        loss, prio = learner.train_step(batch)
        loss = float(loss)
        assert np.isfinite(loss)
        assert torch.isfinite(prio).all() and prio.shape == (72,)
        losses.append(loss)
    assert losses[-1] < losses[0]
    assert_not_poisoned(learner.engine)


def concat_batches(a, b):
    cat = lambda f, d=0: torch.cat([getattr(a, f), getattr(b, f)], d)
    return TrainingBatch(
        obs=cat("obs"), last_action=cat("last_action"),
        last_reward=cat("last_reward"), hidden=cat("hidden", 1),
        action=cat("action"), n_step_reward=cat("n_step_reward"),
        gamma=cat("gamma"), burn_in_steps=cat("burn_in_steps"),
        learning_steps=cat("learning_steps"),
        forward_steps=cat("forward_steps"),
        idxes=np.concatenate([a.idxes, b.idxes]),
        is_weights=cat("is_weights"), old_ptr=0, env_steps=0)


def test_composition_of_two_64_row_batches():
    """Per-sequence priorities do not depend on the rest of the batch: one
    B = 128 step on two concatenated 64-row batches gives the priorities of
    the two B = 64 steps on the same weights."""
    from bench import build_batch
    c, _, hip = make_learners("mspacman", 128, eager=False)
    c64 = copy.copy(c)
    c64.batch_size = 64
    dev = torch.device("cuda")
    b1 = build_batch(c64, dev, seed=21, hwc=True)
    b2 = build_batch(c64, dev, seed=22, hwc=True)
    both = concat_batches(b1, b2)
    eng = hip.engine
    counter = eng.m = CountingExt(eng.m)
    _, p_both = eng.train_step(both)
    assert counter.calls == {"lstm_fwd_multi": 1, "lstm_bwd_multi": 1}
    _, p1 = eng.train_step(b1)
    _, p2 = eng.train_step(b2)
    assert counter.calls == {"lstm_fwd_multi": 1, "lstm_bwd_multi": 1,
                             "lstm_fwd": 2, "lstm_bwd": 2}
    assert_not_poisoned(eng)
    sep = torch.cat([p1, p2])
    print("composition: priorities bit-equal:", torch.equal(p_both, sep),
          "max abs diff", float((p_both - sep).abs().max()))
    np.testing.assert_allclose(p_both.cpu().numpy(), sep.cpu().numpy(),
                               rtol=0.1, atol=0.05)


def test_training_reduces_loss_at_96():
    from bench import build_batch
    c, _, hip = make_learners("mspacman", 96, seed=1, eager=False)
    batch = build_batch(c, torch.device("cuda"), seed=9)
    first = last = None
    for i in range(20):
        loss, _ = hip.train_step(batch)
        assert np.isfinite(float(loss))
        if i == 0:
            first = float(loss)
        last = float(loss)
    assert last < first, (first, last)
    assert_not_poisoned(hip.engine)


def test_gpu_replay_sample_of_96():
    """Ingest -> sample(96) -> engine.train_step -> priorities fed back."""
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    from bench import build_synthetic_block

    c, _, hip = make_learners("mspacman", 96, eager=False, block_length=40,
                              buffer_capacity=32 * 40)
    rng = np.random.default_rng(2)
    replay = GpuReplayBuffer(device="cuda", capacity=32 * 40)
    for _ in range(replay.num_blocks):
        replay.ingest(build_synthetic_block(c, rng),
                      rng.random(replay.spb).astype(np.float32) + 0.5)
    batch = replay.sample()
    torch.cuda.synchronize()
    assert batch.obs.shape[:2] == (96, c.seq_len)
    total0 = replay.total_priority
    loss, prio = hip.engine.train_step(batch)
    assert torch.isfinite(loss)
    assert prio.shape == (96,) and torch.isfinite(prio).all()
    assert_not_poisoned(hip.engine)
    replay.update_priorities(batch.idxes, prio, batch.old_ptr)
    torch.cuda.synchronize()
    assert np.isfinite(replay.total_priority)
    assert replay.total_priority != total0


def test_batch_size_257_raises_the_limit_error():
    c = cfg.apply("mspacman", batch_size=257, **SMALL)
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                    forward_steps=c.forward_steps)
    learner = Learner(None, None, model)
    with pytest.raises(ValueError, match=r"batch_size <= 256"):
        learner.enable_hip_engine()
    assert learner.engine is None
    from r2d2_amd.ops.engine import HipNetworkEngine
    with pytest.raises(ValueError, match=r"batch_size"):
        HipNetworkEngine(learner.online_net, learner.target_net,
                         torch.device("cuda"), c)


def test_train_step_rejects_a_batch_of_257():
    from bench import build_batch
    c, _, hip = make_learners("mspacman", 66, eager=False)
    big = copy.copy(c)
    big.batch_size = 257
    batch = build_batch(big, torch.device("cuda"), seed=3, hwc=True)
    with pytest.raises(ValueError, match=r"batch_size <= 256"):
        hip.engine.train_step(batch)


def test_batch_size_64_stays_on_the_single_pass_kernels():
    from bench import build_batch
    c, _, hip = make_learners("mspacman", 64, eager=False)
    batch = build_batch(c, torch.device("cuda"), seed=5, hwc=True)
    counter = hip.engine.m = CountingExt(hip.engine.m)
    loss, prio = hip.engine.train_step(batch)
    assert torch.isfinite(loss) and prio.shape == (64,)
    assert counter.calls == {"lstm_fwd": 1, "lstm_bwd": 1}
