"""The vector-observation (MLP encoder) path on one GPU: the two first-layer
kernels alone, and one learner update on CartPole-shaped batches.

Kernels, at M = 64 * 19 (the cartpole_hip sequence length) and 64 * 85 (the
flagship one), D = 4:

  mlp_in_fwd          against relu(F.linear(X, W1, b1)) in f32
  mlp_in_wgrad_into   against the autograd backward of that expression
                      (dW1 and db1 from an upstream gradient of A1's shape)

Update: `Learner.train_step` of the cartpole_hip preset on prebuilt batches,
through the HIP engine, through the eager bf16-autocast learner, and through
that learner with the fused loss kernels (the path enable_hip_engine gave
these configs before the engine admitted them), same GPU, same batches.

Everything is timed with device events around a batch of calls, rotating over
several input sets, the variants alternated round by round in one process.
One JSON line per measurement: median [min, max] microseconds per call.

    python tools/mlp_engine_bench.py [rounds] [calls_per_round] [input_sets]
"""

import json
import statistics
import sys

sys.path.insert(0, ".")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, N = 4, 512


def stats(xs):
    return [round(statistics.median(xs), 1), round(min(xs), 1),
            round(max(xs), 1)]


def device_us(fn, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def alternate(variants, rounds, calls):
    for fn in variants.values():
        for i in range(10):
            fn(i)
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(device_us(fn, calls))
    return {k: stats(v) for k, v in res.items()}


def bench_kernels(m, M, rounds, calls, sets):
    g = torch.Generator(device="cuda").manual_seed(M)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    xs = [r(M, D) for _ in range(sets)]
    w, b = r(N, D) * 0.5, r(N) * 0.5
    das = [(r(M, N) * 0.05).bfloat16() for _ in range(sets)]
    dw, db = torch.zeros(N, D, device="cuda"), torch.zeros(N, device="cuda")
    wt, bt = w.clone().requires_grad_(), b.clone().requires_grad_()
    daf = [d.float() for d in das]

    def torch_bwd(i):
        a1 = torch.relu(F.linear(xs[i % sets], wt, bt))
        return torch.autograd.grad(a1, (wt, bt), daf[i % sets])

    fwd = alternate({
        "mlp_in_fwd": lambda i: m.mlp_in_fwd(xs[i % sets], w, b),
        "torch_f32": lambda i: torch.relu(F.linear(xs[i % sets], w, b)),
    }, rounds, calls)
    # the torch variant runs forward + backward (autograd needs the graph);
    # its forward alone is the torch_f32 figure above
    bwd = alternate({
        "mlp_in_wgrad_into": lambda i: m.mlp_in_wgrad_into(
            das[i % sets], xs[i % sets], dw, db),
        "torch_f32_fwd_bwd": torch_bwd,
    }, rounds, calls)
    print(json.dumps(dict(what="kernels", M=M, D=D, fwd_us=fwd,
                          wgrad_us=bwd)), flush=True)


def build_batch(c, seed):
    from r2d2_amd.worker import TrainingBatch
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, T, A = c.batch_size, c.seq_len, c.action_dim
    L = c.learning_steps
    R = B * L
    full = lambda v: torch.full((B,), v, dtype=torch.long)
    la = torch.zeros(B, T, A)
    la[torch.arange(B)[:, None], torch.arange(T)[None, :],
       torch.randint(0, A, (B, T), generator=g)] = 1.0
    return TrainingBatch(
        obs=torch.randn(B, T, c.obs_shape[0], generator=g),
        last_action=la, last_reward=torch.randn(B, T, generator=g) * 0.1,
        hidden=torch.randn(2, B, c.hidden_dim, generator=g) * 0.05,
        action=torch.randint(0, A, (R, 1), generator=g),
        n_step_reward=torch.randn(R, generator=g).abs(),
        gamma=torch.full((R,), c.gamma ** c.forward_steps),
        burn_in_steps=full(c.burn_in_steps), learning_steps=full(L),
        forward_steps=full(c.forward_steps), idxes=np.arange(B),
        is_weights=torch.rand(R, generator=g) * 0.5 + 0.5,
        old_ptr=0, env_steps=0).to(torch.device("cuda"), non_blocking=False)


def bench_step(rounds, calls, sets):
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner

    c = cfg.apply("cartpole_hip")
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="mlp",
                    forward_steps=c.forward_steps, mlp_hidden=c.mlp_hidden)
    eager = Learner(None, None, model)
    assert eager.amp and eager.engine is None
    # what enable_hip_engine left such a config with before the engine
    # admitted it: the eager forward/backward under the fused loss kernels
    fused = Learner(None, None, model)
    fused.hip_engine = True
    hip = Learner(None, None, model)
    hip.enable_hip_engine()
    assert hip.engine is not None
    batches = [build_batch(c, s) for s in range(sets)]
    res = alternate({
        "engine": lambda i: hip.train_step(batches[i % sets]),
        "eager_bf16": lambda i: eager.train_step(batches[i % sets]),
        "eager_bf16_fused_loss":
            lambda i: fused.train_step(batches[i % sets]),
    }, rounds, calls)
    B = c.batch_size
    print(json.dumps(dict(
        what="train_step", preset="cartpole_hip", B=B, T=c.seq_len,
        us_median_min_max=res,
        seq_per_s_median={k: round(B / (v[0] * 1e-6)) for k, v in res.items()},
    )), flush=True)


def main(rounds=7, calls=30, sets=6):
    from r2d2_amd.ops import hip_ops
    m = hip_ops.ext()
    for M in (64 * 19, 64 * 85):
        bench_kernels(m, M, rounds, calls, sets)
    bench_step(rounds, calls, sets)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
