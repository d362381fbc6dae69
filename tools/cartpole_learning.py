"""Real-reward learning validation on the native CartPole env (configs[0]):
trains the full R2D2 stack (prioritized replay, burn-in LSTM, double-Q,
n-step) and emits the reward curve — the reference's only published
evidence is a learning curve (images/MsPacman.jpg); this is the same
artifact on the env this image can actually run end-to-end.

    python tools/cartpole_learning.py [training_steps] [preset] [seed] \
        [eager|engine] [out_dir]

preset `cartpole` (default) trains on the CPU; `cartpole_hip` trains on the
GPU through the HIP engine.  A fourth argument `eager` turns the HIP kernels
off for that preset (the bf16-autocast learner on the same GPU: the yardstick
the engine's curve is read against).  The metrics land in
<out_dir>/cartpole_metrics_<preset>[_eager]_s<seed>.jsonl (out_dir defaults
to metrics/)."""

import json
import os
import sys

sys.path.insert(0, ".")


def main(training_steps=8000, preset="cartpole", seed=0, eager=False,
         out_dir="metrics"):
    from r2d2_amd import config as cfg

    tag = f"{preset}{'_eager' if eager else ''}_s{seed}"
    path = os.path.join(out_dir, f"cartpole_metrics_{tag}.jsonl")
    os.makedirs(out_dir, exist_ok=True)
    if os.path.exists(path):
        os.remove(path)          # the logger appends
    over = dict(use_hip_kernels=False) if eager else {}
    cfg.apply(preset, training_steps=training_steps,
              learning_starts=1500, buffer_capacity=40_000,
              max_episode_steps=500, log_interval=10,
              save_interval=100_000, num_actors=2,
              base_eps=0.15, lr=1e-3,
              metrics_path=path, **over)
    from r2d2_amd.train import train
    train(seed=seed)
    rows = [json.loads(l) for l in open(path)]
    rets = [r["avg_episode_return"] for r in rows
            if "avg_episode_return" in r]
    print(f"reward curve ({tag}):", [round(r, 1) for r in rets])


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 8000,
         a[1] if len(a) > 1 else "cartpole",
         int(a[2]) if len(a) > 2 else 0,
         len(a) > 3 and a[3] == "eager",
         a[4] if len(a) > 4 else "metrics")
