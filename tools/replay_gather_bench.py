"""GPU replay in its two storage modes on one GPU: whole stacks per row
(the default) against one frame per step (config.replay_frame_dedup).

  gather  replay_gather_batch against replay_gather_batch_dedup alone, B = 64,
          T = 85, 160,000-transition stores, the same sampled sequences,
          device events around a batch of calls, alternated rounds
  ingest  host time per ingest() call and blocks/s over 50 full 400-step
          blocks with one sync at the end: plain, dedup with the
          is_frame_stack check, dedup without
  memory  torch.cuda.memory_allocated after constructing the buffer at
          buffer_capacity = 4,000,000 in both modes (only with `memory`)

One JSON line per figure.  Blocks are synthetic and built here.

    python tools/replay_gather_bench.py [rounds] [calls_per_round] [memory]
"""

import json
import statistics
import sys
import time

sys.path.insert(0, ".")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(xs, nd=2):
    return dict(median=round(statistics.median(xs), nd),
                min=round(min(xs), nd), max=round(max(xs), nd))


def device_us(fn, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def stacked_block(c, rng):
    """A full Block whose observations are a real rolling frame stack."""
    from bench import build_synthetic_block
    from r2d2_amd.replay.frame_dedup import stacked_from_frames
    blk = build_synthetic_block(c, rng)
    C = c.obs_shape[0]
    frames = rng.integers(0, 256, size=(blk.obs.shape[0] + C - 1,)
                          + tuple(c.obs_shape[1:]), dtype=np.uint8)
    blk.obs = stacked_from_frames(frames, C)
    return blk


def make_buffer(dedup, verify=True, capacity=160_000):
    from r2d2_amd import config as cfg
    from r2d2_amd.replay.gpu_replay import GpuReplayBuffer
    c = cfg.apply("mspacman", gpu_replay=True, replay_frame_dedup=dedup,
                  replay_dedup_verify=verify)
    return c, GpuReplayBuffer(device="cuda", capacity=capacity)


def bench_gather(pool, rounds, calls):
    bufs = {}
    for name, dedup in (("plain", False), ("dedup", True)):
        c, r = make_buffer(dedup)
        rng = np.random.default_rng(42)
        for i in range(r.num_blocks):
            r.ingest(pool[i % len(pool)],
                     rng.random(r.spb).astype(np.float32) + 0.1)
        bufs[name] = r
    torch.cuda.synchronize()
    p, d = bufs["plain"], bufs["dedup"]
    m, B = p._ext, 64
    torch.manual_seed(0)
    idx, _, weight = m.sumtree_sample(
        p.tree, p.leaf_offset, p.num_levels, torch.rand(B, device="cuda"), B,
        p.beta, p.num_sequences - 1)
    meta, seg = m.replay_gather_meta(idx, p.burn_s, p.learn_s, p.fwd_s,
                                     p.obs_start_s, p.learn_off_s, p.spb)

    def args(r):
        return (r.obs_store, r.la_store, r.lr_store, r.act_store, r.nsr_store,
                r.gam_store, r.hid_store, idx, meta, seg, weight, r.T, r.A,
                r.learn_len, r.H, r.spb)

    variants = {
        "plain": lambda: m.replay_gather_batch(*args(p)),
        "dedup": lambda: m.replay_gather_batch_dedup(*args(d), 4),
    }
    a, b = variants["plain"](), variants["dedup"]()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "gathers disagree"
    del a, b
    for fn in variants.values():
        for _ in range(10):
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):                   # alternated
        for k, fn in variants.items():
            res[k].append(device_us(fn, calls))
    out_mb = B * p.T * p.frame_bytes / 1e6
    for k in variants:
        print(json.dumps(dict(what="gather", variant=k, B=B, T=p.T,
                              out_MB=round(out_mb, 1),
                              device_us=stats(res[k]))), flush=True)


def bench_ingest(pool, rounds, nblocks=50):
    modes = {"plain": (False, True), "dedup_verify": (True, True),
             "dedup_noverify": (True, False)}
    bufs = {k: make_buffer(d, v, capacity=64 * 400)[1]
            for k, (d, v) in modes.items()}
    prio = np.ones(bufs["plain"].spb, dtype=np.float32)
    res = {k: {"host_ms": [], "blocks_per_s": []} for k in modes}
    for rnd in range(rounds + 1):             # round 0 warms up
        for k, r in bufs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(nblocks):
                r.ingest(pool[i % len(pool)], prio)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rnd:
                res[k]["host_ms"].append((t1 - t0) * 1e3 / nblocks)
                res[k]["blocks_per_s"].append(nblocks / (t2 - t0))
    for k in modes:
        print(json.dumps(dict(what="ingest", variant=k, blocks=nblocks,
                              host_ms_per_call=stats(res[k]["host_ms"], 3),
                              blocks_per_s=stats(res[k]["blocks_per_s"], 1))),
              flush=True)
    from r2d2_amd.replay.frame_dedup import is_frame_stack
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        assert is_frame_stack(pool[0].obs)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="is_frame_stack", ms=stats(ts, 3))), flush=True)


def bench_memory():
    for name, dedup in (("plain", False), ("dedup", True)):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        _, r = make_buffer(dedup, capacity=4_000_000)
        torch.cuda.synchronize()
        used = torch.cuda.memory_allocated() - base
        print(json.dumps(dict(
            what="memory", variant=name, buffer_capacity=4_000_000,
            allocated_GB=round(used / 1e9, 2),
            obs_store_GB=round(r.obs_store.numel() / 1e9, 2))), flush=True)
        del r
        torch.cuda.empty_cache()


def main(rounds=7, calls=20, memory=False):
    from r2d2_amd import config as cfg
    c = cfg.apply("mspacman")
    rng = np.random.default_rng(0)
    pool = [stacked_block(c, rng) for _ in range(8)]
    bench_gather(pool, rounds, calls)
    bench_ingest(pool, rounds)
    if memory:
        bench_memory()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7,
         int(sys.argv[2]) if len(sys.argv) > 2 else 20,
         len(sys.argv) > 3 and sys.argv[3] == "memory")
