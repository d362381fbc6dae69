"""The dense-layer forward, dgrad and wgrad GEMMs at the learner's shapes,
kernel alone, on one GPU: automatic dispatch against each forced path.

Headline config: B = 64, T = 85, so M = 5,440 rows through the encoder FC and
the LSTM input GEMM, R = 2,560 learning rows through the heads.  Per shape the
variants are

  auto    what the engine gets (path 0)
  old64   the unstaged 64x64 kernel (path 64)
  s64     the LDS-staged 64x64 tile (path 6464)
  s128    the LDS-staged 128x64 tile (path 12864)

and for the wgrads auto, old64 (the 64x64 kernel, m-tiles of 32) and tile
(the 128x64 output tile, double-buffered m-tiles of 64; path 12864),

timed with device events around a batch of calls, rotating over several input
sets so that no call finds its operands left in cache by the call before, and
alternated round by round in one process.  One JSON line per shape: median
[min, max] microseconds per call for every variant.  Operands are random and
built here.

    python tools/gemm_bench.py [rounds] [calls_per_round] [input_sets]
"""

import json
import statistics
import sys

sys.path.insert(0, ".")

import torch  # noqa: E402

PATHS = {"auto": 0, "old64": 64, "s64": 6464, "s128": 12864}
WGRAD_PATHS = {"auto": 0, "old64": 64, "tile": 12864}

# name, kind, M, reduction length, output columns, flags
SHAPES = [
    ("fc_fwd 3136->512", "fwd", 5440, 3136, 512, dict(act=1)),
    ("lstm_in_fwd 544->2048", "fwd", 5440, 544, 2048, dict(act=0)),
    ("head_hidden_fwd 512->512", "fwd", 2560, 512, 512, dict(act=1)),
    ("fc_dgrad 512->3136", "dgrad", 5440, 512, 3136,
     dict(relu_mask=True, out_mask=True)),
    ("head_hidden_dgrad 512->512", "dgrad", 2560, 512, 512,
     dict(relu_mask=True)),
    ("dlat 2048->512 of 544", "dgrad", 5440, 2048, 544, dict(k_out=512)),
    ("head_out_dgrad 32->512", "dgrad", 2560, 32, 512, dict()),
    # wgrads: reduction = M rows; columns = N (dY), k = K (A)
    ("fc_wgrad 512x3136", "wgrad", 5440, 512, 3136,
     dict(relu_mask=True, bias=True)),
    ("w_ih_wgrad 2048x544", "wgrad", 5440, 2048, 544, dict(bias=True)),
    ("w_hh_wgrad 2048x512", "wgrad", 5440, 2048, 512, dict()),
    ("head_hidden_wgrad 512x512", "wgrad", 2560, 512, 512,
     dict(relu_mask=True, bias=True)),
]


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


def make_call(m, kind, M, red, cols, flags, sets, path):
    """fn(i) running one GEMM on input set i % sets."""
    g = torch.Generator(device="cuda")
    g.manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g).bfloat16()

    e = torch.empty(0, device="cuda")
    tail = () if path is None else (path,)    # a build without the argument
    if kind == "fwd":
        ops = [(rnd(M, red), rnd(cols, red),
                torch.randn(cols, device="cuda", generator=g))
               for _ in range(sets)]
        act = flags["act"]
        return lambda i: m.gemm_bias_act(*ops[i % sets], act, False, *tail)
    rm = flags.get("relu_mask", False)
    if kind == "wgrad":
        N, K = red, cols
        ops = [(rnd(M, N), rnd(M, N) if rm else e, rnd(M, K), rm,
                flags.get("bias", False)) for _ in range(sets)]
        return lambda i: m.gemm_wgrad(*ops[i % sets], *tail)[0]
    k_out = flags.get("k_out", 0)
    ops = [(rnd(M, red), rnd(M, red) if rm else e, rnd(cols, red), rm, k_out,
            rnd(M, k_out or cols) if flags.get("out_mask") else None)
           for _ in range(sets)]
    return lambda i: m.gemm_dgrad(*ops[i % sets], *tail)


def bench_shape(variants, rounds, calls, exact):
    """variants: {label: fn(i)}; alternated rounds.  First results checked:
    equal for forward and dgrad (every path keeps the same accumulation
    chain), close for the wgrads (f32 atomics)."""
    outs = {k: fn(0) for k, fn in variants.items()}
    torch.cuda.synchronize()
    first = next(iter(outs.values()))
    if exact:
        assert all(torch.equal(first, o) for o in outs.values()), \
            "paths disagree"
    else:
        scale = float(first.abs().max())
        assert all(float((first - o).abs().max()) <= 1e-4 * scale
                   for o in outs.values()), "paths disagree"
    del outs
    for fn in variants.values():
        for i in range(10):
            fn(i)
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(device_us(fn, calls))
    return {k: stats(v) for k, v in res.items()}


def main(rounds=7, calls=30, sets=6, extra=None):
    """extra: {label: (module, path)} adds variants from other builds of the
    extension (used when comparing two trees in one process)."""
    from r2d2_amd.ops import hip_ops
    m = hip_ops.ext()
    for name, kind, M, red, cols, flags in SHAPES:
        paths = WGRAD_PATHS if kind == "wgrad" else PATHS
        variants = {k: make_call(m, kind, M, red, cols, flags, sets, p)
                    for k, p in paths.items()}
        for k, (mod, p) in (extra or {}).items():
            variants[k] = make_call(mod, kind, M, red, cols, flags, sets, p)
        flop = 2.0 * M * red * (flags.get("k_out", 0) or cols)
        print(json.dumps(dict(shape=name, M=M, reduction=red, columns=cols,
                              gflop=round(flop / 1e9, 2),
                              us_median_min_max=bench_shape(
                                  variants, rounds, calls,
                                  kind != "wgrad"))),
              flush=True)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
