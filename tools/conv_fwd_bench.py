"""The Nature-CNN conv forwards at the learner's shapes, kernel alone, on one
GPU: conv_fwd_band per layer, and conv1_fwd_dual (both networks' conv1 from
one staging of each frame) against the two conv_fwd_band launches it
replaces, each at the candidate grids.

Headline config: B = 64, T = 85, 5,440 images; mspacman_b128 runs 10,880.
Timed with device events around a batch of calls, rotating over several input
sets so that no call finds its frames left in cache by the call before, and
alternated round by round in one process.  One JSON line per row: median
[min, max] microseconds per call for every variant.  Before timing, every
dual output is checked bit-equal to conv_fwd_band at full size.  Operands are
random and built here.

    python tools/conv_fwd_bench.py [rounds] [calls_per_round] [input_sets]
"""

import json
import statistics
import sys

sys.path.insert(0, ".")

import torch  # noqa: E402

GRIDS = (256, 512, 1024, 2048)
# conv_id, cin -> cout, k, inhw
GEO = {(1, 4): (32, 256, 84), (1, 1): (32, 64, 84), (2, 32): (64, 512, 20),
       (3, 64): (64, 576, 9)}


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


def operands(conv_id, cin, N, sets, nets=1):
    cout, K, inhw = GEO[(conv_id, cin)]
    g = torch.Generator(device="cuda").manual_seed(100 * conv_id + cin)
    if conv_id == 1:
        xs = [torch.randint(0, 256, (N, inhw, inhw, cin), dtype=torch.uint8,
                            device="cuda", generator=g) for _ in range(sets)]
    else:
        xs = [torch.randn(N, inhw, inhw, cin, device="cuda",
                          generator=g).bfloat16() for _ in range(sets)]
    ws = [((torch.randn(cout, K, device="cuda", generator=g) * 0.1).bfloat16(),
           torch.randn(cout, device="cuda", generator=g) * 0.1)
          for _ in range(nets)]
    return xs, ws


def alternate(variants, rounds, calls):
    for fn in variants.values():
        for i in range(5):
            fn(i)
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(device_us(fn, calls))
    return {k: stats(v) for k, v in res.items()}


def main(rounds=5, calls=20, sets=4):
    from r2d2_amd.ops import hip_ops
    m = hip_ops.ext()
    for N in (5440, 10880):
        for conv_id, cin in sorted(GEO):
            xs, ((w, b),) = operands(conv_id, cin, N, sets)
            variants = {
                f"band@{g or 'default'}":
                    (lambda i, g=g: m.conv_fwd_band(xs[i % sets], w, b,
                                                    conv_id, N, g))
                for g in (0,) + GRIDS}
            print(json.dumps(dict(
                row=f"conv_fwd_band conv{conv_id} cin{cin}", images=N,
                us_median_min_max=alternate(variants, rounds, calls))),
                flush=True)
            del xs
        for cin in (4, 1):
            xs, ((w0, b0), (w1, b1)) = operands(1, cin, N, sets, nets=2)
            ref0 = m.conv_fwd_band(xs[0], w0, b0, 1, N)
            ref1 = m.conv_fwd_band(xs[0], w1, b1, 1, N)
            for g in (0,) + GRIDS:
                o0, o1 = m.conv1_fwd_dual(xs[0], w0, b0, w1, b1, N, g)
                assert torch.equal(o0, ref0) and torch.equal(o1, ref1), \
                    f"conv1_fwd_dual differs from conv_fwd_band at grid {g}"
            assert not torch.equal(ref0, ref1)
            del ref0, ref1, o0, o1

            def two(i):
                m.conv_fwd_band(xs[i % sets], w0, b0, 1, N)
                m.conv_fwd_band(xs[i % sets], w1, b1, 1, N)

            variants = {"two_band_calls": two}
            for g in (0,) + GRIDS:
                variants[f"dual@{g or 'default'}"] = (
                    lambda i, g=g: m.conv1_fwd_dual(xs[i % sets], w0, b0, w1,
                                                    b1, N, g))
            print(json.dumps(dict(
                row=f"conv1_fwd_dual cin{cin} vs 2 x conv_fwd_band", images=N,
                bit_equal=True,
                us_median_min_max=alternate(variants, rounds, calls))),
                flush=True)
            del xs


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
