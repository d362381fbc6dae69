"""The Nature-CNN conv weight gradients at the learner's shapes, kernel alone,
on one GPU, stage by stage:

    atomic_masked     act given, atomic flush into fresh zeros (the path
                      before the slab flush; what R2D2_CONV_WGRAD_SLAB=0 runs)
    atomic_premasked  empty act (dY pre-masked, no mask re-read), atomic flush
    slab              empty act, partial sums stored to the workspace, reducer
                      writes dW / db in torch layout (reducer included)
    slab@G            the same at a grid of G workgroups (band kernels only)

Headline config: B = 64, T = 85, 5,440 images.  Timed with device events
around a batch of calls, rotating over several input sets so that no call
finds its operands left in cache by the call before, and alternated round by
round in one process.  One JSON line per layer: median [min, max]
microseconds per call for every variant, the bytes each variant has to move
(inputs read once, flushed floats written, and for the slab read back once)
and the TB/s that makes at the median.  Before timing, the slab result is
compared with the atomic one.  Operands are random and built here.

    python tools/conv_wgrad_bench.py [rounds] [calls_per_round] [input_sets]
"""

import json
import statistics
import sys

sys.path.insert(0, ".")

import torch  # noqa: E402

GRIDS = (256, 512, 1024)
# (conv_id, cin, kernel) -> cout, k, inhw, ohw
ROWS = {(1, 4, "band"): (32, 8, 84, 20), (1, 1, "chunked"): (32, 8, 84, 20),
        (1, 1, "band"): (32, 8, 84, 20), (2, 32, "band"): (64, 4, 20, 9),
        (3, 64, "band"): (64, 3, 9, 7)}


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
        for i in range(5):
            fn(i)
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(device_us(fn, calls))
    return {k: stats(v) for k, v in res.items()}


def band_parts(N, wgs):
    imgs = -(-N // wgs)
    return -(-N // imgs)


def main(rounds=5, calls=20, sets=4, N=5440):
    from r2d2_amd.ops import hip_ops
    m = hip_ops.ext()
    empty = torch.Tensor()
    for (conv_id, cin, kernel), (cout, k, inhw, ohw) in ROWS.items():
        K, M = k * k * cin, N * ohw * ohw
        g = torch.Generator(device="cuda").manual_seed(100 * conv_id + cin)
        if conv_id == 1:
            xs = [torch.randint(0, 256, (N, inhw, inhw, cin),
                                dtype=torch.uint8, device="cuda", generator=g)
                  for _ in range(sets)]
        else:
            xs = [torch.randn(N, inhw, inhw, cin, device="cuda",
                              generator=g).bfloat16() for _ in range(sets)]
        acts = [torch.randn(M, cout, device="cuda", generator=g).bfloat16()
                for _ in range(sets)]
        dYs = [torch.where(a > 0, (torch.randn(M, cout, device="cuda",
                                               generator=g) * 0.5).bfloat16(),
                           torch.zeros((), dtype=torch.bfloat16,
                                       device="cuda")) for a in acts]
        slot = cout * K + 64
        band = kernel == "band"
        n_ws = max(m.conv_wgrad_ws_floats(conv_id, cin, N, band),
                   (max(GRIDS) if band else 0) * slot)
        ws = torch.empty(n_ws, device="cuda")
        dW = torch.empty(cout, cin, k, k, device="cuda")
        db = torch.empty(cout, device="cuda")

        def atomic(i, masked, wgs=0):
            a = acts[i % sets] if masked else empty
            if band:
                return m.conv_wgrad_band(dYs[i % sets], a, xs[i % sets],
                                         conv_id, N, wgs)
            return m.conv_wgrad(dYs[i % sets], a, xs[i % sets], conv_id, N,
                                inhw, inhw, ohw, ohw, cout, K)

        def slab(i, wgs=0):
            if band:
                m.conv_wgrad_band_into(dYs[i % sets], empty, xs[i % sets],
                                       conv_id, N, ws, dW, db, wgs)
            else:
                m.conv_wgrad_into(dYs[i % sets], empty, xs[i % sets], conv_id,
                                  N, inhw, inhw, ohw, ohw, cout, K, ws, dW, db)

        # the three variants compute the same gradient
        dWt, dbt = atomic(0, True)
        dWt2, _ = atomic(0, False)
        slab(0)
        ref = dWt.view(cout, k, k, cin).permute(0, 3, 1, 2)
        for got in (dW, dWt2.view(cout, k, k, cin).permute(0, 3, 1, 2)):
            assert torch.allclose(got, ref, rtol=2e-3, atol=1e-2), \
                float((got - ref).abs().max())
        assert torch.allclose(db, dbt, rtol=2e-3, atol=1e-2)

        variants = {"atomic_masked": lambda i: atomic(i, True),
                    "atomic_premasked": lambda i: atomic(i, False),
                    "slab": slab}
        # workgroups (= flushed slots) at the default grid
        n_def = m.conv_wgrad_ws_floats(conv_id, cin, N, band) // slot
        parts = {"slab": n_def}
        if band:
            for wgs in GRIDS:
                variants[f"slab@{wgs}"] = lambda i, wgs=wgs: slab(i, wgs)
                parts[f"slab@{wgs}"] = band_parts(N, wgs)
        res = alternate(variants, rounds, calls)

        in_b = xs[0].numel() * xs[0].element_size() + M * cout * 2
        mb = {"atomic_masked": in_b + M * cout * 2 + n_def * slot * 4,
              "atomic_premasked": in_b + n_def * slot * 4}
        for name, p in parts.items():
            mb[name] = in_b + 2 * p * slot * 4
        print(json.dumps(dict(
            row=f"conv{conv_id} cin{cin} {kernel}", images=N,
            us_median_min_max=res,
            MB_moved={n: round(b / 1e6, 1) for n, b in mb.items()},
            TBps_at_median={n: round(mb[n] / res[n][0] / 1e6, 2)
                            for n in res})), flush=True)
        del xs, acts, dYs, ws


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:5]))
