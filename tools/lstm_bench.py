"""The persistent LSTM kernels alone, on one GPU, at the learner's shapes.

  fwd2        lstm_fwd, two networks, B = 64, T = 85 (the headline step)
  bwd         lstm_bwd, B = 64, T = 85
  fwd2_multi  lstm_fwd_multi, two networks, B = 128, T = 85
  bwd_multi   lstm_bwd_multi, B = 128, T = 85

Each entry is timed with device events around a batch of launches (the
workspace reset kernel included, as in the engine), rotating over several
input sets so that no launch finds its operands left in cache by the one
before, over several rounds.  One JSON line per entry: median [min, max]
microseconds per launch, the same divided by T, and a SHA-256 digest of the
entry's outputs on input set 0 (the inputs are seeded, so two builds that
compute the same bits print the same digests).

One process times ONE build: this tree's, or with so=PATH another build's
r2d2_hip.so.  To compare builds, run one process per build and alternate
them (two builds imported into one process share their kernels).

With `shapes`, nothing is timed: the digests of the six outputs are printed
for every launch layout at small shapes (B in 1, 32, 33, 48, 49, 64 with
T in 2, 7; the multi-pass entries at B in 65, 128, 129, 256, T = 7, 64 and
128 rows per pass), seeded inputs and mixed length masks.

    python tools/lstm_bench.py [rounds] [calls_per_round] [input_sets] \
        [so=path/to/r2d2_hip.so] [shapes]
"""

import hashlib
import importlib.util
import json
import statistics
import sys

sys.path.insert(0, ".")

import torch  # noqa: E402

H = 512
T = 85


def stats(xs, div=1.0):
    return [round(statistics.median(xs) / div, 2), round(min(xs) / div, 2),
            round(max(xs) / div, 2)]


def device_us(fn, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def load_so(path):
    """Another build of the extension, in place of this tree's."""
    spec = importlib.util.spec_from_file_location("r2d2_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(B, sets):
    """Per set: two networks' X / W_hh / initial state, lens with the
    learner's spread (burn-in 40 + 1..40 learning + 5 forward steps), and an
    upstream gradient.  The stash / Cout / Hout the backward reads are made
    by the timed build's own forward."""
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    out = []
    for _ in range(sets):
        nets = [((r(B, T, 4 * H) * 0.5).bfloat16(),
                 (r(4 * H, H) / H ** 0.5).bfloat16(),
                 torch.stack([r(B, H) * 0.1, r(B, H) * 0.1]).contiguous())
                for _ in range(2)]
        lens = torch.tensor([40 + 1 + (b * 7) % 40 + 4 for b in range(B)],
                            dtype=torch.int32, device="cuda")
        out.append(dict(nets=nets, lens=lens, dHext=r(B, T, H) * 0.1,
                        whh_t=nets[0][1].t().contiguous()))
    return out


def make_calls(m, B, multi, ins, bar):
    (fwd, bwd), tail = ((m.lstm_fwd_multi, m.lstm_bwd_multi), (0,)) if multi \
        else ((m.lstm_fwd, m.lstm_bwd), ())

    def f(i):
        s = ins[i % len(ins)]
        (X0, W0, i0), (X1, W1, i1) = s["nets"]
        return fwd(X0, X1, W0, W1, i0, i1, s["lens"], bar, True, *tail)

    def b(i):
        s = ins[i % len(ins)]
        return bwd(s["S"], s["C"], s["Hk"], s["dHext"], s["whh_t"],
                   s["lens"], bar, *tail)

    return f, b


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def shape_digests(m, so):
    bar = torch.zeros(512, dtype=torch.int32, device="cuda")
    cases = [(B, Tt, None) for B in (1, 32, 33, 48, 49, 64) for Tt in (2, 7)]
    cases += [(B, 7, rows) for B in (65, 128, 129, 256) for rows in (64, 128)]
    for B, Tt, rows in cases:
        g = torch.Generator(device="cuda").manual_seed(1000 * B + Tt)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        X0, X1 = ((r(B, Tt, 4 * H) * 0.5).bfloat16() for _ in range(2))
        W0, W1 = ((r(4 * H, H) / H ** 0.5).bfloat16() for _ in range(2))
        i0, i1 = (r(2, B, H) * 0.1 for _ in range(2))
        dH = r(B, Tt, H) * 0.1
        cyc = [1, max(1, Tt - 1), Tt, max(1, (Tt + 1) // 2)]
        lens = torch.tensor([cyc[b % 4] for b in range(B)],
                            dtype=torch.int32, device="cuda")
        if rows is None:
            outs = m.lstm_fwd(X0, X1, W0, W1, i0, i1, lens, bar, True)
            dg = m.lstm_bwd(outs[4], outs[1], outs[0], dH,
                            W0.t().contiguous(), lens, bar)
        else:
            outs = m.lstm_fwd_multi(X0, X1, W0, W1, i0, i1, lens, bar, True,
                                    rows)
            dg = m.lstm_bwd_multi(outs[4], outs[1], outs[0], dH,
                                  W0.t().contiguous(), lens, bar, rows)
        assert int(bar[256].item()) == 0, "poison word set"
        print(json.dumps(dict(B=B, T=Tt, rows_per_pass=rows,
                              build=so or "this tree",
                              outputs_sha256=digest(list(outs) + [dg]))),
              flush=True)


def main(rounds=5, calls=20, sets=4, so=None, shapes=False):
    if so:
        m = load_so(so)
    else:
        from r2d2_amd.ops import hip_ops
        m = hip_ops.ext(required=True)
    if shapes:
        return shape_digests(m, so)
    bar = torch.zeros(512, dtype=torch.int32, device="cuda")
    for B, multi in ((64, False), (128, True)):
        ins = make_inputs(B, sets)
        fb = make_calls(m, B, multi, ins, bar)
        for i, s in enumerate(ins):
            s["Hk"], s["C"], _, _, s["S"] = fb[0](i)
        for j, name in enumerate(("fwd2", "bwd")):
            out = fb[j](0)
            dig = digest(out if j == 0 else [out])
            for i in range(5):
                fb[j](i)
            res = [device_us(fb[j], calls) for _ in range(rounds)]
            assert int(bar[256].item()) == 0, "poison word set"
            print(json.dumps(dict(
                entry=name + ("_multi" if multi else ""), B=B, T=T,
                build=so or "this tree", us_median_min_max=stats(res),
                us_per_time_step=stats(res, T), outputs_sha256=dig)),
                flush=True)


if __name__ == "__main__":
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    so = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("so=")]
    main(*nums[:3], so=so[0] if so else None, shapes="shapes" in sys.argv)
