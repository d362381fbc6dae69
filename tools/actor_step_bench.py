"""Actor tick alone on one GPU: HipInference.forward against HipInference.step
(nature, four channels), alternated in one process, at E in {5, 64, 256}.

Per variant and E: device time per call (events around a batch of calls) and
host wall time per call (the launching thread's time to ENQUEUE a call, no
sync inside), medians with min/max over rounds.  Then the cell kernel alone
at every (units, rows) tile.  One JSON line per figure.

    python tools/actor_step_bench.py [rounds] [calls_per_round]
"""

import json
import statistics
import sys
import time

sys.path.insert(0, ".")

import torch  # noqa: E402


def stats(xs):
    return dict(median=round(statistics.median(xs), 2),
                min=round(min(xs), 2), max=round(max(xs), 2))


def device_us(fn, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def host_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt * 1e6 / calls


def main(rounds=7, calls=50):
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.ops.engine import HipInference

    c = cfg.apply("mspacman_gpu_replay")
    torch.manual_seed(0)
    net = Network(c.action_dim, c.obs_shape, 512, encoder="nature",
                  forward_steps=c.forward_steps).cuda().eval()
    inf = HipInference(net, "cuda")
    m, p, A = inf.m, inf.pack, c.action_dim
    for E in (5, 64, 256):
        obs = torch.randint(0, 256, (E, 4, 84, 84), device="cuda",
                            dtype=torch.uint8)
        la = torch.zeros(E, A, device="cuda")
        la[:, 0] = 1.0
        lr = torch.zeros(E, 1, device="cuda")
        hid = (torch.randn(1, E, 512, device="cuda") * 0.1,
               torch.randn(1, E, 512, device="cuda") * 0.1)
        variants = {"forward": lambda: inf.forward(obs, la, lr, hid),
                    "step": lambda: inf.step(obs, la, lr, hid)}
        for fn in variants.values():          # warm-up
            for _ in range(10):
                fn()
        res = {k: {"device_us": [], "host_us": []} for k in variants}
        for _ in range(rounds):               # alternated
            for k, fn in variants.items():
                res[k]["device_us"].append(device_us(fn, calls))
                res[k]["host_us"].append(host_us(fn, calls))
        for k in variants:
            print(json.dumps(dict(what="tick", E=E, variant=k,
                                  device_us=stats(res[k]["device_us"]),
                                  host_us=stats(res[k]["host_us"]))),
                  flush=True)

        # the cell kernel alone, every tile
        lat = torch.randn(E, 512, device="cuda").bfloat16()
        lr1 = lr.reshape(E)
        h0, c0 = hid[0][0], hid[1][0]
        h1, c1 = torch.empty_like(h0), torch.empty_like(c0)
        hb = torch.empty(E, 512, device="cuda", dtype=torch.bfloat16)
        tiles = [(u, r) for u in (8, 16) for r in (16, 32, 64)]
        cell = {t: (lambda t=t: m.lstm_cell_step(
            lat, la, lr1, h0, c0, p.wih_t, p.whh_t, p.lstm_bias, h1, c1, hb,
            units=t[0], rows=t[1])) for t in tiles}
        adv1, val1 = torch.empty_like(hb), torch.empty_like(hb)
        hidden = {r: (lambda r=r: m.head_hidden_step(
            hb, p.wa1t, p.ba1, p.wv1t, p.bv1, adv1, val1, rows=r))
            for r in (16, 64)}
        for name, group in (("cell", cell), ("head_hidden", hidden)):
            out = {t: [] for t in group}
            for fn in group.values():
                fn()
            for _ in range(rounds):
                for t, fn in group.items():
                    out[t].append(device_us(fn, 4 * calls))
            for t in group:
                print(json.dumps(dict(what=name, E=E, tile=t,
                                      device_us=stats(out[t]))), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7,
         int(sys.argv[2]) if len(sys.argv) > 2 else 50)
