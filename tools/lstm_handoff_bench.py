"""Microbench: price the LSTM producer-flag handoff protocol per step at a
given workgroup count (the per-step latency floor of the persistent LSTM
kernels — ops/hip/lstm_kernels.hip)."""

import sys
import time

import torch

sys.path.insert(0, ".")
from r2d2_amd.ops import hip_ops  # noqa: E402

m = hip_ops.ext(required=True)
steps = 85
for kind, fn in (("flags", m.handoff_bench),
                 ("counter", m.handoff_counter_bench)):
    for nblocks in (32, 64, 128, 256):
        bar = torch.zeros(512, dtype=torch.int32, device="cuda")
        fn(bar, steps, nblocks)  # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            fn(bar, steps, nblocks)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / reps / steps * 1e6
        print(f"{kind:8s} nblocks={nblocks:4d}: {us:7.2f} us/step "
              f"({us * steps * 1e-3:6.2f} ms per {steps}-step pass)")

# The counter handoff under the LSTM kernels' conditions: every block stores
# kb KB (16 B per lane) in front of each publish.  "dirty+fence": plain
# stores, then the release-fence publish.  "sc1 nofence": write-through
# stores, drain, barrier, counter add, no release fence.
for kind, mode in (("dirty+fence", 0), ("sc1 nofence", 1)):
    for nblocks in (64, 128):
        for kb in (0, 1, 2, 6, 16):
            bar = torch.zeros(512, dtype=torch.int32, device="cuda")
            scratch = torch.zeros(max(1, nblocks * kb * 512),
                                  dtype=torch.bfloat16, device="cuda")
            m.handoff_payload_bench(bar, scratch, steps, nblocks, kb, mode)
            torch.cuda.synchronize()
            assert int(bar[256].item()) == 0, "poison word set"
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for _ in range(20):
                m.handoff_payload_bench(bar, scratch, steps, nblocks, kb, mode)
            b.record()
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / 20 / steps
            print(f"{kind:12s} nblocks={nblocks:4d} kb={kb:3d}: "
                  f"{us:7.2f} us/step")
