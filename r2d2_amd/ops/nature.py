"""Nature-CNN encoder on the gfx950 HIP kernels (the flagship config).

conv1 8x8 s4 -> conv2 4x4 s2 -> conv3 3x3 s1 -> fc 3136->512 through
ops/hip/conv_kernels.hip (implicit-GEMM MFMA, NHWC, fused u8 dequant) and
the dense GEMMs.  Same interface as ops/impala.py and ops/mlp.py: a weight
pack, `prepare_obs`, `fwd_pair` (train step, both networks), `fwd` (actor
inference) and `bwd`.  The extension `m` is an argument of every call.
"""

import torch


class Pack:
    """Prepacked weights for one NatureCNN."""

    def __init__(self, enc, device, with_bwd: bool):
        self.enc = enc
        self.device = device
        self.with_bwd = with_bwd
        self.refresh()

    def refresh(self):
        enc = self.enc
        dev = self.device
        to_bf = lambda t: t.detach().to(dev).bfloat16().contiguous()
        f32 = lambda t: t.detach().to(dev).float().contiguous()

        # convs: (COUT, CIN, KH, KW) -> (COUT, KH*KW*CIN)
        def pack_conv(conv):
            w = conv.weight.detach()
            wt = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
            return to_bf(wt), f32(conv.bias)

        self.w1t, self.b1 = pack_conv(enc.conv1)
        self.w2t, self.b2 = pack_conv(enc.conv2)
        self.w3t, self.b3 = pack_conv(enc.conv3)

        # FC: torch flattens NCHW (64,7,7); conv3 output flattens HWC
        wf = enc.fc.weight.detach()          # (512, 3136) over (c,h,w)
        wf_hwc = (wf.reshape(512, 64, 7, 7).permute(0, 2, 3, 1)
                  .reshape(512, 3136))
        self.wft = to_bf(wf_hwc)
        self.bf = f32(enc.fc.bias)

        if not self.with_bwd:
            return
        # dgrad prepacks (W stored (K, N))
        self.wf_kn = self.wft.t().contiguous()         # (3136, 512)
        w3 = enc.conv3.weight.detach().to(dev)             # (64,64,3,3)
        w3_nhwc = w3.permute(0, 2, 3, 1)                   # (co,dy,dx,ci)
        self.w3d = (w3_nhwc.permute(3, 1, 2, 0)            # (ci,dy,dx,co)
                    .reshape(64, 9 * 64).bfloat16().contiguous())
        # conv2 (stride 2): one (ci, tap, co) slab per parity class
        # (py, px), at index 2*py + px of a single tensor; the class's
        # taps are dy = py, py+2 (outer) by dx = px, px+2
        w2 = enc.conv2.weight.detach().to(dev)             # (64,32,4,4)
        w2_nhwc = w2.permute(0, 2, 3, 1)                   # (co,dy,dx,ci)
        slabs = []
        for py in range(2):
            for px in range(2):
                tap_list = [(dy, dx) for dy in range(py, 4, 2)
                            for dx in range(px, 4, 2)]
                wd = torch.stack([w2_nhwc[:, d, x, :] for d, x in tap_list],
                                 dim=0)                    # (t, co, ci)
                slabs.append(wd.permute(2, 0, 1).reshape(32, 4 * 64))
        self.w2d = torch.stack(slabs).bfloat16().contiguous()  # (4,32,256)


def prepare_obs(obs, B, T, C):
    """(B, T, 84, 84, C) or (B, T, C, 84, 84) u8 -> (B*T, 84, 84, C)."""
    if obs.shape[-1] == C and obs.shape[2] == 84:   # already HWC
        return obs.reshape(B * T, 84, 84, C)
    return obs.permute(0, 1, 3, 4, 2).reshape(B * T, 84, 84, C).contiguous()


def _fc_fwd(m, p, a1, a2, a3):
    flat = a3.view(a3.shape[0] // 49, 3136)
    latent = m.gemm_bias_act(flat, p.wft, p.bf, 1, False)
    return latent, (a1, a2, a3, flat)


def _band_from_a1(m, p, a1):
    """Above conv1 on the per-image band forwards (image LDS-resident, one
    global read per input element): a1 (M*400, 32) bf16 -> latent (M, 512)
    bf16 + stashes."""
    M = a1.shape[0] // 400
    a2 = m.conv_fwd_band(a1, p.w2t, p.b2, 2, M)
    a3 = m.conv_fwd_band(a2, p.w3t, p.b3, 3, M)
    return _fc_fwd(m, p, a1, a2, a3)


def _classic(m, p, obs):
    """The tiled conv_fwd chain: obs (M, 84, 84, C) u8 -> latent + stashes."""
    M = obs.shape[0]
    a1 = m.conv_fwd(obs, p.w1t, p.b1, 1, M, 84, 84, 20, 20, True)
    a2 = m.conv_fwd(a1, p.w2t, p.b2, 2, M, 20, 20, 9, 9, True)
    a3 = m.conv_fwd(a2, p.w3t, p.b3, 3, M, 9, 9, 7, 7, True)
    return _fc_fwd(m, p, a1, a2, a3)


def fwd_pair(m, online, target, obs, *, fwd_band, mark):
    """Both networks over the same frames -> (lat_o, online stash, lat_t).
    With `fwd_band`, conv1 runs once for the two (conv1_fwd_dual: one
    staging of each frame); otherwise two classic passes."""
    if fwd_band:
        a1_o, a1_t = m.conv1_fwd_dual(obs, online.w1t, online.b1, target.w1t,
                                      target.b1, obs.shape[0])
        mark("conv1_dual")
        lat_o, stash = _band_from_a1(m, online, a1_o)
        mark("enc_online")
        lat_t, _ = _band_from_a1(m, target, a1_t)
    else:
        lat_o, stash = _classic(m, online, obs)
        mark("enc_online")
        lat_t, _ = _classic(m, target, obs)
    mark("enc_target")
    return lat_o, stash, lat_t


def fwd(m, pack, obs):
    """Actor inference: obs (E, C, 84, 84) u8 -> latent (E, 512) bf16, on
    the classic chain (the actors' batch sizes)."""
    return _classic(m, pack, obs.permute(0, 2, 3, 1).contiguous())[0]


def _conv_bwd_slab(m, p, enc, dflat3, stash, obs, M, ws):
    """Conv backward on the slab path.  Every dY is already masked (by the
    FC dgrad's and the conv dgrads' stores), so the wgrads get no mask to
    re-read; each reducer overwrites its .grad views of the flat buffer in
    torch layout, so nothing is zeroed or copied."""
    a1, a2 = stash[:2]
    C = obs.shape[-1]
    band1 = C == 4
    need = max(m.conv_wgrad_ws_floats(3, 0, M, True),
               m.conv_wgrad_ws_floats(2, 0, M, True),
               m.conv_wgrad_ws_floats(1, C, M, band1))
    if "wgrad" not in ws or ws["wgrad"].numel() < need:
        # one partial-sum workspace for the three layers (they run one
        # after the other), kept from step to step
        ws["wgrad"] = torch.empty(need, dtype=torch.float32,
                                  device=obs.device)
    part, no_mask = ws["wgrad"], torch.Tensor()
    m.conv_wgrad_band_into(dflat3, no_mask, a2, 3, M, part,
                           enc.conv3.weight.grad, enc.conv3.bias.grad)
    d_a2 = m.conv_dgrad_band(dflat3, p.w3d, a2, 3, M)
    d_a2f = d_a2.view(M * 81, 64)
    m.conv_wgrad_band_into(d_a2f, no_mask, a1, 2, M, part,
                           enc.conv2.weight.grad, enc.conv2.bias.grad)
    d_a1 = m.conv_dgrad_band(d_a2f, p.w2d, a1, 2, M).view(M * 400, 32)
    # conv1: band with four channels, chunked with one (see _conv_bwd_atomic)
    if band1:
        m.conv_wgrad_band_into(d_a1, no_mask, obs, 1, M, part,
                               enc.conv1.weight.grad, enc.conv1.bias.grad)
    else:
        m.conv_wgrad_into(d_a1, no_mask, obs, 1, M, 84, 84, 20, 20,
                          32, 8 * 8 * C, part, enc.conv1.weight.grad,
                          enc.conv1.bias.grad)


def _conv_bwd_atomic(m, p, dflat3, stash, obs, M):
    """R2D2_CONV_WGRAD_SLAB=0: the atomic-flush wgrads (A/B reference).
    Returns (dW, db, packed shape) of conv1..3 for `bwd` to copy: the weight
    grads accumulate in the packed (COUT, ky, kx, c) layout — torch-layout
    atomics scatter each 16-lane wave across 16 cachelines (measured 4-5x
    slower) — and are permuted into .grad afterwards (tiny tensors)."""
    a1, a2, a3 = stash[:3]
    C = obs.shape[-1]
    # per-image band wgrads: whole input image staged in LDS once
    # (single dequant per element; conv1 patch traffic 557 -> 154 MB)
    dW3, db3 = m.conv_wgrad_band(dflat3, a3, a2, 3, M)
    # per-image band dgrad (dY staged once in LDS inside a zero halo, no
    # zero-padded staging copies in memory); the output mask fuses
    # conv2's relu backward into the d_a2 store
    d_a2 = m.conv_dgrad_band(dflat3, p.w3d, a2, 3, M)
    # conv2 backward (d_a2 pre-masked by a2); all four stride-parity
    # classes of the dgrad run in the one launch
    d_a2f = d_a2.view(M * 81, 64)
    dW2, db2 = m.conv_wgrad_band(d_a2f, a2, a1, 2, M)
    d_a1 = m.conv_dgrad_band(d_a2f, p.w2d, a1, 2, M)
    # conv1 wgrad (no dgrad: input is data; d_a1 pre-masked by a1).
    # Each channel count runs the kernel measured faster for it, 5440
    # images, device events, medians of two rounds (docs/STATUS.md):
    # four channels (K = 256) 0.193 ms band vs 0.246-0.250 ms chunked —
    # with the fragments gathered from the LDS image the band no longer
    # pays an im2col copy and two barriers per 32 rows; one channel
    # (K = 64) 0.116-0.117 ms chunked vs 0.120 ms band — the image is a
    # quarter of the size, so there is little staging left to save.
    if C == 4:
        dW1, db1 = m.conv_wgrad_band(d_a1.view(M * 400, 32), a1, obs, 1, M)
    else:
        dW1, db1 = m.conv_wgrad(d_a1.view(M * 400, 32), a1, obs, 1,
                                M, 84, 84, 20, 20, 32, 8 * 8 * C)
    return ((dW1, db1, (32, 8, 8, C)), (dW2, db2, (64, 4, 4, 32)),
            (dW3, db3, (64, 3, 3, 64)))


def bwd(m, pack, enc, stash, dlat, lat_o, obs, *, wgrad_slab, mark, ws):
    """dlat (M, 512) bf16 -> the encoder's .grad views.  `ws` is a dict the
    caller keeps from step to step (the slab wgrads' workspace)."""
    a3, flat = stash[2:]
    M = dlat.shape[0]
    # FC dgrad with BOTH relu backwards fused: the mask of the FC's own
    # relu (lat_o, the forward output) on load, conv3's relu mask (a3) on
    # store — dflat leaves this kernel pre-masked, so no elementwise
    # mask/pad passes run on the conv gradients at all.
    dflat = m.gemm_dgrad(dlat, lat_o, pack.wf_kn, True, 0, a3)
    dWf, dbf = m.gemm_wgrad(dlat, lat_o, flat, True, True)
    mark("fc_bwd")
    dflat3 = dflat.view(M * 49, 64)   # pre-masked by a3
    if wgrad_slab:
        _conv_bwd_slab(m, pack, enc, dflat3, stash, obs, M, ws)
        mark("conv_bwd")
    else:
        packed = _conv_bwd_atomic(m, pack, dflat3, stash, obs, M)
        mark("conv_bwd")
        for conv, (dwt, db, khwc) in zip((enc.conv1, enc.conv2, enc.conv3),
                                         packed):
            conv.weight.grad.copy_(dwt.view(khwc).permute(0, 3, 1, 2))
            conv.bias.grad.copy_(db)
    enc.fc.weight.grad.copy_(
        dWf.view(512, 7, 7, 64).permute(0, 3, 1, 2).reshape(512, 3136))
    enc.fc.bias.grad.copy_(dbf)
