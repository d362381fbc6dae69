"""MLP encoder (vector observations) on the gfx950 HIP kernels.

fc1 D->512 through ops/hip/mlp_kernels.hip (f32 in, bf16 out), fc2
512->512 through the dense GEMMs.  Same interface as ops/nature.py and
ops/impala.py.
"""

import torch


class Pack:
    """Prepacked weights for one MLPEncoder."""

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
        # fc1 stays f32 (the mlp_in kernels read it as it is); fc2 in
        # the GEMMs' bf16 layouts, (N, K) forward and (K, N) dgrad
        self.mw1, self.mb1 = f32(enc.fc1.weight), f32(enc.fc1.bias)
        self.mw2t, self.mb2 = to_bf(enc.fc2.weight), f32(enc.fc2.bias)
        if self.with_bwd:
            self.mw2_kn = self.mw2t.t().contiguous()       # (512, 512)


def prepare_obs(obs, B, T, C):
    """(B, T, D) float32 vector observations -> X (B*T, D), no dequant."""
    if obs.dtype != torch.float32 or tuple(obs.shape[2:]) != (C,):
        raise TypeError(
            f"the mlp encoder takes (B, T, {C}) float32 "
            f"observations, got {tuple(obs.shape)} {obs.dtype}")
    return obs.reshape(B * T, C).contiguous()


def _fwd(m, p, x):
    a1 = m.mlp_in_fwd(x, p.mw1, p.mb1)
    return m.gemm_bias_act(a1, p.mw2t, p.mb2, 1, False), (x, a1)


def fwd_pair(m, online, target, obs, *, fwd_band, mark):
    """Both networks over X (M, D) -> (lat_o, online stash (X, A1), lat_t)."""
    lat_o, stash = _fwd(m, online, obs)
    mark("enc_online")
    lat_t, _ = _fwd(m, target, obs)
    mark("enc_target")
    return lat_o, stash, lat_t


def fwd(m, pack, obs):
    """Actor inference: obs (E, D) float32 -> latent (E, 512) bf16."""
    return _fwd(m, pack, obs.contiguous())[0]


def bwd(m, pack, enc, stash, dlat, lat_o, obs, *, wgrad_slab, mark, ws):
    """fc2 dgrad with fc2's own relu mask (lat_o) on load and fc1's (A1) on
    store; both wgrads add straight into the .grad views."""
    X, a1 = stash
    d_a1 = m.gemm_dgrad(dlat, lat_o, pack.mw2_kn, True, 0, a1)
    m.gemm_wgrad_into(dlat, lat_o, a1, True, enc.fc2.weight.grad,
                      enc.fc2.bias.grad)
    m.mlp_in_wgrad_into(d_a1, X, enc.fc1.weight.grad, enc.fc1.bias.grad)
    mark("mlp_bwd")
