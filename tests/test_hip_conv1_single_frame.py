"""GPU numerics: the one-input-channel conv1 kernels (single 84x84 frame,
K = 64) vs fp32 eager references and vs each other, plus the host launcher
guards.  Helpers and tolerances are those of test_hip_gemm_conv.py — the
arithmetic (bf16 MFMA, f32 accumulation, u8/255 dequant) is the same."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

CIN, COUT, KS, S, INHW, OHW = 1, 32, 8, 4, 84, 20


def close(a, b, rtol=3e-2, atol=None, name=""):
    a = a.float()
    b = b.float()
    if atol is None:
        atol = 3e-2 * max(1.0, float(b.abs().max()))
    ok = torch.allclose(a, b, rtol=rtol, atol=atol)
    if not ok:
        d = (a - b).abs()
        print(f"{name}: max diff {d.max().item()} at scale {b.abs().max().item()}")
    assert ok, name


def prepack_w(w):  # (COUT, CIN, KH, KW) -> (COUT, KH*KW*CIN)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def frames(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (N, INHW, INHW, CIN), dtype=torch.uint8,
                         device="cuda", generator=g)


def weights(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(COUT, CIN, KS, KS, device="cuda", generator=g)
         * 0.2).bfloat16()
    b = torch.randn(COUT, device="cuda", generator=g) * 0.1
    return w, b


def fwd(x, w, b):
    return M_.conv_fwd(x, prepack_w(w), b, 1, x.shape[0], INHW, INHW,
                       OHW, OHW, True)


# N = 1: fewer rows than one 128-row tile per wave set; N = 3: M = 1200 is
# 9 full 128-row tiles + a 48-row tail (row guard).  A whole image covers
# every ox parity, i.e. both 4-byte phases of the patch-row address.
@pytest.mark.parametrize("N", [1, 3])
def test_conv1_c1_fwd_matches_eager(N):
    x = frames(N, 100 + N)
    w, b = weights(1)
    out = fwd(x, w, b)
    assert out.shape == (N * OHW * OHW, COUT)
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).float() / 255.0, w.float(),
                          b, stride=S))
    ref = ref.permute(0, 2, 3, 1).reshape(N * OHW * OHW, COUT)
    close(out, ref, rtol=5e-2, name=f"conv1 c1 fwd N={N}")


# the launcher packs ceil(N/2048) images per workgroup: N = 3 runs one image
# per workgroup, N = 2049 runs two with a one-image last workgroup
@pytest.mark.parametrize("N", [3, 2049])
def test_conv1_c1_fwd_band_matches_classic(N):
    x = frames(N, 200 + N)
    w, b = weights(2)
    ref = fwd(x, w, b)
    out = M_.conv_fwd_band(x, prepack_w(w), b, 1, N)
    # same k order and the same two-MFMA accumulation chain per element
    assert torch.equal(out, ref), (out.float() - ref.float()).abs().max()


def test_conv1_c1_wgrad_matches_autograd():
    N = 3
    x = frames(N, 300)
    w, _ = weights(3)
    b = torch.zeros(COUT, device="cuda")
    out = fwd(x, w, b)
    frac = float((out.float() > 0).float().mean())
    assert 0.1 < frac < 0.9, frac      # the ReLU mask has zeros and ones
    g = torch.Generator(device="cuda").manual_seed(301)
    dY = (torch.randn(N * OHW * OHW, COUT, device="cuda", generator=g)
          * 0.5).bfloat16()

    # the kernel dequantizes to bf16; round the reference the same way
    ref_in = (x.permute(0, 3, 1, 2).float() / 255.0).bfloat16().float()
    w32 = w.float().requires_grad_(True)
    b32 = b.clone().requires_grad_(True)
    out32 = F.relu(F.conv2d(ref_in, w32, b32, stride=S))
    out32.backward(dY.reshape(N, OHW, OHW, COUT).permute(0, 3, 1, 2).float())

    dWt, db = M_.conv_wgrad(dY, out, x, 1, N, INHW, INHW, OHW, OHW, COUT,
                            KS * KS * CIN)
    assert dWt.shape == (COUT, KS * KS * CIN)
    close(dWt, prepack_w(w32.grad), rtol=5e-2, atol=0.5, name="conv1 c1 wgrad")
    close(db, b32.grad, rtol=5e-2, atol=0.5, name="conv1 c1 bgrad")


def test_conv1_c1_wgrad_band_matches_chunked():
    N = 3
    x = frames(N, 400)
    g = torch.Generator(device="cuda").manual_seed(401)
    dY = (torch.randn(N * OHW * OHW, COUT, device="cuda", generator=g)
          * 0.5).bfloat16()
    act = torch.randn(N * OHW * OHW, COUT, device="cuda",
                      generator=g).bfloat16()
    dWt_ref, db_ref = M_.conv_wgrad(dY, act, x, 1, N, INHW, INHW, OHW, OHW,
                                    COUT, KS * KS * CIN)
    dWt, db = M_.conv_wgrad_band(dY, act, x, 1, N)
    close(dWt, dWt_ref, rtol=2e-3, atol=1e-2, name="band wgrad c1")
    close(db, db_ref, rtol=2e-3, atol=1e-2, name="band bgrad c1")


# -------------------------------------------------------------------------
# Host launcher guards: error path only, the checks fire before any launch
# -------------------------------------------------------------------------

def _all_entry_points(x, N):
    w, b = weights(5)
    wt = prepack_w(w)
    dY = torch.zeros(N * OHW * OHW, COUT, device="cuda").bfloat16()
    return [
        lambda: M_.conv_fwd(x, wt, b, 1, N, INHW, INHW, OHW, OHW, True),
        lambda: M_.conv_fwd_band(x, wt, b, 1, N),
        lambda: M_.conv_wgrad(dY, dY, x, 1, N, INHW, INHW, OHW, OHW, COUT,
                              KS * KS * CIN),
        lambda: M_.conv_wgrad_band(dY, dY, x, 1, N),
    ]


def test_conv1_rejects_non_contiguous_input():
    wide = torch.zeros(2, INHW, INHW, 2, dtype=torch.uint8, device="cuda")
    x = wide[..., :1]                      # (2, 84, 84, 1), strided
    assert not x.is_contiguous()
    for call in _all_entry_points(x, 2):
        with pytest.raises(RuntimeError, match="contiguous"):
            call()


def test_conv1_rejects_misaligned_base_pointer():
    buf = torch.zeros(INHW * INHW + 16, dtype=torch.uint8, device="cuda")
    x = buf[1:1 + INHW * INHW].view(1, INHW, INHW, 1)
    assert x.is_contiguous() and x.data_ptr() % 4 == 1
    for call in _all_entry_points(x, 1):
        with pytest.raises(RuntimeError, match="aligned"):
            call()


def test_conv1_rejects_other_channel_counts():
    x = torch.zeros(1, INHW, INHW, 2, dtype=torch.uint8, device="cuda")
    for call in _all_entry_points(x, 1):
        with pytest.raises(RuntimeError, match="1 or 4 input channels"):
            call()
