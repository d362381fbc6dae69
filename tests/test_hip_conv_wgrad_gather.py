"""GPU numerics: the per-image band wgrad, whose MFMA B fragments are
gathered straight out of the LDS image, vs an independent reference.

Reference: the f32 torch weight and bias gradient (autograd of F.conv2d in
float32, on the CPU) of the same bf16-rounded inputs, with the ReLU mask
applied to dY.  The chunked kernel shares WgradTile with the band kernel and
is therefore no reference here.

Tolerance: close(rtol=2e-3, atol=1e-2), as the other wgrad tests use.  Both
sides accumulate exact bf16 products in f32, so it is loose, not tight.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

# layer -> (conv_id, CIN, COUT, kernel, stride, input H = W).  Output pixels
# per image: 400 = 12*32 + 16, 81 = 2*32 + 17, 49 = 32 + 17, so every layer
# ends each image with a partly filled 32-row tile.
GEO = {
    "conv1_c4": (1, 4, 32, 8, 4, 84),
    "conv1_c1": (1, 1, 32, 8, 4, 84),
    "conv2": (2, 32, 64, 4, 2, 20),
    "conv3": (3, 64, 64, 3, 1, 9),
}
LAYERS = list(GEO)


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


def out_hw(layer):
    _, _, _, k, s, inhw = GEO[layer]
    return (inhw - k) // s + 1


def random_input(layer, N, gen):
    conv_id, cin, _, _, _, inhw = GEO[layer]
    if conv_id == 1:
        return torch.randint(0, 256, (N, inhw, inhw, cin), dtype=torch.uint8,
                             device="cuda", generator=gen)
    return torch.randn(N, inhw, inhw, cin, device="cuda",
                       generator=gen).bfloat16()


def position_coded_input(layer, N):
    """Integer codes of the position (y, x, c).  An image has more elements
    (up to 28224) than u8 or bf16 have exact small integers (256), so the
    code is 97 * linear index mod 251, shifted by 5 per image: two elements
    share a value only when their linear indices differ by a multiple of
    251, which no neighbouring pixel, kernel row, channel or image does."""
    conv_id, cin, _, _, _, inhw = GEO[layer]
    idx = torch.arange(inhw * inhw * cin, device="cuda").view(1, inhw, inhw, cin)
    img = torch.arange(N, device="cuda").view(N, 1, 1, 1)
    code = (idx * 97 + img * 5) % 251
    return code.to(torch.uint8) if conv_id == 1 else code.bfloat16()


def random_grads(layer, N, gen):
    _, _, cout, _, _, _ = GEO[layer]
    rows = N * out_hw(layer) ** 2
    dY = (torch.randn(rows, cout, device="cuda", generator=gen) * 0.5).bfloat16()
    act = torch.randn(rows, cout, device="cuda", generator=gen).bfloat16()
    return dY, act


def reference(layer, x_in, dY, act):
    """f32 autograd of F.conv2d on the CPU; dWt in the packed (COUT, ky, kx,
    c) layout the kernels accumulate in."""
    conv_id, cin, cout, k, s, inhw = GEO[layer]
    N, ohw = x_in.shape[0], out_hw(layer)
    x = x_in.cpu()
    if conv_id == 1:        # the kernels' fused dequant: bf16(u8 * (1/255))
        x = (x.float() * torch.tensor(1.0, dtype=torch.float32).div(255.0))
        x = x.bfloat16()
    x = x.float().permute(0, 3, 1, 2).contiguous()
    dym = torch.where(act.float() > 0, dY.float(), torch.zeros((), device="cuda"))
    dym = dym.cpu().view(N, ohw, ohw, cout).permute(0, 3, 1, 2).contiguous()
    w = torch.zeros(cout, cin, k, k, requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    F.conv2d(x, w, b, stride=s).backward(dym)
    return w.grad.permute(0, 2, 3, 1).reshape(cout, -1), b.grad


def check(layer, x_in, dY, act, name):
    conv_id = GEO[layer][0]
    dWt, db = M_.conv_wgrad_band(dY, act, x_in, conv_id, x_in.shape[0])
    dWt_ref, db_ref = reference(layer, x_in, dY, act)
    close(dWt.cpu(), dWt_ref, rtol=2e-3, atol=1e-2, name=f"{name} dWt {layer}")
    close(db.cpu(), db_ref, rtol=2e-3, atol=1e-2, name=f"{name} db {layer}")
    return dWt_ref, db_ref


def gen_for(layer, seed):
    return torch.Generator(device="cuda").manual_seed(
        1000 * seed + LAYERS.index(layer))


@pytest.mark.parametrize("layer", LAYERS)
def test_one_image_with_tail_tile(layer):
    g = gen_for(layer, 1)
    x_in = random_input(layer, 1, g)
    dY, act = random_grads(layer, 1, g)
    check(layer, x_in, dY, act, "N=1")


@pytest.mark.parametrize("layer", LAYERS)
def test_position_coded_input(layer):
    """A fragment piece gathered from a wrong address changes the answer."""
    g = gen_for(layer, 2)
    N = 3
    x_in = position_coded_input(layer, N)
    dY, act = random_grads(layer, N, g)
    check(layer, x_in, dY, act, "position-coded")


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("layer", LAYERS)
def test_single_nonzero_dy_row(layer, where):
    """dY zero except the last pixel of the last image (the tail tile's last
    filled row) / the first pixel of the first image (row 0 offsets): dWt is
    then that one pixel's patch times its dY row."""
    g = gen_for(layer, 3)
    N = 3
    x_in = position_coded_input(layer, N)
    dY, _ = random_grads(layer, N, g)
    row = dY.shape[0] - 1 if where == "last" else 0
    keep = dY[row].clone()
    dY.zero_()
    dY[row] = keep
    act = torch.ones_like(dY)
    dWt_ref, db_ref = check(layer, x_in, dY, act, f"{where} pixel only")
    assert dWt_ref.abs().max() > 0 and db_ref.abs().max() > 0


@pytest.mark.parametrize("layer", LAYERS)
def test_relu_mask_half_nonpositive(layer):
    """act <= 0 (negative or exactly zero) on a random half of the entries."""
    g = gen_for(layer, 4)
    N = 3
    x_in = random_input(layer, N, g)
    dY, act = random_grads(layer, N, g)
    u = torch.rand(act.shape, device="cuda", generator=g)
    act = act.abs() + 0.125
    act = torch.where(u < 0.25, -act, act)
    act = torch.where((u >= 0.25) & (u < 0.5), torch.zeros_like(act), act)
    check(layer, x_in, dY, act, "masked half")


# ceil(N / 512) images per workgroup: N = 1030 gives three, so the later
# images restage over live LDS, and a ragged last workgroup (one image).
# conv3 has the smallest images, one-channel conv1 the narrowest k runs.
@pytest.mark.parametrize("layer", ["conv3", "conv1_c1"])
def test_several_images_per_workgroup(layer):
    g = gen_for(layer, 5)
    N = 1030
    x_in = random_input(layer, N, g)
    dY, act = random_grads(layer, N, g)
    check(layer, x_in, dY, act, "N=1030")
