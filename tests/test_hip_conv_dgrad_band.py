"""GPU: the per-image band dgrad (conv_dgrad_band) against the dense
per-parity-class dgrad (conv_dgrad_dense), which it must equal bit for bit:
both run every output element through the same sequence of MFMA
accumulations (k tap-major, co-minor, 32 per step, out-of-image taps as zero
fragments)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

# conv_id -> CIN, COUT, K, S, XH (dX is XH x XH x CIN, dY is OH x OH x COUT)
GEO = {3: (64, 64, 3, 1, 9), 2: (32, 64, 4, 2, 20)}


def _oh(conv_id):
    _, _, k, s, xh = GEO[conv_id]
    return (xh - k) // s + 1


def _weights(conv_id, seed):
    cin, cout, k, _, _ = GEO[conv_id]
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(cout, cin, k, k, device="cuda", generator=g)
            * 0.2).bfloat16()


def _class_packs(conv_id, w):
    """[(py, px, Wd (CIN, TAPS*COUT), taps)] in class order py*S + px."""
    cin, cout, k, s, _ = GEO[conv_id]
    w_nhwc = w.permute(0, 2, 3, 1)                      # (co, dy, dx, ci)
    out = []
    for py in range(s):
        for px in range(s):
            tap_list = [(dy, dx) for dy in range(py, k, s)
                        for dx in range(px, k, s)]
            wd = torch.stack([w_nhwc[:, d, x, :] for d, x in tap_list], dim=0)
            wd = (wd.permute(2, 0, 1).reshape(cin, len(tap_list) * cout)
                  .contiguous())
            taps = torch.tensor(tap_list, dtype=torch.int32, device="cuda")
            out.append((py, px, wd, taps))
    return out


def _dense(conv_id, w, dy, actx, N):
    cin, cout, _, s, xh = GEO[conv_id]
    oh = _oh(conv_id)
    dX = torch.full((N, xh, xh, cin), float("nan"), device="cuda",
                    dtype=torch.bfloat16)
    for py, px, wd, taps in _class_packs(conv_id, w):
        M_.conv_dgrad_dense(dy.view(-1, cout), wd, taps, actx, N, oh, oh,
                            cout, xh, xh, cin, py, px, s, dX)
    return dX


def _band(conv_id, w, dy, actx, N, max_wgs=0):
    Wd = torch.stack([p[2] for p in _class_packs(conv_id, w)]).contiguous()
    return M_.conv_dgrad_band(dy, Wd, actx, conv_id, N, max_wgs)


def _empty():
    return torch.empty(0, device="cuda", dtype=torch.bfloat16)


@pytest.mark.parametrize("max_wgs", [0, 2])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("conv_id", [3, 2])
def test_band_bit_equal_to_dense(conv_id, N, masked, max_wgs):
    """N = 5 on two workgroups: one takes 3 images, the other 2 (the
    multi-image loop and the tail)."""
    cin, cout, _, _, xh = GEO[conv_id]
    oh = _oh(conv_id)
    g = torch.Generator(device="cuda").manual_seed(100 * conv_id + N)
    w = _weights(conv_id, conv_id)
    dy = torch.randn(N, oh, oh, cout, device="cuda", generator=g).bfloat16()
    actx = (torch.randn(N, xh, xh, cin, device="cuda", generator=g).bfloat16()
            if masked else _empty())
    ref = _dense(conv_id, w, dy, actx, N)
    out = _band(conv_id, w, dy, actx, N, max_wgs)
    assert out.shape == ref.shape
    assert not torch.isnan(ref.float()).any()
    assert torch.equal(out, ref), (out.float() - ref.float()).abs().max()


@pytest.mark.parametrize("corner", [(0, 0), (0, -1), (-1, 0), (-1, -1)])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("conv_id", [3, 2])
def test_single_corner_pixel_reaches_only_its_receptive_field(conv_id, which,
                                                              corner):
    """One image of three has one non-zero dY pixel at a corner; all three
    run through ONE workgroup.  A wrong halo or parity-class offset moves or
    clips the footprint, LDS left from the image before leaks it into the
    next one."""
    cin, cout, k, s, xh = GEO[conv_id]
    oh = _oh(conv_id)
    N = 3
    w = _weights(conv_id, 7)
    g = torch.Generator(device="cuda").manual_seed(9)
    dy = torch.zeros(N, oh, oh, cout, device="cuda", dtype=torch.bfloat16)
    dy[which, corner[0], corner[1]] = torch.randn(
        cout, device="cuda", generator=g).bfloat16()

    # float64 autograd on the host; the same pass over |w|, |dY| bounds the
    # sum of the absolute terms of every element
    def grad64(wt, g):
        x = torch.zeros(N, cin, xh, xh, dtype=torch.float64,
                        requires_grad=True)
        F.conv2d(x, wt.double().cpu(), stride=s).backward(
            g.permute(0, 3, 1, 2).double().cpu())
        return x.grad.permute(0, 2, 3, 1).cuda()        # (N, XH, XH, CIN)

    ref, ref_abs = grad64(w, dy), grad64(w.abs(), dy.abs())

    out = _band(conv_id, w, dy, _empty(), N, max_wgs=1)
    for n in range(N):
        if n != which:
            assert not out[n].float().any(), f"image {n} must stay zero"
    # the receptive field is the k x k window at the pixel's patch origin;
    # random weights make every element of it non-zero in float64
    oy, ox = (corner[0] % oh) * s, (corner[1] % oh) * s
    field = torch.zeros(xh, xh, dtype=torch.bool, device="cuda")
    field[oy:oy + k, ox:ox + k] = True
    assert torch.equal(ref[which].ne(0).all(-1), field)
    assert torch.equal(out[which].float().ne(0).any(-1), field)
    # one dY pixel: every dX element is one 64-term dot product of exact
    # bf16 products, summed in f32 (each of the 64 additions within 2^-24
    # of the absolute sum, doubled for the order inside an MFMA step) and
    # rounded once to bf16 (2^-8 relative, 2^-9 if to nearest)
    err = (out[which].double() - ref[which]).abs()
    bound = 2.0 ** -8 * ref[which].abs() + 2.0 ** -17 * ref_abs[which]
    print("max err", float(err.max()), "largest err/bound",
          float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("conv_id", [3, 2])
def test_mask_all_false_gives_zero_and_no_mask_overwrites_all(conv_id):
    cin, cout, _, _, xh = GEO[conv_id]
    oh = _oh(conv_id)
    N = 3
    w = _weights(conv_id, 11)
    g = torch.Generator(device="cuda").manual_seed(12)
    dy = torch.randn(N, oh, oh, cout, device="cuda", generator=g).bfloat16()
    # a mask that is false everywhere: zeros and negatives
    actx = -torch.rand(N, xh, xh, cin, device="cuda", generator=g).bfloat16()
    actx[0] = 0
    Wd = torch.stack([p[2] for p in _class_packs(conv_id, w)]).contiguous()
    out = M_.conv_dgrad_band(dy, Wd, actx, conv_id, N, 2)
    assert not out.float().any()
    assert not torch.signbit(out.float()).any()

    # no mask: dX is allocated by the call.  Fill the allocator's free
    # blocks of that size with NaN first (equal-size free blocks are handed
    # out before any other), so an element left unwritten shows
    poison = [torch.full((N, xh, xh, cin), float("nan"), device="cuda",
                         dtype=torch.bfloat16) for _ in range(8)]
    ptrs = {t.data_ptr() for t in poison}
    empty = _empty()
    del poison
    out = M_.conv_dgrad_band(dy, Wd, empty, conv_id, N, 2)
    assert out.data_ptr() in ptrs, "dX did not land on a NaN-filled block"
    assert not torch.isnan(out.float()).any()


def test_rejects_bad_arguments():
    w = _weights(3, 1)
    Wd = _class_packs(3, w)[0][2]
    dy = torch.zeros(2, 7, 7, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="conv_dgrad_band"):
        M_.conv_dgrad_band(dy, Wd, _empty(), 1, 2)          # conv1: no dgrad
    with pytest.raises(RuntimeError, match="conv_dgrad_band"):
        M_.conv_dgrad_band(dy, Wd, _empty(), 3, 3)          # N mismatch
    with pytest.raises(RuntimeError, match="conv_dgrad_band"):
        M_.conv_dgrad_band(dy, Wd[:, :512].contiguous(), _empty(), 3, 2)
    with pytest.raises(RuntimeError, match="conv_dgrad_band"):
        M_.conv_dgrad_band(dy, Wd, dy, 3, 2)                # mask size
    with pytest.raises(RuntimeError, match="conv_dgrad_band"):
        M_.conv_dgrad_band(dy.float(), Wd, _empty(), 3, 2)
