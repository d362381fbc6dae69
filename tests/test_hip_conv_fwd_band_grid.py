"""GPU: conv_fwd_band at every grid it can be given.  The k order of an output
element does not depend on how images are dealt to workgroups nor on where
the weights live (an LDS slab for conv1, registers for the 64-output
layers), so every grid is bit-equal to the classic conv_fwd."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

# (conv_id, cin) -> cout, k, s, inhw
GEO = {(1, 4): (32, 8, 4, 84), (1, 1): (32, 8, 4, 84),
       (2, 32): (64, 4, 2, 20), (3, 64): (64, 3, 1, 9)}
N = 5

_cases = {}


def _case(conv_id, cin):
    """inputs and the classic forward's output, computed once per layer"""
    key = (conv_id, cin)
    if key not in _cases:
        cout, k, s, inhw = GEO[key]
        ohw = (inhw - k) // s + 1
        g = torch.Generator(device="cuda").manual_seed(10 * conv_id + cin)
        w = (torch.randn(cout, cin, k, k, device="cuda", generator=g)
             * 0.2).bfloat16()
        wt = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
        b = torch.randn(cout, device="cuda", generator=g) * 0.1
        if conv_id == 1:
            x = torch.randint(0, 256, (N, inhw, inhw, cin), dtype=torch.uint8,
                              device="cuda", generator=g)
        else:
            x = torch.randn(N, inhw, inhw, cin, device="cuda",
                            generator=g).bfloat16()
        ref = M_.conv_fwd(x, wt, b, conv_id, N, inhw, inhw, ohw, ohw, True)
        _cases[key] = (x, wt, b, ref)
    return _cases[key]


@pytest.mark.parametrize("max_wgs", [0, 1, 2])
@pytest.mark.parametrize("conv_id,cin", sorted(GEO))
def test_every_grid_bit_equal_to_classic(conv_id, cin, max_wgs):
    """max_wgs = 1: one workgroup restages its LDS image five times;
    2: runs of 3 and 2 images, the ragged tail."""
    x, wt, b, ref = _case(conv_id, cin)
    out = M_.conv_fwd_band(x, wt, b, conv_id, N, max_wgs)
    assert out.shape == ref.shape and ref.float().abs().max() > 0
    assert torch.equal(out, ref), (out.float() - ref.float()).abs().max()


def test_five_argument_call_is_the_default_grid():
    x, wt, b, ref = _case(3, 64)
    assert torch.equal(M_.conv_fwd_band(x, wt, b, 3, N), ref)
    assert torch.equal(M_.conv_fwd_band(x, wt, b, 3, N, max_wgs=0), ref)
    with pytest.raises(RuntimeError, match="conv_fwd_band"):
        M_.conv_fwd_band(x, wt, b, 3, N, -1)
