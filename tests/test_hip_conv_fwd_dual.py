"""GPU: conv1_fwd_dual, conv1 of the online and the target network from one
LDS staging of each frame.  Each output is bit-equal to conv_fwd_band with
that network's weights at every grid (same k order per output element), the
neighbouring frames in memory never leak in, every bad operand raises before
anything is allocated, and the engine step that runs it reproduces the
classic-forward step."""

import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

NS = (1, 2, 3, 7)
NMAX = max(NS)

_cases = {}


def _case(cin):
    """frames, two different weight draws and their conv_fwd_band outputs at
    NMAX images, computed once per channel count; never written to"""
    if cin not in _cases:
        g = torch.Generator(device="cuda").manual_seed(40 + cin)
        x = torch.randint(0, 256, (NMAX, 84, 84, cin), dtype=torch.uint8,
                          device="cuda", generator=g)
        nets = []
        for _ in range(2):
            w = (torch.randn(32, cin, 8, 8, device="cuda", generator=g)
                 * 0.2).bfloat16()
            wt = w.permute(0, 2, 3, 1).reshape(32, -1).contiguous()
            b = torch.randn(32, device="cuda", generator=g) * 0.1
            nets.append((w, wt, b, M_.conv_fwd_band(x, wt, b, 1, NMAX)))
        assert not torch.equal(nets[0][3], nets[1][3])
        _cases[cin] = (x, nets)
    return _cases[cin]


def _dual(x, nets, n, max_wgs=0):
    (_, w0, b0, _), (_, w1, b1, _) = nets
    return M_.conv1_fwd_dual(x, w0, b0, w1, b1, n, max_wgs)


@pytest.mark.parametrize("max_wgs", [0, 1, 2, 3])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cin", [1, 4])
def test_bit_equal_to_conv_fwd_band(cin, n, max_wgs):
    """one image per workgroup (max_wgs 0), all in one (1), runs with a short
    last workgroup (7 images over 2 or 3); the last image of every run has no
    successor to prefetch.  conv_fwd_band treats images independently, so the
    first n images of its NMAX-image output are the n-image reference."""
    x, nets = _case(cin)
    out0, out1 = _dual(x[:n], nets, n, max_wgs)
    for q, out in enumerate((out0, out1)):
        ref = nets[q][3][:n * 400]
        assert out.shape == ref.shape and out.dtype == torch.bfloat16
        assert ref.float().abs().max() > 0
        assert torch.equal(out, ref), \
            (q, (out.float() - ref.float()).abs().max())


@pytest.mark.parametrize("cin", [1, 4])
def test_identical_weights_give_identical_outputs(cin):
    x, nets = _case(cin)
    _, wt, b, ref = nets[0]
    out0, out1 = M_.conv1_fwd_dual(x, wt, b, wt.clone(), b.clone(), NMAX)
    assert torch.equal(out0, out1) and torch.equal(out0, ref)


@pytest.mark.parametrize("cin", [1, 4])
def test_rounding_against_float64(cin):
    """error against float64 conv2d on the dequantised frames, bounded by 4x
    conv_fwd_band's own error (the project's calibration rule); the kernels
    are bit-equal, so the ratio is 1.00"""
    n = 3
    x, nets = _case(cin)
    outs = _dual(x[:n], nets, n)
    xin = x[:n].permute(0, 3, 1, 2).double() / 255.0
    for q in range(2):
        w, _, b, band = nets[q]
        ref = F.relu(F.conv2d(xin, w.double(), b.double(), stride=4))
        ref = ref.permute(0, 2, 3, 1).reshape(n * 400, 32)
        err_band = float((band[:n * 400].double() - ref).abs().max())
        err_dual = float((outs[q].double() - ref).abs().max())
        print(f"cin {cin} net {q}: band {err_band:.3e} dual {err_dual:.3e} "
              f"ratio {err_dual / err_band:.2f}")
        assert 0 < err_band < 0.1
        assert err_dual <= 4 * err_band


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("cin", [1, 4])
def test_neighbouring_frames_do_not_leak(cin, lead):
    """the n frames sit next to an all-255 frame, after them (lead 0) or
    before them (lead 1): same outputs as on the tight tensor"""
    n = 3
    x, nets = _case(cin)
    big = torch.full((n + 1, 84, 84, cin), 255, dtype=torch.uint8,
                     device="cuda")
    view = big[lead:lead + n]
    view.copy_(x[:n])
    assert view.is_contiguous() and int(big[n * (1 - lead)].min()) == 255
    out0, out1 = _dual(view, nets, n)
    assert torch.equal(out0, nets[0][3][:n * 400])
    assert torch.equal(out1, nets[1][3][:n * 400])


def _bad_operands(cin):
    """(what, positional arguments) of calls that must raise"""
    x, nets = _case(cin)
    (_, w0, b0, _), (_, w1, b1, _) = nets
    n, K = 2, 64 * cin
    x = x[:n]
    good = [x, w0, b0, w1, b1, n]

    def swap(i, v):
        a = list(good)
        a[i] = v
        return a

    bad = [("N = 0", swap(5, 0)),
           ("N other than the frames", swap(5, 3)),
           ("negative max_wgs", good + [-1]),
           ("input dtype", swap(0, x.to(torch.int8))),
           ("input on the host", swap(0, x.cpu())),
           ("input height", swap(0, x[:, :80].contiguous())),
           ("two channels", swap(0, torch.zeros(n, 84, 84, 2,
                                                dtype=torch.uint8,
                                                device="cuda"))),
           ("input strided", swap(0, torch.zeros(
               n, 84, 84, 2 * cin, dtype=torch.uint8,
               device="cuda")[..., :cin]))]
    raw = torch.zeros(n * 84 * 84 * cin + 8, dtype=torch.uint8, device="cuda")
    off4 = raw[4:4 + n * 84 * 84 * cin].view(n, 84, 84, cin)
    assert off4.is_contiguous() and off4.data_ptr() % 8 == 4
    bad.append(("input pointer off 8 bytes", swap(0, off4)))
    for i, w in ((1, w0), (3, w1)):
        bad += [(f"weights {i} dtype", swap(i, w.float())),
                (f"weights {i} on the host", swap(i, w.cpu())),
                (f"weights {i} shape", swap(i, w[:, :K - 32].contiguous())),
                (f"weights {i} rows", swap(i, w[:16].contiguous())),
                (f"weights {i} strided", swap(i, torch.zeros(
                    32, 2 * K, dtype=torch.bfloat16,
                    device="cuda")[:, :K]))]
    for i, b in ((2, b0), (4, b1)):
        bad += [(f"bias {i} dtype", swap(i, b.bfloat16())),
                (f"bias {i} on the host", swap(i, b.cpu())),
                (f"bias {i} length", swap(i, b[:31].contiguous())),
                (f"bias {i} strided", swap(i, torch.zeros(
                    64, device="cuda")[::2]))]
    return bad


@pytest.mark.parametrize("cin", [1, 4])
def test_bad_operands_raise_before_allocation(cin):
    cases = _bad_operands(cin)
    gc.collect()
    torch.cuda.synchronize()

    def allocations():
        # cumulative count of device allocations: frees (a collection of
        # earlier tests' garbage in between) do not move it
        return torch.cuda.memory_stats().get("allocation.all.allocated", 0)

    assert allocations() > 0
    for what, args in cases:
        before = allocations()
        with pytest.raises(RuntimeError, match="conv1_fwd_dual"):
            M_.conv1_fwd_dual(*args)
        assert allocations() == before, what
    torch.cuda.synchronize()        # and nothing was launched that faults


@pytest.mark.parametrize("preset", ["mspacman", "mspacman_reference"])
def test_engine_step_matches_classic_forward(preset):
    """one engine step at B = 8, T = 7 with the dual conv1 against the same
    step of a fresh engine on the classic forwards (R2D2_CONV_FWD_BAND=0),
    online and target weights made different first; tolerance of
    test_hip_engine.py between its paths"""
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner
    from bench import build_batch

    c = cfg.apply(preset, batch_size=8, burn_in_steps=2, learning_steps=4,
                  forward_steps=1, amp=False, dtype="fp32")
    results = []
    for band in (True, False):
        torch.manual_seed(11)
        model = Network(c.action_dim, c.obs_shape, c.hidden_dim,
                        encoder="nature", forward_steps=c.forward_steps)
        hip = Learner(None, None, model)
        hip.enable_hip_engine()
        eng = hip.engine
        eng._fwd_band = band
        g = torch.Generator(device="cuda").manual_seed(3)
        with torch.no_grad():
            eng.flat_param.add_(torch.randn(
                eng.flat_param.shape, device="cuda", generator=g) * 0.01)
        eng.refresh_online()
        assert not torch.equal(eng.online.enc_pack.w1t,
                               eng.target.enc_pack.w1t)
        batch = build_batch(c, torch.device("cuda"), seed=5)
        assert batch.obs.shape[:2] == (8, 7)
        loss, prio = eng.train_step(batch)
        results.append((float(loss), prio.float().cpu().numpy()))
    (l_new, p_new), (l_old, p_old) = results
    print(f"{preset}: loss {l_new!r} vs classic {l_old!r}, "
          f"max |dprio| {np.abs(p_new - p_old).max():.3e}")
    assert np.isfinite(l_new) and p_new.size > 0
    assert abs(l_new - l_old) < 0.05 * max(1.0, abs(l_old)), (l_new, l_old)
    np.testing.assert_allclose(p_new, p_old, rtol=0.1, atol=0.05)
