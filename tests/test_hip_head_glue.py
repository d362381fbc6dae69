"""GPU numerics: the head and glue kernels every learner step runs but no
test called directly — assemble_rin, dueling_combine(_bwd),
segment_priority, gemm_wgrad_into and the dense k_out output of gemm_dgrad.

References are float64 torch.  Each bound is derived from the operation and
the derivation stands next to it; u = 2^-24 is the f32 unit roundoff and
2^-8 stands for one bf16 rounding (the true figure, 2^-9, with margin).
"""

import numpy as np
import pytest
import torch

from test_hip_lstm_layouts import assert_calibrated, bits_equal

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

DEV = "cuda"


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


# ---------------------------------------------------------------------------
# assemble_rin
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("extra_pad", [0, 32])
@pytest.mark.parametrize("A", [2, 9, 18])
@pytest.mark.parametrize("M", [1, 37, 257])
def test_assemble_rin(M, A, extra_pad):
    g = gen(M * 100 + A)
    kin_pad = -(-(513 + A) // 32) * 32 + extra_pad
    latent = randn(g, M, 512).bfloat16()
    la = randn(g, M, A)                 # arbitrary floats: a column shift shows
    lr = torch.arange(M, device=DEV, dtype=torch.float32) * 0.37 + 1.5
    want = torch.zeros(M, kin_pad, device=DEV, dtype=torch.bfloat16)
    want[:, :512] = latent
    want[:, 512:512 + A] = la.bfloat16()
    want[:, 512 + A] = lr.bfloat16()
    # The kernel allocates its own output.  Freeing a NaN-filled block of the
    # same size right before the call makes the caching allocator likely to
    # hand that block back, so an unwritten pad column would read NaN, not a
    # lucky zero.  Best effort: nothing guarantees the block is reused.
    junk = torch.full((M, kin_pad), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    del junk
    rin = M_.assemble_rin(latent, la, lr, kin_pad)
    assert rin.shape == (M, kin_pad) and rin.dtype == torch.bfloat16
    # a pure copy / one RNE cast per element: bit-exact
    assert bits_equal(rin[:, :512].contiguous(), latent), "latent columns"
    assert bits_equal(rin[:, 512:512 + A].contiguous(), la.bfloat16()), \
        "action columns"
    assert bits_equal(rin[:, 512 + A].contiguous(), lr.bfloat16()), \
        "reward column"
    assert (rin[:, 513 + A:].contiguous().view(torch.int16) == 0).all(), \
        "pad columns"
    assert bits_equal(rin, want)


# ---------------------------------------------------------------------------
# dueling_combine / dueling_combine_bwd
# ---------------------------------------------------------------------------

PAD = 32
RS = [1, 3, 4, 5, 130]
AS = [2, 9, 18, 32]


def poison_cols(x, first):
    """+-1e30 in columns >= first: a kernel that read them would be off by
    ~1e30 (or Inf/NaN), far outside any bound below."""
    n = x.shape[1] - first
    if n > 0:
        sign = torch.where(torch.arange(n, device=DEV) % 2 == 0, 1.0, -1.0)
        x[:, first:] = 1e30 * sign
    return x


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("R", RS)
def test_dueling_combine(R, A):
    g = gen(R * 100 + A)
    adv = poison_cols(randn(g, R, PAD) * 3.0, A)
    val = poison_cols(randn(g, R, PAD) * 2.0, 1)
    q = M_.dueling_combine(adv, val, A)
    assert q.shape == (R, A) and q.dtype == torch.float32
    a64 = adv[:, :A].double()
    v64 = val[:, :1].double()
    ref = v64 + a64 - a64.mean(1, keepdim=True)
    # f32 evaluation of v + a - sum(a)/A: the sum makes at most A - 1
    # roundings, each <= u * sum|a| <= u * A * max|a|, so after the division
    # the mean is off by <= (A - 1) u max|a| (+ one rounding for the
    # division); the two additions round a value <= |v| + 2 max|a| once each.
    # In all <= (A + 2) u (|v| + 2 max|a|); the bound allows twice that.
    bound = (A + 2) * 2.0 ** -23 * (v64.abs() + 2 * a64.abs().amax(1, True))
    err = (q.double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("R", RS)
def test_dueling_combine_bwd(R, A):
    g = gen(R * 100 + A + 7)
    # multiples of 2^-12 in [-4, 4]: a row sum of <= 32 of them needs at most
    # 7 + 12 bits, so the f32 row sum is exact in any order
    dq = (randn(g, R, A).clamp(-4, 4) * 4096).round() / 4096
    dadv, dval = M_.dueling_combine_bwd(dq.contiguous(), PAD, PAD)
    assert dadv.shape == (R, PAD) and dval.shape == (R, PAD)
    assert dadv.dtype == dval.dtype == torch.bfloat16
    d64 = dq.double()
    s64 = d64.sum(1, keepdim=True)
    ref = d64 - s64 / A
    # s/A rounds once and the subtraction once, each on a value <= 2 max|dq|
    # (well inside the f32 sum bound (A + 2) * 2^-23 * max|dq| that would
    # hold for inexact sums too); the bf16 store adds one bf16 rounding.
    bound = (2.0 ** -8 * ref.abs()
             + (A + 2) * 2.0 ** -23 * d64.abs().amax(1, True))
    err = (dadv[:, :A].double() - ref).abs()
    assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max().item()
    assert (dadv[:, A:] == 0).all(), "dadv pad columns"
    assert (dval[:, 1:] == 0).all(), "dval pad columns"
    # the row sum is exact in f32, so column 0 is exactly its bf16
    assert bits_equal(dval[:, 0].contiguous(),
                      s64[:, 0].float().bfloat16()), "dval[:, 0]"


# ---------------------------------------------------------------------------
# segment_priority
# ---------------------------------------------------------------------------

SEG_LENS = [1, 63, 64, 65, 200, 0]


@pytest.mark.parametrize("eta", [0.0, 0.9, 1.0])
def test_segment_priority(eta):
    lens = SEG_LENS + SEG_LENS[::-1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    g = gen(11)
    abs_td = randn(g, int(off[-1])).abs() * 2.0
    seg = torch.from_numpy(off).to(DEV)
    prio = M_.segment_priority(abs_td, seg, eta)
    assert prio.shape == (len(lens),) and prio.dtype == torch.float32
    eta32 = float(np.float32(eta))       # the kernel takes eta as an f32
    for i, n in enumerate(lens):
        p = prio[i]
        if n == 0:
            assert p.item() == 0.0, f"empty segment {i}"
            continue
        v = abs_td[off[i]:off[i + 1]]
        if eta == 1.0:
            # 1 * max + 0 * mean: no rounding anywhere
            assert bits_equal(p.reshape(1), v.max().reshape(1)), f"seg {i}"
            continue
        mean = v.double().mean().item()
        ref = eta32 * v.double().max().item() + (1.0 - eta32) * mean
        # the f32 sum of n non-negative terms is off by < n u sum, i.e. the
        # mean by < n u mean (the lane-strided tree does far fewer roundings;
        # at n = 1 it does none); the bound grants 2 n u mean = n 2^-23 mean,
        # which also covers the roundings of (1 - eta) * sum / n.  The final
        # add, and eta * max before it, round a value <= ref: one rounding
        # of the result.
        bound = n * 2.0 ** -23 * mean + 2.0 ** -24 * abs(ref)
        assert abs(p.item() - ref) <= bound, (i, n, p.item(), ref, bound)


# ---------------------------------------------------------------------------
# gemm_wgrad_into: the learner's shapes, scaled down in M
# ---------------------------------------------------------------------------

WGRAD_SHAPES = {
    # name: (N, Nout, K, Kout)
    "head_out": (32, 9, 512, 512),
    "w_ih": (2048, 2048, 544, 531),
    "head_hidden": (512, 512, 512, 512),
}


def pattern(n):
    """A known f32 pattern, exactly representable, |x| < 1."""
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    return ((i * 37) % 101 - 50).float() / 64.0


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "relu"])
@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("shape", list(WGRAD_SHAPES))
def test_gemm_wgrad_into(shape, M, mask, bias):
    N, Nout, K, Kout = WGRAD_SHAPES[shape]
    g = gen(M + N + K)
    A = randn(g, M, K).bfloat16()
    dY = randn(g, M, N).bfloat16()
    e = torch.Tensor()
    act = e
    dout = dY
    if mask:
        # the kernel's own bf16 forward output decides the mask (an f32
        # forward would flip elements at the boundary)
        W = (randn(g, N, K) / np.sqrt(K)).bfloat16()
        act = M_.gemm_bias_act(A, W, randn(g, N), 1, False)
        dout = torch.where(act.float() > 0, dY, torch.zeros_like(dY))
        assert 0 < int((act.float() > 0).sum()) < act.numel()

    # dW and db are views in the middle of one flat f32 buffer, as the
    # parameter gradients are views of the learner's flat gradient buffer
    lo, mid, hi = 1031, 517, 2049
    o_w = lo
    o_b = o_w + Nout * Kout + mid
    total = o_b + Nout + hi
    before = pattern(total)
    buf = before.clone()
    dW = buf[o_w:o_w + Nout * Kout].view(Nout, Kout)
    db = buf[o_b:o_b + Nout]
    M_.gemm_wgrad_into(dY, act, A, mask, dW, db if bias else e)
    torch.cuda.synchronize()

    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    inside[o_w:o_w + Nout * Kout] = True
    if bias:
        inside[o_b:o_b + Nout] = True
    assert torch.equal(buf[~inside].view(torch.int32),
                       before[~inside].view(torch.int32)), \
        "gemm_wgrad_into wrote outside its views"

    # the kernel accumulates: view == pattern + dY^T A.  The yardstick is the
    # f32 torch product of the same bf16 operands added to the same pattern.
    pw = before[o_w:o_w + Nout * Kout].view(Nout, Kout)
    exact = pw.double() + (dout.double().t() @ A.double())[:Nout, :Kout]
    model = pw + (dout.float().t() @ A.float())[:Nout, :Kout]
    tag = f"wgrad_into {shape} M{M} {'relu' if mask else 'nomask'}"
    assert_calibrated(f"{tag} dW", dW, model, exact)
    if bias:
        pb = before[o_b:o_b + Nout]
        ones = torch.ones(1, M, device=DEV)
        exact_b = pb.double() + (ones.double() @ dout.double())[0, :Nout]
        model_b = pb + (ones @ dout.float())[0, :Nout]
        assert_calibrated(f"{tag} db", db, model_b, exact_b)


# ---------------------------------------------------------------------------
# gemm_dgrad with a dense k_out-column output
# ---------------------------------------------------------------------------

def dgrad_bound(dY, W_kn, ref, k_out):
    """|bf16(f32 dot) - exact| per element: the f32 accumulation of N
    products (each exact in f32) is off by <= N u sum|dy||w|, and the bf16
    store rounds that sum once: <= 2^-9 (|exact| + N u S).  The bound grants
    2^-8 |exact| + 2 N u S."""
    N = dY.shape[1]
    S = (dY.double().abs() @ W_kn.double().abs().t())[:, :k_out]
    return 2.0 ** -8 * ref.abs() + 2 * N * 2.0 ** -24 * S


@pytest.mark.parametrize("with_mask", [False, True], ids=["plain", "outmask"])
@pytest.mark.parametrize("M", [200, 1100], ids=["M200-64x64", "M1100-128x128"])
def test_gemm_dgrad_k_out(M, with_mask):
    N, K, k_out = 2048, 544, 512
    g = gen(M)
    dY = randn(g, M, N).bfloat16()
    W_kn = (randn(g, K, N) / np.sqrt(N)).bfloat16()      # (K, N)
    e = torch.Tensor()
    full = M_.gemm_dgrad(dY, e, W_kn, False, 0)
    assert full.shape == (M, K)
    ref = (dY.double() @ W_kn.double().t())[:, :k_out]
    if with_mask:
        om = randn(g, M, k_out).bfloat16()
        om[:, ::5] = 0.0                                 # zeros do not pass
        out = M_.gemm_dgrad(dY, e, W_kn, False, k_out, om)
        keep = om.float() > 0
        assert 0 < int(keep.sum()) < keep.numel()
        ref = torch.where(keep, ref, torch.zeros_like(ref))
        want = torch.where(keep, full[:, :k_out], torch.zeros_like(om))
    else:
        out = M_.gemm_dgrad(dY, e, W_kn, False, k_out)
        want = full[:, :k_out].contiguous()
    assert out.shape == (M, k_out) and out.is_contiguous()
    assert out.dtype == torch.bfloat16
    err = (out.double() - ref).abs()
    bound = dgrad_bound(dY, W_kn, ref, k_out)
    assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max().item()
    # same tiles, same k-loop per element: the dense output is the slice of
    # the full one, bit for bit (where the mask keeps it)
    same = bits_equal(out, want)
    print(f"DGRAD k_out M{M} mask={with_mask}: bit-equal to sliced full "
          f"output: {same}")
    assert same
