"""The LDS-staged, double-buffered forward, dgrad and wgrad GEMMs against the
64x64 kernels on the same operands.

Every output element of the staged kernels keeps one accumulator fed by the
same MFMA chain (k0 = 0, 32, 64, ... ascending) as the 64x64 kernels, so the
comparison is torch.equal, not a tolerance.  The trailing ``path`` argument
forces a kernel: 64 the unstaged one, 6464 / 12864 the staged 64x64 / 128x64
instantiations; the shapes are the smallest that reach each code path (row
edge of either tile, a single half k-tile, full tile + half-tile tail, the
engine's 17-chunk reduction, column edges, a column count that is no multiple
of 8 and takes the per-element store).
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

OLD = 64
STAGED = (6464, 12864)
MS = (1, 127, 128, 129, 300)
REDS = (32, 64, 96, 544)
COLS = (8, 120, 128, 136, 512, 100)     # 100: not a multiple of 8


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def empty():
    return torch.empty(0, device="cuda")


def close(a, b, rtol, name):
    a, b = a.float(), b.float()
    atol = 3e-2 * max(1.0, float(b.abs().max()))
    assert torch.allclose(a, b, rtol=rtol, atol=atol), \
        f"{name}: max diff {(a - b).abs().max().item()}"


# -------------------------------------------------------------------------
# forward
# -------------------------------------------------------------------------

@pytest.mark.parametrize("path", STAGED)
@pytest.mark.parametrize("M", MS)
def test_forward_bit_equal(path, M):
    g = gen(10 + M)
    for K, N in itertools.product(REDS, COLS):
        A = randn(g, M, K).bfloat16()
        W = randn(g, N, K).bfloat16()
        b = randn(g, N)
        for bias, act, f32 in itertools.product((b, empty()), (0, 1),
                                                (False, True)):
            ref = M_.gemm_bias_act(A, W, bias, act, f32, OLD)
            out = M_.gemm_bias_act(A, W, bias, act, f32, path)
            assert out.dtype == ref.dtype and out.shape == ref.shape
            assert torch.equal(out, ref), \
                (path, M, K, N, bias.numel() > 0, act, f32)


def test_forward_dispatch_boundaries():
    """Automatic dispatch on both sides of its thresholds (staged from
    M = 1024 rows and 128 columns), and at a wide output."""
    g = gen(2)
    for M, N in ((1023, 128), (1024, 128), (1024, 120), (1024, 4032),
                 (1024, 4096)):
        A = randn(g, M, 96).bfloat16()
        W = randn(g, N, 96).bfloat16()
        b = randn(g, N)
        assert torch.equal(M_.gemm_bias_act(A, W, b, 1, False),
                           M_.gemm_bias_act(A, W, b, 1, False, OLD)), (M, N)


@pytest.mark.parametrize("path", (0,) + STAGED)
def test_forward_matches_fp32(path):
    g = gen(6)
    M, K, N = 1100, 96, 160
    A = randn(g, M, K).bfloat16()
    W = randn(g, N, K).bfloat16()
    b = randn(g, N)
    out = M_.gemm_bias_act(A, W, b, 1, False, path)
    ref = torch.relu(A.float() @ W.float().t() + b)
    close(out, ref, 5e-2, f"forward path {path}")


@pytest.mark.parametrize("path", STAGED)
def test_forward_ignores_rows_past_the_operands(path):
    """NaN in the storage behind A's row M and Wt's row N, which the edge
    tiles cover, must not reach the output."""
    g = gen(7)
    for M, K, N in ((1, 32, 8), (129, 96, 100), (300, 544, 136)):
        Af = randn(g, M + 130, K).bfloat16()
        Wf = randn(g, N + 70, K).bfloat16()
        b = randn(g, N)
        ref = M_.gemm_bias_act(Af[:M], Wf[:N], b, 0, True, path)
        Af[M:] = float("nan")
        Wf[N:] = float("nan")
        out = M_.gemm_bias_act(Af[:M], Wf[:N], b, 0, True, path)
        assert torch.equal(out, ref), (path, M, K, N)
        assert torch.isfinite(out).all()


# -------------------------------------------------------------------------
# dgrad: dA(M, C) = (dY * [act > 0])(M, R) @ W(C, R)^T  [* (out_mask > 0)]
# -------------------------------------------------------------------------

def dgrad_case(g, M, R, C, k_out):
    dY = randn(g, M, R).bfloat16()
    act = randn(g, M, R).bfloat16()
    W = randn(g, C, R).bfloat16()
    om = randn(g, M, k_out or C).bfloat16()
    return dY, act, W, om


def dgrad_flags(path, dY, act, W, om, k_out, tag):
    for rm, use_om in itertools.product((False, True), (False, True)):
        a = act if rm else empty()
        o = om if use_om else None
        ref = M_.gemm_dgrad(dY, a, W, rm, k_out, o, OLD)
        out = M_.gemm_dgrad(dY, a, W, rm, k_out, o, path)
        assert out.shape == ref.shape
        assert torch.equal(out, ref), tag + (rm, use_om)


@pytest.mark.parametrize("path", STAGED)
@pytest.mark.parametrize("M", MS)
def test_dgrad_bit_equal(path, M):
    g = gen(20 + M)
    for R, C in itertools.product(REDS, COLS):
        dgrad_flags(path, *dgrad_case(g, M, R, C, 0), 0, (path, M, R, C))
    # the dense k_out output: 512 of 544 columns (the LSTM input's latent
    # slice), over every reduction length
    for R in REDS:
        dgrad_flags(path, *dgrad_case(g, M, R, 544, 512), 512,
                    (path, M, R, 544, 512))


def test_dgrad_dispatch_boundaries():
    g = gen(3)
    for M, C in ((1023, 128), (1024, 128), (1024, 120), (1024, 4032),
                 (1024, 4096)):
        dY, act, W, om = dgrad_case(g, M, 96, C, 0)
        assert torch.equal(M_.gemm_dgrad(dY, act, W, True, 0, om),
                           M_.gemm_dgrad(dY, act, W, True, 0, om, OLD)), (M, C)


@pytest.mark.parametrize("path", (0,) + STAGED)
def test_dgrad_matches_fp32(path):
    g = gen(8)
    M, R, C = 1100, 96, 160
    dY, act, W, om = dgrad_case(g, M, R, C, 0)
    out = M_.gemm_dgrad(dY, act, W, True, 0, om, path)
    ref = ((dY.float() * (act.float() > 0)) @ W.float().t()) \
        * (om.float() > 0)
    close(out, ref, 5e-2, f"dgrad path {path}")


@pytest.mark.parametrize("path", STAGED)
def test_dgrad_ignores_rows_past_m_and_columns_past_k_out(path):
    """NaN behind row M of dY and act, and in W's rows k_out..K (the output
    columns that k_out drops), must not reach the output."""
    g = gen(9)
    for M, R, C, k_out in ((1, 32, 544, 512), (129, 96, 136, 100),
                           (300, 544, 544, 512)):
        dYf = randn(g, M + 130, R).bfloat16()
        actf = randn(g, M + 130, R).bfloat16()
        W = randn(g, C, R).bfloat16()
        om = randn(g, M, k_out).bfloat16()
        ref = M_.gemm_dgrad(dYf[:M], actf[:M], W, True, k_out, om, path)
        dYf[M:] = float("nan")
        actf[M:] = float("nan")
        W[k_out:] = float("nan")
        out = M_.gemm_dgrad(dYf[:M], actf[:M], W, True, k_out, om, path)
        assert torch.equal(out, ref), (path, M, R, C, k_out)
        assert torch.isfinite(out).all()


# -------------------------------------------------------------------------
# wgrad: the 128x64 tile kernel (path 12864) against the 64x64 kernel.
# Both accumulate row chunks with f32 atomics, so the comparison is the
# calibrated one: err = max|x - exact| / max|exact| against the float64
# product of the same bf16 operands, and err(tile) <= 4 * err(64x64).
# -------------------------------------------------------------------------

from test_hip_lstm_layouts import assert_calibrated  # noqa: E402

TILE = 12864
WG_MS = (1, 33, 64, 65, 200)
WG_NK = ((64, 64), (72, 96), (136, 544))


def wgrad_operands(g, M, N, K, mask):
    """dY's elements are spread over 13 binades.  A column sum of unit-scale
    bf16 values is usually exactly representable in f32, so the bias gradient
    of either kernel would be exact or off by one lucky rounding and their
    ratio would say nothing; with the spread every partial sum rounds."""
    A = randn(g, M, K).bfloat16()
    scale = torch.exp2(-torch.randint(0, 13, (M, N), device="cuda",
                                      generator=g).float())
    dY = (randn(g, M, N) * scale).bfloat16()
    act = randn(g, M, N).bfloat16() if mask else torch.Tensor()
    dout = torch.where(act.float() > 0, dY, torch.zeros_like(dY)) \
        if mask else dY
    return A, dY, act, dout


def pattern(n):
    """A known f32 pattern, |x| < 1 (the one of test_hip_head_glue)."""
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    return ((i * 37) % 101 - 50).float() / 64.0


def wgrad_onto_pattern(path, dY, act, A, mask, bias, dims=(0, 0, 0)):
    """gemm_wgrad_into accumulating onto the pattern.  A sum of a few hundred
    bf16 values is often exactly representable in f32, which would leave the
    yardstick with an error of exactly zero; on top of the pattern every
    element needs a rounding, in both kernels."""
    N, K = dY.shape[1], A.shape[1]
    dW = pattern(N * K).view(N, K)
    db = pattern(N) if bias else torch.Tensor()
    M_.gemm_wgrad_into(dY, act, A, mask, dW, db, *dims, path)
    return dW, db


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "relu"])
@pytest.mark.parametrize("M", WG_MS)
def test_wgrad_tile_calibrated(M, mask, bias):
    g = gen(30 + M)
    for N, K in WG_NK:
        A, dY, act, dout = wgrad_operands(g, M, N, K, mask)
        exact = pattern(N * K).view(N, K).double() \
            + dout.double().t() @ A.double()
        exact_b = pattern(N).double() + dout.double().sum(0)
        old_w, old_b = wgrad_onto_pattern(OLD, dY, act, A, mask, bias)
        new_w, new_b = wgrad_onto_pattern(TILE, dY, act, A, mask, bias)
        tag = f"wgrad M{M} N{N} K{K} mask{int(mask)}"
        assert_calibrated(f"{tag} dW", new_w, old_w, exact)
        if bias:
            assert_calibrated(f"{tag} db", new_b, old_b, exact_b)


def test_wgrad_tile_kperm():
    """(d0, d1, d2) -> (d2, d0, d1) store permutation of the k axis, the
    encoder FC's (7, 7, 64) flatten at a small size."""
    g = gen(40)
    M, N, dims = 200, 72, (7, 7, 8)
    K = dims[0] * dims[1] * dims[2]
    A, dY, act, dout = wgrad_operands(g, M, N, K, True)
    exact = pattern(N * K).view(N, K).double() \
        + (dout.double().t() @ A.double()).view(N, *dims) \
        .permute(0, 3, 1, 2).reshape(N, K)
    exact_b = pattern(N).double() + dout.double().sum(0)
    old_w, old_b = wgrad_onto_pattern(OLD, dY, act, A, True, True, dims)
    new_w, new_b = wgrad_onto_pattern(TILE, dY, act, A, True, True, dims)
    assert_calibrated("wgrad kperm dW", new_w, old_w, exact)
    assert_calibrated("wgrad kperm db", new_b, old_b, exact_b)


@pytest.mark.parametrize("M", [65, 200])
def test_wgrad_tile_into_views(M):
    """Narrowed (Nout < N, Kout < K) views in the middle of a patterned flat
    buffer: accumulated into, and nothing outside them touched."""
    g = gen(50 + M)
    N, Nout, K, Kout = 136, 131, 96, 83
    A, dY, act, dout = wgrad_operands(g, M, N, K, True)
    lo, mid, hi = 1031, 517, 2049
    o_w = lo
    o_b = o_w + Nout * Kout + mid
    total = o_b + Nout + hi
    before = pattern(total)
    bufs = {}
    for path in (OLD, TILE):
        buf = before.clone()
        M_.gemm_wgrad_into(dY, act, A, True,
                           buf[o_w:o_w + Nout * Kout].view(Nout, Kout),
                           buf[o_b:o_b + Nout], 0, 0, 0, path)
        bufs[path] = buf
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device="cuda")
    inside[o_w:o_w + Nout * Kout] = True
    inside[o_b:o_b + Nout] = True
    assert torch.equal(bufs[TILE][~inside].view(torch.int32),
                       before[~inside].view(torch.int32)), \
        "the tile kernel wrote outside its views"
    sw, sb = slice(o_w, o_w + Nout * Kout), slice(o_b, o_b + Nout)
    exact_w = before[sw].double() \
        + (dout.double().t() @ A.double())[:Nout, :Kout].reshape(-1)
    exact_b = before[sb].double() + dout.double().sum(0)[:Nout]
    assert_calibrated(f"wgrad into M{M} dW", bufs[TILE][sw], bufs[OLD][sw],
                      exact_w)
    assert_calibrated(f"wgrad into M{M} db", bufs[TILE][sb], bufs[OLD][sb],
                      exact_b)


def test_wgrad_dispatch_boundary():
    """gemm_wgrad under automatic dispatch on both sides of its thresholds:
    the tile kernel from M = 1024 rows and N = 128 columns.  Each column sums
    a thousand values here, so the yardstick's error is not zero."""
    g = gen(60)
    for M, N in ((1023, 128), (1024, 128), (1024, 120)):
        A, dY, act, dout = wgrad_operands(g, M, N, 96, False)
        exact = dout.double().t() @ A.double()
        old_w, old_b = M_.gemm_wgrad(dY, act, A, False, True, OLD)
        new_w, new_b = M_.gemm_wgrad(dY, act, A, False, True)
        assert_calibrated(f"wgrad auto M{M} N{N} dW", new_w, old_w, exact)
        assert_calibrated(f"wgrad auto M{M} N{N} db", new_b, old_b,
                          dout.double().sum(0))
