"""GPU numerics: the MLP encoder's first-layer kernels, mlp_in_fwd and
mlp_in_wgrad_into (ops/hip/mlp_kernels.hip).

Error measure (test_hip_lstm_layouts.rel_err): max|x - exact| / max|exact|
against float64 on the operands as the kernel sees them (f32 X, W1, b1; bf16
dA1).  The yardstick is a float32 torch model that rounds to bf16 where the
kernel stores bf16; the bound is FACTOR (4) times the yardstick's own error.

mlp_in_wgrad_into adds its per-workgroup partial sums with f32 atomics, so two
runs may differ in the last bits when more than one workgroup runs
(M > 64 here): results are compared to float64, never to each other.
"""

import pytest
import torch
import torch.nn.functional as F

from test_hip_lstm_layouts import assert_calibrated, bits_equal

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

DEV = "cuda"
N = 512
MS = [1, 63, 64, 65, 200]          # both sides of a 64-row chunk, tails
DS = [1, 3, 4, 5, 8, 16]           # rows of 4 D bytes: unaligned widths too
GRID = [pytest.param(M, D, id=f"M{M}-D{D}") for M in MS for D in DS]
PATTERN = 1234.5


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def make_x(g, M, D):
    """CartPole-scale states (position, velocity, angle, angular velocity
    repeating over the columns), negatives included, with exact zeros."""
    scale = torch.tensor([2.4, 3.0, 0.21, 3.0], device=DEV).repeat(4)[:D]
    x = torch.randn(M, D, device=DEV, generator=g) * scale
    x[torch.rand(M, D, device=DEV, generator=g) < 0.1] = 0.0
    return x.contiguous()


def make_w(g, D):
    """nn.Linear's init range, U(-1/sqrt(D), 1/sqrt(D))."""
    k = D ** -0.5
    w = (torch.rand(N, D, device=DEV, generator=g) * 2 - 1) * k
    b = (torch.rand(N, device=DEV, generator=g) * 2 - 1) * k
    return w.contiguous(), b.contiguous()


# ---------------------------------------------------------------------------
# Forward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,D", GRID)
def test_fwd_calibrated(M, D):
    g = gen(1000 * M + D)
    x = make_x(g, M, D)
    w, b = make_w(g, D)
    a1 = M_.mlp_in_fwd(x, w, b)
    assert a1.shape == (M, N) and a1.dtype == torch.bfloat16
    pre = x.double() @ w.double().t() + b.double()
    exact = torch.relu(pre)
    model = torch.relu(F.linear(x, w, b)).bfloat16()
    assert_calibrated(f"mlp_in_fwd M{M} D{D}", a1, model, exact)
    # relu zeros are exact (+0) zeros wherever the pre-activation is
    # negative beyond any f32 rounding of a sum of D + 1 terms of this scale
    neg = pre < -1e-4
    assert neg.any() and (~neg).any()
    assert (a1.view(torch.int16)[neg] == 0).all()
    assert (a1.float() >= 0).all()

    # row isolation: perturb the first and the last row
    x2 = x.clone()
    x2[0] = x2[0] * -1.5 + 0.3
    x2[M - 1] = x2[M - 1] * 2.0 - 0.7
    a2 = M_.mlp_in_fwd(x2, w, b)
    if M > 2:
        assert bits_equal(a2[1:M - 1], a1[1:M - 1])
    assert not bits_equal(a2[0], a1[0])
    assert not bits_equal(a2[M - 1], a1[M - 1])


@pytest.mark.parametrize("D", DS)
def test_fwd_layout_invariance_and_no_reads_past_M(D):
    g = gen(77 + D)
    x = make_x(g, 200, D)
    w, b = make_w(g, D)
    big = M_.mlp_in_fwd(x, w, b)
    small = M_.mlp_in_fwd(x[:5].contiguous(), w, b)
    assert bits_equal(big[:5], small)
    # NaN in the storage past row M is never read
    for M in (1, 5, 63, 65):
        store = torch.full((M + 3, D), float("nan"), device=DEV)
        store[:M] = x[:M]
        got = M_.mlp_in_fwd(store[:M], w, b)
        assert not torch.isnan(got.float()).any()
        assert bits_equal(got, M_.mlp_in_fwd(x[:M].contiguous(), w, b))


# ---------------------------------------------------------------------------
# Weight gradient
# ---------------------------------------------------------------------------

def pattern(n):
    """A known f32 pattern, exactly representable, |x| < 1."""
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    return ((i * 37) % 101 - 50).float() / 64.0


def make_da1(g, M):
    """A ReLU-masked upstream gradient: about half the entries zero."""
    d = torch.randn(M, N, device=DEV, generator=g) * 0.05
    d[torch.rand(M, N, device=DEV, generator=g) < 0.5] = 0.0
    return d.bfloat16().contiguous()


def flat_views(D, lo=1031, mid=517, hi=2049):
    """dW1 and db1 as views in the middle of one flat f32 buffer."""
    o_w = lo
    o_b = o_w + N * D + mid
    total = o_b + N + hi
    before = pattern(total)
    buf = before.clone()
    dW = buf[o_w:o_w + N * D].view(N, D)
    db = buf[o_b:o_b + N]
    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    inside[o_w:o_w + N * D] = True
    inside[o_b:o_b + N] = True
    pw = before[o_w:o_w + N * D].view(N, D)
    pb = before[o_b:o_b + N]
    return before, buf, dW, db, inside, pw, pb


@pytest.mark.parametrize("M,D", GRID)
def test_wgrad_into(M, D):
    g = gen(5000 + 1000 * M + D)
    x = make_x(g, M, D)
    da1 = make_da1(g, M)
    before, buf, dW, db, inside, pw, pb = flat_views(D)
    M_.mlp_in_wgrad_into(da1, x, dW, db)
    torch.cuda.synchronize()
    assert torch.equal(buf[~inside].view(torch.int32),
                       before[~inside].view(torch.int32)), \
        "mlp_in_wgrad_into wrote outside its views"

    gw64 = da1.double().t() @ x.double()
    gb64 = da1.double().sum(0)
    gw32 = da1.float().t() @ x
    gb32 = da1.float().sum(0)
    tag = f"M{M} D{D}"
    assert_calibrated(f"mlp_in_wgrad dW1 {tag}", dW, pw + gw32,
                      pw.double() + gw64)
    assert_calibrated(f"mlp_in_wgrad db1 {tag}", db, pb + gb32,
                      pb.double() + gb64)

    # a second call on the same views adds, it does not overwrite
    M_.mlp_in_wgrad_into(da1, x, dW, db)
    torch.cuda.synchronize()
    assert torch.equal(buf[~inside].view(torch.int32),
                       before[~inside].view(torch.int32))
    assert_calibrated(f"mlp_in_wgrad dW1 twice {tag}", dW,
                      pw + gw32 + gw32, pw.double() + 2 * gw64)
    assert_calibrated(f"mlp_in_wgrad db1 twice {tag}", db,
                      pb + gb32 + gb32, pb.double() + 2 * gb64)


@pytest.mark.parametrize("M,D", GRID)
def test_wgrad_single_row_outer_product(M, D):
    """dA1 zero except one row: every other row adds exact zeros, the views
    start at zero, so the result is that row's outer product with one f32
    rounding per product — bit for bit."""
    g = gen(9000 + 1000 * M + D)
    x = make_x(g, M, D)
    for row in sorted({0, M // 2, M - 1}):
        da1 = torch.zeros(M, N, device=DEV).bfloat16()
        da1[row] = make_da1(g, 1)[0]
        dW = torch.zeros(N, D, device=DEV)
        db = torch.zeros(N, device=DEV)
        M_.mlp_in_wgrad_into(da1, x, dW, db)
        want = da1[row].float()[:, None] * x[row][None, :]
        assert torch.equal(dW, want), (M, D, row)
        assert torch.equal(db, da1[row].float()), (M, D, row)


def test_wgrad_no_reads_past_M():
    D = 5
    g = gen(31)
    for M in (1, 63, 65):
        x = make_x(g, M, D)
        da1 = make_da1(g, M)
        xs = torch.full((M + 3, D), float("nan"), device=DEV)
        xs[:M] = x
        ds = torch.full((M + 3, N), float("nan"), device=DEV).bfloat16()
        ds[:M] = da1
        dW = torch.zeros(N, D, device=DEV)
        db = torch.zeros(N, device=DEV)
        M_.mlp_in_wgrad_into(ds[:M], xs[:M], dW, db)
        assert torch.isfinite(dW).all() and torch.isfinite(db).all()
        assert_calibrated(f"past-M dW1 M{M}", dW, da1.float().t() @ x,
                          da1.double().t() @ x.double())


# ---------------------------------------------------------------------------
# Operand checks: raises, the outputs' pattern untouched
# ---------------------------------------------------------------------------

def _fwd_args(M=5, D=4):
    g = gen(3)
    return [make_x(g, M, D), *make_w(g, D)]


def _bad_fwd_cases():
    def x_dtype(a): a[0] = a[0].double()
    def x_bf16(a): a[0] = a[0].bfloat16()
    def x_shape(a): a[0] = a[0].reshape(-1)
    def x_stride(a): a[0] = torch.randn(5, 8, device=DEV)[:, :4]
    def x_cpu(a): a[0] = a[0].cpu()
    def w_dtype(a): a[1] = a[1].bfloat16()
    def w_shape(a): a[1] = torch.zeros(N, 5, device=DEV)
    def w_stride(a): a[1] = torch.zeros(4, N, device=DEV).t()
    def w_cpu(a): a[1] = a[1].cpu()
    def b_dtype(a): a[2] = a[2].double()
    def b_shape(a): a[2] = torch.zeros(N + 1, device=DEV)
    def b_stride(a): a[2] = torch.zeros(2 * N, device=DEV)[::2]
    def b_cpu(a): a[2] = a[2].cpu()
    def d0(a):
        a[0] = torch.zeros(5, 0, device=DEV)
        a[1] = torch.zeros(N, 0, device=DEV)
    def d17(a):
        a[0] = torch.zeros(5, 17, device=DEV)
        a[1] = torch.zeros(N, 17, device=DEV)
    def n256(a):
        a[1] = torch.zeros(256, 4, device=DEV)
        a[2] = torch.zeros(256, device=DEV)
    def m0(a): a[0] = a[0][:0]
    return [x_dtype, x_bf16, x_shape, x_stride, x_cpu, w_dtype, w_shape,
            w_stride, w_cpu, b_dtype, b_shape, b_stride, b_cpu, d0, d17,
            n256, m0]


@pytest.mark.parametrize("mutate", _bad_fwd_cases(), ids=lambda f: f.__name__)
def test_fwd_rejects(mutate):
    a = _fwd_args()
    mutate(a)
    with pytest.raises((RuntimeError, TypeError)):
        M_.mlp_in_fwd(*a)
    torch.cuda.synchronize()


def _wgrad_args(M=5, D=4):
    g = gen(4)
    return [make_da1(g, M), make_x(g, M, D),
            torch.full((N, D), PATTERN, device=DEV),
            torch.full((N,), PATTERN, device=DEV)]


def _bad_wgrad_cases():
    def da_dtype(a): a[0] = a[0].float()
    def da_shape(a): a[0] = a[0][:4].contiguous()
    def da_stride(a):
        a[0] = torch.zeros(5, 2 * N, device=DEV).bfloat16()[:, :N]
    def da_cpu(a): a[0] = a[0].cpu()
    def x_dtype(a): a[1] = a[1].bfloat16()
    def x_shape(a): a[1] = a[1].reshape(-1)
    def x_stride(a): a[1] = torch.randn(5, 8, device=DEV)[:, :4]
    def x_cpu(a): a[1] = a[1].cpu()
    def dw_shape(a): a[2] = torch.full((N, 5), PATTERN, device=DEV)
    def dw_stride(a): a[2] = torch.full((4, N), PATTERN, device=DEV).t()
    def dw_dtype(a): a[2] = a[2].double()
    def dw_cpu(a): a[2] = a[2].cpu()
    def db_shape(a): a[3] = torch.full((N + 1,), PATTERN, device=DEV)
    def db_stride(a): a[3] = torch.full((2 * N,), PATTERN, device=DEV)[::2]
    def db_dtype(a): a[3] = a[3].double()
    def db_cpu(a): a[3] = a[3].cpu()
    def d0(a):
        a[1] = torch.zeros(5, 0, device=DEV)
        a[2] = torch.zeros(N, 0, device=DEV)
    def d17(a):
        a[1] = torch.zeros(5, 17, device=DEV)
        a[2] = torch.full((N, 17), PATTERN, device=DEV)
    def n256(a):
        a[0] = torch.zeros(5, 256, device=DEV).bfloat16()
        a[2] = torch.full((256, 4), PATTERN, device=DEV)
        a[3] = torch.full((256,), PATTERN, device=DEV)
    def m0(a):
        a[0] = a[0][:0]
        a[1] = a[1][:0]
    return [da_dtype, da_shape, da_stride, da_cpu, x_dtype, x_shape,
            x_stride, x_cpu, dw_shape, dw_stride, dw_dtype, dw_cpu, db_shape,
            db_stride, db_dtype, db_cpu, d0, d17, n256, m0]


@pytest.mark.parametrize("mutate", _bad_wgrad_cases(),
                         ids=lambda f: f.__name__)
def test_wgrad_rejects(mutate):
    a = _wgrad_args()
    mutate(a)
    outs = [a[2], a[3]]          # the outputs this call was handed
    with pytest.raises((RuntimeError, TypeError)):
        M_.mlp_in_wgrad_into(*a)
    torch.cuda.synchronize()
    for o in outs:
        if o.numel():
            assert (o.float() == PATTERN).all()
