"""GPU numerics: the fused single-step actor kernels (lstm_cell_step,
head_hidden_step, head_out_step) and HipInference.step on top of them.

Error measure (test_hip_lstm_layouts.rel_err): max|x - exact| / max|exact|.
`exact` is float64 computed from the operands as the kernels see them:
bf16-rounded weights, bf16-rounded rin and h0, f32 bias and c0.  The
yardstick is the EXISTING path on identical inputs — assemble_rin, the
gemm_bias_act calls, the torch elementwise cell update, dueling_combine, as
HipInference.forward chains them — measured the same way; the new kernel is
never its own yardstick.

Bound: err(kernel) <= 4 * err(yardstick), the project's factor.  For the f32
outputs h1 / c1 the bound is max(4 * err(yardstick), 2^-12): the yardstick
runs exact torch.sigmoid where the kernel runs __expf as the persistent LSTM
does, every consumer of h rounds it to bf16 (half-ulp 2^-9), and 2^-12 is an
eighth of that.  Each CALIB line printed says whether the floor decided.

Definition tested for the pad columns of wih_t (k >= 512 + A + 1): UNREAD.
The kernel masks them, so NaN there changes nothing.
"""

import functools
import queue

import numpy as np
import pytest
import torch

from test_hip_lstm_layouts import FACTOR, bits_equal, rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

H = 512
FLOOR = 2.0 ** -12
ES = [1, 5, 16, 17, 64, 65, 256]
AS = [2, 9, 18, 31]
GRID = [pytest.param(E, A, id=f"E{E}-A{A}") for E in ES for A in AS]
PATTERN = 1234.5


def kin_pad(A):
    return (H + A + 1 + 31) // 32 * 32


def assert_bound(name, kernel, model, exact, floor=0.0):
    """err(kernel) <= max(FACTOR * err(model), floor), both against exact;
    prints the figures first so a run with -rP records them."""
    assert kernel.shape == exact.shape == model.shape, name
    assert torch.isfinite(kernel.float()).all(), f"{name}: non-finite"
    ek, em = rel_err(kernel, exact), rel_err(model, exact)
    by_floor = ek > FACTOR * em
    print(f"CALIB {name}: kernel {ek:.3e} yardstick {em:.3e} "
          f"{'FLOOR decided' if by_floor else 'within 4x'}")
    assert ek <= max(FACTOR * em, floor), (name, ek, em)
    return ek, em


# ---------------------------------------------------------------------------
# Cell step
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cell_weights(A):
    g = torch.Generator(device="cuda").manual_seed(100 + A)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    kin, KP = H + A + 1, kin_pad(A)
    wih = torch.zeros(4 * H, KP, device="cuda")
    wih[:, :kin] = r(4 * H, kin) / np.sqrt(kin)
    whh = r(4 * H, H) / np.sqrt(H)
    bias = r(4 * H) * 0.1
    return wih.bfloat16().contiguous(), whh.bfloat16().contiguous(), bias


def cell_inputs(E, A, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    latent = torch.relu(r(E, H)).bfloat16()
    la = torch.zeros(E, A, device="cuda")
    idx = torch.randint(0, A, (E,), device="cuda", generator=g)
    la[torch.arange(E, device="cuda"), idx] = 1.0
    lr = r(E) * 0.7                       # not bf16-representable
    h0 = r(E, H) * scale                  # scale 0 -> the reset state
    c0 = r(E, H) * scale
    return latent, la, lr, h0, c0


def cell_outputs(E):
    return (torch.full((E, H), PATTERN, device="cuda"),
            torch.full((E, H), PATTERN, device="cuda"),
            torch.full((E, H), PATTERN, device="cuda").bfloat16())


def run_cell(inp, w, **tile):
    E = inp[0].shape[0]
    h1, c1, hb = cell_outputs(E)
    M_.lstm_cell_step(*inp, *w, h1, c1, hb, **tile)
    return h1, c1, hb


def rin_of(latent, la, lr, A):
    """The bf16 rin row the kernels see, built in torch."""
    E = latent.shape[0]
    rin = torch.zeros(E, kin_pad(A), device="cuda", dtype=torch.bfloat16)
    rin[:, :H] = latent
    rin[:, H:H + A] = la.bfloat16()
    rin[:, H + A] = lr.bfloat16()
    return rin


def cell_exact(inp, w):
    latent, la, lr, h0, c0 = inp
    wih, whh, bias = w
    A = la.shape[1]
    rin = rin_of(latent, la, lr, A).double()
    gates = (rin @ wih.double().t() + bias.double()
             + h0.bfloat16().double() @ whh.double().t()).view(-1, 4, H)
    i_, f_ = torch.sigmoid(gates[:, 0]), torch.sigmoid(gates[:, 1])
    g_, o_ = torch.tanh(gates[:, 2]), torch.sigmoid(gates[:, 3])
    c1 = f_ * c0.double() + i_ * g_
    return o_ * torch.tanh(c1), c1


def cell_yardstick(inp, w):
    """HipInference.forward's post-encoder chain up to h1 / c1."""
    latent, la, lr, h0, c0 = inp
    wih, whh, bias = w
    E = latent.shape[0]
    rin = M_.assemble_rin(latent, la, lr, wih.shape[1])
    x = M_.gemm_bias_act(rin, wih, bias, 0, True)
    hg = M_.gemm_bias_act(h0.bfloat16().contiguous(), whh, torch.Tensor(),
                          0, True)
    gates = (x + hg).view(E, 4, H)
    i_, f_ = torch.sigmoid(gates[:, 0]), torch.sigmoid(gates[:, 1])
    g_, o_ = torch.tanh(gates[:, 2]), torch.sigmoid(gates[:, 3])
    c1 = f_ * c0 + i_ * g_
    return o_ * torch.tanh(c1), c1


@pytest.mark.parametrize("E,A", GRID)
def test_cell_step_calibrated(E, A):
    w = cell_weights(A)
    for scale in (0.0, 0.1, 1.0):
        inp = cell_inputs(E, A, 7 * E + A, scale)
        h1, c1, hb = run_cell(inp, w)
        he, ce = cell_exact(inp, w)
        hy, cy = cell_yardstick(inp, w)
        tag = f"E{E} A{A} s{scale}"
        assert_bound(f"cell h1 {tag}", h1, hy, he, FLOOR)
        assert_bound(f"cell c1 {tag}", c1, cy, ce, FLOOR)
        assert bits_equal(hb, h1.bfloat16()), tag


def test_cell_step_rin_rounding_matches_assemble_rin():
    """The rows the kernel builds round as assemble_rin does.  W_ih is an
    identity block from the action and reward columns onto the g gate of
    units 0..A, everything else zero and c0 = 0, so
    c1 = sigmoid(0) * tanh(rin entry) = 0.5 * tanh(rin entry).  An entry
    rounded any other way would be off by a bf16 ulp, 2^-8 relative."""
    E, A = 5, 9
    latent, _, lr, h0, c0 = cell_inputs(E, A, 3, 1.0)
    la = torch.randn(E, A, device="cuda")        # not one-hot, not bf16
    KP = kin_pad(A)
    wih = torch.zeros(4 * H, KP, device="cuda")
    for j in range(A + 1):
        wih[2 * H + j, H + j] = 1.0
    w = (wih.bfloat16(), torch.zeros(4 * H, H, device="cuda").bfloat16(),
         torch.zeros(4 * H, device="cuda"))
    _, c1, _ = run_cell((latent, la, lr, h0, torch.zeros_like(c0)), w)
    rin = M_.assemble_rin(latent, la, lr, KP)
    want = 0.5 * torch.tanh(rin[:, H:H + A + 1].double())
    assert rel_err(c1[:, :A + 1], want) < 1e-6


def test_cell_step_tile_variants_bit_equal():
    """Every (units, rows) tile the wrapper offers computes the same bits."""
    for E, A in ((17, 9), (65, 31), (256, 2)):
        w = cell_weights(A)
        inp = cell_inputs(E, A, 11, 1.0)
        ref = run_cell(inp, w)
        for units in (8, 16):
            for rows in (16, 32, 64):
                got = run_cell(inp, w, units=units, rows=rows)
                for a, b in zip(got, ref):
                    assert bits_equal(a, b), (E, units, rows)


@pytest.mark.parametrize("row,keep", [(16, slice(0, 16)), (0, slice(1, 17))])
def test_cell_step_row_isolation(row, keep):
    E, A = 17, 9
    w = cell_weights(A)
    inp = cell_inputs(E, A, 5, 1.0)
    ref = run_cell(inp, w)
    latent, la, lr, h0, c0 = [t.clone() for t in inp]
    latent[row] = (latent[row].float() * 3 + 1).bfloat16()
    la[row] = torch.roll(la[row], 1)
    lr[row] += 2.0
    h0[row] = -h0[row] + 0.5
    c0[row] = c0[row] * 2 - 1
    got = run_cell((latent, la, lr, h0, c0), w)
    for a, b in zip(got, ref):
        assert bits_equal(a[keep], b[keep])
        assert not bits_equal(a[row], b[row])


def test_cell_step_layout_invariance():
    A = 18
    w = cell_weights(A)
    big = cell_inputs(256, A, 9, 1.0)
    small = tuple(t[:5].contiguous() for t in big)
    for a, b in zip(run_cell(big, w), run_cell(small, w)):
        assert bits_equal(a[:5], b)


def test_cell_step_untouched_memory():
    E, A = 17, 9
    w = cell_weights(A)
    inp = cell_inputs(E, A, 13, 1.0)
    n, lead = E * H, 1000
    bufs = [torch.full((n + 2 * lead,), PATTERN, device="cuda"),
            torch.full((n + 2 * lead,), PATTERN, device="cuda"),
            torch.full((n + 2 * lead,), PATTERN, device="cuda").bfloat16()]
    outs = [b[lead:lead + n].view(E, H) for b in bufs]
    M_.lstm_cell_step(*inp, *w, *outs)
    ref = run_cell(inp, w)
    for b, o, r in zip(bufs, outs, ref):
        assert bits_equal(o, r)
        pat = torch.full((lead,), PATTERN, device="cuda").to(b.dtype)
        assert bits_equal(b[:lead], pat) and bits_equal(b[lead + n:], pat)


def test_cell_step_pad_columns_unread():
    """NaN in the pad columns of wih_t (k >= 512 + A + 1) changes nothing."""
    for A in (2, 18):
        wih, whh, bias = cell_weights(A)
        inp = cell_inputs(17, A, 21, 1.0)
        ref = run_cell(inp, (wih, whh, bias))
        bad = wih.clone()
        assert H + A + 1 < bad.shape[1]
        bad[:, H + A + 1:] = float("nan")
        for a, b in zip(run_cell(inp, (bad, whh, bias)), ref):
            assert bits_equal(a, b), A


def test_cell_step_no_reads_past_E():
    """NaN in the storage rows past E of every per-row input: no output is
    NaN and the result equals the tightly allocated launch."""
    E, A, extra = 17, 9, 3
    w = cell_weights(A)
    inp = cell_inputs(E, A, 23, 1.0)
    ref = run_cell(inp, w)
    over = []
    for t in inp:
        big = torch.full((E + extra,) + tuple(t.shape[1:]), float("nan"),
                         device="cuda", dtype=t.dtype)
        big[:E] = t
        over.append(big[:E])
    got = run_cell(tuple(over), w)
    for a, b in zip(got, ref):
        assert not torch.isnan(a.float()).any()
        assert bits_equal(a, b)


# ---------------------------------------------------------------------------
# Heads
# ---------------------------------------------------------------------------

PAD = 32


@functools.lru_cache(maxsize=None)
def head_weights(A):
    g = torch.Generator(device="cuda").manual_seed(200 + A)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    bf = lambda t: t.bfloat16().contiguous()

    def out(rows):
        wt = torch.zeros(PAD, H, device="cuda")
        wt[:rows] = r(rows, H) / np.sqrt(H)
        b = torch.zeros(PAD, device="cuda")
        b[:rows] = r(rows) * 0.1
        return bf(wt), b

    wa1, ba1 = bf(r(H, H) / np.sqrt(H)), r(H) * 0.1
    wv1, bv1 = bf(r(H, H) / np.sqrt(H)), r(H) * 0.1
    wa2, ba2 = out(A)
    wv2, bv2 = out(1)
    return dict(wa1=wa1, ba1=ba1, wv1=wv1, bv1=bv1, wa2=wa2, ba2=ba2,
                wv2=wv2, bv2=bv2)


def head_input(E, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(E, H, device="cuda", generator=g).bfloat16()


def run_heads(hb, w, A):
    E = hb.shape[0]
    adv1 = torch.full((E, H), PATTERN, device="cuda").bfloat16()
    val1 = adv1.clone()
    q = torch.full((E, A), PATTERN, device="cuda")
    greedy = torch.full((E,), -7, device="cuda", dtype=torch.int32)
    M_.head_hidden_step(hb, w["wa1"], w["ba1"], w["wv1"], w["bv1"],
                        adv1, val1)
    M_.head_out_step(adv1, val1, w["wa2"], w["ba2"], w["wv2"], w["bv2"],
                     q, greedy)
    return q, greedy, adv1, val1


def heads_yardstick(hb, w, A):
    adv1 = M_.gemm_bias_act(hb, w["wa1"], w["ba1"], 1, False)
    adv2 = M_.gemm_bias_act(adv1, w["wa2"], w["ba2"], 0, True)
    val1 = M_.gemm_bias_act(hb, w["wv1"], w["bv1"], 1, False)
    val2 = M_.gemm_bias_act(val1, w["wv2"], w["bv2"], 0, True)
    return M_.dueling_combine(adv2, val2, A), adv1, val1


def heads_exact(hb, w, A):
    """float64, no rounding of the hidden layer: its bf16 storage is part of
    the error of both paths."""
    x = hb.double()
    a1 = torch.relu(x @ w["wa1"].double().t() + w["ba1"].double())
    v1 = torch.relu(x @ w["wv1"].double().t() + w["bv1"].double())
    adv = (a1 @ w["wa2"].double().t() + w["ba2"].double())[:, :A]
    val = (v1 @ w["wv2"].double().t() + w["bv2"].double())[:, :1]
    return val + adv - adv.mean(1, keepdim=True), a1, v1


@pytest.mark.parametrize("E,A", GRID)
def test_heads_calibrated(E, A):
    w = head_weights(A)
    hb = head_input(E, 31 * E + A)
    q, greedy, adv1, val1 = run_heads(hb, w, A)
    qy, a1y, v1y = heads_yardstick(hb, w, A)
    qe, a1e, v1e = heads_exact(hb, w, A)
    tag = f"E{E} A{A}"
    assert_bound(f"heads adv1 {tag}", adv1, a1y, a1e)
    assert_bound(f"heads val1 {tag}", val1, v1y, v1e)
    assert_bound(f"heads q {tag}", q, qy, qe)
    assert greedy.dtype == torch.int32
    assert torch.equal(greedy.long(), q.argmax(1)), tag


@pytest.mark.parametrize("A", AS)
def test_heads_greedy_ties_and_margin(A):
    E = 17
    hb = head_input(E, 77)
    z = {k: torch.zeros_like(v) for k, v in head_weights(A).items()}
    q, greedy, _, _ = run_heads(hb, z, A)
    assert torch.equal(q, torch.zeros_like(q))
    assert torch.equal(greedy, torch.zeros_like(greedy)), "first index on ties"
    # one real column raised by a known margin wins — on zero weights and on
    # random ones whose advantages are O(1)
    for base in (z, head_weights(A)):
        for col in sorted({0, A // 2, A - 1}):
            w = dict(base)
            w["ba2"] = base["ba2"].clone()
            w["ba2"][col] += 100.0
            q, greedy, _, _ = run_heads(hb, w, A)
            assert torch.equal(greedy, torch.full_like(greedy, col)), col
            assert torch.equal(greedy.long(), q.argmax(1))
    # two equal maxima: the lower index wins
    if A >= 3:
        w = dict(z)
        w["ba2"] = z["ba2"].clone()
        w["ba2"][A - 1] = 5.0
        w["ba2"][1] = 5.0
        _, greedy, _, _ = run_heads(hb, w, A)
        assert torch.equal(greedy, torch.full_like(greedy, 1))


@pytest.mark.parametrize("row,keep", [(16, slice(0, 16)), (0, slice(1, 17))])
def test_heads_row_isolation(row, keep):
    E, A = 17, 9
    w = head_weights(A)
    hb = head_input(E, 41)
    ref = run_heads(hb, w, A)
    hb2 = hb.clone()
    hb2[row] = (-hb2[row].float() + 0.25).bfloat16()
    got = run_heads(hb2, w, A)
    for a, b in zip(got, ref):
        assert bits_equal(a[keep], b[keep])
    assert not bits_equal(got[0][row], ref[0][row])


def test_heads_layout_invariance():
    A = 18
    w = head_weights(A)
    hb = head_input(256, 43)
    big = run_heads(hb, w, A)
    small = run_heads(hb[:5].contiguous(), w, A)
    for a, b in zip(big, small):
        assert bits_equal(a[:5], b)
    # and across the hidden kernel's two row tiles
    for rows in (16, 64):
        adv1 = torch.empty_like(big[2])
        val1 = torch.empty_like(big[3])
        M_.head_hidden_step(hb, w["wa1"], w["ba1"], w["wv1"], w["bv1"],
                            adv1, val1, rows=rows)
        assert bits_equal(adv1, big[2]) and bits_equal(val1, big[3])


def test_heads_untouched_memory_and_past_E():
    E, A, lead = 17, 9, 1000
    w = head_weights(A)
    big = torch.full((E + 3, H), float("nan"), device="cuda").bfloat16()
    big[:E] = head_input(E, 47)
    hb = big[:E]
    ref = run_heads(hb.clone(), w, A)
    qbuf = torch.full((E * A + 2 * lead,), PATTERN, device="cuda")
    gbuf = torch.full((E + 2 * lead,), -7, device="cuda", dtype=torch.int32)
    hbuf = torch.full((2, E * H + 2 * lead), PATTERN,
                      device="cuda").bfloat16()
    adv1 = hbuf[0, lead:lead + E * H].view(E, H)
    val1 = hbuf[1, lead:lead + E * H].view(E, H)
    q = qbuf[lead:lead + E * A].view(E, A)
    greedy = gbuf[lead:lead + E]
    M_.head_hidden_step(hb, w["wa1"], w["ba1"], w["wv1"], w["bv1"],
                        adv1, val1)
    M_.head_out_step(adv1, val1, w["wa2"], w["ba2"], w["wv2"], w["bv2"],
                     q, greedy)
    for a, b in zip((q, greedy, adv1, val1), ref):
        assert bits_equal(a, b)
    assert (qbuf[:lead] == PATTERN).all() and (qbuf[-lead:] == PATTERN).all()
    assert (gbuf[:lead] == -7).all() and (gbuf[-lead:] == -7).all()
    pat = torch.tensor(PATTERN).bfloat16().item()
    assert (hbuf[:, :lead] == pat).all() and (hbuf[:, -lead:] == pat).all()


# ---------------------------------------------------------------------------
# Operand rejection: raises, outputs' pattern untouched
# ---------------------------------------------------------------------------

def _cell_args(E=5, A=9):
    inp = cell_inputs(E, A, 1, 1.0)
    return list(inp) + list(cell_weights(A)) + list(cell_outputs(E))


def _bad_cell_cases():
    E, A = 5, 9

    def dtype(a): a[0] = a[0].float()
    def shape(a): a[3] = a[3][:, :256].contiguous()
    def stride(a):
        a[3] = torch.randn(E, 2 * H, device="cuda")[:, :H]
    def cpu(a): a[4] = a[4].cpu()
    def alias(a): a[8] = a[3]
    def alias_c(a): a[9] = a[4]
    def out_dtype(a): a[10] = a[10].float()
    def bias_shape(a): a[7] = a[7][:H].contiguous()
    def kin_small(a): a[5] = a[5][:, :512].contiguous()
    def kin_mod(a):
        a[5] = torch.zeros(4 * H, 552, device="cuda").bfloat16()
    return [dtype, shape, stride, cpu, alias, alias_c, out_dtype, bias_shape,
            kin_small, kin_mod]


@pytest.mark.parametrize("mutate", _bad_cell_cases(),
                         ids=lambda f: f.__name__)
def test_cell_step_rejects(mutate):
    a = _cell_args()
    outs = a[8:11]
    mutate(a)
    with pytest.raises((RuntimeError, TypeError)):
        M_.lstm_cell_step(*a)
    torch.cuda.synchronize()
    for o in outs:
        assert (o.float() == torch.tensor(PATTERN).to(o.dtype).float()).all()


@pytest.mark.parametrize("E,A", [(0, 9), (5, 33)], ids=["E0", "A33"])
def test_cell_step_rejects_sizes(E, A):
    latent = torch.zeros(E, H, device="cuda").bfloat16()
    la = torch.zeros(E, A, device="cuda")
    lr = torch.zeros(E, device="cuda")
    h0 = torch.zeros(E, H, device="cuda")
    c0 = torch.zeros(E, H, device="cuda")
    wih = torch.zeros(4 * H, kin_pad(A), device="cuda").bfloat16()
    _, whh, bias = cell_weights(9)
    outs = cell_outputs(E)
    with pytest.raises(RuntimeError):
        M_.lstm_cell_step(latent, la, lr, h0, c0, wih, whh, bias, *outs)
    torch.cuda.synchronize()
    for o in outs:
        assert (o.float() == torch.tensor(PATTERN).to(o.dtype).float()).all()


def test_heads_reject():
    E, A = 5, 9
    w = head_weights(A)
    hb = head_input(E, 3)
    pat_bf = torch.tensor(PATTERN).bfloat16().item()

    def fresh():
        return dict(
            adv1=torch.full((E, H), PATTERN, device="cuda").bfloat16(),
            val1=torch.full((E, H), PATTERN, device="cuda").bfloat16(),
            q=torch.full((E, A), PATTERN, device="cuda"),
            greedy=torch.full((E,), -7, device="cuda", dtype=torch.int32))

    def hidden(o, hb=hb, **kw):
        ww = dict(w, **kw)
        M_.head_hidden_step(hb, ww["wa1"], ww["ba1"], ww["wv1"], ww["bv1"],
                            o["adv1"], o["val1"])

    def out(o, **kw):
        ww = dict(w, **kw)
        M_.head_out_step(kw.get("adv1", o["adv1"]), o["val1"], ww["wa2"],
                         ww["ba2"], ww["wv2"], ww["bv2"], o["q"], o["greedy"])

    bad = [
        lambda o: hidden(o, hb=hb.float()),                       # dtype
        lambda o: hidden(o, hb=hb[:, :256].contiguous()),         # shape
        lambda o: hidden(o, hb=torch.zeros(E, 2 * H, device="cuda")
                         .bfloat16()[:, :H]),                     # stride
        lambda o: hidden(o, hb=hb.cpu()),                         # CPU
        lambda o: hidden(o, hb=hb[:0]),                           # E = 0
        lambda o: hidden(o, hb=o["adv1"]),                        # alias
        lambda o: hidden(o, ba1=w["ba1"][:100].contiguous()),
        lambda o: out(o, wa2=w["wa2"].float()),                   # dtype
        lambda o: out(o, wa2=w["wa2"][:16].contiguous()),         # shape
        lambda o: out(o, bv2=w["bv2"].cpu()),                     # CPU
        lambda o: out(o, adv1=torch.zeros(E, 2 * H, device="cuda")
                      .bfloat16()[:, :H]),                        # stride
        lambda o: out(dict(o, q=torch.full((E, 33), PATTERN,
                                           device="cuda"))),      # A = 33
        lambda o: out(dict(o, greedy=o["greedy"].long())),        # dtype
        lambda o: out(dict(o, adv1=o["adv1"][:0], val1=o["val1"][:0],
                           q=o["q"][:0], greedy=o["greedy"][:0])),  # E = 0
    ]
    for i, f in enumerate(bad):
        o = fresh()
        with pytest.raises((RuntimeError, TypeError)):
            f(o)
        torch.cuda.synchronize()
        assert (o["adv1"] == pat_bf).all() and (o["val1"] == pat_bf).all(), i
        assert (o["q"] == PATTERN).all() and (o["greedy"] == -7).all(), i


# ---------------------------------------------------------------------------
# HipInference.step against HipInference.forward
# ---------------------------------------------------------------------------

class _Spy:
    """Stands in for the extension module on one HipInference: records the
    latent each path hands to its first post-encoder call."""

    def __init__(self, m):
        self._m = m
        self.latents = {"assemble_rin": [], "lstm_cell_step": []}

    def __getattr__(self, name):
        f = getattr(self._m, name)
        if name not in self.latents:
            return f

        def wrapped(*a, **k):
            self.latents[name].append(a[0].clone())
            return f(*a, **k)
        return wrapped


NETS = [pytest.param("mspacman", id="nature4"),
        pytest.param("mspacman_reference", id="nature1"),
        pytest.param("seaquest_impala", id="impala")]


def make_inference(preset):
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.ops.engine import HipInference
    c = cfg.apply(preset)
    torch.manual_seed(3)
    net = Network(c.action_dim, c.obs_shape, 512, encoder=c.encoder,
                  forward_steps=c.forward_steps).cuda().eval()
    inf = HipInference(net, "cuda")
    inf.m = _Spy(inf.m)
    return c, inf


def tick_inputs(c, E, seed, scale=0.3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randint(0, 256, (E,) + tuple(c.obs_shape), device="cuda",
                        dtype=torch.uint8, generator=g)
    la = torch.zeros(E, c.action_dim, device="cuda")
    idx = torch.randint(0, c.action_dim, (E,), device="cuda", generator=g)
    la[torch.arange(E, device="cuda"), idx] = 1.0
    lr = torch.randn(E, 1, device="cuda", generator=g) * 0.3
    h = torch.randn(1, E, 512, device="cuda", generator=g) * scale
    cc = torch.randn(1, E, 512, device="cuda", generator=g) * scale
    return obs, la, lr, h, cc


def pack_exact(p, latent, la, lr, h0_64, c0_64, A):
    """float64 tick from the packed weights; h0 is rounded to bf16 as both
    paths round it, everything after stays float64."""
    w = (p.wih_t, p.whh_t, p.lstm_bias)
    E = latent.shape[0]
    rin = rin_of(latent, la, lr.reshape(E), A).double()
    hb0 = h0_64.float().bfloat16().double()
    gates = (rin @ w[0].double().t() + w[2].double()
             + hb0 @ w[1].double().t()).view(E, 4, H)
    i_, f_ = torch.sigmoid(gates[:, 0]), torch.sigmoid(gates[:, 1])
    g_, o_ = torch.tanh(gates[:, 2]), torch.sigmoid(gates[:, 3])
    c1 = f_ * c0_64 + i_ * g_
    h1 = o_ * torch.tanh(c1)
    a1 = torch.relu(h1 @ p.wa1t.double().t() + p.ba1.double())
    v1 = torch.relu(h1 @ p.wv1t.double().t() + p.bv1.double())
    adv = (a1 @ p.wa2t.double().t() + p.ba2.double())[:, :A]
    val = (v1 @ p.wv2t.double().t() + p.bv2.double())[:, :1]
    return val + adv - adv.mean(1, keepdim=True), h1, c1


@pytest.mark.parametrize("E", [5, 64])
@pytest.mark.parametrize("preset", NETS)
def test_step_matches_forward(preset, E):
    from r2d2_amd import config as cfg
    try:
        c, inf = make_inference(preset)
        obs, la, lr, h, cc = tick_inputs(c, E, 5)
        h_in, c_in = h.clone(), cc.clone()
        qf, (hf, cf) = inf.forward(obs, la, lr, (h, cc))
        q, greedy, (h1, c1) = inf.step(obs, la, lr, (h, cc))
        assert bits_equal(h, h_in) and bits_equal(cc, c_in)
        assert q.shape == qf.shape == (E, c.action_dim)
        assert h1.shape == hf.shape == (1, E, 512) and c1.shape == cf.shape
        assert greedy.shape == (E,) and greedy.dtype == torch.int32
        lat_f, = inf.m.latents["assemble_rin"]
        lat_s, = inf.m.latents["lstm_cell_step"]
        assert bits_equal(lat_f, lat_s), "same encoder calls, same latent"
        qe, he, ce = pack_exact(inf.pack, lat_s, la, lr, h[0].double(),
                                cc[0].double(), c.action_dim)
        tag = f"{preset} E{E}"
        assert_bound(f"step h1 {tag}", h1[0], hf[0], he, FLOOR)
        assert_bound(f"step c1 {tag}", c1[0], cf[0], ce, FLOOR)
        assert_bound(f"step q {tag}", q, qf, qe)
        assert torch.equal(greedy.long(), q.argmax(1))
        # the reset path zeroes one env's state in place
        h1[0, 1].zero_()
        assert (h1[0, 1] == 0).all() and (h1[0, 0] != 0).any()
    finally:
        cfg.apply("mspacman")


def test_step_eight_teacher_forced_ticks():
    """Fixed observation / action / reward sequences, state fed back.  The
    float64 recurrence applies the per-tick roundings of both paths: rin and
    the h operand to bf16 (c and the carried h stay unrounded)."""
    from r2d2_amd import config as cfg
    try:
        E, T = 5, 8
        c, inf = make_inference("mspacman")
        A = c.action_dim
        seq = [tick_inputs(c, E, 100 + t) for t in range(T)]
        _, _, _, h, cc = tick_inputs(c, E, 99, scale=0.1)
        hs, cs = h, cc
        hf, cf = h, cc
        he, ce = h[0].double(), cc[0].double()
        for obs, la, lr, _, _ in seq:
            _, _, (hs, cs) = inf.step(obs, la, lr, (hs, cs))
            _, (hf, cf) = inf.forward(obs, la, lr, (hf, cf))
            lat = inf.m.latents["lstm_cell_step"][-1]
            assert bits_equal(lat, inf.m.latents["assemble_rin"][-1])
            _, he, ce = pack_exact(inf.pack, lat, la, lr, he, ce, A)
        assert_bound("8 ticks h", hs[0], hf[0], he, FLOOR)
        assert_bound("8 ticks c", cs[0], cf[0], ce, FLOOR)
    finally:
        cfg.apply("mspacman")


# ---------------------------------------------------------------------------
# VectorActor
# ---------------------------------------------------------------------------

def _run_actor(fused):
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.train import epsilon_ladder
    from r2d2_amd.worker import VectorActor

    # episodes capped at 12 steps: with E = 4 and 120 env steps every env
    # cuts blocks and resets (truncation) at least once
    c = cfg.apply("mspacman_gpu_replay", num_actors=4, block_length=8,
                  burn_in_steps=4, learning_steps=4, forward_steps=2,
                  actor_update_interval=64, max_episode_steps=12,
                  fused_actor_step=fused)
    torch.manual_seed(0)
    model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                    forward_steps=c.forward_steps)
    sq = queue.Queue()
    va = VectorActor(epsilon_ladder(4), model, [sq], device="cuda", seed=4)
    assert va.hip_inf is not None, "K15 path must be active on GPU"
    calls = {"step": [], "forward": 0}
    step, forward = va.hip_inf.step, va.hip_inf.forward

    def spy_step(*a):
        out = step(*a)
        h, cc = out[2]
        calls["step"].append(torch.stack((h[0], cc[0]), 1).cpu().numpy())
        return out

    def spy_forward(*a):
        calls["forward"] += 1
        return forward(*a)

    va.hip_inf.step, va.hip_inf.forward = spy_step, spy_forward
    total = va.run(stop_after_steps=120)
    assert total >= 120
    blocks = []
    while not sq.empty():
        blocks.append(sq.get())
    return c, calls, blocks


def test_vector_actor_fused_step():
    from r2d2_amd import config as cfg
    try:
        c, calls, blocks = _run_actor(True)
        assert calls["forward"] == 0 and len(calls["step"]) >= 30
        assert len(blocks) >= 4
        seen = {row.tobytes() for tick in calls["step"] for row in tick}
        seen.add(np.zeros((2, 512), np.float32).tobytes())   # the reset state
        n_from_step = 0
        for block, prio, reward in blocks:
            assert np.isfinite(prio).all()
            assert block.obs.dtype == np.uint8
            assert block.obs.shape[1:] == (4, 84, 84)
            assert block.hidden.shape == (block.num_sequences, 2, 512)
            assert block.hidden.dtype == np.float32
            assert block.last_action.shape[1] == c.action_dim
            for s in range(block.num_sequences):
                assert block.hidden[s].tobytes() in seen
                n_from_step += bool(block.hidden[s].any())
        assert n_from_step > 0, "some stored state came from step"
    finally:
        cfg.apply("mspacman")


def test_vector_actor_field_off_never_steps():
    from r2d2_amd import config as cfg
    try:
        _, calls, blocks = _run_actor(False)
        assert calls["step"] == [] and calls["forward"] >= 30
        assert len(blocks) >= 4
    finally:
        cfg.apply("mspacman")
