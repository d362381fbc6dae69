"""GPU numerics: the persistent LSTM at every launch layout.

The host wrappers pick a template instantiation from the batch size B:

    B            lstm_fwd                      lstm_bwd
    <= 32        <512, 64, 8>                  <512, 16, 16>, KSPLIT 4, 4 quarters
    33 .. 48     <512, 32, 16>, 2 halves       <512, 32, 16>, KSPLIT 2, 2 halves
    49 .. 64     <512, 32, 16>, 2 halves       <512, 16, 16>, KSPLIT 4, 4 quarters

(These four instantiations are all the build has; the same two templates
also serve lstm_fwd_multi / lstm_bwd_multi, see test_hip_lstm_multi.py.
With B <= 32 the backward's quarters past the batch hold no rows: a build
whose quartered backward used the wrong rows failed these tests at B = 32 as
well as at 49 and 64.)

B in {1, 32, 33, 48, 49, 64} runs every column at a full last tile and at a
one-row last tile (1: one row in all; 33: second half holds 1 row; 49:
fourth quarter holds 1).

Two references, both plain torch on the same bf16-rounded X / W_hh:
  * exact: the recurrence in float64 (test_hip_lstm.ref_lstm) and float64
    autograd.  Every error is measured against this one.
  * rounding model: a float32 forward and BPTT that round to bf16 exactly
    where the kernels store bf16 (Hout per step and read back, the gate
    stash, dgates before the recurrent product).  It only says how much
    error that storage format costs.
Tolerance: err = max|x - exact| / max|exact|, and the kernel must satisfy
err(kernel) <= 4 * err(rounding model).  The 4 covers the different f32
accumulation order (MFMA k-blocking, K-split partial sums) and the fast
sigmoid/tanh.  The kernel is never its own yardstick.
"""

import functools

import numpy as np
import pytest
import torch

from test_hip_lstm import ref_lstm

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

H = 512
FACTOR = 4.0

BS = [1, 32, 33, 48, 49, 64]
TS = [1, 2, 7]


def column(B):
    """Which column of the layout table a batch size runs."""
    return "le32" if B <= 32 else ("33to48" if B <= 48 else "49to64")


# ---------------------------------------------------------------------------
# The calibrated tolerance, implemented once (test_hip_head_glue imports it)
# ---------------------------------------------------------------------------

def rel_err(x, exact):
    """max |x - exact| / max |exact|, in float64."""
    exact = exact.double()
    return ((x.double() - exact).abs().max()
            / exact.abs().max().clamp_min(1e-300)).item()


def assert_calibrated(name, kernel, model, exact, factor=FACTOR):
    """err(kernel) <= factor * err(model), both against `exact`.  Prints the
    two figures first so a run with -rP records them."""
    assert kernel.shape == exact.shape == model.shape, name
    assert torch.isfinite(kernel.float()).all(), f"{name}: non-finite"
    ek, em = rel_err(kernel, exact), rel_err(model, exact)
    print(f"CALIB {name}: kernel {ek:.3e} model {em:.3e} "
          f"ratio {ek / em if em > 0 else float('inf') if ek > 0 else 0:.2f}")
    assert ek <= factor * em, (name, ek, em)
    return ek, em


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---------------------------------------------------------------------------
# Length masks: deterministic lists.  lens >= 1 always holds in the engine:
# both engine._positions and the positions_meta kernel set
# lens = burn_in + learning + forward steps, and a stored sequence has at
# least one learning step — so lens = 0 cannot occur and is not tested.
# ---------------------------------------------------------------------------

def make_lens(B, T, kind):
    if kind == "full":
        l = [T] * B
    elif kind == "ones":
        l = [1] * B
    else:
        cyc = [1, max(1, T - 1), T, max(1, (T + 1) // 2)]
        l = [cyc[b % 4] for b in range(B)]
        l[B - 1] = T if B > 1 else max(1, T - 1)
        if kind == "q3ones":       # the whole last quarter masked from step 1
            l[48:64] = [1] * 16
            l[0] = T
        elif kind == "q0ones":      # the whole first quarter
            l[0:16] = [1] * 16
        else:
            assert kind == "mixed", kind
    return torch.tensor(l, dtype=torch.int32, device="cuda")


def case_list():
    out = []
    for B in BS:
        for T in TS:
            kinds = ["full"] if T == 1 else ["full", "ones", "mixed"]
            if B == 64 and T > 1:
                kinds += ["q3ones", "q0ones"]
            for k in kinds:
                out.append(pytest.param(B, T, k,
                                        id=f"{column(B)}-B{B}-T{T}-{k}"))
    return out


CASES = case_list()
# the two-network forward: every B and T, the mixed mask (full at T = 1)
CASES2 = [pytest.param(B, T, "full" if T == 1 else "mixed",
                       id=f"{column(B)}-B{B}-T{T}")
          for B in BS for T in TS]


def make_inputs(B, T, seed, scale=0.5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    X = (r(B, T, 4 * H) * scale).bfloat16()
    Whh = (r(4 * H, H) / np.sqrt(H)).bfloat16()
    # f32 initial state that is NOT bf16-representable, as in a real run:
    # the kernel's rounding of h0 into Hout[:, 0] is part of the format cost
    h0 = r(B, H) * 0.1
    c0 = r(B, H) * 0.1
    dHext = r(B, T, H) * 0.1        # non-zero at masked steps too
    return X, Whh, h0, c0, dHext


# ---------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------

def gates_of(X, Whh, Hs, lens):
    """Post-nonlinearity gates (B, T, 4H) of a recurrence whose hidden states
    are Hs; zero at t >= lens[b] (what the kernel stashes)."""
    B, T, _ = X.shape
    pre = X + Hs[:, :T] @ Whh.t()
    i, f, g, o = pre.split(H, dim=2)
    st = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g),
                    torch.sigmoid(o)], dim=2)
    act = (torch.arange(T, device=X.device)[None, :] < lens[:, None])
    return st * act.unsqueeze(2).to(st.dtype)


def exact_ref(X, Whh, h0, c0, lens, dHext=None):
    """float64 recurrence (+ autograd): Hs, Cs, stash, dL/dX, dL/dWhh for the
    loss sum(Hs[:, 1:] * dHext)."""
    X64 = X.double().requires_grad_(dHext is not None)
    W64 = Whh.double().requires_grad_(dHext is not None)
    Hs, Cs = ref_lstm(X64, W64, h0.double(), c0.double(), lens)
    out = dict(H=Hs.detach(), C=Cs.detach(),
               stash=gates_of(X64.detach(), W64.detach(), Hs.detach(), lens))
    if dHext is not None:
        (Hs[:, 1:] * dHext.double()).sum().backward()
        out["dX"] = X64.grad
        out["dWhh"] = W64.grad
    return out


def bf(x):
    return x.bfloat16().float()


def model_fwd(X, Whh, h0, c0, lens):
    """float32 forward, bf16 where lstm_fwd_kernel stores bf16: h is rounded
    when written to Hout and the next step reads that rounded value; the
    stash is bf16; c stays f32."""
    B, T, _ = X.shape
    Xf, W = X.float(), Whh.float()
    h, c = bf(h0), c0.clone()
    hs, cs, st = [h], [c], []
    for t in range(T):
        gates = Xf[:, t] + h @ W.t()
        i, f, g, o = gates.split(H, dim=1)
        i, f, g, o = (torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g),
                      torch.sigmoid(o))
        c_new = f * c + i * g
        h_new = bf(o * torch.tanh(c_new))
        act = (t < lens).unsqueeze(1)
        h = torch.where(act, h_new, h)
        c = torch.where(act, c_new, c)
        hs.append(h)
        cs.append(c)
        st.append(bf(torch.where(act, torch.cat([i, f, g, o], 1),
                                 torch.zeros_like(gates))))
    return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(st, 1)


def model_bwd(stash, Cs, dHext, Whh, lens):
    """float32 BPTT on the model's own bf16 stash and f32 c, with dgates
    rounded to bf16 before the recurrent product, as lstm_bwd_kernel does.
    A masked step carries dh and dc through to the last active step."""
    B, T, _ = stash.shape
    W = Whh.float()                               # (4H, H)
    dG = torch.zeros(B, T, 4 * H, device=stash.device)
    dh_s = torch.zeros(B, H, device=stash.device)
    dc_s = torch.zeros(B, H, device=stash.device)
    for t in range(T - 1, -1, -1):
        ext = dHext[:, t]
        if t == T - 1:
            dh, dc_in = ext, torch.zeros_like(ext)
        else:
            nxt = ((t + 1) < lens).unsqueeze(1)
            rec = dG[:, t + 1] @ W
            f_next = stash[:, t + 1, H:2 * H]
            dh = ext + torch.where(nxt, rec, dh_s)
            dc_in = torch.where(nxt, dc_s * f_next, dc_s)
        act = (t < lens).unsqueeze(1)
        i, f, g, o = stash[:, t].split(H, dim=1)
        tc = torch.tanh(Cs[:, t + 1])
        dc = dc_in + dh * o * (1 - tc * tc)
        d = torch.cat([dc * g * i * (1 - i), dc * Cs[:, t] * f * (1 - f),
                       dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dG[:, t] = bf(torch.where(act, d, torch.zeros_like(d)))
        dh_s = dh
        dc_s = torch.where(act, dc, dc_in)
    return dG


# ---------------------------------------------------------------------------
# Kernel runners
# ---------------------------------------------------------------------------

def new_bar():
    return torch.zeros(512, dtype=torch.int32, device="cuda")


def poison(bar):
    """The poison word (reading it synchronises).  A set word means a
    workgroup gave up waiting on a handoff counter: nothing more should run
    on that GPU, so the whole session stops instead of launching again."""
    p = int(bar[256].item())
    if p:
        pytest.exit("LSTM poison word set: stopping all GPU work",
                    returncode=3)
    return p


def kernel_fwd(X, Whh, h0, c0, lens, bar=None, second=None):
    """One-network forward, or two networks when `second` = (X1, Whh1, h1,
    c1).  Returns [H0, C0, H1, C1, stash] and asserts the poison word."""
    bar = new_bar() if bar is None else bar
    init = torch.stack([h0, c0]).contiguous()
    e = torch.Tensor()
    if second is None:
        outs = M_.lstm_fwd(X, e, Whh, e, init, e, lens, bar, True)
    else:
        X1, Whh1, h1, c1 = second
        outs = M_.lstm_fwd(X, X1, Whh, Whh1, init,
                           torch.stack([h1, c1]).contiguous(), lens, bar, True)
    assert poison(bar) == 0, "lstm_fwd tripped the poison word"
    return outs


def kernel_bwd(stash, C, Hk, dHext, Whh, lens, bar=None):
    bar = new_bar() if bar is None else bar
    dg = M_.lstm_bwd(stash, C, Hk, dHext.contiguous(),
                     Whh.t().contiguous(), lens, bar)
    assert poison(bar) == 0, "lstm_bwd tripped the poison word"
    return dg


@functools.lru_cache(maxsize=None)
def case(B, T, kind, seed=0):
    """Inputs, the two references and the kernel's forward + backward for
    one (B, T, mask).  Computed once and shared by the tests; nothing in it
    is modified afterwards."""
    X, Whh, h0, c0, dHext = make_inputs(B, T, seed=1000 * B + 10 * T + seed)
    lens = make_lens(B, T, kind)
    ex = exact_ref(X, Whh, h0, c0, lens, dHext)
    mH, mC, mS = model_fwd(X, Whh, h0, c0, lens)
    mdG = model_bwd(mS, mC, dHext, Whh, lens)
    kH, kC, _, _, kS = kernel_fwd(X, Whh, h0, c0, lens)
    kdG = kernel_bwd(kS, kC, kH, dHext, Whh, lens)
    torch.cuda.synchronize()
    return dict(X=X, Whh=Whh, h0=h0, c0=c0, dHext=dHext, lens=lens, ex=ex,
                mH=mH, mC=mC, mS=mS, mdG=mdG, kH=kH, kC=kC, kS=kS, kdG=kdG)


def check_fwd(tag, lens, kH, kC, kS, mH, mC, mS, ex):
    B, T1, _ = kH.shape
    T = T1 - 1
    assert_calibrated(f"{tag} H", kH, mH, ex["H"])
    assert_calibrated(f"{tag} C", kC, mC, ex["C"])
    if kS is not None:
        assert_calibrated(f"{tag} stash", kS, mS, ex["stash"])
    for b in range(B):
        L = int(lens[b])
        if L < T:
            # frozen rows: every later step bit-identical to the last active
            assert bits_equal(kH[b, L + 1:], kH[b, L:L + 1].expand(T - L, H))
            assert bits_equal(kC[b, L + 1:], kC[b, L:L + 1].expand(T - L, H))
            if kS is not None:
                assert (kS[b, L:] == 0).all(), f"stash row {b} not zero"


# ---------------------------------------------------------------------------
# 1. forward, one and two networks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,kind", CASES)
def test_fwd_one_network(B, T, kind):
    c = case(B, T, kind)
    check_fwd(f"fwd1 B{B} T{T} {kind}", c["lens"], c["kH"], c["kC"], c["kS"],
              c["mH"], c["mC"], c["mS"], c["ex"])


def run_two_networks(B, T, kind, bar=None):
    c = case(B, T, kind)
    # the second net: its own weights, inputs and initial state
    X1, Whh1, h1, c1, _ = make_inputs(B, T, seed=777 + 1000 * B + 10 * T)
    outs = kernel_fwd(c["X"], c["Whh"], c["h0"], c["c0"], c["lens"], bar=bar,
                      second=(X1, Whh1, h1, c1))
    return c, (X1, Whh1, h1, c1), outs


@pytest.mark.parametrize("B,T,kind", CASES2)
def test_fwd_two_networks(B, T, kind):
    c, (X1, Whh1, h1, c1), (H0, C0, H1, C1, S0) = run_two_networks(B, T, kind)
    lens = c["lens"]
    check_fwd(f"fwd2/net0 B{B} T{T}", lens, H0, C0, S0,
              c["mH"], c["mC"], c["mS"], c["ex"])
    ex1 = exact_ref(X1, Whh1, h1, c1, lens)
    mH1, mC1, mS1 = model_fwd(X1, Whh1, h1, c1, lens)
    check_fwd(f"fwd2/net1 B{B} T{T}", lens, H1, C1, None, mH1, mC1, mS1, ex1)


# ---------------------------------------------------------------------------
# 2. backward
# ---------------------------------------------------------------------------

def check_dgates_masked_zero(dg, lens):
    T = dg.shape[1]
    for b in range(dg.shape[0]):
        L = int(lens[b])
        if L < T:
            assert (dg[b, L:] == 0).all(), f"dgates row {b} not zero"


@pytest.mark.parametrize("B,T,kind", CASES)
def test_bwd(B, T, kind):
    c = case(B, T, kind)
    # dHext is non-zero at masked steps: the exact dL/dX carries that
    # gradient through the frozen state to the last active step
    assert_calibrated(f"bwd B{B} T{T} {kind} dgates", c["kdG"], c["mdG"],
                      c["ex"]["dX"])
    check_dgates_masked_zero(c["kdG"], c["lens"])


# ---------------------------------------------------------------------------
# 3. row independence, exact
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bstar", [0, 15, 16, 47, 48, 63])
def test_bwd_row_independence(bstar):
    B, T = 64, 7
    c = case(B, T, "mixed")
    lens = c["lens"]
    dH1 = torch.zeros_like(c["dHext"])
    dH1[bstar] = c["dHext"][bstar]
    dg = kernel_bwd(c["kS"], c["kC"], c["kH"], dH1, c["Whh"], lens)
    others = [b for b in range(B) if b != bstar]
    nz = (dg[others] != 0).flatten(1).any(1)
    assert not nz.any(), \
        f"rows {[others[i] for i in nz.nonzero().flatten().tolist()]} non-zero"
    # rows never interact, so row b* of the full-batch exact gradient is the
    # exact gradient of this loss
    sl = slice(bstar, bstar + 1)
    assert_calibrated(f"rowind b*={bstar} dgates", dg[sl], c["mdG"][sl],
                      c["ex"]["dX"][sl])
    assert bits_equal(dg[bstar], c["kdG"][bstar])


@pytest.mark.parametrize("bstar", [0, 15, 16, 31, 32, 63])
def test_fwd_row_independence(bstar):
    B, T = 64, 7
    c = case(B, T, "mixed")
    X2 = c["X"].clone()
    X2[bstar] = (X2[bstar].float() * -0.75 + 0.25).bfloat16()
    kH, kC, _, _, kS = kernel_fwd(X2, c["Whh"], c["h0"], c["c0"], c["lens"])
    others = [b for b in range(B) if b != bstar]
    for name, a, b in (("H", kH, c["kH"]), ("C", kC, c["kC"]),
                       ("stash", kS, c["kS"])):
        assert bits_equal(a[others], b[others]), f"{name}: neighbour changed"
        assert not bits_equal(a[bstar], b[bstar]), f"{name}: row unchanged"


# ---------------------------------------------------------------------------
# 4. layout invariance: rows 0..15 as a B=16 launch and inside the B=64
# launch.  The forward layouts differ (<64,8> against <32,16> halves); the
# backward is the quartered kernel both times (see the table above), once
# with three empty quarters.  Measured bit-equal in both directions — every
# output element sees the same k order — but only the tolerance is required.
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["full", "mixed"])
def test_layout_invariance(kind):
    T = 7
    c = case(64, T, kind)
    s = slice(0, 16)
    lens = c["lens"][s].contiguous()
    kH, kC, _, _, kS = kernel_fwd(c["X"][s].contiguous(), c["Whh"],
                                  c["h0"][s].contiguous(),
                                  c["c0"][s].contiguous(), lens)
    dg = kernel_bwd(kS, kC, kH, c["dHext"][s].contiguous(), c["Whh"], lens)
    ex = c["ex"]
    for name, small, big, model, exact in (
            ("H", kH, c["kH"][s], c["mH"][s], ex["H"][s]),
            ("C", kC, c["kC"][s], c["mC"][s], ex["C"][s]),
            ("stash", kS, c["kS"][s], c["mS"][s], ex["stash"][s]),
            ("dgates", dg, c["kdG"][s], c["mdG"][s], ex["dX"][s])):
        assert_calibrated(f"layout B16 {kind} {name}", small, model, exact)
        # the two launches differ only in f32 accumulation order, which can
        # move a stored bf16 by the same one rounding the model measures
        diff = ((small.double() - big.double()).abs().max()
                / exact.abs().max()).item()
        em = rel_err(model, exact)
        print(f"LAYOUT {kind} {name}: B16 vs B64 diff {diff:.3e} "
              f"(model {em:.3e}) bit-equal {bits_equal(small, big)}")
        assert diff <= FACTOR * em, (name, diff, em)


# ---------------------------------------------------------------------------
# 5. workspace reuse and determinism
# ---------------------------------------------------------------------------

def test_workspace_reuse_is_deterministic():
    """One barrier workspace through fwd, bwd, fwd, bwd, as the engine does
    with self.bar.  No data atomics and fixed-order K-split sums: the second
    pair is bit-identical.  kernel_fwd/kernel_bwd assert bar[256] == 0 after
    every launch."""
    B, T = 64, 7
    bar = new_bar()
    runs = []
    for _ in range(2):
        c, _, (H0, C0, H1, C1, S0) = run_two_networks(B, T, "mixed", bar=bar)
        dg = kernel_bwd(S0, C0, H0, c["dHext"], c["Whh"], c["lens"], bar=bar)
        runs.append((H0, C0, H1, C1, S0, dg))
    for name, a, b in zip(("H0", "C0", "H1", "C1", "stash", "dgates"), *runs):
        assert bits_equal(a, b), f"{name} differs between the two runs"
    # and the one-network launch of the shared case gave the same net 0
    assert bits_equal(runs[0][0], c["kH"]) and bits_equal(runs[0][5], c["kdG"])


# ---------------------------------------------------------------------------
# 6. weight gradients at the learner's layout
# ---------------------------------------------------------------------------

def wgrad_check(tag, c, B, T):
    """dW_hh, dW_ih, db from the kernel's dgates through gemm_wgrad_into into
    zeroed buffers, as the engine does, against float64 autograd."""
    A = 18
    kin, kpad = 512 + A + 1, 544
    g = torch.Generator(device="cuda").manual_seed(5)
    rin = torch.zeros(B * T, kpad, device="cuda")
    rin[:, :kin] = torch.randn(B * T, kin, device="cuda", generator=g)
    rin = rin.bfloat16()
    e = torch.Tensor()
    dgk = c["kdG"].reshape(B * T, 4 * H)
    hk = c["kH"][:, :T].reshape(B * T, H).contiguous()
    dWhh = torch.zeros(4 * H, H, device="cuda")
    dWih = torch.zeros(4 * H, kin, device="cuda")
    dbih = torch.zeros(4 * H, device="cuda")
    M_.gemm_wgrad_into(dgk, e, hk, False, dWhh, e)
    M_.gemm_wgrad_into(dgk, e, rin, False, dWih, dbih)
    # exact: X enters the gates additively and X = rin @ W_ih^T + b, so
    # dL/dW_ih = (dL/dX)^T @ rin and dL/db = sum (dL/dX) — the products
    # float64 autograd forms for that graph
    dX = c["ex"]["dX"].reshape(B * T, 4 * H)
    r64 = rin.double()[:, :kin]
    mdg = c["mdG"].reshape(B * T, 4 * H)
    mh = c["mH"][:, :T].reshape(B * T, H)
    assert_calibrated(f"{tag} dW_hh", dWhh, mdg.t() @ mh, c["ex"]["dWhh"])
    assert_calibrated(f"{tag} dW_ih", dWih, mdg.t() @ rin.float()[:, :kin],
                      dX.t() @ r64)
    assert_calibrated(f"{tag} db_ih", dbih, mdg.sum(0), dX.sum(0))


@pytest.mark.parametrize("kind", ["full", "mixed", "q3ones"])
def test_weight_grads_learner_layout(kind):
    B, T = 64, 7
    wgrad_check(f"wgrad B{B} T{T} {kind}", case(B, T, kind), B, T)


# ---------------------------------------------------------------------------
# the learner's own shape: B = 64, T = 85, two networks.  Rounding drift
# grows with T and the handoff counters reach 32 * 85 only here.
# ---------------------------------------------------------------------------

def test_learner_shape_two_networks():
    B, T = 64, 85
    X, Whh, h0, c0, dHext = make_inputs(B, T, seed=85, scale=0.5)
    X1, Whh1, h1, c1, _ = make_inputs(B, T, seed=86, scale=0.5)
    # burn-in 40 + learning 1..40 + forward 5, and a few short rows
    l = [40 + 1 + (b * 7) % 40 + 4 for b in range(B)]
    l[0], l[17], l[40], l[63] = T, 1, T - 1, 2
    lens = torch.tensor(l, dtype=torch.int32, device="cuda")
    bar = new_bar()
    H0, C0, H1, C1, S0 = kernel_fwd(X, Whh, h0, c0, lens, bar=bar,
                                    second=(X1, Whh1, h1, c1))
    dg = kernel_bwd(S0, C0, H0, dHext, Whh, lens, bar=bar)
    ex = exact_ref(X, Whh, h0, c0, lens, dHext)
    mH, mC, mS = model_fwd(X, Whh, h0, c0, lens)
    mdG = model_bwd(mS, mC, dHext, Whh, lens)
    check_fwd("learner net0", lens, H0, C0, S0, mH, mC, mS, ex)
    ex1 = exact_ref(X1, Whh1, h1, c1, lens)
    check_fwd("learner net1", lens, H1, C1, None,
              *model_fwd(X1, Whh1, h1, c1, lens), ex1)
    assert_calibrated("learner dgates", dg, mdG, ex["dX"])
    check_dgates_masked_zero(dg, lens)
    wgrad_check("learner", dict(kdG=dg, kH=H0, mdG=mdG, mH=mH, ex=ex), B, T)


# ---------------------------------------------------------------------------
# host checks: one bad operand each, RuntimeError before anything launches
# ---------------------------------------------------------------------------

def good_bwd_args(B=4, T=3):
    d = "cuda"
    return dict(
        stash=torch.zeros(B, T, 4 * H, device=d).bfloat16(),
        Cout=torch.zeros(B, T + 1, H, device=d),
        Hout=torch.zeros(B, T + 1, H, device=d).bfloat16(),
        dHext=torch.zeros(B, T, H, device=d),
        Whh_bwd=torch.zeros(H, 4 * H, device=d).bfloat16(),
        lens=torch.full((B,), T, dtype=torch.int32, device=d))


BWD_ORDER = ("stash", "Cout", "Hout", "dHext", "Whh_bwd", "lens")


def bad_bwd_operands():
    B, T = 4, 3
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    return {
        "B65": lambda a: {k: good_bwd_args(65, T)[k] for k in a},
        "H4_not_2048": lambda a: dict(a, stash=z(B, T, 1024).bfloat16()),
        "stash_f32": lambda a: dict(a, stash=a["stash"].float()),
        "stash_cpu": lambda a: dict(a, stash=a["stash"].cpu()),
        "stash_strided": lambda a: dict(
            a, stash=z(B, T, 8 * H).bfloat16()[:, :, ::2]),
        "Hout_f32": lambda a: dict(a, Hout=a["Hout"].float()),
        "Hout_strided": lambda a: dict(
            a, Hout=z(B, T + 1, 2 * H).bfloat16()[:, :, ::2]),
        "Hout_shape": lambda a: dict(a, Hout=z(B, T, H).bfloat16()),
        "Whh_f32": lambda a: dict(a, Whh_bwd=a["Whh_bwd"].float()),
        "Whh_cpu": lambda a: dict(a, Whh_bwd=a["Whh_bwd"].cpu()),
        "Whh_transposed": lambda a: dict(
            a, Whh_bwd=z(4 * H, H).bfloat16()),
        "Whh_strided": lambda a: dict(a, Whh_bwd=z(4 * H, H).bfloat16().t()),
        "Cout_bf16": lambda a: dict(a, Cout=a["Cout"].bfloat16()),
        "Cout_shape_T": lambda a: dict(a, Cout=z(B, T, H)),
        "Cout_strided": lambda a: dict(a, Cout=z(B, T + 1, 2 * H)[:, :, ::2]),
        "dHext_bf16": lambda a: dict(a, dHext=a["dHext"].bfloat16()),
        "dHext_shape_T1": lambda a: dict(a, dHext=z(B, T + 1, H)),
        "dHext_strided": lambda a: dict(a, dHext=z(B, T, 2 * H)[:, :, ::2]),
        "lens_int64": lambda a: dict(a, lens=a["lens"].long()),
        "lens_short": lambda a: dict(a, lens=a["lens"][:B - 1].contiguous()),
    }


BAD_BWD = ["B65", "H4_not_2048", "stash_f32", "stash_cpu", "stash_strided",
           "Hout_f32", "Hout_strided", "Hout_shape", "Whh_f32", "Whh_cpu",
           "Whh_transposed", "Whh_strided", "Cout_bf16", "Cout_shape_T",
           "Cout_strided", "dHext_bf16", "dHext_shape_T1", "dHext_strided",
           "lens_int64", "lens_short"]


class _Sentinel:
    """A workspace pre-filled with a pattern: a wrapper that raises before
    launching never runs the reset kernel, so the pattern survives."""

    def __init__(self):
        self.bar = torch.full((512,), 0x5A5A, dtype=torch.int32,
                              device="cuda")

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.bar == 0x5A5A).all())


@pytest.mark.parametrize("which", BAD_BWD)
def test_lstm_bwd_rejects_bad_operand(which):
    args = bad_bwd_operands()[which](good_bwd_args())
    s = _Sentinel()
    with pytest.raises(RuntimeError):
        M_.lstm_bwd(*[args[k] for k in BWD_ORDER], s.bar)
    assert s.untouched(), "lstm_bwd touched the workspace before raising"


def test_lstm_bwd_accepts_good_operands():
    """The operands the rejection tests start from are themselves valid."""
    bar = new_bar()
    dg = M_.lstm_bwd(*[good_bwd_args()[k] for k in BWD_ORDER], bar)
    assert poison(bar) == 0 and (dg == 0).all()


def good_fwd_args(B=4, T=3, two=True):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    e = torch.Tensor()
    return dict(
        X0=z(B, T, 4 * H).bfloat16(),
        X1=z(B, T, 4 * H).bfloat16() if two else e,
        Whh0=z(4 * H, H).bfloat16(),
        Whh1=z(4 * H, H).bfloat16() if two else e,
        init0=z(2, B, H), init1=z(2, B, H) if two else e,
        lens=torch.full((B,), T, dtype=torch.int32, device="cuda"))


FWD_ORDER = ("X0", "X1", "Whh0", "Whh1", "init0", "init1", "lens")


def bad_fwd_operands():
    B, T = 4, 3
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    return {
        "B65": lambda a: good_fwd_args(65, T),
        "H4_not_2048": lambda a: dict(a, X0=z(B, T, 1024).bfloat16(),
                                      X1=z(B, T, 1024).bfloat16()),
        "Whh0_shape": lambda a: dict(a, Whh0=z(H, 4 * H).bfloat16()),
        "Whh0_f32": lambda a: dict(a, Whh0=a["Whh0"].float()),
        "Whh0_strided": lambda a: dict(a, Whh0=z(H, 4 * H).bfloat16().t()),
        "Whh1_shape": lambda a: dict(a, Whh1=z(H, 4 * H).bfloat16()),
        "init0_shape": lambda a: dict(a, init0=z(2, B + 1, H)),
        "init0_bf16": lambda a: dict(a, init0=a["init0"].bfloat16()),
        "init1_shape": lambda a: dict(a, init1=z(1, B, H)),
        "lens_int64": lambda a: dict(a, lens=a["lens"].long()),
        "lens_short": lambda a: dict(a, lens=a["lens"][:B - 1].contiguous()),
        "X1_T_differs": lambda a: dict(a, X1=z(B, T + 1, 4 * H).bfloat16()),
        "X1_B_differs": lambda a: dict(a, X1=z(B - 1, T, 4 * H).bfloat16()),
        "X1_f32": lambda a: dict(a, X1=a["X1"].float()),
    }


BAD_FWD = ["B65", "H4_not_2048", "Whh0_shape", "Whh0_f32", "Whh0_strided",
           "Whh1_shape", "init0_shape", "init0_bf16", "init1_shape",
           "lens_int64", "lens_short", "X1_T_differs", "X1_B_differs",
           "X1_f32"]


@pytest.mark.parametrize("which", BAD_FWD)
def test_lstm_fwd_rejects_bad_operand(which):
    args = bad_fwd_operands()[which](good_fwd_args())
    s = _Sentinel()
    with pytest.raises(RuntimeError):
        M_.lstm_fwd(*[args[k] for k in FWD_ORDER], s.bar, True)
    assert s.untouched(), "lstm_fwd touched the workspace before raising"


def test_lstm_fwd_accepts_good_operands():
    for two in (True, False):
        bar = new_bar()
        outs = M_.lstm_fwd(*[good_fwd_args(two=two)[k] for k in FWD_ORDER],
                           bar, True)
        assert poison(bar) == 0 and (outs[0] == 0).all()
