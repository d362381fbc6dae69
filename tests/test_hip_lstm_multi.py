"""GPU numerics: the multi-pass persistent LSTM (lstm_fwd_multi /
lstm_bwd_multi), batches of 65 .. 256 rows in one launch.

The batch is cut into passes of P rows (the `rows` argument of the bindings,
64 or 128); every pass runs the forward as <512, 32, 16> row groups and the
backward as <512, 16, 16> quarters, the layouts a 64-row launch uses.  The
whole file runs once per value in ROWS.

Method and tolerance are those of test_hip_lstm_layouts (its helpers are
imported, not copied): errors are max|x - exact| / max|exact| against a
float64 recurrence and float64 autograd, the yardstick is a float32 torch
model that rounds to bf16 where the kernels store bf16, and the kernel must
stay within 4x of the model's error.  On top of that every full 64-row chunk
must be BIT-equal to lstm_fwd / lstm_bwd run on those rows alone: that is
what catches a wrong counter offset, state carried across passes or a wrong
`init` stride.
"""

import functools

import pytest
import torch

from test_hip_lstm_layouts import (
    H, _Sentinel, assert_calibrated, bits_equal, check_dgates_masked_zero,
    check_fwd, exact_ref, make_inputs, model_bwd, model_fwd, new_bar, poison)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

# pass sizes the extension ships
ROWS = [64, 128]

per_pass_size = pytest.mark.parametrize("rows", ROWS,
                                        ids=[f"P{r}" for r in ROWS])

BS = [65, 96, 97, 128, 129, 192, 256]
TS = [1, 2, 7]
KINDS = ["full", "ones", "mixed", "pass0ones", "quarter1ones"]


def make_lens(B, T, kind, rows):
    if kind == "full":
        l = [T] * B
    elif kind == "ones":
        l = [1] * B
    else:
        cyc = [1, max(1, T - 1), T, max(1, (T + 1) // 2)]
        l = [cyc[b % 4] for b in range(B)]
        l[B - 1] = T
        if kind == "pass0ones":          # the whole first pass
            n = min(rows, B)
            l[:n] = [1] * n
        elif kind == "quarter1ones":
            # the second 16-row quarter of the second pass; where the second
            # pass is shorter than that (or, at P = 128, absent), the same
            # quarter of the second 64-row chunk, or its first row
            s = rows + 16 if B > rows + 16 else (80 if B > 80 else 64)
            e = min(s + 16, B)
            l[s:e] = [1] * (e - s)
            l[0] = T
        else:
            assert kind == "mixed", kind
    return torch.tensor(l, dtype=torch.int32, device="cuda")


def case_list():
    out = []
    for rows in ROWS:
        for B in BS:
            for T in TS:
                for k in (["full"] if T == 1 else KINDS):
                    out.append(pytest.param(
                        B, T, k, rows, id=f"P{rows}-B{B}-T{T}-{k}"))
    return out


CASES = case_list()
CASES2 = [pytest.param(B, T, "full" if T == 1 else "mixed", rows,
                       id=f"P{rows}-B{B}-T{T}")
          for rows in ROWS for B in BS for T in TS]


# ---------------------------------------------------------------------------
# kernel runners
# ---------------------------------------------------------------------------

def multi_fwd(X, Whh, h0, c0, lens, rows, bar=None, second=None):
    bar = new_bar() if bar is None else bar
    init = torch.stack([h0, c0]).contiguous()
    e = torch.Tensor()
    if second is None:
        outs = M_.lstm_fwd_multi(X, e, Whh, e, init, e, lens, bar, True, rows)
    else:
        X1, Whh1, h1, c1 = second
        outs = M_.lstm_fwd_multi(X, X1, Whh, Whh1, init,
                                 torch.stack([h1, c1]).contiguous(), lens,
                                 bar, True, rows)
    assert poison(bar) == 0, "lstm_fwd_multi tripped the poison word"
    return outs


def multi_bwd(stash, C, Hk, dHext, Whh, lens, rows, bar=None):
    bar = new_bar() if bar is None else bar
    dg = M_.lstm_bwd_multi(stash, C, Hk, dHext.contiguous(),
                           Whh.t().contiguous(), lens, bar, rows)
    assert poison(bar) == 0, "lstm_bwd_multi tripped the poison word"
    return dg


def single_fwd(X, Whh, h0, c0, lens, second=None, bar=None):
    """lstm_fwd (the 64-row entry) on contiguous copies of a row slice."""
    bar = new_bar() if bar is None else bar
    e = torch.Tensor()
    init = torch.stack([h0, c0]).contiguous()
    if second is None:
        outs = M_.lstm_fwd(X.contiguous(), e, Whh, e, init, e,
                           lens.contiguous(), bar, True)
    else:
        X1, Whh1, h1, c1 = second
        outs = M_.lstm_fwd(X.contiguous(), X1.contiguous(), Whh, Whh1, init,
                           torch.stack([h1, c1]).contiguous(),
                           lens.contiguous(), bar, True)
    assert poison(bar) == 0
    return outs


@functools.lru_cache(maxsize=None)
def reference(B, T, kind, rows_for_mask):
    """Inputs and the two references for one (B, T, mask).  Computed once,
    shared, never modified.  The mask kinds that name a pass depend on P."""
    X, Whh, h0, c0, dHext = make_inputs(B, T, seed=1000 * B + 10 * T)
    lens = make_lens(B, T, kind, rows_for_mask)
    ex = exact_ref(X, Whh, h0, c0, lens, dHext)
    mH, mC, mS = model_fwd(X, Whh, h0, c0, lens)
    mdG = model_bwd(mS, mC, dHext, Whh, lens)
    return dict(X=X, Whh=Whh, h0=h0, c0=c0, dHext=dHext, lens=lens, ex=ex,
                mH=mH, mC=mC, mS=mS, mdG=mdG)


def ref_for(B, T, kind, rows):
    # masks that do not name a pass are the same for every P
    return reference(B, T, kind,
                     rows if kind in ("pass0ones", "quarter1ones") else 0)


@functools.lru_cache(maxsize=None)
def case(B, T, kind, rows):
    c = dict(ref_for(B, T, kind, rows))
    kH, kC, _, _, kS = multi_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                 c["lens"], rows)
    kdG = multi_bwd(kS, kC, kH, c["dHext"], c["Whh"], c["lens"], rows)
    torch.cuda.synchronize()
    c.update(kH=kH, kC=kC, kS=kS, kdG=kdG)
    return c


# ---------------------------------------------------------------------------
# 1. numerics
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,kind,rows", CASES)
def test_fwd_one_network(B, T, kind, rows):
    c = case(B, T, kind, rows)
    # check_fwd also asserts that masked steps carry h and c through bit for
    # bit and stash zeros
    check_fwd(f"multi fwd1 P{rows} B{B} T{T} {kind}", c["lens"], c["kH"],
              c["kC"], c["kS"], c["mH"], c["mC"], c["mS"], c["ex"])


def second_net(B, T):
    X1, Whh1, h1, c1, _ = make_inputs(B, T, seed=777 + 1000 * B + 10 * T)
    return X1, Whh1, h1, c1


@pytest.mark.parametrize("B,T,kind,rows", CASES2)
def test_fwd_two_networks(B, T, kind, rows):
    c = case(B, T, kind, rows)
    X1, Whh1, h1, c1 = second_net(B, T)
    H0, C0, H1, C1, S0 = multi_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                   c["lens"], rows,
                                   second=(X1, Whh1, h1, c1))
    lens = c["lens"]
    # the first network does not depend on the presence of the second
    for name, a, b in (("H", H0, c["kH"]), ("C", C0, c["kC"]),
                       ("stash", S0, c["kS"])):
        assert bits_equal(a, b), f"net0 {name} differs from the 1-net launch"
    ex1 = exact_ref(X1, Whh1, h1, c1, lens)
    mH1, mC1, mS1 = model_fwd(X1, Whh1, h1, c1, lens)
    check_fwd(f"multi fwd2/net1 P{rows} B{B} T{T}", lens, H1, C1, None,
              mH1, mC1, mS1, ex1)


@pytest.mark.parametrize("B,T,kind,rows", CASES)
def test_bwd(B, T, kind, rows):
    c = case(B, T, kind, rows)
    assert_calibrated(f"multi bwd P{rows} B{B} T{T} {kind} dgates", c["kdG"],
                      c["mdG"], c["ex"]["dX"])
    check_dgates_masked_zero(c["kdG"], c["lens"])


# ---------------------------------------------------------------------------
# 2. every full 64-row chunk is bit-equal to the 64-row kernels
# ---------------------------------------------------------------------------

@per_pass_size
@pytest.mark.parametrize("B", [64, 128, 192])
def test_chunks_bit_equal_to_single_pass_kernels(B, rows):
    T = 7
    c = ref_for(B, T, "mixed", rows)
    X1, Whh1, h1, c1 = second_net(B, T)
    H0, C0, H1, C1, S0 = multi_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                   c["lens"], rows,
                                   second=(X1, Whh1, h1, c1))
    dg = multi_bwd(S0, C0, H0, c["dHext"], c["Whh"], c["lens"], rows)
    for lo in range(0, B, 64):
        s = slice(lo, lo + 64)
        lens = c["lens"][s]
        h0_, c0_, h1_, c1_, s0_ = single_fwd(
            c["X"][s], c["Whh"], c["h0"][s], c["c0"][s], lens,
            second=(X1[s], Whh1, h1[s], c1[s]))
        bar = new_bar()
        dg_ = M_.lstm_bwd(s0_, c0_, h0_, c["dHext"][s].contiguous(),
                          c["Whh"].t().contiguous(), lens.contiguous(), bar)
        assert poison(bar) == 0
        for name, a, b in (("H0", H0[s], h0_), ("C0", C0[s], c0_),
                           ("H1", H1[s], h1_), ("C1", C1[s], c1_),
                           ("stash", S0[s], s0_), ("dgates", dg[s], dg_)):
            assert bits_equal(a, b), f"rows {lo}..{lo + 63}: {name} differs"


# ---------------------------------------------------------------------------
# 3. isolation across passes and row groups, exact
# ---------------------------------------------------------------------------

EDGE_ROWS = [0, 63, 64, 79, 80, 127, 128]
ISO_B, ISO_T = 129, 7


@per_pass_size
@pytest.mark.parametrize("bstar", EDGE_ROWS)
def test_bwd_row_isolation(bstar, rows):
    c = case(ISO_B, ISO_T, "mixed", rows)
    dH1 = torch.zeros_like(c["dHext"])
    dH1[bstar] = c["dHext"][bstar]
    dg = multi_bwd(c["kS"], c["kC"], c["kH"], dH1, c["Whh"], c["lens"], rows)
    others = [b for b in range(ISO_B) if b != bstar]
    nz = (dg[others] != 0).flatten(1).any(1)
    assert not nz.any(), \
        f"rows {[others[i] for i in nz.nonzero().flatten().tolist()]} non-zero"
    assert bits_equal(dg[bstar], c["kdG"][bstar])
    assert (dg[bstar] != 0).any()


@per_pass_size
@pytest.mark.parametrize("bstar", EDGE_ROWS)
def test_fwd_row_isolation(bstar, rows):
    c = case(ISO_B, ISO_T, "mixed", rows)
    X2 = c["X"].clone()
    X2[bstar] = (X2[bstar].float() * -0.75 + 0.25).bfloat16()
    kH, kC, _, _, kS = multi_fwd(X2, c["Whh"], c["h0"], c["c0"], c["lens"],
                                 rows)
    others = [b for b in range(ISO_B) if b != bstar]
    for name, a, b in (("H", kH, c["kH"]), ("C", kC, c["kC"]),
                       ("stash", kS, c["kS"])):
        assert bits_equal(a[others], b[others]), f"{name}: another row changed"
        assert not bits_equal(a[bstar], b[bstar]), f"{name}: row unchanged"


# ---------------------------------------------------------------------------
# 4. workspace
# ---------------------------------------------------------------------------

@per_pass_size
def test_workspace_reuse_is_deterministic(rows):
    """One workspace through fwd, bwd, fwd, bwd, as the engine uses self.bar;
    multi_fwd / multi_bwd assert bar[256] == 0 after every launch."""
    B, T = 129, 7
    c = case(B, T, "mixed", rows)
    sec = second_net(B, T)
    bar = new_bar()
    runs = []
    for _ in range(2):
        H0, C0, H1, C1, S0 = multi_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                       c["lens"], rows, bar=bar, second=sec)
        dg = multi_bwd(S0, C0, H0, c["dHext"], c["Whh"], c["lens"], rows,
                       bar=bar)
        runs.append((H0, C0, H1, C1, S0, dg))
    for name, a, b in zip(("H0", "C0", "H1", "C1", "stash", "dgates"), *runs):
        assert bits_equal(a, b), f"{name} differs between the two runs"
    assert bits_equal(runs[0][0], c["kH"]) and bits_equal(runs[0][5], c["kdG"])


@per_pass_size
def test_single_pass_launch_after_multi_on_one_workspace(rows):
    """The multi launch leaves its counters far above anything a 64-row launch
    counts to; lstm_fwd / lstm_bwd reset the workspace themselves."""
    B, T = 129, 7
    c = case(B, T, "mixed", rows)
    s = slice(0, 64)
    args = (c["X"][s], c["Whh"], c["h0"][s], c["c0"][s], c["lens"][s])
    fresh = single_fwd(*args)
    bar = new_bar()
    kH, kC, _, _, kS = multi_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                 c["lens"], rows, bar=bar)
    multi_bwd(kS, kC, kH, c["dHext"], c["Whh"], c["lens"], rows, bar=bar)
    used = single_fwd(*args, bar=bar)
    for name, a, b in zip(("H", "C"), fresh[:2], used[:2]):
        assert bits_equal(a, b), name
    assert bits_equal(fresh[4], used[4]), "stash"


# ---------------------------------------------------------------------------
# 5. the learner's shape at B = 128: T = 85, two networks
# ---------------------------------------------------------------------------

@per_pass_size
def test_learner_shape_two_networks(rows):
    B, T = 128, 85
    r = learner_reference()
    lens = r["lens"]
    bar = new_bar()
    H0, C0, H1, C1, S0 = multi_fwd(r["X"], r["Whh"], r["h0"], r["c0"], lens,
                                   rows, bar=bar, second=r["second"])
    dg = multi_bwd(S0, C0, H0, r["dHext"], r["Whh"], lens, rows, bar=bar)
    check_fwd(f"multi learner P{rows} net0", lens, H0, C0, S0, r["mH"],
              r["mC"], r["mS"], r["ex"])
    check_fwd(f"multi learner P{rows} net1", lens, H1, C1, None, *r["m1"],
              r["ex1"])
    assert_calibrated(f"multi learner P{rows} dgates", dg, r["mdG"],
                      r["ex"]["dX"])
    check_dgates_masked_zero(dg, lens)


@functools.lru_cache(maxsize=None)
def learner_reference():
    B, T = 128, 85
    X, Whh, h0, c0, dHext = make_inputs(B, T, seed=185, scale=0.5)
    X1, Whh1, h1, c1, _ = make_inputs(B, T, seed=186, scale=0.5)
    # burn-in 40 + learning 1..40 + forward 5, and a few short rows
    l = [40 + 1 + (b * 7) % 40 + 4 for b in range(B)]
    l[0], l[17], l[63], l[64], l[100], l[127] = T, 1, 2, T - 1, 1, T
    lens = torch.tensor(l, dtype=torch.int32, device="cuda")
    ex = exact_ref(X, Whh, h0, c0, lens, dHext)
    mH, mC, mS = model_fwd(X, Whh, h0, c0, lens)
    return dict(X=X, Whh=Whh, h0=h0, c0=c0, dHext=dHext, lens=lens, ex=ex,
                mH=mH, mC=mC, mS=mS,
                mdG=model_bwd(mS, mC, dHext, Whh, lens),
                second=(X1, Whh1, h1, c1),
                ex1=exact_ref(X1, Whh1, h1, c1, lens),
                m1=model_fwd(X1, Whh1, h1, c1, lens))


# ---------------------------------------------------------------------------
# 6. host checks: one bad operand each, RuntimeError before anything launches
# ---------------------------------------------------------------------------

def z(*s, **k):
    return torch.zeros(*s, device="cuda", **k)


def good_fwd_args(B=70, T=3):
    return dict(X0=z(B, T, 4 * H).bfloat16(), X1=z(B, T, 4 * H).bfloat16(),
                Whh0=z(4 * H, H).bfloat16(), Whh1=z(4 * H, H).bfloat16(),
                init0=z(2, B, H), init1=z(2, B, H),
                lens=torch.full((B,), T, dtype=torch.int32, device="cuda"))


FWD_ORDER = ("X0", "X1", "Whh0", "Whh1", "init0", "init1", "lens")


def bad_fwd_operands(B=70, T=3):
    return {
        "B257": lambda a: good_fwd_args(257, T),
        "B0": lambda a: good_fwd_args(0, T),
        "H4_not_2048": lambda a: dict(a, X0=z(B, T, 1024).bfloat16(),
                                      X1=z(B, T, 1024).bfloat16()),
        "X0_f32": lambda a: dict(a, X0=a["X0"].float()),
        "X0_2d": lambda a: dict(a, X0=z(B * T, 4 * H).bfloat16()),
        "X0_strided": lambda a: dict(
            a, X0=z(B, 2 * T, 4 * H).bfloat16()[:, ::2]),
        "X0_cpu": lambda a: dict(a, X0=a["X0"].cpu()),
        "X1_f32": lambda a: dict(a, X1=a["X1"].float()),
        "X1_T_differs": lambda a: dict(a, X1=z(B, T + 1, 4 * H).bfloat16()),
        "X1_B_differs": lambda a: dict(a, X1=z(B - 1, T, 4 * H).bfloat16()),
        "X1_strided": lambda a: dict(
            a, X1=z(B, 2 * T, 4 * H).bfloat16()[:, ::2]),
        "Whh0_f32": lambda a: dict(a, Whh0=a["Whh0"].float()),
        "Whh0_shape": lambda a: dict(a, Whh0=z(H, 4 * H).bfloat16()),
        "Whh0_strided": lambda a: dict(a, Whh0=z(H, 4 * H).bfloat16().t()),
        "Whh1_f32": lambda a: dict(a, Whh1=a["Whh1"].float()),
        "Whh1_shape": lambda a: dict(a, Whh1=z(H, 4 * H).bfloat16()),
        "Whh1_strided": lambda a: dict(a, Whh1=z(H, 4 * H).bfloat16().t()),
        "init0_bf16": lambda a: dict(a, init0=a["init0"].bfloat16()),
        "init0_shape": lambda a: dict(a, init0=z(2, B + 1, H)),
        "init0_strided": lambda a: dict(a, init0=z(2, B, 2 * H)[:, :, ::2]),
        "init1_bf16": lambda a: dict(a, init1=a["init1"].bfloat16()),
        "init1_shape": lambda a: dict(a, init1=z(1, B, H)),
        "init1_strided": lambda a: dict(a, init1=z(2, B, 2 * H)[:, :, ::2]),
        "lens_int64": lambda a: dict(a, lens=a["lens"].long()),
        "lens_short": lambda a: dict(a, lens=a["lens"][:B - 1].contiguous()),
        "lens_strided": lambda a: dict(
            a, lens=z(2 * B, dtype=torch.int32)[::2]),
    }


BAD_FWD = list(bad_fwd_operands())


@per_pass_size
@pytest.mark.parametrize("which", BAD_FWD)
def test_fwd_multi_rejects_bad_operand(which, rows):
    args = bad_fwd_operands()[which](good_fwd_args())
    s = _Sentinel()
    with pytest.raises(RuntimeError):
        M_.lstm_fwd_multi(*[args[k] for k in FWD_ORDER], s.bar, True, rows)
    assert s.untouched(), "lstm_fwd_multi touched the workspace before raising"


def good_bwd_args(B=70, T=3):
    return dict(stash=z(B, T, 4 * H).bfloat16(), Cout=z(B, T + 1, H),
                Hout=z(B, T + 1, H).bfloat16(), dHext=z(B, T, H),
                Whh_bwd=z(H, 4 * H).bfloat16(),
                lens=torch.full((B,), T, dtype=torch.int32, device="cuda"))


BWD_ORDER = ("stash", "Cout", "Hout", "dHext", "Whh_bwd", "lens")


def bad_bwd_operands(B=70, T=3):
    return {
        "B257": lambda a: good_bwd_args(257, T),
        "B0": lambda a: good_bwd_args(0, T),
        "H4_not_2048": lambda a: dict(a, stash=z(B, T, 1024).bfloat16()),
        "stash_f32": lambda a: dict(a, stash=a["stash"].float()),
        "stash_cpu": lambda a: dict(a, stash=a["stash"].cpu()),
        "stash_2d": lambda a: dict(a, stash=z(B * T, 4 * H).bfloat16()),
        "stash_strided": lambda a: dict(
            a, stash=z(B, T, 8 * H).bfloat16()[:, :, ::2]),
        "Cout_bf16": lambda a: dict(a, Cout=a["Cout"].bfloat16()),
        "Cout_shape_T": lambda a: dict(a, Cout=z(B, T, H)),
        "Cout_strided": lambda a: dict(a, Cout=z(B, T + 1, 2 * H)[:, :, ::2]),
        "Hout_f32": lambda a: dict(a, Hout=a["Hout"].float()),
        "Hout_shape": lambda a: dict(a, Hout=z(B, T, H).bfloat16()),
        "Hout_strided": lambda a: dict(
            a, Hout=z(B, T + 1, 2 * H).bfloat16()[:, :, ::2]),
        "dHext_bf16": lambda a: dict(a, dHext=a["dHext"].bfloat16()),
        "dHext_shape_T1": lambda a: dict(a, dHext=z(B, T + 1, H)),
        "dHext_strided": lambda a: dict(a, dHext=z(B, T, 2 * H)[:, :, ::2]),
        "Whh_f32": lambda a: dict(a, Whh_bwd=a["Whh_bwd"].float()),
        "Whh_transposed": lambda a: dict(a, Whh_bwd=z(4 * H, H).bfloat16()),
        "Whh_strided": lambda a: dict(a, Whh_bwd=z(4 * H, H).bfloat16().t()),
        "lens_int64": lambda a: dict(a, lens=a["lens"].long()),
        "lens_short": lambda a: dict(a, lens=a["lens"][:B - 1].contiguous()),
        "lens_strided": lambda a: dict(
            a, lens=z(2 * B, dtype=torch.int32)[::2]),
    }


BAD_BWD = list(bad_bwd_operands())


@per_pass_size
@pytest.mark.parametrize("which", BAD_BWD)
def test_bwd_multi_rejects_bad_operand(which, rows):
    args = bad_bwd_operands()[which](good_bwd_args())
    s = _Sentinel()
    with pytest.raises(RuntimeError):
        M_.lstm_bwd_multi(*[args[k] for k in BWD_ORDER], s.bar, rows)
    assert s.untouched(), "lstm_bwd_multi touched the workspace before raising"


def test_rejects_bad_pass_size_and_workspace():
    f, b = good_fwd_args(), good_bwd_args()
    s = _Sentinel()
    for rows in (32, 96, 256, -1):
        with pytest.raises(RuntimeError):
            M_.lstm_fwd_multi(*[f[k] for k in FWD_ORDER], s.bar, True, rows)
        with pytest.raises(RuntimeError):
            M_.lstm_bwd_multi(*[b[k] for k in BWD_ORDER], s.bar, rows)
    assert s.untouched()
    small = torch.full((256,), 0x5A5A, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        M_.lstm_fwd_multi(*[f[k] for k in FWD_ORDER], small, True, 64)
    with pytest.raises(RuntimeError):
        M_.lstm_bwd_multi(*[b[k] for k in BWD_ORDER], small, 64)
    torch.cuda.synchronize()
    assert bool((small == 0x5A5A).all())


@pytest.mark.parametrize("rows", ROWS + [0],
                         ids=[f"P{r}" for r in ROWS] + ["default"])
def test_accepts_good_operands(rows):
    """The operands the rejection tests start from are themselves valid;
    rows = 0 takes the shipped default."""
    bar = new_bar()
    outs = M_.lstm_fwd_multi(*[good_fwd_args()[k] for k in FWD_ORDER], bar,
                             True, rows)
    assert poison(bar) == 0 and (outs[0] == 0).all() and (outs[2] == 0).all()
    dg = M_.lstm_bwd_multi(*[good_bwd_args()[k] for k in BWD_ORDER], bar, rows)
    assert poison(bar) == 0 and (dg == 0).all()
