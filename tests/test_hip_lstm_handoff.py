"""GPU: what the write-through handoff and the hoisted loads of the persistent
LSTM can break — stale or unpublished bytes, and misplaced prefetches.

The accuracy gate stays test_hip_lstm_layouts.py / test_hip_lstm_multi.py;
this file reuses their helpers and their 4x rounding-model bound unchanged.

The wrappers allocate their outputs themselves (torch::empty), so the tests
that need to own the outputs' memory route those allocations into a private
torch.cuda.MemPool: inside `use_mem_pool` nothing but the wrapper's own
torch::empty calls allocates, so the pool holds exactly the outputs' blocks.
  * Reuse: after every launch the outputs are released into the pool and
    every free block of the pool is filled with NaN, so every later launch
    writes into memory that held NaN (asserted: each output's address range
    lies inside a range that was filled).
  * Guard: dgates is made to land on a released block that lies between two
    live guard blocks (asserted by address); the guards must come back
    unchanged.
Inputs "ending where their storage ends" are exact-size allocations; a read
past them cannot fault inside an allocator segment, so what the tight case
can show is that no value read past T or Bl is ever consumed.

Every launch in this file is followed by a check that the poison word is 0.
"""

import pytest
import torch

import test_hip_lstm_layouts as L
import test_hip_lstm_multi as MU

pytestmark = pytest.mark.gpu

H = L.H
NAMES = ("H0", "C0", "H1", "C1", "stash", "dgates")


def launch_pair(ins, lens, bar):
    """Two-network forward + backward of net 0: the six outputs."""
    (X, Whh, h0, c0, dHext), (X1, Whh1, h1, c1, _) = ins
    H0, C0, H1, C1, S0 = L.kernel_fwd(X, Whh, h0, c0, lens, bar=bar,
                                      second=(X1, Whh1, h1, c1))
    dg = L.kernel_bwd(S0, C0, H0, dHext, Whh, lens, bar=bar)
    return [H0, C0, H1, C1, S0, dg]


def seeded(B, T, k):
    return (L.make_inputs(B, T, seed=31 * k + B + T),
            L.make_inputs(B, T, seed=31 * k + B + T + 5000))


# ---------------------------------------------------------------------------
# 1. one set of output blocks and one workspace over 8 launches
# ---------------------------------------------------------------------------

def prepared(ins):
    """Everything a raw launch needs, allocated OUTSIDE the private pool."""
    (X, Whh, h0, c0, dHext), (X1, Whh1, h1, c1, _) = ins
    return dict(X=X, X1=X1, Whh=Whh, Whh1=Whh1,
                i0=torch.stack([h0, c0]).contiguous(),
                i1=torch.stack([h1, c1]).contiguous(),
                whh_t=Whh.t().contiguous(), dH=dHext.contiguous())


def raw_pair(p, lens, bar, pool):
    """launch_pair with the wrappers' allocations — the six outputs and
    nothing else — routed into `pool`."""
    with torch.cuda.use_mem_pool(pool):
        H0, C0, H1, C1, S0 = L.M_.lstm_fwd(
            p["X"], p["X1"], p["Whh"], p["Whh1"], p["i0"], p["i1"], lens,
            bar, True)
        dg = L.M_.lstm_bwd(S0, C0, H0, p["dH"], p["whh_t"], lens, bar)
    assert L.poison(bar) == 0
    return [H0, C0, H1, C1, S0, dg]


def poison_free_blocks(pool):
    """Fill every free block of `pool` with NaN: for each one in the pool's
    snapshot, allocate tensors that tile it exactly (an exact-size request is
    the best fit for its block; blocks of the 2 MiB small-allocation
    segments are tiled in pieces of at most 1 MiB so that the requests stay
    in that size class), fill them, release them.  Returns the [start, end)
    ranges actually filled."""
    held = []
    with torch.cuda.use_mem_pool(pool):
        for seg in pool.snapshot():
            small = seg["segment_type"] == "small"
            for blk in seg["blocks"]:
                if blk["state"] != "inactive":
                    continue
                left = blk["size"]
                while left > 0:
                    n = min(left, 1 << 20) if small else left
                    held.append(torch.empty(n, dtype=torch.uint8,
                                            device="cuda"))
                    left -= n
    ranges = []
    for t in held:
        t.view(torch.float32).fill_(float("nan"))
        ranges.append((t.data_ptr(), t.data_ptr() + t.numel()))
    del held, t
    merged = []                      # adjacent pieces form one range
    for r0, r1 in sorted(ranges):
        if merged and merged[-1][1] == r0:
            merged[-1] = (merged[-1][0], r1)
        else:
            merged.append((r0, r1))
    return merged


@pytest.mark.parametrize("T", [2, 7, 40])
@pytest.mark.parametrize("B", [1, 33, 64])
def test_reused_outputs_over_eight_launches(B, T):
    lens = L.make_lens(B, T, "mixed")
    sets = [seeded(B, T, k) for k in range(8)]
    fresh = [launch_pair(s, lens, L.new_bar()) for s in sets]   # kept alive
    preps = [prepared(s) for s in sets]
    pool = torch.cuda.MemPool()
    bar = L.new_bar()
    ranges = None
    for k, p in enumerate(preps):
        outs = raw_pair(p, lens, bar, pool)
        for name, a in zip(NAMES, outs):
            lo = a.data_ptr()
            hi = lo + a.numel() * a.element_size()
            # the first launch creates the pool's segments; every later
            # one must land on memory that was filled with NaN
            assert ranges is None or any(
                r0 <= lo and hi <= r1 for r0, r1 in ranges), \
                f"launch {k}: {name} is not on NaN-filled memory"
        for name, a, b in zip(NAMES, outs, fresh[k]):
            assert not torch.isnan(a.float()).any(), f"launch {k} {name}: NaN"
            assert torch.equal(a, b), f"launch {k} {name} differs from fresh"
        del outs, a, b
        ranges = poison_free_blocks(pool)


# ---------------------------------------------------------------------------
# 2. the same launch ten times: no atomics in either data path
# ---------------------------------------------------------------------------

def test_same_launch_ten_times_bit_equal():
    B, T = 64, 7
    lens = L.make_lens(B, T, "mixed")
    s = seeded(B, T, 99)
    bar = L.new_bar()
    first = launch_pair(s, lens, bar)
    for rep in range(1, 10):
        for name, a, b in zip(NAMES, launch_pair(s, lens, bar), first):
            assert torch.equal(a, b), f"repeat {rep}: {name} differs"


# ---------------------------------------------------------------------------
# 3. length masks: the per-pass lens and the t+1 stash / Cout guards
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ones", "full", "mixed", "q0ones"])
@pytest.mark.parametrize("T", [2, 7])
def test_length_masks(T, kind):
    """Inputs of its own (seed 1; the layout tests use seed 0) through the
    two-network forward and the backward."""
    B = 64
    c = L.case(B, T, kind, 1)
    lens = c["lens"]
    X1, Whh1, h1, c1, _ = L.make_inputs(B, T, seed=4242 + T)
    H0, C0, H1, C1, S0 = L.kernel_fwd(c["X"], c["Whh"], c["h0"], c["c0"],
                                      lens, second=(X1, Whh1, h1, c1))
    L.check_fwd(f"handoff net0 T{T} {kind}", lens, H0, C0, S0,
                c["mH"], c["mC"], c["mS"], c["ex"])
    L.check_fwd(f"handoff net1 T{T} {kind}", lens, H1, C1, None,
                *L.model_fwd(X1, Whh1, h1, c1, lens),
                L.exact_ref(X1, Whh1, h1, c1, lens))
    dg = L.kernel_bwd(S0, C0, H0, c["dHext"], c["Whh"], lens)
    L.assert_calibrated(f"handoff bwd T{T} {kind} dgates", dg, c["mdG"],
                        c["ex"]["dX"])
    L.check_dgates_masked_zero(dg, lens)


# ---------------------------------------------------------------------------
# 4. tight allocations: stash, Cout and dHext end where their storage ends
# ---------------------------------------------------------------------------

def tight(x):
    """A copy whose storage ends with its last element."""
    t = torch.empty(x.numel(), dtype=x.dtype, device=x.device)
    t.copy_(x.reshape(-1))
    t = t.view(x.shape)
    st = t.untyped_storage()
    assert t.storage_offset() * t.element_size() + t.numel() * \
        t.element_size() == st.nbytes()
    return t


def slack(x):
    """The same values as a view followed by NaN slack in its storage."""
    n = x.numel()
    t = torch.full((n + 4096,), float("nan"), dtype=x.dtype, device=x.device)
    t[:n].copy_(x.reshape(-1))
    return t[:n].view(x.shape)


GUARD = 4096          # bytes on either side of dgates
PATTERN = 0xA5


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_bwd_tight_allocations(B, T):
    X, Whh, h0, c0, dHext = L.make_inputs(B, T, seed=7 * B + T)
    lens = L.make_lens(B, T, "full" if T == 1 else "mixed")
    Hk, Ck, _, _, Sk = L.kernel_fwd(X, Whh, h0, c0, lens)
    whh_t = Whh.t().contiguous()
    tS, tC, tD = tight(Sk), tight(Ck), tight(dHext)
    # dgates between two live guard blocks of a private pool
    nbytes = B * T * 4 * H * 2
    pool = torch.cuda.MemPool()
    u8 = dict(dtype=torch.uint8, device="cuda")
    with torch.cuda.use_mem_pool(pool):
        lo = torch.empty(GUARD, **u8)
        mid = torch.empty(nbytes, **u8)
        hi = torch.empty(GUARD, **u8)
    for t in (lo, mid, hi):
        t.fill_(PATTERN)
    where = mid.data_ptr()
    assert lo.data_ptr() + GUARD == where and where + nbytes == hi.data_ptr()
    del mid, t
    bar = L.new_bar()
    with torch.cuda.use_mem_pool(pool):
        a = L.M_.lstm_bwd(tS, tC, Hk, tD, whh_t, lens, bar)
    assert L.poison(bar) == 0
    assert a.data_ptr() == where, "dgates is not between the guards"
    assert bool((lo == PATTERN).all()) and bool((hi == PATTERN).all()), \
        "guard pattern around dgates changed"
    b = L.kernel_bwd(slack(Sk), slack(Ck), Hk, slack(dHext), Whh, lens)
    assert not torch.isnan(a.float()).any() and torch.equal(a, b)
    assert torch.equal(a, L.kernel_bwd(Sk, Ck, Hk, dHext, Whh, lens))


# ---------------------------------------------------------------------------
# 5. multi-pass: the pass-boundary publish
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("B", [65, 129])
def test_multi_pass_chunks_bit_equal(B, rows):
    T = 7
    X, Whh, h0, c0, dHext = L.make_inputs(B, T, seed=B + rows)
    X1, Whh1, h1, c1, _ = L.make_inputs(B, T, seed=B + rows + 1)
    lens = L.make_lens(B, T, "mixed")
    bar = L.new_bar()
    H0, C0, H1, C1, S0 = MU.multi_fwd(X, Whh, h0, c0, lens, rows, bar=bar,
                                      second=(X1, Whh1, h1, c1))
    dg = MU.multi_bwd(S0, C0, H0, dHext, Whh, lens, rows, bar=bar)
    for r0 in range(0, B - 63, 64):
        s = slice(r0, r0 + 64)
        cut = lambda x: x[s].contiguous()
        ls = cut(lens)
        h0_, c0_, h1_, c1_, s0_ = L.kernel_fwd(
            cut(X), Whh, cut(h0), cut(c0), ls,
            second=(cut(X1), Whh1, cut(h1), cut(c1)))
        dg_ = L.kernel_bwd(s0_, c0_, h0_, cut(dHext), Whh, ls)
        for name, big, small in zip(NAMES, (H0, C0, H1, C1, S0, dg),
                                    (h0_, c0_, h1_, c1_, s0_, dg_)):
            assert torch.equal(big[s], small), f"rows {r0}+64 {name} differ"
