"""GPU numerics: the conv wgrads without atomics (conv_wgrad_band_into /
conv_wgrad_into: per-workgroup partial sums stored to a workspace, one
reducer that overwrites the .grad views in torch layout) and the empty-mask
convention (an empty act = dY is pre-masked) of all four entry points.

Reference: the f32 torch weight and bias gradient (autograd of F.conv2d in
float32, on the CPU) of the same bf16-rounded inputs, with the ReLU mask
applied to dY, as tests/test_hip_conv_wgrad_gather.py builds it; tolerance
that file's rtol=2e-3, atol=1e-2.  It is computed once per (layer, N).

Shapes: N in {1, 2, 3, 7} x max_wgs in {0, 1, 2, 3}; at N = 7 a workgroup
runs 1, 7, 4 or 3 images, the last workgroup fewer (7 = 4 + 3 = 3 + 3 + 1).
Every layer ends its image on a partly filled 32-row tile (400, 81, 49
pixels).  The destination always sits inside a larger f32 buffer of a known
pattern at an offset that is only 4-byte aligned, and every run checks that
nothing outside it changed.
"""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd.ops import hip_ops
    M_ = hip_ops.ext()

# layer -> (conv_id, CIN, COUT, kernel, stride, input H = W)
GEO = {
    "conv1_c4": (1, 4, 32, 8, 4, 84),
    "conv1_c1": (1, 1, 32, 8, 4, 84),
    "conv2": (2, 32, 64, 4, 2, 20),
    "conv3": (3, 64, 64, 3, 1, 9),
}
LAYERS = list(GEO)
NS = (1, 2, 3, 7)
GRIDS = (0, 1, 2, 3)
# (layer, kernel): the band kernel for every layer; the chunked one where the
# engine runs it (one-channel conv1) and for a 64-output layer (two co tiles)
BAND = [(l, "band") for l in LAYERS]
CHUNKED = [("conv1_c1", "chunked"), ("conv3", "chunked")]
RTOL, ATOL = 2e-3, 1e-2


def out_hw(layer):
    _, _, _, k, s, inhw = GEO[layer]
    return (inhw - k) // s + 1


def slot(layer):
    _, cin, cout, k, _, _ = GEO[layer]
    return cout * k * k * cin + 64


def parts(layer, kernel, N, max_wgs=0):
    """Workgroups = partial sums of a launch."""
    if kernel == "band":
        imgs = -(-N // (max_wgs or 512))
        return -(-N // imgs)
    M = N * out_hw(layer) ** 2
    rows = -(-max(32, -(-M // 1024)) // 32) * 32
    return -(-M // rows)


_cases = {}


def case(layer, N):
    """Seeded operands of (layer, N) and their CPU reference, built once and
    never modified: x, raw dY, act, masked dY, dW_ref (torch layout), db_ref."""
    if (layer, N) in _cases:
        return _cases[(layer, N)]
    conv_id, cin, cout, k, s, inhw = GEO[layer]
    g = torch.Generator(device="cuda").manual_seed(
        7000 + 10 * LAYERS.index(layer) + N)
    if conv_id == 1:
        x = torch.randint(0, 256, (N, inhw, inhw, cin), dtype=torch.uint8,
                          device="cuda", generator=g)
    else:
        x = torch.randn(N, inhw, inhw, cin, device="cuda",
                        generator=g).bfloat16()
    rows, ohw = N * out_hw(layer) ** 2, out_hw(layer)
    dY = (torch.randn(rows, cout, device="cuda", generator=g) * 0.5).bfloat16()
    act = torch.randn(rows, cout, device="cuda", generator=g).bfloat16()
    dYm = torch.where(act > 0, dY, torch.zeros_like(dY))

    xr = x.cpu()
    if conv_id == 1:        # the kernels' fused dequant: bf16(u8 * (1/255))
        xr = (xr.float() * torch.tensor(1.0).div(255.0)).bfloat16()
    xr = xr.float().permute(0, 3, 1, 2).contiguous()
    gy = dYm.float().cpu().view(N, ohw, ohw, cout).permute(0, 3, 1, 2)
    w = torch.zeros(cout, cin, k, k, requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    F.conv2d(xr, w, b, stride=s).backward(gy.contiguous())
    _cases[(layer, N)] = (x, dY, act, dYm, w.grad, b.grad)
    return _cases[(layer, N)]


class Dest:
    """dW and db views in the middle of one flat f32 buffer holding a known
    bit pattern, 3 and 5 floats away from its ends and from each other."""

    def __init__(self, layer):
        _, cin, cout, k, _, _ = GEO[layer]
        nw = cout * cin * k * k
        self.lo, self.mid = 3, 3 + nw + 5
        n = self.mid + cout + 3
        bits = (torch.arange(n, dtype=torch.int32, device="cuda") * 2654435
                + 0x3f000000)
        self.flat = bits.view(torch.float32).clone()
        self.before = self.flat.clone()
        self.dW = self.flat[self.lo:self.lo + nw].view(cout, cin, k, k)
        self.db = self.flat[self.mid:self.mid + cout]

    def outside_unchanged(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        keep[self.lo:self.lo + self.dW.numel()] = False
        keep[self.mid:self.mid + self.db.numel()] = False
        a = self.flat.view(torch.int32)[keep]
        return torch.equal(a, self.before.view(torch.int32)[keep])

    def untouched(self):
        return torch.equal(self.flat.view(torch.int32),
                           self.before.view(torch.int32))


def into(layer, kernel, x, dY, act, max_wgs=0, ws=None):
    """Run an _into entry point; returns (dW, db) clones after checking that
    the destination's surroundings are bit-unchanged."""
    conv_id, cin, cout, k, _, inhw = GEO[layer]
    N = x.shape[0]
    if ws is None:
        ws = torch.empty(parts(layer, kernel, N, max_wgs) * slot(layer),
                         device="cuda")
    d = Dest(layer)
    if kernel == "band":
        M_.conv_wgrad_band_into(dY, act, x, conv_id, N, ws, d.dW, d.db,
                                max_wgs)
    else:
        ohw = out_hw(layer)
        M_.conv_wgrad_into(dY, act, x, conv_id, N, inhw, inhw, ohw, ohw, cout,
                           k * k * cin, ws, d.dW, d.db)
    torch.cuda.synchronize()
    assert d.outside_unchanged(), "wrote outside the .grad views"
    return d.dW.clone(), d.db.clone()


def returning(layer, kernel, x, dY, act, max_wgs=0):
    """The returning entry points; dWt (COUT, ky, kx, c) to torch layout."""
    conv_id, cin, cout, k, _, inhw = GEO[layer]
    N = x.shape[0]
    if kernel == "band":
        dWt, db = M_.conv_wgrad_band(dY, act, x, conv_id, N, max_wgs)
    else:
        ohw = out_hw(layer)
        dWt, db = M_.conv_wgrad(dY, act, x, conv_id, N, inhw, inhw, ohw, ohw,
                                cout, k * k * cin)
    return dWt.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous(), db


def close(a, b, name):
    a, b = a.float().cpu(), b.float().cpu()
    d = (a - b).abs()
    print(f"{name}: max diff {d.max().item():.3e} at scale "
          f"{b.abs().max().item():.3e}")
    assert torch.allclose(a, b, rtol=RTOL, atol=ATOL), name


EMPTY = torch.Tensor()


@pytest.mark.parametrize("max_wgs", GRIDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("layer,kernel", BAND)
def test_band_matches_reference(layer, kernel, N, max_wgs):
    x, dY, act, dYm, dW_ref, db_ref = case(layer, N)
    dW, db = into(layer, kernel, x, dYm, EMPTY, max_wgs)
    close(dW, dW_ref, f"into dW {layer} N={N} wgs={max_wgs}")
    close(db, db_ref, f"into db {layer} N={N} wgs={max_wgs}")
    dW, db = returning(layer, kernel, x, dYm, EMPTY, max_wgs)
    close(dW, dW_ref, f"returning dW {layer} N={N} wgs={max_wgs}")
    close(db, db_ref, f"returning db {layer} N={N} wgs={max_wgs}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("layer,kernel", CHUNKED)
def test_chunked_matches_reference(layer, kernel, N):
    x, dY, act, dYm, dW_ref, db_ref = case(layer, N)
    dW, db = into(layer, kernel, x, dYm, EMPTY)
    close(dW, dW_ref, f"into dW {layer} N={N}")
    close(db, db_ref, f"into db {layer} N={N}")
    dW, db = returning(layer, kernel, x, dYm, EMPTY)
    close(dW, dW_ref, f"returning dW {layer} N={N}")
    close(db, db_ref, f"returning db {layer} N={N}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("layer,kernel", BAND + CHUNKED)
def test_mask_equivalence_and_reproducibility(layer, kernel, N):
    """act with raw dY == empty act with where(act > 0, dY, 0), bit for bit,
    and two launches on the same inputs give the same bits."""
    x, dY, act, dYm, _, _ = case(layer, N)
    wgs = 2 if kernel == "band" else 0
    dW_m, db_m = into(layer, kernel, x, dY, act, wgs)
    dW_e, db_e = into(layer, kernel, x, dYm, EMPTY, wgs)
    assert torch.equal(dW_m, dW_e) and torch.equal(db_m, db_e)
    dW_2, db_2 = into(layer, kernel, x, dYm, EMPTY, wgs)
    assert torch.equal(dW_2, dW_e) and torch.equal(db_2, db_e)
    assert torch.isfinite(dW_e).all() and dW_e.abs().max() > 0


@pytest.mark.parametrize("layer,kernel", BAND + CHUNKED)
def test_workspace_contents_do_not_matter(layer, kernel):
    """NaN-filled, and used at N = 7 before N = 1: the reducer reads only the
    partial sums that the launch wrote."""
    x7, _, _, dYm7, _, _ = case(layer, 7)
    x1, _, _, dYm1, _, _ = case(layer, 1)
    fresh7 = into(layer, kernel, x7, dYm7, EMPTY)
    fresh1 = into(layer, kernel, x1, dYm1, EMPTY)
    # one slot more than the launch needs, so a reducer that reads a partial
    # too many stays inside the workspace and meets NaN
    ws = torch.full(((parts(layer, kernel, 7) + 1) * slot(layer),),
                    float("nan"), device="cuda")
    got7 = into(layer, kernel, x7, dYm7, EMPTY, ws=ws)
    assert torch.isfinite(got7[0]).all() and torch.isfinite(got7[1]).all()
    assert torch.equal(got7[0], fresh7[0]) and torch.equal(got7[1], fresh7[1])
    got1 = into(layer, kernel, x1, dYm1, EMPTY, ws=ws)
    assert torch.equal(got1[0], fresh1[0]) and torch.equal(got1[1], fresh1[1])


def padded(t, fill):
    """t as a view into a larger buffer: two rows (images) of `fill` before
    and after it.  A row is a multiple of 16 bytes for every operand here."""
    big = torch.full((t.shape[0] + 4,) + tuple(t.shape[1:]), fill,
                     dtype=t.dtype, device=t.device)
    big[2:-2] = t
    v = big[2:-2]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layer,kernel", BAND + CHUNKED)
def test_neighbouring_memory_is_not_read(layer, kernel, masked):
    """NaN (bf16) / 255 (u8) right before and after every operand."""
    N = 3
    x, dY, act, dYm, _, _ = case(layer, N)
    wgs = 2 if kernel == "band" else 0
    g, a = (dY, act) if masked else (dYm, EMPTY)
    tight = into(layer, kernel, x, g, a, wgs)
    xp = padded(x, 255 if x.dtype == torch.uint8 else float("nan"))
    gp = padded(g, float("nan"))
    ap = padded(a, float("nan")) if masked else EMPTY
    got = into(layer, kernel, xp, gp, ap, wgs)
    assert torch.equal(got[0], tight[0]) and torch.equal(got[1], tight[1])


@pytest.mark.parametrize("layer,kernel", BAND + CHUNKED)
def test_bad_operands_raise_before_any_launch(layer, kernel):
    conv_id, cin, cout, k, _, inhw = GEO[layer]
    N, ohw = 3, out_hw(layer)
    x, dY, act, dYm, _, _ = case(layer, N)
    n_ws = parts(layer, kernel, N) * slot(layer)
    d = Dest(layer)
    ws = torch.full((n_ws,), 7.0, device="cuda")
    good = dict(dY=dYm, act=EMPTY, x=x, ws=ws, dW=d.dW, db=d.db)

    def run(**over):
        a = {**good, **over}
        if kernel == "band":
            M_.conv_wgrad_band_into(a["dY"], a["act"], a["x"], conv_id, N,
                                    a["ws"], a["dW"], a["db"])
        else:
            M_.conv_wgrad_into(a["dY"], a["act"], a["x"], conv_id, N, inhw,
                               inhw, ohw, ohw, cout, k * k * cin, a["ws"],
                               a["dW"], a["db"])

    wide = torch.zeros(dYm.shape[0], 2 * cout, dtype=torch.bfloat16,
                       device="cuda")
    bad = {
        "dY dtype": dict(dY=dYm.float()),
        "dY shape": dict(dY=dYm[:-1]),
        "dY stride": dict(dY=wide[:, :cout]),
        "dY on the CPU": dict(dY=dYm.cpu()),
        "dY misaligned": dict(dY=torch.cat([dYm.flatten()[:1], dYm.flatten()])
                              [1:].view_as(dYm)),
        "act size": dict(act=act[:-1]),
        "act dtype": dict(act=act.float()),
        "x count": dict(x=x[:-1]),
        "ws too small": dict(ws=ws[:-1]),
        "ws dtype": dict(ws=ws.double()),
        "ws on the CPU": dict(ws=ws.cpu()),
        "dW layout": dict(dW=d.dW.permute(0, 2, 3, 1)),
        "dW shape": dict(dW=d.dW.reshape(cout, -1)),
        "dW dtype": dict(dW=d.dW.double()),
        "db size": dict(db=d.flat[d.mid:d.mid + cout - 1]),
        "db on the CPU": dict(db=d.db.cpu()),
    }
    for what, over in bad.items():
        with pytest.raises(RuntimeError):
            run(**over)
            torch.cuda.synchronize()
            pytest.fail(f"{what}: no error")
    torch.cuda.synchronize()
    assert d.untouched(), "destination written by a refused call"
    assert bool((ws == 7.0).all()), "workspace written by a refused call"
    run()
    torch.cuda.synchronize()
    assert d.outside_unchanged() and not d.untouched()


def test_workspace_size_helper_matches_the_grids():
    for layer in LAYERS:
        conv_id, cin = GEO[layer][:2]
        for N in (1, 7, 700, 5440):
            for kernel in ("band", "chunked"):
                assert M_.conv_wgrad_ws_floats(
                    conv_id, cin, N, kernel == "band") == \
                    parts(layer, kernel, N) * slot(layer)


# --- engine: one step at B = 8, T = 7 in a fresh child process per setting ---
_CHILD = r"""
import sys, torch
from r2d2_amd import config as cfg
from r2d2_amd.models.network import Network
from r2d2_amd.worker import Learner
from bench import build_batch
preset, out = sys.argv[1], sys.argv[2]
c = cfg.apply(preset, batch_size=8, burn_in_steps=2, learning_steps=4,
              forward_steps=1, amp=False, dtype="fp32")
torch.manual_seed(0)
model = Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder="nature",
                forward_steps=c.forward_steps)
hip = Learner(None, None, model)
hip.enable_hip_engine()
batch = build_batch(c, torch.device("cuda"), seed=5)
res = {}
for step in range(2):
    loss, prio = hip.engine.train_step(batch)
    res[f"loss{step}"] = loss.detach().float().cpu()
    res[f"prio{step}"] = torch.as_tensor(prio).float().cpu()
    for n, p in hip.online_net.named_parameters():
        if n.startswith("encoder.conv"):
            res[f"{n}{step}"] = p.grad.detach().cpu().clone()
torch.save(res, out)
"""


def _engine_step(preset, slab, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / f"{preset}_{slab}.pt"
    env = dict(os.environ, R2D2_CONV_WGRAD_SLAB=slab,
               PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", _CHILD, preset, str(out)], env=env,
                   cwd=root, check=True, timeout=300)
    return torch.load(out)


@pytest.mark.parametrize("preset", ["mspacman", "mspacman_reference"])
def test_engine_step_slab_on_and_off(preset, tmp_path):
    """T = 2 + 4 + 1 = 7, B = 8: 56 images, four channels and single frame.
    Loss and priorities of the two flushes agree within the engine-vs-eager
    tolerance of tests/test_hip_engine.py (the forward is the same code, so
    in fact far closer); with the slab flush the conv gradients of two steps
    on the same batch and weights are the same bits."""
    on = _engine_step(preset, "1", tmp_path)
    off = _engine_step(preset, "0", tmp_path)
    l_on, l_off = float(on["loss0"]), float(off["loss0"])
    assert abs(l_on - l_off) < 0.05 * max(1.0, abs(l_off)), (l_on, l_off)
    assert torch.allclose(on["prio0"], off["prio0"], rtol=0.1, atol=0.05)
    names = [k[:-1] for k in on if k.startswith("encoder.conv")
             and k.endswith("0")]
    assert len(names) == 6, names
    for n in names:
        assert torch.isfinite(on[n + "0"]).all() and on[n + "0"].abs().max() > 0
        assert torch.equal(on[n + "0"], on[n + "1"]), n
        close(on[n + "0"], off[n + "0"], f"{preset} {n} slab vs atomic")
