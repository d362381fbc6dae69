"""The extension calls of one engine train step and of one actor tick, in
order, for every encoder.

engine.m (inf.m for HipInference) is swapped for a recorder and the ordered
list of extension function names is compared with the lists written out
below.  Those lists were produced by running this recorder on the parent of
the commit that moved the encoders into ops/nature.py, ops/impala.py and
ops/mlp.py — not on the code under test — so they pin that refactor, and any
later one, to the launch sequence the engine had before.  A change that means
to add, drop or reorder a launch updates the list with it.

The recorder sees extension calls only; torch ops (index_select, cat, copy_)
pass it by.  No eager model runs here.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from r2d2_amd import config as cfg
    from r2d2_amd.models.network import Network
    from r2d2_amd.worker import Learner

PRESETS = ["mspacman", "mspacman_reference", "seaquest_impala",
           "cartpole_hip"]
# B = 72 is the multi-pass LSTM
TRAIN_CASES = [(p, 8) for p in PRESETS] + [("mspacman", 72)]


class Recorder:
    """The extension module behind a recorder of the CountingExt kind
    (tests/test_hip_engine_large_batch.py): every function fetched from it
    appends its name to `names` when called."""

    def __init__(self, m):
        self._m = m
        self.names = []

    def __getattr__(self, name):
        fn = getattr(self._m, name)
        if not callable(fn):
            return fn

        def recorded(*a, **k):
            self.names.append(name)
            return fn(*a, **k)
        return recorded


def make_net(c, seed):
    torch.manual_seed(seed)
    return Network(c.action_dim, c.obs_shape, c.hidden_dim, encoder=c.encoder,
                   forward_steps=c.forward_steps, mlp_hidden=c.mlp_hidden)


def record_train_step(preset, B):
    """Names of one train_step at T = 7 (burn 2, learn 4, fwd 1)."""
    from bench import build_batch
    c = cfg.apply(preset, batch_size=B, burn_in_steps=2, learning_steps=4,
                  forward_steps=1, amp=False, dtype="fp32")
    hip = Learner(None, None, make_net(c, 0))
    hip.enable_hip_engine()
    eng = hip.engine
    assert eng is not None
    batch = build_batch(c, torch.device("cuda"), seed=5)
    assert batch.obs.shape[:2] == (B, 7)
    if c.encoder == "mlp":
        g = torch.Generator(device="cuda").manual_seed(5)
        batch.obs = torch.randn(B, 7, c.obs_shape[0], device="cuda",
                                generator=g)
    rec = eng.m = Recorder(eng.m)
    loss, prio = eng.train_step(batch)
    torch.cuda.synchronize()
    assert int(eng.bar[256].item()) == 0      # LSTM watchdog: not poisoned
    assert bool(torch.isfinite(loss)) and prio.shape == (B,)
    return rec.names


def record_inference(preset, E=5):
    """Names of one HipInference.forward and of one HipInference.step."""
    from r2d2_amd.ops.engine import HipInference
    c = cfg.apply(preset)
    inf = HipInference(make_net(c, 3).cuda().eval(), "cuda", c)
    g = torch.Generator(device="cuda").manual_seed(7)
    A = c.action_dim
    if c.encoder == "mlp":
        obs = torch.randn(E, c.obs_shape[0], device="cuda", generator=g)
    else:
        obs = torch.randint(0, 256, (E,) + tuple(c.obs_shape), device="cuda",
                            dtype=torch.uint8, generator=g)
    la = torch.zeros(E, A, device="cuda")
    la[torch.arange(E, device="cuda"),
       torch.randint(0, A, (E,), device="cuda", generator=g)] = 1.0
    lr = torch.randn(E, 1, device="cuda", generator=g) * 0.1
    h = torch.randn(1, E, 512, device="cuda", generator=g) * 0.1
    cc = torch.randn(1, E, 512, device="cuda", generator=g) * 0.1
    rec = inf.m = Recorder(inf.m)
    q, _ = inf.forward(obs, la, lr, (h, cc))
    fwd_names, rec.names = rec.names, []
    qs, greedy, _ = inf.step(obs, la, lr, (h, cc))
    torch.cuda.synchronize()
    assert q.shape == qs.shape == (E, A) and greedy.shape == (E,)
    return fwd_names, rec.names


# -- the recorded sequences, in pieces ---------------------------------------
# encoder forwards of the train step: online network, then target
NATURE_FWD_PAIR = ["conv1_fwd_dual",
                   "conv_fwd_band", "conv_fwd_band", "gemm_bias_act",
                   "conv_fwd_band", "conv_fwd_band", "gemm_bias_act"]
IMPALA_STAGE = ["conv3p_pool", "conv3p", "conv3p", "conv3p", "conv3p"]
IMPALA_FROM_XP = 3 * IMPALA_STAGE + ["pad2dense", "gemm_bias_act"]
IMPALA_FWD_PAIR = ["pack_frames"] + IMPALA_FROM_XP + IMPALA_FROM_XP
MLP_FWD = ["mlp_in_fwd", "gemm_bias_act"]

HEADS_FWD = 4 * ["gemm_bias_act"] + ["dueling_combine"]


def lstm_heads_loss_and_back(lstm_fwd, lstm_bwd):
    """From the LSTM input of both networks to the latent's gradient."""
    return (2 * ["assemble_rin", "gemm_bias_act"] + [lstm_fwd]
            + HEADS_FWD + HEADS_FWD
            + ["fused_double_q_loss", "segment_priority",
               "dueling_combine_bwd"]
            + 4 * ["gemm_dgrad"] + 4 * ["gemm_wgrad_into"]
            + ["scatter_dh", lstm_bwd]
            + ["gemm_wgrad_into", "gemm_wgrad_into", "gemm_dgrad"])


def nature_bwd(conv1_wgrad):
    return (["gemm_dgrad", "gemm_wgrad"] + 3 * ["conv_wgrad_ws_floats"]
            + ["conv_wgrad_band_into", "conv_dgrad_band",
               "conv_wgrad_band_into", "conv_dgrad_band", conv1_wgrad])


IMPALA_RES_BWD = 2 * ["conv3p_wgrad", "conv3p", "conv3p_wgrad", "conv3p"]
IMPALA_BWD = (["gemm_dgrad", "gemm_wgrad", "dense2pad_mask"]
              + 2 * (IMPALA_RES_BWD
                     + ["maxpool3s2_bwd", "conv3p_wgrad", "conv3p"])
              + IMPALA_RES_BWD + ["maxpool3s2_bwd", "conv3p_wgrad"])
MLP_BWD = ["gemm_dgrad", "gemm_wgrad_into", "mlp_in_wgrad_into"]

SINGLE = lstm_heads_loss_and_back("lstm_fwd", "lstm_bwd")
EXPECTED_TRAIN = {
    ("mspacman", 8):
        NATURE_FWD_PAIR + SINGLE + nature_bwd("conv_wgrad_band_into"),
    ("mspacman_reference", 8):
        NATURE_FWD_PAIR + SINGLE + nature_bwd("conv_wgrad_into"),
    ("seaquest_impala", 8): IMPALA_FWD_PAIR + SINGLE + IMPALA_BWD,
    ("cartpole_hip", 8): MLP_FWD + MLP_FWD + SINGLE + MLP_BWD,
    ("mspacman", 72):
        NATURE_FWD_PAIR
        + lstm_heads_loss_and_back("lstm_fwd_multi", "lstm_bwd_multi")
        + nature_bwd("conv_wgrad_band_into"),
}

# actor inference: the encoder, then forward's GEMM tail or step's three
# fused launches
NATURE_CLASSIC = ["conv_fwd", "conv_fwd", "conv_fwd", "gemm_bias_act"]
ENCODER_FWD = {"mspacman": NATURE_CLASSIC,
               "mspacman_reference": NATURE_CLASSIC,
               "seaquest_impala": ["pack_frames"] + IMPALA_FROM_XP,
               "cartpole_hip": MLP_FWD}
FORWARD_TAIL = (["assemble_rin"] + 6 * ["gemm_bias_act"]
                + ["dueling_combine"])
STEP_TAIL = ["lstm_cell_step", "head_hidden_step", "head_out_step"]
EXPECTED_FORWARD = {p: ENCODER_FWD[p] + FORWARD_TAIL for p in PRESETS}
EXPECTED_STEP = {p: ENCODER_FWD[p] + STEP_TAIL for p in PRESETS}


@pytest.mark.parametrize("preset,B", TRAIN_CASES,
                         ids=[f"{p}-B{b}" for p, b in TRAIN_CASES])
def test_train_step_launch_sequence(preset, B):
    assert record_train_step(preset, B) == EXPECTED_TRAIN[preset, B]


@pytest.mark.parametrize("preset", PRESETS)
def test_inference_launch_sequence(preset):
    fwd_names, step_names = record_inference(preset)
    assert fwd_names == EXPECTED_FORWARD[preset]
    assert step_names == EXPECTED_STEP[preset]
