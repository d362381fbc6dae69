// Python bindings for the r2d2_amd gfx950 HIP kernels.
#include <torch/extension.h>

#include <vector>

// loss_kernels.hip
std::vector<torch::Tensor> fused_double_q_loss(
    torch::Tensor q_learn, torch::Tensor q_online_tgt, torch::Tensor q_target_tgt,
    torch::Tensor action, torch::Tensor n_step_reward, torch::Tensor gamma_n,
    torch::Tensor is_weights, double eps, double kappa, int64_t loss_kind);
torch::Tensor segment_priority(torch::Tensor abs_td, torch::Tensor seg_offsets,
                               double eta);

// sumtree.hip
void sumtree_update(torch::Tensor tree, int64_t leaf_offset, torch::Tensor idxes,
                    torch::Tensor td, double alpha, int64_t old_ptr,
                    int64_t cur_ptr, int64_t seq_per_block, int64_t num_blocks);
std::vector<torch::Tensor> sumtree_sample(torch::Tensor tree, int64_t leaf_offset,
                                          int64_t num_levels, torch::Tensor jitter,
                                          int64_t n, double beta,
                                          int64_t max_idx);

// replay_gather.hip
std::vector<torch::Tensor> positions_meta(torch::Tensor meta, torch::Tensor seg,
                                          int64_t T, int64_t n, int64_t R,
                                          int64_t max_learn);
std::vector<torch::Tensor> replay_gather_meta(
    torch::Tensor idx, torch::Tensor burn_s, torch::Tensor learn_s,
    torch::Tensor fwd_s, torch::Tensor obs_start_s, torch::Tensor learn_off_s,
    int64_t spb);
std::vector<torch::Tensor> replay_gather_batch(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb);
std::vector<torch::Tensor> replay_gather_batch_dedup(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb, int64_t C);
std::vector<torch::Tensor> replay_gather_batch_vec(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb,
    c10::optional<std::vector<torch::Tensor>> out);

// gemm_kernels.hip
torch::Tensor gemm_bias_act(torch::Tensor A, torch::Tensor Wt,
                            torch::Tensor bias, int64_t act, bool out_f32,
                            int64_t path);
torch::Tensor gemm_dgrad(torch::Tensor dY, torch::Tensor act_out,
                         torch::Tensor W, bool relu_mask, int64_t k_out,
                         c10::optional<torch::Tensor> out_mask, int64_t path);
std::vector<torch::Tensor> gemm_wgrad(torch::Tensor dY, torch::Tensor act_out,
                                      torch::Tensor A, bool relu_mask,
                                      bool want_bias, int64_t path);
void gemm_wgrad_into(torch::Tensor dY, torch::Tensor act_out, torch::Tensor A,
                     bool relu_mask, torch::Tensor dW_out,
                     torch::Tensor db_out,
                     int64_t kd0, int64_t kd1, int64_t kd2, int64_t path);

// conv_kernels.hip
torch::Tensor conv_fwd(torch::Tensor in, torch::Tensor Wt, torch::Tensor bias,
                       int64_t conv_id, int64_t N, int64_t INH, int64_t INW,
                       int64_t OH, int64_t OW, bool relu);
torch::Tensor conv_dgrad_dense(torch::Tensor dY, torch::Tensor Wd,
                               torch::Tensor taps, torch::Tensor actx,
                               int64_t N, int64_t OH, int64_t OW, int64_t COUT,
                               int64_t XH, int64_t XW, int64_t CIN,
                               int64_t y0, int64_t x0, int64_t S,
                               torch::Tensor dX);
std::vector<torch::Tensor> conv_wgrad(torch::Tensor dY, torch::Tensor act,
                                      torch::Tensor in, int64_t conv_id,
                                      int64_t N, int64_t INH, int64_t INW,
                                      int64_t OH, int64_t OW, int64_t COUT,
                                      int64_t K);
void conv_wgrad_into(torch::Tensor dY, torch::Tensor act, torch::Tensor in,
                     int64_t conv_id, int64_t N, int64_t INH, int64_t INW,
                     int64_t OH, int64_t OW, int64_t COUT, int64_t K,
                     torch::Tensor ws, torch::Tensor dW, torch::Tensor db);
std::vector<torch::Tensor> conv_wgrad_band(torch::Tensor dY, torch::Tensor act,
                                           torch::Tensor in, int64_t conv_id,
                                           int64_t N, int64_t max_wgs);
void conv_wgrad_band_into(torch::Tensor dY, torch::Tensor act,
                          torch::Tensor in, int64_t conv_id, int64_t N,
                          torch::Tensor ws, torch::Tensor dW, torch::Tensor db,
                          int64_t max_wgs);
int64_t conv_wgrad_ws_floats(int64_t conv_id, int64_t cin1, int64_t N,
                             bool band);
torch::Tensor conv_fwd_band(torch::Tensor in, torch::Tensor Wt,
                            torch::Tensor bias, int64_t conv_id, int64_t N,
                            int64_t max_wgs);
std::vector<torch::Tensor> conv1_fwd_dual(torch::Tensor in, torch::Tensor Wt0,
                                          torch::Tensor bias0,
                                          torch::Tensor Wt1,
                                          torch::Tensor bias1, int64_t N,
                                          int64_t max_wgs);
torch::Tensor conv_dgrad_band(torch::Tensor dY, torch::Tensor Wd,
                              torch::Tensor actx, int64_t conv_id, int64_t N,
                              int64_t max_wgs);

// lstm_kernels.hip
torch::Tensor assemble_rin(torch::Tensor latent, torch::Tensor la,
                           torch::Tensor lr, int64_t kin_pad);
void handoff_bench(torch::Tensor barrier_ws, int64_t steps, int64_t nblocks);
void handoff_payload_bench(torch::Tensor barrier_ws, torch::Tensor scratch,
                           int64_t steps, int64_t nblocks, int64_t kb,
                           int64_t mode);
void handoff_counter_bench(torch::Tensor barrier_ws, int64_t steps,
                           int64_t nblocks);
std::vector<torch::Tensor> lstm_fwd(
    torch::Tensor X0, torch::Tensor X1, torch::Tensor Whh0, torch::Tensor Whh1,
    torch::Tensor init0, torch::Tensor init1, torch::Tensor lens,
    torch::Tensor barrier_ws, bool want_stash);
torch::Tensor dueling_combine(torch::Tensor adv, torch::Tensor val, int64_t A);
torch::Tensor scatter_dh(torch::Tensor dh_a, torch::Tensor dh_v,
                         torch::Tensor row_of, int64_t BT);
std::vector<torch::Tensor> dueling_combine_bwd(torch::Tensor dq, int64_t PADA,
                                               int64_t PADV);
torch::Tensor lstm_bwd(torch::Tensor stash, torch::Tensor Cout,
                       torch::Tensor Hout, torch::Tensor dHext,
                       torch::Tensor Whh_bwd, torch::Tensor lens,
                       torch::Tensor barrier_ws);
std::vector<torch::Tensor> lstm_fwd_multi(
    torch::Tensor X0, torch::Tensor X1, torch::Tensor Whh0, torch::Tensor Whh1,
    torch::Tensor init0, torch::Tensor init1, torch::Tensor lens,
    torch::Tensor barrier_ws, bool want_stash, int64_t rows);
torch::Tensor lstm_bwd_multi(torch::Tensor stash, torch::Tensor Cout,
                             torch::Tensor Hout, torch::Tensor dHext,
                             torch::Tensor Whh_bwd, torch::Tensor lens,
                             torch::Tensor barrier_ws, int64_t rows);

// impala_kernels.hip
void conv3p_pool(torch::Tensor in, torch::Tensor Wt, torch::Tensor bias,
                 torch::Tensor pout, torch::Tensor parg, int64_t N,
                 int64_t stage);
void conv3p(torch::Tensor in, torch::Tensor Wt, torch::Tensor bias,
            torch::Tensor res, torch::Tensor mask, torch::Tensor out,
            int64_t N, int64_t H, int64_t W, bool relu_in, bool has_bias,
            int64_t epi);
std::vector<torch::Tensor> conv3p_wgrad(torch::Tensor dY, torch::Tensor in,
                                        int64_t N, int64_t H, int64_t W,
                                        bool relu_in);
void maxpool3s2_fwd(torch::Tensor in, torch::Tensor out, torch::Tensor arg,
                    int64_t N, int64_t H, int64_t W);
void maxpool3s2_bwd(torch::Tensor dOut, torch::Tensor arg, torch::Tensor dIn,
                    int64_t N, int64_t H, int64_t W, int64_t OH, int64_t OW);
void pack_frames(torch::Tensor frames, torch::Tensor out, int64_t H,
                 int64_t W);
torch::Tensor pad2dense(torch::Tensor in, int64_t N, int64_t H, int64_t W,
                        bool relu);
void dense2pad_mask(torch::Tensor dflat, torch::Tensor act_pad,
                    torch::Tensor out, int64_t N, int64_t H, int64_t W);

// optim_kernels.hip
void gather_pack(torch::Tensor flat, torch::Tensor m1, torch::Tensor m2,
                 torch::Tensor out);
torch::Tensor grad_sumsq(torch::Tensor grad, torch::Tensor norm_buf);
void adam_step(torch::Tensor param, torch::Tensor grad, torch::Tensor m,
               torch::Tensor v, torch::Tensor norm_buf, double max_norm,
               double lr, double beta1, double beta2, double eps,
               int64_t step);

// actor_step_kernels.hip
void lstm_cell_step(torch::Tensor latent, torch::Tensor last_action,
                    torch::Tensor last_reward, torch::Tensor h0,
                    torch::Tensor c0, torch::Tensor wih_t,
                    torch::Tensor whh_t, torch::Tensor lstm_bias,
                    torch::Tensor h1, torch::Tensor c1, torch::Tensor hb,
                    int64_t units, int64_t rows);
void head_hidden_step(torch::Tensor hb, torch::Tensor wa1t, torch::Tensor ba1,
                      torch::Tensor wv1t, torch::Tensor bv1,
                      torch::Tensor adv1, torch::Tensor val1, int64_t rows);
void head_out_step(torch::Tensor adv1, torch::Tensor val1, torch::Tensor wa2t,
                   torch::Tensor ba2, torch::Tensor wv2t, torch::Tensor bv2,
                   torch::Tensor q, torch::Tensor greedy);

// mlp_kernels.hip
torch::Tensor mlp_in_fwd(torch::Tensor X, torch::Tensor W1, torch::Tensor b1);
void mlp_in_wgrad_into(torch::Tensor dA1, torch::Tensor X,
                       torch::Tensor dW1_out, torch::Tensor db1_out);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "r2d2_amd gfx950 HIP kernels";
    m.def("fused_double_q_loss", &fused_double_q_loss,
          "Fused double-Q target + TD + loss + dLoss/dQ (returns loss, dq, "
          "abs_td, target)");
    m.def("segment_priority", &segment_priority,
          "Per-sequence mixed max/mean |TD| priority over ragged segments");
    m.def("sumtree_update", &sumtree_update,
          "GPU sum-tree priority update (duplicate-safe, ring-stale-masked)");
    m.def("sumtree_sample", &sumtree_sample,
          "GPU sum-tree stratified sample -> (idx, prio, is_weight)");
    m.def("replay_gather_meta", &replay_gather_meta,
          "Sampled-sequence metadata + segment offsets");
    m.def("positions_meta", &positions_meta,
          "engine gather/scatter position arrays from device-side sample "
          "metadata (no host round trip per ragged batch)");
    m.def("replay_gather_batch", &replay_gather_batch,
          "On-device padded batch assembly from the GPU block store");
    m.def("replay_gather_batch_dedup", &replay_gather_batch_dedup,
          "replay_gather_batch from the frame-once store: one (H, W) frame "
          "per step, obs_rows + C - 1 frames per slot; the (B, T, H*W*C) HWC "
          "stacks are rebuilt in the gather");
    m.def("replay_gather_batch_vec", &replay_gather_batch_vec,
          "replay_gather_batch from the float row store of vector "
          "observations: obs store (num_blocks, obs_rows, D) f32, obs_out "
          "(B, T, D) f32, one workgroup per sample copying its contiguous "
          "span; `out` = the eight outputs preallocated by the caller",
          py::arg("obs_store"), py::arg("la_store"), py::arg("lr_store"),
          py::arg("act_store"), py::arg("nsr_store"), py::arg("gam_store"),
          py::arg("hid_store"), py::arg("idx"), py::arg("meta"),
          py::arg("seg"), py::arg("weights"), py::arg("T"), py::arg("A"),
          py::arg("max_learn"), py::arg("H"), py::arg("spb"),
          py::arg("out") = py::none());
    // path: 0 automatic, 64 the unstaged 64x64 kernel, 6464 / 12864 the
    // LDS-staged 64x64 / 128x64 instantiations (tests and tools force one)
    m.def("gemm_bias_act", &gemm_bias_act, "MFMA GEMM + bias + activation",
          pybind11::arg("A"), pybind11::arg("Wt"), pybind11::arg("bias"),
          pybind11::arg("act"), pybind11::arg("out_f32"),
          pybind11::arg("path") = 0);
    m.def("gemm_dgrad", &gemm_dgrad,
          "MFMA GEMM backward-data (+ fused ReLU mask; optional dense "
          "k_out-column output; optional fused output ReLU mask)",
          pybind11::arg("dY"), pybind11::arg("act_out"), pybind11::arg("W"),
          pybind11::arg("relu_mask"), pybind11::arg("k_out") = 0,
          pybind11::arg("out_mask") = pybind11::none(),
          pybind11::arg("path") = 0);
    // wgrad path: 0 automatic, 64 the 64x64 kernel, 12864 the 128x64 tile
    m.def("gemm_wgrad", &gemm_wgrad, "MFMA GEMM backward-weight (+ bias grad)",
          pybind11::arg("dY"), pybind11::arg("act_out"), pybind11::arg("A"),
          pybind11::arg("relu_mask"), pybind11::arg("want_bias"),
          pybind11::arg("path") = 0);
    m.def("gemm_wgrad_into", &gemm_wgrad_into,
          "GEMM backward-weight accumulated straight into .grad views "
          "(optional (d0,d1,d2)->(d2,d0,d1) k-axis store permutation)",
          pybind11::arg("dY"), pybind11::arg("act_out"), pybind11::arg("A"),
          pybind11::arg("relu_mask"), pybind11::arg("dW_out"),
          pybind11::arg("db_out"), pybind11::arg("kd0") = 0,
          pybind11::arg("kd1") = 0, pybind11::arg("kd2") = 0,
          pybind11::arg("path") = 0);
    m.def("conv_fwd", &conv_fwd, "Implicit-GEMM MFMA conv forward (NHWC)");
    m.def("conv_dgrad_dense", &conv_dgrad_dense,
          "MFMA conv backward-data from dense pre-masked dY (bounds-checked "
          "taps, optional fused output ReLU mask)");
    m.def("scatter_dh", &scatter_dh,
          "dHext (BT, H) from head-backward rows via inverse position map");
    m.def("conv_wgrad", &conv_wgrad, "MFMA conv backward-weight");
    m.def("conv_wgrad_band", &conv_wgrad_band,
          "per-image band wgrad (whole input image LDS-staged, one dequant "
          "per element, register accumulation, one atomic flush per wg); an "
          "empty act = dY is pre-masked",
          py::arg("dY"), py::arg("act"), py::arg("in"), py::arg("conv_id"),
          py::arg("N"), py::arg("max_wgs") = 0);
    m.def("conv_wgrad_band_into", &conv_wgrad_band_into,
          "band wgrad without atomics: per-workgroup partial sums stored to "
          "the workspace ws, then one reducer overwrites dW (torch layout) "
          "and db; bitwise reproducible",
          py::arg("dY"), py::arg("act"), py::arg("in"), py::arg("conv_id"),
          py::arg("N"), py::arg("ws"), py::arg("dW"), py::arg("db"),
          py::arg("max_wgs") = 0);
    m.def("conv_wgrad_into", &conv_wgrad_into,
          "chunked wgrad with the slab flush and reducer of "
          "conv_wgrad_band_into");
    m.def("conv_wgrad_ws_floats", &conv_wgrad_ws_floats,
          "f32 elements of workspace conv_wgrad_band_into (band) or "
          "conv_wgrad_into needs for N images at the default grid",
          py::arg("conv_id"), py::arg("cin1"), py::arg("N"), py::arg("band"));
    m.def("conv_fwd_band", &conv_fwd_band,
          "per-image band forward (image LDS-resident; weights in LDS for "
          "conv1, in registers for the 64-output layers)",
          py::arg("in"), py::arg("Wt"), py::arg("bias"), py::arg("conv_id"),
          py::arg("N"), py::arg("max_wgs") = 0);
    m.def("conv1_fwd_dual", &conv1_fwd_dual,
          "conv1 of two networks from one LDS staging of each frame (both "
          "weight sets in registers, 16-byte stores); returns (out0, out1)",
          py::arg("in"), py::arg("Wt0"), py::arg("bias0"), py::arg("Wt1"),
          py::arg("bias1"), py::arg("N"), py::arg("max_wgs") = 0);
    m.def("conv_dgrad_band", &conv_dgrad_band,
          "per-image band dgrad: dY staged once in LDS in a zero halo, all "
          "parity classes in one launch, dX stored through LDS with the "
          "optional fused output ReLU mask",
          py::arg("dY"), py::arg("Wd"), py::arg("actx"), py::arg("conv_id"),
          py::arg("N"), py::arg("max_wgs") = 0);
    m.def("lstm_fwd", &lstm_fwd,
          "Persistent fused LSTM forward (dual-network, length-masked)");
    m.def("lstm_bwd", &lstm_bwd, "Persistent fused LSTM BPTT backward");
    m.def("lstm_fwd_multi", &lstm_fwd_multi,
          "Persistent fused LSTM forward for 1 <= B <= 256: one launch, "
          "passes of `rows` (64 or 128; 0 = R2D2_LSTM_MULTI_ROWS / default) "
          "batch rows with W_hh LDS-resident across passes",
          py::arg("X0"), py::arg("X1"), py::arg("Whh0"), py::arg("Whh1"),
          py::arg("init0"), py::arg("init1"), py::arg("lens"),
          py::arg("barrier_ws"), py::arg("want_stash"), py::arg("rows") = 0);
    m.def("lstm_bwd_multi", &lstm_bwd_multi,
          "Persistent fused LSTM BPTT backward for 1 <= B <= 256 (multi-pass)",
          py::arg("stash"), py::arg("Cout"), py::arg("Hout"),
          py::arg("dHext"), py::arg("Whh_bwd"), py::arg("lens"),
          py::arg("barrier_ws"), py::arg("rows") = 0);
    m.def("assemble_rin", &assemble_rin,
          "fused LSTM-input row assembly (latent | action | reward | pad)");
    m.def("handoff_bench", &handoff_bench, "producer-flag handoff microbench");
    m.def("handoff_payload_bench", &handoff_payload_bench,
          "counter handoff behind kb KB of stores per block: mode 0 plain "
          "stores + release fence, mode 1 sc1 stores, no fence");
    m.def("handoff_counter_bench", &handoff_counter_bench,
          "counter-aggregated handoff microbench");
    m.def("dueling_combine", &dueling_combine, "q = V + A - mean(A)");
    m.def("dueling_combine_bwd", &dueling_combine_bwd, "dueling combine backward");
    m.def("conv3p", &conv3p,
          "IMPALA 3x3 s1 p1 conv on halo-padded NHWC (fwd & dgrad-as-conv, "
          "fused relu-in / residual / mask epilogues)");
    m.def("conv3p_pool", &conv3p_pool,
          "IMPALA stage conv FUSED with maxpool 3x3 s2 (conv output stays "
          "in LDS; emits pooled activations + tap argmax)");
    m.def("conv3p_wgrad", &conv3p_wgrad,
          "IMPALA 3x3 conv backward-weight (padded dY, relu-in patches)");
    m.def("maxpool3s2_fwd", &maxpool3s2_fwd,
          "maxpool 3x3 s2 p1 forward + tap argmax");
    m.def("maxpool3s2_bwd", &maxpool3s2_bwd,
          "maxpool backward (atomic-free input-side gather)");
    m.def("pack_frames", &pack_frames,
          "u8 HWC frames -> halo-padded 8-channel u8");
    m.def("pad2dense", &pad2dense, "padded NHWC -> dense rows (+relu)");
    m.def("dense2pad_mask", &dense2pad_mask,
          "dense grad -> padded, masked by act>0 (relu backward)");
    m.def("lstm_cell_step", &lstm_cell_step,
          "fused single-step LSTM cell for actor inference: input-row "
          "assembly, both gate GEMMs, bias, nonlinearities and cell update "
          "in one launch; writes h1, c1 (f32) and hb = bf16(h1)",
          py::arg("latent"), py::arg("last_action"), py::arg("last_reward"),
          py::arg("h0"), py::arg("c0"), py::arg("wih_t"), py::arg("whh_t"),
          py::arg("lstm_bias"), py::arg("h1"), py::arg("c1"), py::arg("hb"),
          py::arg("units") = 0, py::arg("rows") = 0);
    m.def("head_hidden_step", &head_hidden_step,
          "both dueling-head 512 -> 512 ReLU hidden layers in one launch",
          py::arg("hb"), py::arg("wa1t"), py::arg("ba1"), py::arg("wv1t"),
          py::arg("bv1"), py::arg("adv1"), py::arg("val1"),
          py::arg("rows") = 0);
    m.def("head_out_step", &head_out_step,
          "both dueling-head output layers + q = V + A - mean(A) + greedy "
          "action (first index of the row maximum) in one launch");
    m.def("mlp_in_fwd", &mlp_in_fwd,
          "MLP encoder first layer: A1 (M, 512) bf16 = relu(X (M, D) f32 . "
          "W1 (512, D)^T + b1), 1 <= D <= 16, f32 accumulation",
          py::arg("X"), py::arg("W1"), py::arg("b1"));
    m.def("mlp_in_wgrad_into", &mlp_in_wgrad_into,
          "MLP encoder first-layer weight gradient accumulated into .grad "
          "views: dW1 (512, D) += dA1^T . X, db1 (512,) += column sums of "
          "dA1 (bf16, already ReLU-masked)",
          py::arg("dA1"), py::arg("X"), py::arg("dW1_out"),
          py::arg("db1_out"));
    m.def("gather_pack", &gather_pack,
          "regenerate prepacked weights from the flat param buffer "
          "(index-map gather, one launch per dtype)");
    m.def("grad_sumsq", &grad_sumsq, "flat gradient squared-norm reduction");
    m.def("adam_step", &adam_step,
          "fused multi-tensor clip + Adam on the flat parameter buffer");
}
