// On-device batch assembly from the GPU-resident block store (gfx950).
//
// Replaces the reference's single-threaded Python slice loop + pad_sequence
// (worker.py:176-214) with device gather kernels reading directly from the
// HBM block store the sampled sequences live in.  No host round-trip: the
// sum-tree sample output feeds these kernels on the same stream.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

// ---------------------------------------------------------------------------
// Kernel A: per-sample sequence metadata + segment offsets (single block).
//   idx -> (block, seq); read per-seq meta; exclusive-scan learn -> seg.
// ---------------------------------------------------------------------------
__global__ void gather_meta_kernel(
    const long* __restrict__ idx,          // (B,) sampled sequence indexes
    const int* __restrict__ burn_s,        // (num_blocks*spb,)
    const int* __restrict__ learn_s,
    const int* __restrict__ fwd_s,
    const int* __restrict__ obs_start_s,
    const int* __restrict__ learn_off_s,
    int* __restrict__ out_meta,            // (5, B): burn, learn, fwd, obs_start, learn_off
    int* __restrict__ seg,                 // (B+1,)
    int B, int spb) {
    __shared__ int scan_buf[1024];
    int i = threadIdx.x;
    int learn = 0;
    if (i < B) {
        long s = idx[i];
        out_meta[0 * B + i] = burn_s[s];
        learn = learn_s[s];
        out_meta[1 * B + i] = learn;
        out_meta[2 * B + i] = fwd_s[s];
        out_meta[3 * B + i] = obs_start_s[s];
        out_meta[4 * B + i] = learn_off_s[s];
    }
    scan_buf[i] = learn;
    __syncthreads();
    // inclusive scan (Hillis-Steele) over blockDim.x
    for (int off = 1; off < blockDim.x; off <<= 1) {
        int v = (i >= off) ? scan_buf[i - off] : 0;
        __syncthreads();
        scan_buf[i] += v;
        __syncthreads();
    }
    if (i < B) seg[i + 1] = scan_buf[i];
    if (i == 0) seg[0] = 0;
}

// ---------------------------------------------------------------------------
// Kernel B: padded sequence tensors.
//   grid.x = B * T; each block copies one (sample, time) frame (16B chunks)
//   and lane 0..A-1 fill the one-hot last_action, lane 0 the last_reward.
// ---------------------------------------------------------------------------
__global__ void gather_frames_kernel(
    const unsigned char* __restrict__ obs_store,  // (num_blocks, obs_rows, FB)
    const unsigned char* __restrict__ la_store,   // (num_blocks, obs_rows)
    const float* __restrict__ lr_store,           // (num_blocks, obs_rows)
    const int* __restrict__ meta,                 // (5, B)
    unsigned char* __restrict__ obs_out,          // (B, T, FB)
    float* __restrict__ la_out,                   // (B, T, A)
    float* __restrict__ lr_out,                   // (B, T)
    int B, int T, int A, long frame_bytes, long obs_rows, int spb) {
    int bt = blockIdx.x;
    int b = bt / T, t = bt % T;
    int burn = meta[0 * B + b], learn = meta[1 * B + b], fwd = meta[2 * B + b];
    int obs_start = meta[3 * B + b];
    int valid = burn + learn + fwd;
    long blk = 0;  // encoded inside obs_start: obs_start = block*obs_rows + row
    long row = (long)obs_start - burn + t;
    unsigned char* dst = obs_out + ((long)b * T + t) * frame_bytes;
    if (t < valid) {
        const unsigned char* src = obs_store + row * frame_bytes;
        for (long o = threadIdx.x * 16; o + 16 <= frame_bytes; o += blockDim.x * 16)
            *reinterpret_cast<uint4*>(dst + o) =
                *reinterpret_cast<const uint4*>(src + o);
        // frame_bytes tail (not multiple of 16)
        long tail = (frame_bytes / 16) * 16;
        for (long o = tail + threadIdx.x; o < frame_bytes; o += blockDim.x)
            dst[o] = src[o];
        if (threadIdx.x < A)
            la_out[((long)b * T + t) * A + threadIdx.x] =
                (la_store[row] == threadIdx.x) ? 1.f : 0.f;
        if (threadIdx.x == 0) lr_out[(long)b * T + t] = lr_store[row];
    } else {
        for (long o = threadIdx.x * 16; o + 16 <= frame_bytes; o += blockDim.x * 16)
            *reinterpret_cast<uint4*>(dst + o) = uint4{0, 0, 0, 0};
        long tail = (frame_bytes / 16) * 16;
        for (long o = tail + threadIdx.x; o < frame_bytes; o += blockDim.x)
            dst[o] = 0;
        if (threadIdx.x < A) la_out[((long)b * T + t) * A + threadIdx.x] = 0.f;
        if (threadIdx.x == 0) lr_out[(long)b * T + t] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// Kernel B': padded sequence tensors from the frame-once store.
//   The store keeps ONE (H, W) frame per step: slot `blk` holds
//   obs_rows + C - 1 frames, the first C - 1 being the lead-in of the slot's
//   first stack, so row r's stack is frames r .. r + C - 1 of its slot and
//   r + c never leaves the slot.  grid.x = B * T as in Kernel B; each block
//   rebuilds one HWC stack:
//     obs_out[((b*T + t)*HW + p)*C + c] = frame[blk*(obs_rows+C-1) + r + c][p]
//   kVec4 (C == 4, HW % 16 == 0): a thread loads 16 pixels of each of the
//   four frames, transposes every 4x4 byte tile in registers (v_perm_b32) and
//   stores 64 contiguous bytes.  Otherwise one byte per thread-iteration.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 interleave4(unsigned a, unsigned b,
                                             unsigned c, unsigned d) {
    // a..d: 4 pixels of frames 0..3 (byte k = pixel k).  v_perm_b32 picks
    // bytes 0-3 from its SECOND operand and 4-7 from its first.
    unsigned ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    unsigned ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    unsigned cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);
    unsigned cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
    uint4 o;
    o.x = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);     // a0 b0 c0 d0
    o.y = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);     // a1 b1 c1 d1
    o.z = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
    o.w = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
    return o;
}

template <bool kVec4>
__global__ void gather_frames_stack_kernel(
    const unsigned char* __restrict__ obs_store,  // (num_blocks, obs_rows+C-1, HW)
    const unsigned char* __restrict__ la_store,   // (num_blocks, obs_rows)
    const float* __restrict__ lr_store,           // (num_blocks, obs_rows)
    const int* __restrict__ meta,                 // (5, B)
    unsigned char* __restrict__ obs_out,          // (B, T, HW, C)
    float* __restrict__ la_out,                   // (B, T, A)
    float* __restrict__ lr_out,                   // (B, T)
    int B, int T, int A, int C, long HW, long obs_rows, long num_blocks) {
    int bt = blockIdx.x;
    int b = bt / T, t = bt % T;
    int burn = meta[0 * B + b], learn = meta[1 * B + b], fwd = meta[2 * B + b];
    int obs_start = meta[3 * B + b];
    int valid = burn + learn + fwd;
    long g = (long)obs_start - burn + t;  // global row: slot*obs_rows + r
    long out_bytes = HW * C;
    unsigned char* dst = obs_out + ((long)b * T + t) * out_bytes;
    // a row outside the store (corrupt metadata) pads like t >= valid
    if (t < valid && g >= 0 && g < num_blocks * obs_rows) {
        long blk = g / obs_rows, r = g % obs_rows;
        const unsigned char* src =
            obs_store + (blk * (obs_rows + C - 1) + r) * HW;
        if (kVec4) {
            for (long q = threadIdx.x; q < HW / 16; q += blockDim.x) {
                uint4 f0 = *reinterpret_cast<const uint4*>(src + q * 16);
                uint4 f1 = *reinterpret_cast<const uint4*>(src + HW + q * 16);
                uint4 f2 = *reinterpret_cast<const uint4*>(src + 2 * HW + q * 16);
                uint4 f3 = *reinterpret_cast<const uint4*>(src + 3 * HW + q * 16);
                uint4* o = reinterpret_cast<uint4*>(dst + q * 64);
                o[0] = interleave4(f0.x, f1.x, f2.x, f3.x);
                o[1] = interleave4(f0.y, f1.y, f2.y, f3.y);
                o[2] = interleave4(f0.z, f1.z, f2.z, f3.z);
                o[3] = interleave4(f0.w, f1.w, f2.w, f3.w);
            }
        } else {
            for (long o = threadIdx.x; o < out_bytes; o += blockDim.x) {
                long p = o / C, c = o % C;
                dst[o] = src[c * HW + p];
            }
        }
        if (threadIdx.x < A)
            la_out[((long)b * T + t) * A + threadIdx.x] =
                (la_store[g] == threadIdx.x) ? 1.f : 0.f;
        if (threadIdx.x == 0) lr_out[(long)b * T + t] = lr_store[g];
    } else {
        if (kVec4) {
            for (long o = threadIdx.x * 16; o < out_bytes; o += blockDim.x * 16)
                *reinterpret_cast<uint4*>(dst + o) = uint4{0, 0, 0, 0};
        } else {
            for (long o = threadIdx.x; o < out_bytes; o += blockDim.x)
                dst[o] = 0;
        }
        if (threadIdx.x < A) la_out[((long)b * T + t) * A + threadIdx.x] = 0.f;
        if (threadIdx.x == 0) lr_out[(long)b * T + t] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// Kernel B'': padded sequence tensors from the float row store (vector
//   observations, D float32 per step).  A (sample, time) row is at most a few
//   dozen bytes, so a grid of B * T workgroups as in Kernel B would be all
//   launch and no copy.  The valid rows of one sample are CONTIGUOUS in the
//   store — obs_start - burn .. + valid, inside one slot — so grid.x = B and
//   each workgroup reads its five metadata words once and copies one span:
//     obs_out[b*T*D + i] = obs_store[(obs_start - burn)*D + i],  i < valid*D
//   and zero-fills i = valid*D .. T*D.  kVec4 (D % 4 == 0 and both bases
//   16-byte aligned; every row offset is then a multiple of 16 bytes) moves
//   float4, otherwise one float per thread-iteration.  la_out / lr_out as in
//   Kernel B.  A span that is not wholly inside the store (corrupt metadata)
//   pads as if valid = 0, the guard of Kernel B'.
// ---------------------------------------------------------------------------
template <bool kVec4>
__global__ void gather_rows_f32_kernel(
    const float* __restrict__ obs_store,          // (num_blocks, obs_rows, D)
    const unsigned char* __restrict__ la_store,   // (num_blocks, obs_rows)
    const float* __restrict__ lr_store,           // (num_blocks, obs_rows)
    const int* __restrict__ meta,                 // (5, B)
    float* __restrict__ obs_out,                  // (B, T, D)
    float* __restrict__ la_out,                   // (B, T, A)
    float* __restrict__ lr_out,                   // (B, T)
    int B, int T, int A, long D, long total_rows) {
    int b = blockIdx.x;
    long burn = meta[0 * B + b], learn = meta[1 * B + b], fwd = meta[2 * B + b];
    long g0 = (long)meta[3 * B + b] - burn;  // first global row of the span
    long valid = burn + learn + fwd;
    if (valid > T) valid = T;                // Kernel B copies t < T only
    if (burn < 0 || learn < 0 || fwd < 0 || g0 < 0 || g0 + valid > total_rows) {
        valid = 0;
        g0 = 0;
    }
    const float* src = obs_store + g0 * D;
    float* dst = obs_out + (long)b * T * D;
    long n = valid * D, total = (long)T * D;
    if (kVec4) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        float4* dst4 = reinterpret_cast<float4*>(dst);
        for (long i = threadIdx.x; i < total / 4; i += blockDim.x)
            dst4[i] = (i < n / 4) ? src4[i] : float4{0.f, 0.f, 0.f, 0.f};
    } else {
        for (long i = threadIdx.x; i < total; i += blockDim.x)
            dst[i] = (i < n) ? src[i] : 0.f;
    }
    for (long t = threadIdx.x; t < T; t += blockDim.x)
        lr_out[(long)b * T + t] = (t < valid) ? lr_store[g0 + t] : 0.f;
    for (long i = threadIdx.x; i < (long)T * A; i += blockDim.x) {
        long t = i / A, a = i % A;
        la_out[(long)b * T * A + i] =
            (t < valid && la_store[g0 + t] == a) ? 1.f : 0.f;
    }
}

// ---------------------------------------------------------------------------
// Kernel C: flat per-learning-step arrays + hidden states + repeated weights.
//   grid over B * max_learn threads.
// ---------------------------------------------------------------------------
__global__ void gather_flat_kernel(
    const unsigned char* __restrict__ act_store,  // (num_blocks, block_len)
    const float* __restrict__ nsr_store,
    const float* __restrict__ gam_store,
    const float* __restrict__ hid_store,          // (num_blocks*spb, 2*H)
    const long* __restrict__ idx,                 // (B,)
    const int* __restrict__ meta,                 // (5, B)
    const int* __restrict__ seg,                  // (B+1,)
    const float* __restrict__ weights,            // (B,)
    long* __restrict__ act_out,                   // (Rmax,)
    float* __restrict__ nsr_out, float* __restrict__ gam_out,
    float* __restrict__ w_out,
    float* __restrict__ hid_out,                  // (2, B, H)
    int B, int max_learn, int H, long block_len, int spb) {
    int tid = blockIdx.x * blockDim.x + threadIdx.x;
    int b = tid / max_learn, j = tid % max_learn;
    if (b >= B) return;
    int learn = meta[1 * B + b];
    long s = idx[b];
    long blk = s / spb;
    if (j < learn) {
        long src = blk * block_len + meta[4 * B + b] + j;
        long dst = seg[b] + j;
        act_out[dst] = (long)act_store[src];
        nsr_out[dst] = nsr_store[src];
        gam_out[dst] = gam_store[src];
        w_out[dst] = weights[b];
    }
    // hidden: reuse threads j < 2*H strided
    for (int h = j; h < 2 * H; h += max_learn) {
        int which = h / H, hi = h % H;
        hid_out[((long)which * B + b) * H + hi] = hid_store[s * 2 * H + h];
    }
}

// ---------------------------------------------------------------------------
// positions_meta: the engine's gather/scatter position arrays straight from
// the device-side sample metadata — lp/tp (learning- and
// target-position rows of the (B, T+1, H) LSTM output), the inverse map
// feeding the dHext scatter, and per-sample lengths.  Replay-sampled
// batches have a different ragged layout every step, so the host-side
// numpy rebuild this replaces sat in the headline loop.
// ---------------------------------------------------------------------------
__global__ void positions_meta_kernel(
    const int* __restrict__ meta,   // (5, B): burn, learn, fwd, ...
    const int* __restrict__ seg,    // (B+1,)
    long* __restrict__ lp,          // (R,)
    long* __restrict__ tp,          // (R,)
    int* __restrict__ row_of,       // (B*T,) pre-filled with -1
    int* __restrict__ lens,         // (B,)
    int B, int T, int n, int max_learn) {
    int tid = blockIdx.x * blockDim.x + threadIdx.x;
    int b = tid / max_learn, j = tid % max_learn;
    if (b >= B) return;
    int burn = meta[b], learn = meta[B + b], fwd = meta[2 * B + b];
    if (j == 0) lens[b] = burn + learn + fwd;
    if (j < learn) {
        long r = seg[b] + j;
        int tl = burn + j;
        int tt = min(tl + n, burn + learn + fwd - 1);
        lp[r] = (long)b * (T + 1) + tl + 1;
        tp[r] = (long)b * (T + 1) + tt + 1;
        row_of[(long)b * T + tl] = (int)r;
    }
}

std::vector<torch::Tensor> positions_meta(torch::Tensor meta, torch::Tensor seg,
                                          int64_t T, int64_t n, int64_t R,
                                          int64_t max_learn) {
    TORCH_CHECK(meta.is_cuda() && meta.dtype() == torch::kInt32);
    int B = meta.size(1);
    auto i64 = meta.options().dtype(torch::kInt64);
    auto i32 = meta.options();
    auto lp = torch::empty({R}, i64);
    auto tp = torch::empty({R}, i64);
    auto row_of = torch::full({B * T}, -1, i32);
    auto lens = torch::empty({B}, i32);
    long total = (long)B * max_learn;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(positions_meta_kernel,
                       dim3((int)((total + 255) / 256)), dim3(256), 0,
                       stream.stream(), meta.data_ptr<int>(),
                       seg.data_ptr<int>(), lp.data_ptr<long>(),
                       tp.data_ptr<long>(), row_of.data_ptr<int>(),
                       lens.data_ptr<int>(), B, (int)T, (int)n,
                       (int)max_learn);
    return {lp, tp, row_of, lens};
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

std::vector<torch::Tensor> replay_gather_meta(
    torch::Tensor idx, torch::Tensor burn_s, torch::Tensor learn_s,
    torch::Tensor fwd_s, torch::Tensor obs_start_s, torch::Tensor learn_off_s,
    int64_t spb) {
    int B = idx.size(0);
    TORCH_CHECK(B <= 1024);
    auto opts_i = idx.options().dtype(torch::kInt32);
    auto meta = torch::empty({5, B}, opts_i);
    auto seg = torch::empty({B + 1}, opts_i);
    int threads = 64;
    while (threads < B) threads *= 2;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gather_meta_kernel, dim3(1), dim3(threads), 0,
                       stream.stream(), idx.data_ptr<long>(),
                       burn_s.data_ptr<int>(), learn_s.data_ptr<int>(),
                       fwd_s.data_ptr<int>(), obs_start_s.data_ptr<int>(),
                       learn_off_s.data_ptr<int>(), meta.data_ptr<int>(),
                       seg.data_ptr<int>(), B, (int)spb);
    return {meta, seg};
}

std::vector<torch::Tensor> replay_gather_batch(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb) {
    int B = idx.size(0);
    long obs_rows = obs_store.size(1);
    long frame_bytes = obs_store.size(2);
    long block_len = act_store.size(1);
    auto u8 = obs_store.options();
    auto f32 = lr_store.options();
    auto i64 = idx.options();
    auto obs_out = torch::empty({B, T, frame_bytes}, u8);
    auto la_out = torch::empty({B, T, A}, f32);
    auto lr_out = torch::empty({B, T}, f32);
    long Rmax = (long)B * max_learn;
    auto act_out = torch::empty({Rmax}, i64);
    auto nsr_out = torch::empty({Rmax}, f32);
    auto gam_out = torch::empty({Rmax}, f32);
    auto w_out = torch::empty({Rmax}, f32);
    auto hid_out = torch::empty({2, B, H}, f32);
    auto stream = at::cuda::getCurrentCUDAStream();

    hipLaunchKernelGGL(gather_frames_kernel, dim3(B * T), dim3(256), 0,
                       stream.stream(), obs_store.data_ptr<unsigned char>(),
                       la_store.data_ptr<unsigned char>(), lr_store.data_ptr<float>(),
                       meta.data_ptr<int>(), obs_out.data_ptr<unsigned char>(),
                       la_out.data_ptr<float>(), lr_out.data_ptr<float>(),
                       B, (int)T, (int)A, frame_bytes, obs_rows, (int)spb);

    int total = B * (int)max_learn;
    hipLaunchKernelGGL(gather_flat_kernel, dim3((total + 255) / 256), dim3(256),
                       0, stream.stream(), act_store.data_ptr<unsigned char>(),
                       nsr_store.data_ptr<float>(), gam_store.data_ptr<float>(),
                       hid_store.data_ptr<float>(), idx.data_ptr<long>(),
                       meta.data_ptr<int>(), seg.data_ptr<int>(),
                       weights.data_ptr<float>(), act_out.data_ptr<long>(),
                       nsr_out.data_ptr<float>(), gam_out.data_ptr<float>(),
                       w_out.data_ptr<float>(), hid_out.data_ptr<float>(),
                       B, (int)max_learn, (int)H, block_len, (int)spb);

    return {obs_out, la_out, lr_out, act_out, nsr_out, gam_out, w_out, hid_out};
}

// Frame-once store: same outputs as replay_gather_batch, the (B, T, HW*C)
// HWC stacks rebuilt from single frames by gather_frames_stack_kernel.
std::vector<torch::Tensor> replay_gather_batch_dedup(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb, int64_t C) {
    TORCH_CHECK(C >= 2 && C <= 8, "replay_gather_batch_dedup: C must be in "
                "[2, 8], got ", C);
    TORCH_CHECK(obs_store.is_cuda() && la_store.is_cuda() && lr_store.is_cuda()
                && act_store.is_cuda() && nsr_store.is_cuda()
                && gam_store.is_cuda() && hid_store.is_cuda() && idx.is_cuda()
                && meta.is_cuda() && seg.is_cuda() && weights.is_cuda(),
                "replay_gather_batch_dedup: every tensor must be on the GPU");
    TORCH_CHECK(obs_store.dtype() == torch::kUInt8
                && la_store.dtype() == torch::kUInt8
                && act_store.dtype() == torch::kUInt8,
                "replay_gather_batch_dedup: obs/la/act stores must be uint8");
    TORCH_CHECK(lr_store.dtype() == torch::kFloat32
                && nsr_store.dtype() == torch::kFloat32
                && gam_store.dtype() == torch::kFloat32
                && hid_store.dtype() == torch::kFloat32
                && weights.dtype() == torch::kFloat32,
                "replay_gather_batch_dedup: lr/nsr/gam/hid/weights must be "
                "float32");
    TORCH_CHECK(idx.dtype() == torch::kInt64 && meta.dtype() == torch::kInt32
                && seg.dtype() == torch::kInt32,
                "replay_gather_batch_dedup: idx int64, meta/seg int32");
    TORCH_CHECK(obs_store.is_contiguous() && la_store.is_contiguous()
                && lr_store.is_contiguous() && act_store.is_contiguous()
                && nsr_store.is_contiguous() && gam_store.is_contiguous()
                && hid_store.is_contiguous() && idx.is_contiguous()
                && meta.is_contiguous() && seg.is_contiguous()
                && weights.is_contiguous(),
                "replay_gather_batch_dedup: every tensor must be contiguous");
    TORCH_CHECK(obs_store.dim() == 3 && la_store.dim() == 2
                && lr_store.dim() == 2 && act_store.dim() == 2);
    TORCH_CHECK(obs_store.size(1) == la_store.size(1) + C - 1,
                "replay_gather_batch_dedup: the frame store holds ",
                obs_store.size(1), " frames per slot, expected obs_rows + C - 1"
                " = ", la_store.size(1) + C - 1);
    TORCH_CHECK(obs_store.size(0) == la_store.size(0)
                && lr_store.sizes() == la_store.sizes()
                && act_store.size(0) == la_store.size(0)
                && nsr_store.sizes() == act_store.sizes()
                && gam_store.sizes() == act_store.sizes(),
                "replay_gather_batch_dedup: store shapes disagree");
    int B = idx.size(0);
    TORCH_CHECK(B >= 1 && B <= 1024, "replay_gather_batch_dedup: B must be in "
                "[1, 1024], got ", B);
    TORCH_CHECK(meta.dim() == 2 && meta.size(0) == 5 && meta.size(1) == B
                && seg.numel() == B + 1 && weights.numel() == B);
    TORCH_CHECK(T >= 1 && A >= 1 && A <= 256 && max_learn >= 1 && H >= 1
                && spb >= 1);
    TORCH_CHECK(hid_store.dim() == 2 && hid_store.size(1) == 2 * H
                && hid_store.size(0) == la_store.size(0) * spb);
    long num_blocks = obs_store.size(0);
    long obs_rows = la_store.size(1);
    long HW = obs_store.size(2);
    long block_len = act_store.size(1);
    bool vec4 = (C == 4);
    if (vec4)
        TORCH_CHECK(HW % 16 == 0, "replay_gather_batch_dedup: the C = 4 "
                    "vector path needs H*W % 16 == 0, got ", HW);
    auto u8 = obs_store.options();
    auto f32 = lr_store.options();
    auto i64 = idx.options();
    auto obs_out = torch::empty({B, T, HW * C}, u8);
    auto la_out = torch::empty({B, T, A}, f32);
    auto lr_out = torch::empty({B, T}, f32);
    long Rmax = (long)B * max_learn;
    auto act_out = torch::empty({Rmax}, i64);
    auto nsr_out = torch::empty({Rmax}, f32);
    auto gam_out = torch::empty({Rmax}, f32);
    auto w_out = torch::empty({Rmax}, f32);
    auto hid_out = torch::empty({2, B, H}, f32);
    auto stream = at::cuda::getCurrentCUDAStream();

    auto frames = vec4 ? gather_frames_stack_kernel<true>
                       : gather_frames_stack_kernel<false>;
    hipLaunchKernelGGL(frames, dim3(B * (int)T), dim3(256), 0,
                       stream.stream(), obs_store.data_ptr<unsigned char>(),
                       la_store.data_ptr<unsigned char>(), lr_store.data_ptr<float>(),
                       meta.data_ptr<int>(), obs_out.data_ptr<unsigned char>(),
                       la_out.data_ptr<float>(), lr_out.data_ptr<float>(),
                       B, (int)T, (int)A, (int)C, HW, obs_rows, num_blocks);

    int total = B * (int)max_learn;
    hipLaunchKernelGGL(gather_flat_kernel, dim3((total + 255) / 256), dim3(256),
                       0, stream.stream(), act_store.data_ptr<unsigned char>(),
                       nsr_store.data_ptr<float>(), gam_store.data_ptr<float>(),
                       hid_store.data_ptr<float>(), idx.data_ptr<long>(),
                       meta.data_ptr<int>(), seg.data_ptr<int>(),
                       weights.data_ptr<float>(), act_out.data_ptr<long>(),
                       nsr_out.data_ptr<float>(), gam_out.data_ptr<float>(),
                       w_out.data_ptr<float>(), hid_out.data_ptr<float>(),
                       B, (int)max_learn, (int)H, block_len, (int)spb);

    return {obs_out, la_out, lr_out, act_out, nsr_out, gam_out, w_out, hid_out};
}

// Float row store (vector observations): same outputs as replay_gather_batch
// with obs_out (B, T, D) float32, copied by gather_rows_f32_kernel, one
// workgroup per sample.  `out`, when given, holds the eight output tensors
// preallocated by the caller (contiguous, shapes as returned); they are
// checked like the inputs and nothing is written before every check passed.
std::vector<torch::Tensor> replay_gather_batch_vec(
    torch::Tensor obs_store, torch::Tensor la_store, torch::Tensor lr_store,
    torch::Tensor act_store, torch::Tensor nsr_store, torch::Tensor gam_store,
    torch::Tensor hid_store, torch::Tensor idx, torch::Tensor meta,
    torch::Tensor seg, torch::Tensor weights, int64_t T, int64_t A,
    int64_t max_learn, int64_t H, int64_t spb,
    c10::optional<std::vector<torch::Tensor>> out) {
    TORCH_CHECK(obs_store.is_cuda() && la_store.is_cuda() && lr_store.is_cuda()
                && act_store.is_cuda() && nsr_store.is_cuda()
                && gam_store.is_cuda() && hid_store.is_cuda() && idx.is_cuda()
                && meta.is_cuda() && seg.is_cuda() && weights.is_cuda(),
                "replay_gather_batch_vec: every tensor must be on the GPU");
    TORCH_CHECK(obs_store.dtype() == torch::kFloat32,
                "replay_gather_batch_vec: the obs store must be float32");
    TORCH_CHECK(la_store.dtype() == torch::kUInt8
                && act_store.dtype() == torch::kUInt8,
                "replay_gather_batch_vec: la/act stores must be uint8");
    TORCH_CHECK(lr_store.dtype() == torch::kFloat32
                && nsr_store.dtype() == torch::kFloat32
                && gam_store.dtype() == torch::kFloat32
                && hid_store.dtype() == torch::kFloat32
                && weights.dtype() == torch::kFloat32,
                "replay_gather_batch_vec: lr/nsr/gam/hid/weights must be "
                "float32");
    TORCH_CHECK(idx.dtype() == torch::kInt64 && meta.dtype() == torch::kInt32
                && seg.dtype() == torch::kInt32,
                "replay_gather_batch_vec: idx int64, meta/seg int32");
    TORCH_CHECK(obs_store.is_contiguous() && la_store.is_contiguous()
                && lr_store.is_contiguous() && act_store.is_contiguous()
                && nsr_store.is_contiguous() && gam_store.is_contiguous()
                && hid_store.is_contiguous() && idx.is_contiguous()
                && meta.is_contiguous() && seg.is_contiguous()
                && weights.is_contiguous(),
                "replay_gather_batch_vec: every tensor must be contiguous");
    TORCH_CHECK(obs_store.dim() == 3 && la_store.dim() == 2
                && lr_store.dim() == 2 && act_store.dim() == 2
                && idx.dim() == 1,
                "replay_gather_batch_vec: obs store (num_blocks, obs_rows, D),"
                " la/lr/act stores 2-d, idx 1-d");
    TORCH_CHECK(obs_store.size(0) == la_store.size(0)
                && obs_store.size(1) == la_store.size(1)
                && lr_store.sizes() == la_store.sizes()
                && act_store.size(0) == la_store.size(0)
                && nsr_store.sizes() == act_store.sizes()
                && gam_store.sizes() == act_store.sizes(),
                "replay_gather_batch_vec: store shapes disagree");
    int64_t B64 = idx.size(0);
    TORCH_CHECK(B64 >= 1 && B64 <= 1024, "replay_gather_batch_vec: B must be "
                "in [1, 1024], got ", B64);
    int B = (int)B64;
    long D = obs_store.size(2);
    TORCH_CHECK(D >= 1, "replay_gather_batch_vec: D must be >= 1, got ", D);
    TORCH_CHECK(A >= 1 && A <= 256, "replay_gather_batch_vec: A must be in "
                "[1, 256], got ", A);
    TORCH_CHECK(meta.dim() == 2 && meta.size(0) == 5 && meta.size(1) == B
                && seg.numel() == B + 1 && weights.numel() == B,
                "replay_gather_batch_vec: meta (5, B), seg (B + 1,), "
                "weights (B,)");
    TORCH_CHECK(T >= 1 && max_learn >= 1 && H >= 1 && spb >= 1);
    TORCH_CHECK(T * D < (1L << 31) && T * A < (1L << 31)
                && (long)B * max_learn < (1L << 31));
    TORCH_CHECK(hid_store.dim() == 2 && hid_store.size(1) == 2 * H
                && hid_store.size(0) == la_store.size(0) * spb,
                "replay_gather_batch_vec: hid store must be "
                "(num_blocks * spb, 2 * H)");
    long total_rows = obs_store.size(0) * obs_store.size(1);
    long block_len = act_store.size(1);
    long Rmax = (long)B * max_learn;
    auto f32 = lr_store.options();
    auto i64 = idx.options();
    torch::Tensor obs_out, la_out, lr_out, act_out, nsr_out, gam_out, w_out,
        hid_out;
    if (out.has_value()) {
        auto& o = *out;
        TORCH_CHECK(o.size() == 8, "replay_gather_batch_vec: out must hold the"
                    " eight output tensors, got ", o.size());
        const std::vector<int64_t> shapes[8] = {
            {B, T, D}, {B, T, A}, {B, T}, {Rmax}, {Rmax}, {Rmax}, {Rmax},
            {2, B, H}};
        for (int k = 0; k < 8; ++k) {
            TORCH_CHECK(o[k].is_cuda() && o[k].is_contiguous()
                        && o[k].dtype() == (k == 3 ? torch::kInt64
                                                   : torch::kFloat32)
                        && o[k].sizes() == c10::IntArrayRef(shapes[k]),
                        "replay_gather_batch_vec: out[", k, "] must be a "
                        "contiguous GPU tensor of the returned shape and "
                        "dtype");
        }
        obs_out = o[0]; la_out = o[1]; lr_out = o[2]; act_out = o[3];
        nsr_out = o[4]; gam_out = o[5]; w_out = o[6]; hid_out = o[7];
    } else {
        obs_out = torch::empty({B, T, D}, f32);
        la_out = torch::empty({B, T, A}, f32);
        lr_out = torch::empty({B, T}, f32);
        act_out = torch::empty({Rmax}, i64);
        nsr_out = torch::empty({Rmax}, f32);
        gam_out = torch::empty({Rmax}, f32);
        w_out = torch::empty({Rmax}, f32);
        hid_out = torch::empty({2, B, H}, f32);
    }
    auto stream = at::cuda::getCurrentCUDAStream();

    // 16-byte moves need D % 4 == 0 (every row offset a multiple of 16 bytes)
    // and both bases aligned: allocator bases are, a caller's view may not be
    bool vec4 = D % 4 == 0
        && reinterpret_cast<uintptr_t>(obs_store.data_ptr<float>()) % 16 == 0
        && reinterpret_cast<uintptr_t>(obs_out.data_ptr<float>()) % 16 == 0;
    auto rows = vec4 ? gather_rows_f32_kernel<true>
                     : gather_rows_f32_kernel<false>;
    hipLaunchKernelGGL(rows, dim3(B), dim3(256), 0, stream.stream(),
                       obs_store.data_ptr<float>(),
                       la_store.data_ptr<unsigned char>(),
                       lr_store.data_ptr<float>(), meta.data_ptr<int>(),
                       obs_out.data_ptr<float>(), la_out.data_ptr<float>(),
                       lr_out.data_ptr<float>(), B, (int)T, (int)A, D,
                       total_rows);

    int total = B * (int)max_learn;
    hipLaunchKernelGGL(gather_flat_kernel, dim3((total + 255) / 256), dim3(256),
                       0, stream.stream(), act_store.data_ptr<unsigned char>(),
                       nsr_store.data_ptr<float>(), gam_store.data_ptr<float>(),
                       hid_store.data_ptr<float>(), idx.data_ptr<long>(),
                       meta.data_ptr<int>(), seg.data_ptr<int>(),
                       weights.data_ptr<float>(), act_out.data_ptr<long>(),
                       nsr_out.data_ptr<float>(), gam_out.data_ptr<float>(),
                       w_out.data_ptr<float>(), hid_out.data_ptr<float>(),
                       B, (int)max_learn, (int)H, block_len, (int)spb);

    return {obs_out, la_out, lr_out, act_out, nsr_out, gam_out, w_out, hid_out};
}
