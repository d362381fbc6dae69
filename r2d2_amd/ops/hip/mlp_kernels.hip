// First layer of the MLP encoder for vector observations (gfx950, wave64).
//
// MLPEncoder is relu(fc2(relu(fc1(x)))).  fc2 (512 -> 512) is a shape the MFMA
// GEMMs in gemm_kernels.hip already serve.  fc1 reduces over the observation
// width D (4 for CartPole), far below the GEMMs' K % 32 == 0 granule, so it
// gets two plain-VALU kernels that keep X, W1 and the accumulation in f32:
//
//   mlp_in_fwd         A1 = relu(X . W1^T + b1), rounded to bf16 once
//   mlp_in_wgrad_into  dW1 += dA1^T . X, db1 += column sums of dA1
//
// Both are bound by the (M, 512) bf16 tensor they stream (written by the
// forward, read by the wgrad); the f32 operands are a few kilobytes.  There is
// no dgrad: the input is data.  Design notes and compiler figures:
// docs/KERNELS.md.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

constexpr int MLP_N = 512;            // fc1 output width (fixed)
constexpr int MLP_DMAX = 16;          // widest observation served
constexpr int MLP_FWD_ROWS = 16;      // rows per forward workgroup
constexpr int MLP_FWD_COLS = 4;       // columns per forward thread
constexpr int MLP_WG_ROWS = 64;       // wgrad row-chunk granule
constexpr int MLP_WG_COLS = 2;        // columns per wgrad thread
constexpr int MLP_WG_MAX_WGS = 256;   // one workgroup per CU at the most

// ---------------------------------------------------------------------------
// mlp_in_fwd.  256 threads; thread t owns the 4 columns 4 * (t % 128) of row
// parity t / 128, with its W1 rows (4 x D f32) and biases in registers.  A
// workgroup walks MLP_FWD_ROWS rows two at a time; each wave stores 512
// contiguous bytes of a row per pass (8 bytes per lane).  The X row is one
// address for the whole half-workgroup, read element by element (rows are
// 4 * D bytes: no alignment beyond 4 is assumed).  Slots d >= D hold zeros on
// both sides, so the unrolled 16-step chain adds exact zeros after the D real
// terms.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_in_fwd_kernel(
    const float* __restrict__ X,        // (M, D)
    const float* __restrict__ W1,       // (512, D)
    const float* __restrict__ b1,       // (512,)
    __hip_bfloat16* __restrict__ A1,    // (M, 512)
    long M, int D) {
    int col0 = (threadIdx.x & 127) * MLP_FWD_COLS;
    int rpar = threadIdx.x >> 7;

    float w[MLP_FWD_COLS][MLP_DMAX];
    float bias[MLP_FWD_COLS];
#pragma unroll
    for (int c = 0; c < MLP_FWD_COLS; ++c) {
        bias[c] = b1[col0 + c];
#pragma unroll
        for (int d = 0; d < MLP_DMAX; ++d)
            w[c][d] = (d < D) ? W1[(long)(col0 + c) * D + d] : 0.f;
    }

    long row0 = (long)blockIdx.x * MLP_FWD_ROWS;
    long rend = min(M, row0 + MLP_FWD_ROWS);
    for (long r = row0 + rpar; r < rend; r += 2) {
        const float* xr = X + r * D;
        float x[MLP_DMAX];
#pragma unroll
        for (int d = 0; d < MLP_DMAX; ++d) x[d] = (d < D) ? xr[d] : 0.f;
        union { __hip_bfloat16 h[MLP_FWD_COLS]; uint2 u; } pk;
#pragma unroll
        for (int c = 0; c < MLP_FWD_COLS; ++c) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < MLP_DMAX; ++d) acc = fmaf(x[d], w[c][d], acc);
            acc += bias[c];
            pk.h[c] = f2bf(acc > 0.f ? acc : 0.f);   // relu zeros are +0
        }
        *reinterpret_cast<uint2*>(A1 + r * MLP_N + col0) = pk.u;
    }
}

// ---------------------------------------------------------------------------
// mlp_in_wgrad_into.  Each workgroup takes a chunk of rows (a multiple of
// MLP_WG_ROWS, grown until the grid is at most MLP_WG_MAX_WGS workgroups: every
// workgroup adds into the same 512 * (D + 1) addresses and those atomics
// serialise, so the grid stays inside one resident round).  Thread t owns
// columns 2t, 2t + 1 and keeps 2 * (D + 1) f32 partial sums in registers over
// the whole chunk: its dA1 reads are 4 bytes, 256 contiguous bytes per wave,
// and the X row is the same address for every lane.  One f32 atomic per
// output element and workgroup at the end, into views the caller pre-zeroed
// (or wants added to).  dA1 arrives already masked by fc1's ReLU.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_in_wgrad_kernel(
    const __hip_bfloat16* __restrict__ dA1,  // (M, 512)
    const float* __restrict__ X,             // (M, D)
    float* __restrict__ dW1,                 // (512, D) accumulate
    float* __restrict__ db1,                 // (512,) accumulate
    long M, int D, long rows_per_chunk) {
    int col0 = threadIdx.x * MLP_WG_COLS;
    long mstart = (long)blockIdx.x * rows_per_chunk;
    long mend = min(M, mstart + rows_per_chunk);

    float acc[MLP_WG_COLS][MLP_DMAX] = {};
    float bacc[MLP_WG_COLS] = {};
    for (long m = mstart; m < mend; ++m) {
        unsigned int raw =
            *reinterpret_cast<const unsigned int*>(dA1 + m * MLP_N + col0);
        // bf16 -> f32 is a 16-bit shift
        float g0 = __uint_as_float(raw << 16);
        float g1 = __uint_as_float(raw & 0xffff0000u);
        const float* xr = X + m * D;
        bacc[0] += g0;
        bacc[1] += g1;
#pragma unroll
        for (int d = 0; d < MLP_DMAX; ++d) {
            float x = (d < D) ? xr[d] : 0.f;
            acc[0][d] = fmaf(g0, x, acc[0][d]);
            acc[1][d] = fmaf(g1, x, acc[1][d]);
        }
    }
#pragma unroll
    for (int c = 0; c < MLP_WG_COLS; ++c) {
        atomicAdd(&db1[col0 + c], bacc[c]);
#pragma unroll
        for (int d = 0; d < MLP_DMAX; ++d)
            if (d < D) atomicAdd(&dW1[(long)(col0 + c) * D + d], acc[c][d]);
    }
}

// ---------------------------------------------------------------------------
// Host wrappers.  Every operand is checked before anything is launched or
// allocated, so a rejected call leaves the outputs untouched.
// ---------------------------------------------------------------------------
static void mlp_check_x(const torch::Tensor& X, const char* what) {
    TORCH_CHECK(X.is_cuda(), what, ": X must be a device tensor");
    TORCH_CHECK(X.dtype() == torch::kFloat32, what, ": X must be float32");
    TORCH_CHECK(X.dim() == 2 && X.is_contiguous(), what,
                ": X must be a contiguous (M, D) tensor");
    TORCH_CHECK(X.size(0) >= 1, what, ": M must be at least 1");
    TORCH_CHECK(X.size(1) >= 1 && X.size(1) <= MLP_DMAX, what,
                ": the observation width D must be in 1..16, got ", X.size(1));
}

torch::Tensor mlp_in_fwd(torch::Tensor X, torch::Tensor W1, torch::Tensor b1) {
    mlp_check_x(X, "mlp_in_fwd");
    long M = X.size(0), D = X.size(1);
    TORCH_CHECK(W1.is_cuda() && W1.dtype() == torch::kFloat32
                && W1.dim() == 2 && W1.is_contiguous(),
                "mlp_in_fwd: W1 must be a contiguous float32 device tensor");
    TORCH_CHECK(W1.size(0) == MLP_N,
                "mlp_in_fwd: N must be 512, got ", W1.size(0));
    TORCH_CHECK(W1.size(1) == D, "mlp_in_fwd: W1 must be (512, D)");
    TORCH_CHECK(b1.is_cuda() && b1.dtype() == torch::kFloat32
                && b1.dim() == 1 && b1.is_contiguous()
                && b1.size(0) == MLP_N,
                "mlp_in_fwd: b1 must be a contiguous float32 (512,) device "
                "tensor");
    TORCH_CHECK(W1.get_device() == X.get_device()
                && b1.get_device() == X.get_device(),
                "mlp_in_fwd: operands on different devices");
    auto A1 = torch::empty({M, (long)MLP_N},
                           X.options().dtype(torch::kBFloat16));
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(mlp_in_fwd_kernel, dim3(cdiv(M, MLP_FWD_ROWS)),
                       dim3(256), 0, stream.stream(), X.data_ptr<float>(),
                       W1.data_ptr<float>(), b1.data_ptr<float>(),
                       reinterpret_cast<__hip_bfloat16*>(A1.data_ptr()), M,
                       (int)D);
    return A1;
}

void mlp_in_wgrad_into(torch::Tensor dA1, torch::Tensor X,
                       torch::Tensor dW1_out, torch::Tensor db1_out) {
    mlp_check_x(X, "mlp_in_wgrad_into");
    long M = X.size(0), D = X.size(1);
    TORCH_CHECK(dA1.is_cuda() && dA1.dtype() == torch::kBFloat16
                && dA1.dim() == 2 && dA1.is_contiguous(),
                "mlp_in_wgrad_into: dA1 must be a contiguous bfloat16 device "
                "tensor");
    TORCH_CHECK(dA1.size(1) == MLP_N,
                "mlp_in_wgrad_into: N must be 512, got ", dA1.size(1));
    TORCH_CHECK(dA1.size(0) == M,
                "mlp_in_wgrad_into: dA1 and X differ in M");
    TORCH_CHECK(dW1_out.is_cuda() && dW1_out.dtype() == torch::kFloat32
                && dW1_out.dim() == 2 && dW1_out.is_contiguous()
                && dW1_out.size(0) == MLP_N && dW1_out.size(1) == D,
                "mlp_in_wgrad_into: dW1 must be a contiguous float32 (512, D) "
                "device tensor");
    TORCH_CHECK(db1_out.is_cuda() && db1_out.dtype() == torch::kFloat32
                && db1_out.dim() == 1 && db1_out.is_contiguous()
                && db1_out.size(0) == MLP_N,
                "mlp_in_wgrad_into: db1 must be a contiguous float32 (512,) "
                "device tensor");
    TORCH_CHECK(dA1.get_device() == X.get_device()
                && dW1_out.get_device() == X.get_device()
                && db1_out.get_device() == X.get_device(),
                "mlp_in_wgrad_into: operands on different devices");
    // whole granules per chunk, at most MLP_WG_MAX_WGS chunks
    long per = (M + MLP_WG_MAX_WGS - 1) / MLP_WG_MAX_WGS;
    long rows_per_chunk =
        std::max(1L, (per + MLP_WG_ROWS - 1) / MLP_WG_ROWS) * MLP_WG_ROWS;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(mlp_in_wgrad_kernel, dim3(cdiv(M, rows_per_chunk)),
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<const __hip_bfloat16*>(dA1.data_ptr()),
                       X.data_ptr<float>(), dW1_out.data_ptr<float>(),
                       db1_out.data_ptr<float>(), M, (int)D, rows_per_chunk);
}
