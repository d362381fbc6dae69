// MFMA GEMM kernels for the R2D2 network's dense layers (gfx950).
//
// C(M,N) = A(M,K) @ W^T + bias, optional ReLU.  Weights are prepacked
// row-major as Wt(N,K) so both A and B fragments load 8 CONTIGUOUS bf16
// (16 B) per lane — the mfma_f32_16x16x32_bf16 operand layout puts 8
// consecutive k-elements in each lane (A: row = lane&15; B: col = lane&15;
// k = (lane>>4)*8 + j).  Replaces hipBLASLt/eager Linear for the encoder FC
// (3136->512), the dueling heads, and the LSTM gate GEMMs.
//
// Structure: 4-wave workgroups throughout.  Small shapes (head outputs,
// actor inference) run 64x64 block tiles whose waves load their fragments
// straight from global memory.  The large forward and dgrad GEMMs share one
// LDS-staged core (nt_core): k-tiles of 64 fetched in whole 128-byte lines,
// padded LDS rows, two buffers with the next tile's loads in flight under the
// current tile's MFMAs, one barrier per k-tile, and an epilogue that goes
// through LDS to store 16 bytes per lane.  The large wgrads use the same
// pipeline over the m axis with a 128x64 output tile.  Tile table, dispatch
// rule and measurements: docs/KERNELS.md.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

// ---------------------------------------------------------------------------
// gemm_bias_act: out(M,N) = act(A(M,K) @ Wt(N,K)^T + bias)
//   OUT_F32: write f32 (head outputs feeding the loss kernel) else bf16.
//   ACT: 0 none, 1 relu.
// ---------------------------------------------------------------------------
template <int ACT, bool HAS_BIAS, bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_bias_act_kernel(
    const __hip_bfloat16* __restrict__ A,   // (M, K)
    const __hip_bfloat16* __restrict__ Wt,  // (N, K)
    const float* __restrict__ bias,         // (N,)
    void* __restrict__ out,                 // (M, N) bf16 or f32
    int M, int N, int K) {
    // block tile 64x64: wave w covers rows [wr*32, +32), cols [wc*32, +32)
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    long row0 = (long)blockIdx.x * 64 + wr * 32;
    long col0 = (long)blockIdx.y * 64 + wc * 32;

    int frow = lane & 15;            // fragment row (A) / col (B)
    int kseg = (lane >> 4) * 8;      // k offset of this lane's 8 elements

    f32x4 acc[2][2] = {};
    for (int k0 = 0; k0 < K; k0 += 32) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            long r = row0 + i * 16 + frow;
            a[i] = (r < M) ? load_bf16x8(A + r * K + k0 + kseg) : zero_bf16x8();
            long c = col0 + i * 16 + frow;
            b[i] = (c < N) ? load_bf16x8(Wt + c * K + k0 + kseg) : zero_bf16x8();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[i], b[j], acc[i][j], 0, 0, 0);
    }

    // C/D layout: col = lane&15, row = (lane>>4)*4 + r
    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long rr = row0 + i * 16 + crow + r;
                long cc = col0 + j * 16 + ccol;
                if (rr < M && cc < N) {
                    float v = acc[i][j][r];
                    if (HAS_BIAS) v += bias[cc];
                    if (ACT == 1) v = fmaxf(v, 0.f);
                    if (OUT_F32)
                        reinterpret_cast<float*>(out)[rr * N + cc] = v;
                    else
                        reinterpret_cast<__hip_bfloat16*>(out)[rr * N + cc] =
                            f2bf(v);
                }
            }
}

// ---------------------------------------------------------------------------
// gemm_dgrad: dA(M,K) = dY(M,N) @ W(K,N)^T-with-W-stored-(K,N)... i.e.
//   dA[m][k] = sum_n dY[m][n] * W[k][n], W prepacked row-major (K, N).
//   RELU_MASK: multiply dY by (act_out > 0) on load (fused ReLU backward,
//   act_out is the forward output of this layer, same shape as dY).
//   OUT_MASK: multiply dA by (outm > 0) on store — fuses the ReLU backward
//   of the layer BELOW (e.g. conv3's mask applied to the FC dgrad output),
//   so no separate elementwise mask pass runs on the big dX tensors.
// ---------------------------------------------------------------------------
template <bool RELU_MASK, bool OUT_MASK = false>
__global__ __launch_bounds__(256) void gemm_dgrad_kernel(
    const __hip_bfloat16* __restrict__ dY,      // (M, N)
    const __hip_bfloat16* __restrict__ act,     // (M, N) or null
    const __hip_bfloat16* __restrict__ W,       // (K, N) row-major
    __hip_bfloat16* __restrict__ dA,            // (M, K)
    const __hip_bfloat16* __restrict__ outm,    // (M, Kout) or null
    int M, int N, int K, int Kout) {
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    long row0 = (long)blockIdx.x * 64 + wr * 32;   // m
    long col0 = (long)blockIdx.y * 64 + wc * 32;   // k (output feature dim)
    int frow = lane & 15;
    int nseg = (lane >> 4) * 8;

    f32x4 acc[2][2] = {};
    for (int n0 = 0; n0 < N; n0 += 32) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            long r = row0 + i * 16 + frow;
            if (r < M) {
                a[i] = load_bf16x8(dY + r * N + n0 + nseg);
                if (RELU_MASK) {
                    bf16x8 mv = load_bf16x8(act + r * N + n0 + nseg);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float vv = (float)a[i][e];
                        a[i][e] = (__bf16)(((float)mv[e] > 0.f) ? vv : 0.f);
                    }
                }
            } else {
                a[i] = zero_bf16x8();
            }
            long c = col0 + i * 16 + frow;
            b[i] = (c < K) ? load_bf16x8(W + c * N + n0 + nseg) : zero_bf16x8();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[i], b[j], acc[i][j], 0, 0, 0);
    }
    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long rr = row0 + i * 16 + crow + r;
                long cc = col0 + j * 16 + ccol;
                if (rr < M && cc < Kout) {
                    float v = acc[i][j][r];
                    if (OUT_MASK)
                        v = (bf2f(outm[rr * Kout + cc]) > 0.f) ? v : 0.f;
                    dA[rr * Kout + cc] = f2bf(v);
                }
            }
}

// ---------------------------------------------------------------------------
// LDS-staged NT core shared by the large forward and dgrad GEMMs.
//
// Both are C(M,Nc) = X(M,K) . Y(Nc,K)^T with the two operands contiguous
// along the reduction axis (forward: X = A, Y = Wt; dgrad: X = dY, Y = W).
// A 256-thread workgroup owns a BM x BN tile, its four waves a 2x2 grid of
// (BM/2) x (BN/2) sub-tiles.  The reduction runs in k-tiles of 64: every
// global row segment is one full 128-byte line, fetched as eight 16-byte
// pieces by eight neighbouring lanes, and lands in LDS rows padded to 64 + 8
// elements, from which the MFMA fragments are read back as 8 contiguous
// k-elements per lane (the operand layout of the 64x64 kernels above).
//
// Two LDS buffers: the loads of k-tile t+1 are issued into registers before
// the MFMAs of k-tile t and written to the other buffer after them, with one
// __syncthreads per k-tile.  K is a multiple of 32: an odd count of 32-chunks
// ends in a half tile that issues one MFMA step instead of two.
//
// Every output element keeps ONE accumulator fed by mfma_f32_16x16x32_bf16
// over k0 = 0, 32, 64, ... ascending — the chain of the 64x64 kernels, so
// results are bit-equal to theirs.
// ---------------------------------------------------------------------------
constexpr int NT_KT = 64;            // k-tile
constexpr int NT_LD = NT_KT + 8;     // padded LDS row stride (elements)
constexpr int NT_CPAD = 4;           // f32 epilogue tile row padding

template <int BM, int BN>
struct NtTile {
    static constexpr int FM = BM / 32;                      // frags per wave, m
    static constexpr int FN = BN / 32;                      // frags per wave, n
    static constexpr int X_PIECES = BM * NT_KT / 8 / 256;   // 16 B per thread
    static constexpr int Y_PIECES = BN * NT_KT / 8 / 256;
    static constexpr int STAGE = (BM + BN) * NT_LD;         // elements / buffer
    static constexpr int LDS_ELEMS = 2 * STAGE;
    static_assert(BM * (BN + NT_CPAD) * 4 <= LDS_ELEMS * 2,
                  "epilogue tile must fit in the operand buffers");
};

// Issue the 16-byte loads of one k-tile of ROWS rows.  Out-of-range pieces
// (row >= nrows, or the upper half of a half tile) load from the tensor base
// instead, so every load is unconditional; nt_stage zeroes them.
template <int PIECES>
__device__ __forceinline__ void nt_fetch(const __hip_bfloat16* __restrict__ P,
                                         long row0, long nrows, int K, int k0,
                                         bf16x8 (&v)[PIECES]) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        int p = threadIdx.x + i * 256;
        long r = row0 + (p >> 3);
        int k = k0 + (p & 7) * 8;
        bool ok = (r < nrows) && (k < K);
        v[i] = load_bf16x8(ok ? P + r * K + k : P);
    }
}

template <int PIECES, bool RELU_MASK>
__device__ __forceinline__ void nt_stage(__hip_bfloat16* s, long row0,
                                         long nrows, int K, int k0,
                                         bf16x8 (&v)[PIECES],
                                         bf16x8 (&mv)[PIECES]) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        int p = threadIdx.x + i * 256;
        int rl = p >> 3, kc = (p & 7) * 8;
        bool ok = (row0 + rl < nrows) && (k0 + kc < K);
        bf16x8 x = v[i];
        if (RELU_MASK) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float vv = (float)x[e];
                x[e] = (__bf16)(((float)mv[i][e] > 0.f) ? vv : 0.f);
            }
        }
        *reinterpret_cast<bf16x8*>(s + rl * NT_LD + kc) =
            ok ? x : zero_bf16x8();
    }
}

// acc += X[row0.., :] . Y[col0.., :]^T over the whole reduction axis.
// RELU_MASK multiplies X by (xmask > 0) once, as the tile is staged.
template <int BM, int BN, bool RELU_MASK>
__device__ __forceinline__ void nt_core(
    const __hip_bfloat16* __restrict__ X,      // (M, K)
    const __hip_bfloat16* __restrict__ xmask,  // (M, K) or null
    const __hip_bfloat16* __restrict__ Y,      // (>= Nc, K)
    long M, long Nc, int K, long row0, long col0,
    __hip_bfloat16* smem, f32x4 (&acc)[BM / 32][BN / 32]) {
    using T = NtTile<BM, BN>;
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    int frow = lane & 15;
    int kseg = (lane >> 4) * 8;

    bf16x8 xr[T::X_PIECES], mr[T::X_PIECES], yr[T::Y_PIECES];
    int nt = (K + NT_KT - 1) / NT_KT;

    nt_fetch<T::X_PIECES>(X, row0, M, K, 0, xr);
    if (RELU_MASK) nt_fetch<T::X_PIECES>(xmask, row0, M, K, 0, mr);
    nt_fetch<T::Y_PIECES>(Y, col0, Nc, K, 0, yr);
    nt_stage<T::X_PIECES, RELU_MASK>(smem, row0, M, K, 0, xr, mr);
    nt_stage<T::Y_PIECES, false>(smem + BM * NT_LD, col0, Nc, K, 0, yr, yr);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        int k0 = t * NT_KT;
        const __hip_bfloat16* sx = smem + (t & 1) * T::STAGE;
        const __hip_bfloat16* sy = sx + BM * NT_LD;
        bool more = (t + 1 < nt);
        if (more) {
            nt_fetch<T::X_PIECES>(X, row0, M, K, k0 + NT_KT, xr);
            if (RELU_MASK)
                nt_fetch<T::X_PIECES>(xmask, row0, M, K, k0 + NT_KT, mr);
            nt_fetch<T::Y_PIECES>(Y, col0, Nc, K, k0 + NT_KT, yr);
        }
        int ksteps = (K - k0 >= NT_KT) ? 2 : 1;     // half-tile tail
        for (int ks = 0; ks < ksteps; ++ks) {
            bf16x8 a[T::FM], b[T::FN];
#pragma unroll
            for (int i = 0; i < T::FM; ++i)
                a[i] = *reinterpret_cast<const bf16x8*>(
                    sx + (wr * (BM / 2) + i * 16 + frow) * NT_LD
                    + ks * 32 + kseg);
#pragma unroll
            for (int j = 0; j < T::FN; ++j)
                b[j] = *reinterpret_cast<const bf16x8*>(
                    sy + (wc * (BN / 2) + j * 16 + frow) * NT_LD
                    + ks * 32 + kseg);
#pragma unroll
            for (int i = 0; i < T::FM; ++i)
#pragma unroll
                for (int j = 0; j < T::FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            __hip_bfloat16* dx = smem + ((t + 1) & 1) * T::STAGE;
            nt_stage<T::X_PIECES, RELU_MASK>(dx, row0, M, K, k0 + NT_KT,
                                             xr, mr);
            nt_stage<T::Y_PIECES, false>(dx + BM * NT_LD, col0, Nc, K,
                                         k0 + NT_KT, yr, yr);
        }
        __syncthreads();
    }
}

// Wide epilogue: the accumulators go through LDS (the operand buffers are
// free after the k loop's last barrier) so that each lane owns 8 consecutive
// columns of one row and stores them as 16 bytes (32 for f32 output).  Bias,
// ReLU and the output mask are applied on the way, per element in the order
// of the 64x64 kernels.  A column count that is no multiple of 8 leaves rows
// unaligned; it takes the per-element store instead.
template <int BM, int BN, int ACT, bool HAS_BIAS, bool OUT_F32, bool OUT_MASK>
__device__ __forceinline__ void nt_epilogue(
    f32x4 (&acc)[BM / 32][BN / 32], __hip_bfloat16* smem,
    const float* __restrict__ bias,           // (Nc,) or null
    const __hip_bfloat16* __restrict__ outm,  // (M, Nc) or null
    void* __restrict__ out,                   // (M, Nc)
    long M, long Nc, long row0, long col0) {
    constexpr int LDC = BN + NT_CPAD;
    float* sc = reinterpret_cast<float*>(smem);
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
#pragma unroll
        for (int j = 0; j < BN / 32; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sc[(wr * (BM / 2) + i * 16 + crow + r) * LDC
                   + wc * (BN / 2) + j * 16 + ccol] = acc[i][j][r];
    __syncthreads();

    constexpr int TPR = BN / 8;               // threads per row
    constexpr int RPP = 256 / TPR;            // rows per pass
    int tc = (threadIdx.x % TPR) * 8;
    int tr = threadIdx.x / TPR;
    long cc = col0 + tc;
    bool wide = (Nc % 8 == 0);
    if (cc >= Nc) return;
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        bv[e] = (HAS_BIAS && cc + e < Nc) ? bias[cc + e] : 0.f;
#pragma unroll
    for (int ps = 0; ps < BM / RPP; ++ps) {
        int rl = ps * RPP + tr;
        long rr = row0 + rl;
        if (rr >= M) break;
        float v[8];
        *reinterpret_cast<f32x4*>(&v[0]) =
            *reinterpret_cast<const f32x4*>(sc + rl * LDC + tc);
        *reinterpret_cast<f32x4*>(&v[4]) =
            *reinterpret_cast<const f32x4*>(sc + rl * LDC + tc + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (HAS_BIAS) v[e] += bv[e];
            if (ACT == 1) v[e] = fmaxf(v[e], 0.f);
        }
        long o = rr * Nc + cc;
        if (wide) {
            if (OUT_MASK) {
                bf16x8 m = load_bf16x8(outm + o);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    v[e] = ((float)m[e] > 0.f) ? v[e] : 0.f;
            }
            if (OUT_F32) {
                float* op = reinterpret_cast<float*>(out) + o;
                *reinterpret_cast<f32x4*>(op) =
                    *reinterpret_cast<f32x4*>(&v[0]);
                *reinterpret_cast<f32x4*>(op + 4) =
                    *reinterpret_cast<f32x4*>(&v[4]);
            } else {
                union { __hip_bfloat16 h[8]; uint4 u; } pk;
#pragma unroll
                for (int e = 0; e < 8; ++e) pk.h[e] = f2bf(v[e]);
                *reinterpret_cast<uint4*>(
                    reinterpret_cast<__hip_bfloat16*>(out) + o) = pk.u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (cc + e >= Nc) break;
                float x = v[e];
                if (OUT_MASK) x = (bf2f(outm[o + e]) > 0.f) ? x : 0.f;
                if (OUT_F32)
                    reinterpret_cast<float*>(out)[o + e] = x;
                else
                    reinterpret_cast<__hip_bfloat16*>(out)[o + e] = f2bf(x);
            }
        }
    }
}

// forward: out(M,N) = act(A(M,K) @ Wt(N,K)^T + bias)
template <int BM, int BN, int ACT, bool HAS_BIAS, bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_nt_fwd_kernel(
    const __hip_bfloat16* __restrict__ A,   // (M, K)
    const __hip_bfloat16* __restrict__ Wt,  // (N, K)
    const float* __restrict__ bias,         // (N,)
    void* __restrict__ out,                 // (M, N) bf16 or f32
    int M, int N, int K) {
    __shared__ __attribute__((aligned(16)))
        __hip_bfloat16 smem[NtTile<BM, BN>::LDS_ELEMS];
    long row0 = (long)blockIdx.x * BM;
    long col0 = (long)blockIdx.y * BN;
    f32x4 acc[BM / 32][BN / 32] = {};
    nt_core<BM, BN, false>(A, nullptr, Wt, M, N, K, row0, col0, smem, acc);
    nt_epilogue<BM, BN, ACT, HAS_BIAS, OUT_F32, false>(
        acc, smem, bias, nullptr, out, M, N, row0, col0);
}

// dgrad: dA(M,Kout) = (dY * [act > 0])(M,N) @ W(K,N)^T [* (outm > 0)], first
// Kout of the K output columns, dense
template <int BM, int BN, bool RELU_MASK, bool OUT_MASK>
__global__ __launch_bounds__(256) void gemm_nt_dgrad_kernel(
    const __hip_bfloat16* __restrict__ dY,      // (M, N)
    const __hip_bfloat16* __restrict__ act,     // (M, N) or null
    const __hip_bfloat16* __restrict__ W,       // (K, N) row-major
    __hip_bfloat16* __restrict__ dA,            // (M, Kout)
    const __hip_bfloat16* __restrict__ outm,    // (M, Kout) or null
    int M, int N, int Kout) {
    __shared__ __attribute__((aligned(16)))
        __hip_bfloat16 smem[NtTile<BM, BN>::LDS_ELEMS];
    long row0 = (long)blockIdx.x * BM;
    long col0 = (long)blockIdx.y * BN;
    f32x4 acc[BM / 32][BN / 32] = {};
    nt_core<BM, BN, RELU_MASK>(dY, act, W, M, Kout, N, row0, col0, smem, acc);
    nt_epilogue<BM, BN, 0, false, false, OUT_MASK>(
        acc, smem, nullptr, outm, dA, M, Kout, row0, col0);
}

// Tile choice for the NT GEMMs.  path: 0 automatic, GEMM_PATH_64 the unstaged
// 64x64 kernels, GEMM_PATH_S64 / GEMM_PATH_S128 the staged 64x64 / 128x64
// instantiations.  Automatic: small problems (M < 1024 or fewer than 128
// output columns: head outputs, actor inference) keep the unstaged kernel,
// the rest take the staged 64x64 tile.  The 128x64 tile measured 5-25 %
// slower than the staged 64x64 one at every shape the learner runs at
// B = 64 (docs/KERNELS.md), so nothing selects it automatically.
constexpr int64_t GEMM_PATH_64 = 64;
constexpr int64_t GEMM_PATH_S64 = 6464;
constexpr int64_t GEMM_PATH_S128 = 12864;

static int64_t nt_pick_path(long M, long Nc, int64_t path) {
    TORCH_CHECK(path == 0 || path == GEMM_PATH_64 || path == GEMM_PATH_S64
                || path == GEMM_PATH_S128,
                "path must be 0, 64, 6464 or 12864");
    if (path != 0) return path;
    return (M < 1024 || Nc < 128) ? GEMM_PATH_64 : GEMM_PATH_S64;
}

// ---------------------------------------------------------------------------
// gemm_wgrad: dWt(N,K) += dY(M,N)^T @ A(M,K), reduction over M with
// LDS-staged 32-row tiles; row-chunked grid with f32 atomics into dW.
// Also accumulates db(N) = sum_m dY[m][n] when HAS_BIAS.
//   RELU_MASK as in dgrad (applied to dY).
// ---------------------------------------------------------------------------
// KPERM: the k axis is a packed (d0, d1, d2) index (e.g. conv taps (ky, kx,
// cin) or the FC's flattened (h, w, c)); remap each store to torch's
// (d2, d0, d1) order so gradients accumulate STRAIGHT into the module
// .grad views with no per-step permute-copy kernels.
template <bool RELU_MASK, bool HAS_BIAS, bool KPERM = false>
__global__ __launch_bounds__(256) void gemm_wgrad_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (M, N)
    const __hip_bfloat16* __restrict__ act,  // (M, N) or null
    const __hip_bfloat16* __restrict__ A,    // (M, K)
    float* __restrict__ dWt,                 // (N, K) f32 accumulate
    float* __restrict__ db,                  // (N,) f32 accumulate
    int M, int N, int K, int rows_per_chunk, int Nout, int Kout,
    int kd0 = 0, int kd1 = 0, int kd2 = 0) {
    // grid.x: row chunks; grid.y: N tiles of 64; grid.z: K tiles of 64
    __shared__ __hip_bfloat16 s_dy[32][64 + 8];  // [m][n]
    __shared__ __hip_bfloat16 s_a[32][64 + 8];   // [m][k]
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    long mstart = (long)blockIdx.x * rows_per_chunk;
    long mend = min((long)M, mstart + rows_per_chunk);
    long ncol0 = (long)blockIdx.y * 64;
    long kcol0 = (long)blockIdx.z * 64;

    int frow = lane & 15;
    int mseg = (lane >> 4) * 8;

    f32x4 acc[2][2] = {};
    float bias_acc = 0.f;   // lane-partial db for column ncol0 + (tid%64)

    for (long m0 = mstart; m0 < mend; m0 += 32) {
        // stage 32 rows x 64 cols of dY and A into LDS (coalesced)
        __syncthreads();
        // 256 threads, each loads 8 elements: 32*64/8 = 256 loads per tile
        {
            int t = threadIdx.x;
            int mrow = t / 8;           // 0..31
            int ncol = (t % 8) * 8;     // 0..56
            long gm = m0 + mrow;
            bf16x8 v = zero_bf16x8();
            if (gm < mend) {
                if (ncol0 + ncol + 8 <= N) {
                    v = load_bf16x8(dY + gm * N + ncol0 + ncol);
                    if (RELU_MASK) {
                        bf16x8 mv = load_bf16x8(act + gm * N + ncol0 + ncol);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float vv = (float)v[e];
                            v[e] = (__bf16)(((float)mv[e] > 0.f) ? vv : 0.f);
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        long c = ncol0 + ncol + e;
                        float vv = (c < N) ? (float)((const __bf16*)dY)[gm * N + c]
                                           : 0.f;
                        if (RELU_MASK) {
                            float m_ = (c < N)
                                ? (float)((const __bf16*)act)[gm * N + c] : 0.f;
                            vv = (m_ > 0.f) ? vv : 0.f;
                        }
                        v[e] = (__bf16)vv;
                    }
                }
            }
            *reinterpret_cast<bf16x8*>(&s_dy[mrow][ncol]) = v;
            bf16x8 w = zero_bf16x8();
            if (gm < mend) {
                if (kcol0 + ncol + 8 <= K)
                    w = load_bf16x8(A + gm * K + kcol0 + ncol);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        long c = kcol0 + ncol + e;
                        if (c < K) w[e] = ((const __bf16*)A)[gm * K + c];
                    }
                }
            }
            *reinterpret_cast<bf16x8*>(&s_a[mrow][ncol]) = w;
        }
        __syncthreads();

        // MFMA: out tile (n, k); gemm-M = n-dim, gemm-N = k-dim, gemm-K = m
        // A-frag: s_dy column (n = row0 + frow), 8 m values
        // B-frag: s_a column (k), 8 m values — both gathered by hardware
        // transpose-reads (ds_read_b64_tr_b16, common.h lds_col_frag8)
        {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = lds_col_frag8<64 + 8>(&s_dy[0][0], mseg,
                                              wr * 32 + i * 16, lane);
                fb[i] = lds_col_frag8<64 + 8>(&s_a[0][0], mseg,
                                              wc * 32 + i * 16, lane);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (HAS_BIAS) {
            // db: threads 0..63 own column tid%64; sum the 32 rows staged
            int c = threadIdx.x % 64;
            if (threadIdx.x < 64) {
                for (int mr = 0; mr < 32; ++mr)
                    bias_acc += (float)s_dy[mr][c];
            }
        }
    }

    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long nn = ncol0 + wr * 32 + i * 16 + crow + r;
                long kk = kcol0 + wc * 32 + j * 16 + ccol;
                if (nn < Nout && kk < Kout) {
                    if (KPERM) {
                        int d2 = (int)(kk % kd2);
                        int t_ = (int)(kk / kd2);
                        int d1 = t_ % kd1;
                        int d0 = t_ / kd1;
                        kk = ((long)d2 * kd0 + d0) * kd1 + d1;
                    }
                    atomicAdd(&dWt[nn * Kout + kk], acc[i][j][r]);
                }
            }
    if (HAS_BIAS && threadIdx.x < 64 && blockIdx.z == 0) {
        long c = ncol0 + threadIdx.x;
        if (c < Nout) atomicAdd(&db[c], bias_acc);
    }
}

// ---------------------------------------------------------------------------
// gemm_wgrad, large shapes: 128 (n) x 64 (k) output tile per workgroup, each
// wave a 64 x 32 sub-tile (4x2 fragments).  The m axis runs in tiles of 64
// rows through two LDS buffers as in nt_core (loads of tile t+1 issued before
// the MFMAs of tile t, written after them, one barrier per tile), so a wave
// issues 16 MFMAs per barrier.  Fragments come from lds_col_frag8.  The bias
// column sum is taken by all 256 threads (thread t: column t % 128, the upper
// or lower 32 rows of each m-tile) and reduced through LDS: one atomic per
// column and workgroup.  Needs N % 8 == 0 and K % 8 == 0 (whole 16-byte
// pieces).
// ---------------------------------------------------------------------------
constexpr int WG_BN = 128;           // output tile, n
constexpr int WG_BK = 64;            // output tile, k
constexpr int WG_MT = 64;            // m-tile
constexpr int WG_LDY = WG_BN + 8;    // s_dy row stride
constexpr int WG_LDA = WG_BK + 8;    // s_a row stride
constexpr int WG_STAGE = WG_MT * (WG_LDY + WG_LDA);
constexpr int WG_YP = WG_MT * WG_BN / 8 / 256;   // dY pieces per thread
constexpr int WG_AP = WG_MT * WG_BK / 8 / 256;   // A pieces per thread

// pieces of a (WG_MT x COLS) tile: PPR = COLS / 8 pieces per row
template <int PIECES, int COLS>
__device__ __forceinline__ void wg_fetch(const __hip_bfloat16* __restrict__ P,
                                         long m0, long mend, long c0, int ld,
                                         bf16x8 (&v)[PIECES]) {
    constexpr int PPR = COLS / 8;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        int p = threadIdx.x + i * 256;
        long gm = m0 + p / PPR;
        long c = c0 + (p % PPR) * 8;
        bool ok = (gm < mend) && (c < ld);
        v[i] = load_bf16x8(ok ? P + gm * ld + c : P);
    }
}

template <int PIECES, int COLS, int LDE, bool RELU_MASK>
__device__ __forceinline__ void wg_stage(__hip_bfloat16* s, long m0, long mend,
                                         long c0, int ld, bf16x8 (&v)[PIECES],
                                         bf16x8 (&mv)[PIECES]) {
    constexpr int PPR = COLS / 8;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        int p = threadIdx.x + i * 256;
        int rl = p / PPR, cl = (p % PPR) * 8;
        bool ok = (m0 + rl < mend) && (c0 + cl < ld);
        bf16x8 x = v[i];
        if (RELU_MASK) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float vv = (float)x[e];
                x[e] = (__bf16)(((float)mv[i][e] > 0.f) ? vv : 0.f);
            }
        }
        *reinterpret_cast<bf16x8*>(s + rl * LDE + cl) = ok ? x : zero_bf16x8();
    }
}

template <bool RELU_MASK, bool HAS_BIAS, bool KPERM = false>
__global__ __launch_bounds__(256) void gemm_wgrad_tile_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (M, N)
    const __hip_bfloat16* __restrict__ act,  // (M, N) or null
    const __hip_bfloat16* __restrict__ A,    // (M, K)
    float* __restrict__ dWt,                 // (Nout, Kout) f32 accumulate
    float* __restrict__ db,                  // (Nout,) f32 accumulate
    int M, int N, int K, int rows_per_chunk, int Nout, int Kout,
    int kd0 = 0, int kd1 = 0, int kd2 = 0) {
    // grid.x: row chunks; grid.y: N tiles of 128; grid.z: K tiles of 64
    __shared__ __attribute__((aligned(16)))
        __hip_bfloat16 smem[2 * WG_STAGE];
    int wave = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int wr = wave >> 1, wc = wave & 1;
    long mstart = (long)blockIdx.x * rows_per_chunk;
    long mend = min((long)M, mstart + rows_per_chunk);
    long ncol0 = (long)blockIdx.y * WG_BN;
    long kcol0 = (long)blockIdx.z * WG_BK;
    int mseg = (lane >> 4) * 8;
    bool do_bias = HAS_BIAS && blockIdx.z == 0;

    f32x4 acc[4][2] = {};
    float bias_acc = 0.f;   // partial db: column tid % 128, rows of one half
    bf16x8 yr[WG_YP], mr[WG_YP], ar[WG_AP];
    int nt = (int)((mend - mstart + WG_MT - 1) / WG_MT);

    wg_fetch<WG_YP, WG_BN>(dY, mstart, mend, ncol0, N, yr);
    if (RELU_MASK) wg_fetch<WG_YP, WG_BN>(act, mstart, mend, ncol0, N, mr);
    wg_fetch<WG_AP, WG_BK>(A, mstart, mend, kcol0, K, ar);
    wg_stage<WG_YP, WG_BN, WG_LDY, RELU_MASK>(smem, mstart, mend, ncol0, N,
                                              yr, mr);
    wg_stage<WG_AP, WG_BK, WG_LDA, false>(smem + WG_MT * WG_LDY, mstart, mend,
                                          kcol0, K, ar, ar);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        long m1 = mstart + (long)(t + 1) * WG_MT;
        const __hip_bfloat16* sy = smem + (t & 1) * WG_STAGE;
        const __hip_bfloat16* sa = sy + WG_MT * WG_LDY;
        bool more = (t + 1 < nt);
        if (more) {
            wg_fetch<WG_YP, WG_BN>(dY, m1, mend, ncol0, N, yr);
            if (RELU_MASK) wg_fetch<WG_YP, WG_BN>(act, m1, mend, ncol0, N, mr);
            wg_fetch<WG_AP, WG_BK>(A, m1, mend, kcol0, K, ar);
        }
        // out tile (n, k): gemm-M = n, gemm-N = k, gemm-K = m; both operands
        // are columns of the staged tiles, gathered by transpose-reads
#pragma unroll
        for (int ks = 0; ks < WG_MT / 32; ++ks) {
            bf16x8 fa[4], fb[2];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                fa[i] = lds_col_frag8<WG_LDY>(sy, ks * 32 + mseg,
                                              wr * 64 + i * 16, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                fb[j] = lds_col_frag8<WG_LDA>(sa, ks * 32 + mseg,
                                              wc * 32 + j * 16, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (do_bias) {
            int c = threadIdx.x % WG_BN;
            int r0 = (threadIdx.x / WG_BN) * (WG_MT / 2);
#pragma unroll 8
            for (int mr_ = 0; mr_ < WG_MT / 2; ++mr_)
                bias_acc += bf2f(sy[(r0 + mr_) * WG_LDY + c]);
        }
        if (more) {
            __hip_bfloat16* dy_ = smem + ((t + 1) & 1) * WG_STAGE;
            wg_stage<WG_YP, WG_BN, WG_LDY, RELU_MASK>(dy_, m1, mend, ncol0, N,
                                                      yr, mr);
            wg_stage<WG_AP, WG_BK, WG_LDA, false>(dy_ + WG_MT * WG_LDY, m1,
                                                  mend, kcol0, K, ar, ar);
        }
        __syncthreads();
    }

    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long nn = ncol0 + wr * 64 + i * 16 + crow + r;
                long kk = kcol0 + wc * 32 + j * 16 + ccol;
                if (nn < Nout && kk < Kout) {
                    if (KPERM) {
                        int d2 = (int)(kk % kd2);
                        int t_ = (int)(kk / kd2);
                        int d1 = t_ % kd1;
                        int d0 = t_ / kd1;
                        kk = ((long)d2 * kd0 + d0) * kd1 + d1;
                    }
                    atomicAdd(&dWt[nn * Kout + kk], acc[i][j][r]);
                }
            }
    if (do_bias) {
        // the operand buffers are free after the loop's last barrier
        float* sb = reinterpret_cast<float*>(smem);
        if (threadIdx.x >= WG_BN) sb[threadIdx.x - WG_BN] = bias_acc;
        __syncthreads();
        if (threadIdx.x < WG_BN) {
            long c = ncol0 + threadIdx.x;
            if (c < Nout) atomicAdd(&db[c], bias_acc + sb[threadIdx.x]);
        }
    }
}

// Row chunking for the wgrad grids: about `target` workgroups, chunks of whole
// m-tiles of `mt` rows, at least `min_rows` each.  64x64 kernel: ~1024
// workgroups.  Tile kernel: three workgroups are resident per CU (LDS), so
// 768 on 256 CUs is one resident round; chunks shorter than four m-tiles
// spend their time in the pipeline prologue and the atomics (docs/KERNELS.md).
static long wgrad_rows_per_chunk(long M, long tiles, long target, long mt,
                                 long min_rows) {
    long target_chunks = std::max(1L, target / std::max(1L, tiles));
    long rows = std::max(min_rows, (M + target_chunks - 1) / target_chunks);
    return ((rows + mt - 1) / mt) * mt;
}

// path: 0 automatic, 64 the 64x64 kernel, 12864 the 128x64 tile kernel.
// Automatic takes the tile kernel from N >= 128 output rows and M >= 1024
// (the head outputs, N = 32, keep the 64x64 kernel).
static bool wgrad_use_tile(long M, long N, long K, int64_t path) {
    TORCH_CHECK(path == 0 || path == GEMM_PATH_64 || path == GEMM_PATH_S128,
                "wgrad path must be 0, 64 or 12864");
    bool can = (N % 8 == 0) && (K % 8 == 0);
    TORCH_CHECK(can || path != GEMM_PATH_S128,
                "the wgrad tile kernel needs N and K to be multiples of 8");
    if (path != 0) return path == GEMM_PATH_S128;
    return can && M >= 1024 && N >= 128;
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

torch::Tensor gemm_bias_act(torch::Tensor A, torch::Tensor Wt,
                            torch::Tensor bias, int64_t act, bool out_f32,
                            int64_t path) {
    TORCH_CHECK(A.is_cuda() && A.dtype() == torch::kBFloat16 && A.is_contiguous());
    TORCH_CHECK(Wt.dtype() == torch::kBFloat16 && Wt.is_contiguous());
    long M = A.size(0), K = A.size(1), N = Wt.size(0);
    TORCH_CHECK(Wt.size(1) == K && K % 32 == 0, "K must be a multiple of 32");
    bool has_bias = bias.defined() && bias.numel() > 0;
    auto out = torch::empty({M, N}, A.options().dtype(
        out_f32 ? torch::kFloat32 : torch::kBFloat16));
    path = nt_pick_path(M, N, path);
    if (M == 0 || N == 0) return out;
    int bm = (path == GEMM_PATH_S128) ? 128 : 64;
    dim3 grid(cdiv(M, bm), cdiv(N, 64));
    auto stream = at::cuda::getCurrentCUDAStream();
    const float* bptr = has_bias ? bias.data_ptr<float>() : nullptr;
    auto* a = reinterpret_cast<const __hip_bfloat16*>(A.data_ptr());
    auto* w = reinterpret_cast<const __hip_bfloat16*>(Wt.data_ptr());

#define LAUNCH(ACT, HB, OF)                                                    \
    do {                                                                       \
        if (path == GEMM_PATH_S128)                                            \
            hipLaunchKernelGGL((gemm_nt_fwd_kernel<128, 64, ACT, HB, OF>),     \
                               grid, dim3(256), 0, stream.stream(), a, w,      \
                               bptr, out.data_ptr(), (int)M, (int)N, (int)K);  \
        else if (path == GEMM_PATH_S64)                                        \
            hipLaunchKernelGGL((gemm_nt_fwd_kernel<64, 64, ACT, HB, OF>),      \
                               grid, dim3(256), 0, stream.stream(), a, w,      \
                               bptr, out.data_ptr(), (int)M, (int)N, (int)K);  \
        else                                                                   \
            hipLaunchKernelGGL((gemm_bias_act_kernel<ACT, HB, OF>), grid,      \
                               dim3(256), 0, stream.stream(), a, w, bptr,      \
                               out.data_ptr(), (int)M, (int)N, (int)K);        \
    } while (0)
    if (has_bias) {
        if (act == 1) { if (out_f32) LAUNCH(1, true, true); else LAUNCH(1, true, false); }
        else          { if (out_f32) LAUNCH(0, true, true); else LAUNCH(0, true, false); }
    } else {
        if (act == 1) { if (out_f32) LAUNCH(1, false, true); else LAUNCH(1, false, false); }
        else          { if (out_f32) LAUNCH(0, false, true); else LAUNCH(0, false, false); }
    }
#undef LAUNCH
    return out;
}

torch::Tensor gemm_dgrad(torch::Tensor dY, torch::Tensor act_out,
                         torch::Tensor W, bool relu_mask, int64_t k_out,
                         c10::optional<torch::Tensor> out_mask_opt,
                         int64_t path) {
    torch::Tensor out_mask =
        out_mask_opt.has_value() ? *out_mask_opt : torch::Tensor();
    TORCH_CHECK(dY.is_cuda() && dY.dtype() == torch::kBFloat16 && dY.is_contiguous());
    TORCH_CHECK(W.dtype() == torch::kBFloat16 && W.is_contiguous());
    long M = dY.size(0), N = dY.size(1), K = W.size(0);
    TORCH_CHECK(W.size(1) == N && N % 32 == 0, "N must be a multiple of 32");
    // k_out: emit only the first k_out input-feature columns as a DENSE
    // (M, k_out) tensor (e.g. the latent slice of the padded LSTM input)
    long Kout = (k_out > 0) ? k_out : K;
    TORCH_CHECK(Kout <= K);
    bool has_om = out_mask.defined() && out_mask.numel() > 0;
    if (has_om)
        TORCH_CHECK(out_mask.dtype() == torch::kBFloat16
                    && out_mask.is_contiguous()
                    && out_mask.numel() == M * Kout);
    auto dA = torch::empty({M, Kout}, dY.options());
    // the staged kernels read the output mask 16 bytes at a time
    bool om_aligned = !has_om
        || reinterpret_cast<uintptr_t>(out_mask.data_ptr()) % 16 == 0;
    TORCH_CHECK(om_aligned || path == 0 || path == GEMM_PATH_64,
                "out_mask must be 16-byte aligned for the staged kernels");
    path = om_aligned ? nt_pick_path(M, Kout, path) : GEMM_PATH_64;
    if (M == 0) return dA;
    int bm = (path == GEMM_PATH_S128) ? 128 : 64;
    dim3 grid(cdiv(M, bm), cdiv(Kout, 64));
    auto stream = at::cuda::getCurrentCUDAStream();
    auto* dy = reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr());
    auto* ac = relu_mask
        ? reinterpret_cast<const __hip_bfloat16*>(act_out.data_ptr()) : nullptr;
    auto* w = reinterpret_cast<const __hip_bfloat16*>(W.data_ptr());
    auto* da = reinterpret_cast<__hip_bfloat16*>(dA.data_ptr());
    auto* om = has_om
        ? reinterpret_cast<const __hip_bfloat16*>(out_mask.data_ptr()) : nullptr;
#define LAUNCHD(RM, OM)                                                        \
    do {                                                                       \
        if (path == GEMM_PATH_S128)                                            \
            hipLaunchKernelGGL((gemm_nt_dgrad_kernel<128, 64, RM, OM>), grid,  \
                               dim3(256), 0, stream.stream(), dy, ac, w, da,   \
                               om, (int)M, (int)N, (int)Kout);                 \
        else if (path == GEMM_PATH_S64)                                        \
            hipLaunchKernelGGL((gemm_nt_dgrad_kernel<64, 64, RM, OM>), grid,   \
                               dim3(256), 0, stream.stream(), dy, ac, w, da,   \
                               om, (int)M, (int)N, (int)Kout);                 \
        else                                                                   \
            hipLaunchKernelGGL((gemm_dgrad_kernel<RM, OM>), grid, dim3(256),   \
                               0, stream.stream(), dy, ac, w, da, om, (int)M,  \
                               (int)N, (int)K, (int)Kout);                     \
    } while (0)
    if (relu_mask) { if (has_om) LAUNCHD(true, true); else LAUNCHD(true, false); }
    else           { if (has_om) LAUNCHD(false, true); else LAUNCHD(false, false); }
#undef LAUNCHD
    return dA;
}

std::vector<torch::Tensor> gemm_wgrad(torch::Tensor dY, torch::Tensor act_out,
                                      torch::Tensor A, bool relu_mask,
                                      bool want_bias, int64_t path) {
    TORCH_CHECK(dY.is_cuda() && dY.dtype() == torch::kBFloat16 && dY.is_contiguous());
    TORCH_CHECK(A.dtype() == torch::kBFloat16 && A.is_contiguous());
    long M = dY.size(0), N = dY.size(1), K = A.size(1);
    auto dWt = torch::zeros({N, K}, dY.options().dtype(torch::kFloat32));
    auto db = torch::zeros({want_bias ? N : 1},
                           dY.options().dtype(torch::kFloat32));
    bool tile = wgrad_use_tile(M, N, K, path);
    long rows_per_chunk = tile
        ? wgrad_rows_per_chunk(M, (long)cdiv(N, WG_BN) * cdiv(K, WG_BK), 768,
                               WG_MT, 4 * WG_MT)
        : wgrad_rows_per_chunk(M, (long)cdiv(N, 64) * cdiv(K, 64), 1024, 32, 32);
    dim3 grid(cdiv(M, rows_per_chunk), cdiv(N, tile ? WG_BN : 64),
              cdiv(K, tile ? WG_BK : 64));
    auto stream = at::cuda::getCurrentCUDAStream();
    auto* dy = reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr());
    auto* ac = relu_mask
        ? reinterpret_cast<const __hip_bfloat16*>(act_out.data_ptr()) : nullptr;
    auto* a = reinterpret_cast<const __hip_bfloat16*>(A.data_ptr());
#define LAUNCHW(KERNEL, RM, HB)                                                \
    hipLaunchKernelGGL((KERNEL<RM, HB>), grid, dim3(256), 0,                   \
                       stream.stream(), dy, ac, a, dWt.data_ptr<float>(),      \
                       db.data_ptr<float>(), (int)M, (int)N, (int)K,           \
                       (int)rows_per_chunk, (int)N, (int)K, 0, 0, 0)
#define LAUNCHW2(RM, HB)                                                       \
    do {                                                                       \
        if (tile) LAUNCHW(gemm_wgrad_tile_kernel, RM, HB);                     \
        else LAUNCHW(gemm_wgrad_kernel, RM, HB);                               \
    } while (0)
    if (relu_mask) { if (want_bias) LAUNCHW2(true, true); else LAUNCHW2(true, false); }
    else           { if (want_bias) LAUNCHW2(false, true); else LAUNCHW2(false, false); }
#undef LAUNCHW2
#undef LAUNCHW
    return {dWt, db};
}

// accumulate straight into pre-zeroed .grad tensors (possibly narrower than
// the padded compute width: Nout <= N, Kout <= K) — removes the per-step
// grad-copy kernels from the engine's backward.
void gemm_wgrad_into(torch::Tensor dY, torch::Tensor act_out, torch::Tensor A,
                     bool relu_mask, torch::Tensor dW_out,
                     torch::Tensor db_out,
                     int64_t kd0, int64_t kd1, int64_t kd2, int64_t path) {
    TORCH_CHECK(dY.is_cuda() && dY.dtype() == torch::kBFloat16 && dY.is_contiguous());
    TORCH_CHECK(A.dtype() == torch::kBFloat16 && A.is_contiguous());
    TORCH_CHECK(dW_out.dtype() == torch::kFloat32 && dW_out.is_contiguous());
    long M = dY.size(0), N = dY.size(1), K = A.size(1);
    long Nout = dW_out.size(0), Kout = dW_out.numel() / Nout;
    bool want_bias = db_out.defined() && db_out.numel() > 0;
    bool kperm = kd2 > 0;
    if (kperm) TORCH_CHECK(kd0 * kd1 * kd2 == Kout, "kperm dims mismatch");
    bool tile = wgrad_use_tile(M, N, K, path);
    long rows_per_chunk = tile
        ? wgrad_rows_per_chunk(M, (long)cdiv(N, WG_BN) * cdiv(K, WG_BK), 768,
                               WG_MT, 4 * WG_MT)
        : wgrad_rows_per_chunk(M, (long)cdiv(N, 64) * cdiv(K, 64), 1024, 32, 32);
    dim3 grid(cdiv(M, rows_per_chunk), cdiv(N, tile ? WG_BN : 64),
              cdiv(K, tile ? WG_BK : 64));
    auto stream = at::cuda::getCurrentCUDAStream();
    auto* dy = reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr());
    auto* ac = relu_mask
        ? reinterpret_cast<const __hip_bfloat16*>(act_out.data_ptr()) : nullptr;
    auto* a = reinterpret_cast<const __hip_bfloat16*>(A.data_ptr());
    float* dbp = want_bias ? db_out.data_ptr<float>() : nullptr;
#define LAUNCHW(KERNEL, RM, HB, KP)                                            \
    hipLaunchKernelGGL((KERNEL<RM, HB, KP>), grid, dim3(256), 0,               \
                       stream.stream(), dy, ac, a, dW_out.data_ptr<float>(),   \
                       dbp, (int)M, (int)N, (int)K,                            \
                       (int)rows_per_chunk, (int)Nout, (int)Kout,              \
                       (int)kd0, (int)kd1, (int)kd2)
#define LAUNCHW2(RM, HB)                                                       \
    do {                                                                       \
        if (tile) {                                                            \
            if (kperm) LAUNCHW(gemm_wgrad_tile_kernel, RM, HB, true);          \
            else LAUNCHW(gemm_wgrad_tile_kernel, RM, HB, false);               \
        } else {                                                               \
            if (kperm) LAUNCHW(gemm_wgrad_kernel, RM, HB, true);               \
            else LAUNCHW(gemm_wgrad_kernel, RM, HB, false);                    \
        }                                                                      \
    } while (0)
    if (relu_mask) { if (want_bias) LAUNCHW2(true, true); else LAUNCHW2(true, false); }
    else           { if (want_bias) LAUNCHW2(false, true); else LAUNCHW2(false, false); }
#undef LAUNCHW2
#undef LAUNCHW
}
