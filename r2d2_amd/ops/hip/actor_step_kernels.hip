// Fused single-step kernels for actor inference (gfx950) — K15.
//
// The post-encoder part of one actor tick in three launches:
//
//   lstm_cell_step    latent | one-hot | reward | pad | bf16(h0) rows built in
//                     LDS, both gate GEMMs, bias, nonlinearities and the cell
//                     update -> h1, c1 (f32) and hb = bf16(h1)
//   head_hidden_step  both 512 -> 512 ReLU hidden layers from hb
//   head_out_step     both output layers, q = V + A - mean(A), greedy action
//
// The launch boundaries are the dependencies that cross workgroups (all of h1
// feeds the heads; all of the hidden layer feeds the outputs).  Inside a
// launch NO workgroup waits on another: no flags, no spins, no grid barrier,
// no global atomics.  Every workgroup reads kernel inputs only and writes its
// own output elements only, so these kernels cannot hang — or be hung by —
// the learner's persistent LSTM launches sharing the card.
//
// Accumulation order.  The sum behind one output element is a fixed chain of
// 16x16x32 MFMAs that depends on neither E nor the row tile the row lands in
// (nor on the tile shape chosen by the host):
//   cell    (x-part over kin_pad, ascending k  + bias) + (h-part over 512)
//   hidden  ((k-quarter 0 + quarter 1) + (quarter 2 + quarter 3)) + bias
//   out     the same four quarters, + bias
// so a row computes bit-identically at E = 5 and inside an E = 256 launch.
//
// Gate order matches torch.nn.LSTM and the persistent kernel: [i, f, g, o]
// chunks of H = 512.  MFMA 16x16x32 bf16, f32 accumulation, wave64; fragment
// conventions of common.h.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace {

constexpr int AH = 512;             // hidden size (and latent width)
constexpr int AKP_MAX = 576;        // kin_pad for A <= 32: 512 + 33 -> 576
constexpr int ALDA = AKP_MAX + AH + 8;   // LDS row stride (bf16 elements)
constexpr int APAD_HEAD = 32;       // rows of the packed head-output weights

__device__ __forceinline__ float sigmoidf_(float x) {
    return 1.f / (1.f + __expf(-x));
}

__device__ __forceinline__ void lds_store8(__hip_bfloat16* p, bf16x8 v) {
    bf16x8_u r;
    r.v = v;
    *reinterpret_cast<uint4*>(p) = r.u;
}

// ---------------------------------------------------------------------------
// lstm_cell_step: one workgroup per (U hidden units, RT batch rows).
// It owns gate columns c = g * U + j  <->  weight row g * 512 + u0 + j.
// U = 8: waves = 2 column fragments x {x-part, h-part}; U = 16: one column
// fragment per wave, which runs both parts.  Each wave keeps its B fragment
// (straight from global: every weight element is used once per row fragment)
// and loops the row fragments of the tile.
// ---------------------------------------------------------------------------
template <int U, int RT>
__global__ __launch_bounds__(256) void lstm_cell_step_kernel(
    const __hip_bfloat16* __restrict__ latent,   // (E, 512)
    const float* __restrict__ la,                // (E, A)
    const float* __restrict__ lr,                // (E,)
    const float* __restrict__ h0,                // (E, 512)
    const float* __restrict__ c0,                // (E, 512)
    const __hip_bfloat16* __restrict__ wih,      // (2048, KP)
    const __hip_bfloat16* __restrict__ whh,      // (2048, 512)
    const float* __restrict__ bias,              // (2048,)
    float* __restrict__ h1, float* __restrict__ c1,   // (E, 512)
    __hip_bfloat16* __restrict__ hb,             // (E, 512)
    int E, int A, int KP) {
    constexpr int GC = 4 * U;                 // gate columns of this wg
    constexpr int NCF = GC / 16;              // column fragments (2 or 4)
    constexpr int NRF = RT / 16;              // row fragments
    constexpr int PPW = (NCF == 4) ? 2 : 1;   // K parts run by one wave
    constexpr int LDG = GC + 4;               // f32 row stride of the sums
    constexpr int A_BYTES = RT * ALDA * 2;
    constexpr int S_BYTES = 2 * RT * LDG * 4;
    constexpr int SM_BYTES = A_BYTES > S_BYTES ? A_BYTES : S_BYTES;
    // the partial sums reuse the operand rows' storage after the K loops
    __shared__ __attribute__((aligned(16))) unsigned char smem[SM_BYTES];
    __hip_bfloat16* s_a = reinterpret_cast<__hip_bfloat16*>(smem);
    float* s_sum = reinterpret_cast<float*>(smem);

    const int u0 = blockIdx.x * U;
    const int r0 = blockIdx.y * RT;
    const int rows = min(E - r0, RT);
    const int kin = AH + A + 1;               // real input features
    const int tid = threadIdx.x;

    // ---- A-operand rows: latent | one-hot | reward | 0 pad | bf16(h0) ------
    // rows past E are zeros and are never read from memory
    {
        const unsigned CH = (unsigned)(KP + AH) / 8;     // 16-B chunks / row
        for (unsigned e = tid; e < (unsigned)RT * CH; e += 256) {
            const int row = (int)(e / CH);
            const int k = (int)(e % CH) * 8;
            bf16x8 v = zero_bf16x8();
            if (row < rows) {
                const long gr = r0 + row;
                if (k < AH) {
                    v = load_bf16x8(latent + gr * AH + k);
                } else if (k < KP) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int kk = k + i;
                        float f = 0.f;
                        if (kk < AH + A) f = la[gr * A + (kk - AH)];
                        else if (kk == AH + A) f = lr[gr];
                        v[i] = (__bf16)f;
                    }
                } else {
                    const float4* hp = reinterpret_cast<const float4*>(
                        h0 + gr * AH + (k - KP));
                    const float4 x = hp[0], y = hp[1];
                    v[0] = (__bf16)x.x; v[1] = (__bf16)x.y;
                    v[2] = (__bf16)x.z; v[3] = (__bf16)x.w;
                    v[4] = (__bf16)y.x; v[5] = (__bf16)y.y;
                    v[6] = (__bf16)y.z; v[7] = (__bf16)y.w;
                }
            }
            lds_store8(s_a + row * ALDA + k, v);
        }
    }
    __syncthreads();

    const int wave = tid / WAVE;
    const int lane = tid & (WAVE - 1);
    const int frow = lane & 15;
    const int kseg = (lane >> 4) * 8;
    const int cf = (NCF == 4) ? wave : (wave & 1);
    const int n = cf * 16 + frow;             // gate column within the wg
    const long wrow = (long)(n / U) * AH + u0 + (n % U);

    f32x4 acc[PPW][NRF] = {};
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int part = (NCF == 4) ? pp : (wave >> 1);
        if (part == 0) {
            // x-part: rin @ W_ih^T over kin_pad
            const __hip_bfloat16* wp = wih + wrow * KP + kseg;
            const __hip_bfloat16* ap = s_a + frow * ALDA + kseg;
#pragma unroll 4
            for (int k0 = 0; k0 < AH; k0 += 32) {
                const bf16x8 b = load_bf16x8(wp + k0);
#pragma unroll
                for (int i = 0; i < NRF; ++i)
                    if (i * 16 < rows)
                        acc[pp][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            load_bf16x8(ap + i * 16 * ALDA + k0), b,
                            acc[pp][i], 0, 0, 0);
            }
            // one-hot | reward | pad: the pad columns of W_ih (k >= kin)
            // are defined as unread — masked to zero here
            for (int k0 = AH; k0 < KP; k0 += 32) {
                bf16x8 b = load_bf16x8(wp + k0);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (k0 + kseg + i >= kin) b[i] = (__bf16)0.f;
#pragma unroll
                for (int i = 0; i < NRF; ++i)
                    if (i * 16 < rows)
                        acc[pp][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            load_bf16x8(ap + i * 16 * ALDA + k0), b,
                            acc[pp][i], 0, 0, 0);
            }
        } else {
            // h-part: bf16(h0) @ W_hh^T over 512
            const __hip_bfloat16* wp = whh + wrow * AH + kseg;
            const __hip_bfloat16* ap = s_a + frow * ALDA + KP + kseg;
#pragma unroll 4
            for (int k0 = 0; k0 < AH; k0 += 32) {
                const bf16x8 b = load_bf16x8(wp + k0);
#pragma unroll
                for (int i = 0; i < NRF; ++i)
                    if (i * 16 < rows)
                        acc[pp][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            load_bf16x8(ap + i * 16 * ALDA + k0), b,
                            acc[pp][i], 0, 0, 0);
            }
        }
    }
    __syncthreads();          // every wave is done with the operand rows
    {
        const int crow = (lane >> 4) * 4;
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) {
            const int part = (NCF == 4) ? pp : (wave >> 1);
#pragma unroll
            for (int i = 0; i < NRF; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s_sum[(part * RT + i * 16 + crow + r) * LDG + n] =
                        acc[pp][i][r];
        }
    }
    __syncthreads();

    // ---- bias, nonlinearities, cell update; stores masked to rows < E ------
    for (int p = tid; p < RT * U; p += 256) {
        const int row = p / U, j = p % U;
        if (row >= rows) continue;
        const int u = u0 + j;
        const long o = (long)(r0 + row) * AH + u;
        const float* sx = s_sum + row * LDG + j;
        const float* sh = s_sum + (RT + row) * LDG + j;
        const float gi = (sx[0 * U] + bias[0 * AH + u]) + sh[0 * U];
        const float gf = (sx[1 * U] + bias[1 * AH + u]) + sh[1 * U];
        const float gg = (sx[2 * U] + bias[2 * AH + u]) + sh[2 * U];
        const float go = (sx[3 * U] + bias[3 * AH + u]) + sh[3 * U];
        const float i_ = sigmoidf_(gi);
        const float f_ = sigmoidf_(gf);
        const float g_ = tanhf(gg);
        const float o_ = sigmoidf_(go);
        const float c = f_ * c0[o] + i_ * g_;
        const float h = o_ * tanhf(c);
        c1[o] = c;
        h1[o] = h;
        *reinterpret_cast<__bf16*>(hb + o) = (__bf16)h;
    }
}

// ---------------------------------------------------------------------------
// head_hidden_step: one workgroup per (16 of the 1024 hidden columns — 512
// advantage then 512 value — and RT rows).  Wave w runs k-quarter w; A
// fragments come straight from hb (each is used by one wave only).
// ---------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(256) void head_hidden_step_kernel(
    const __hip_bfloat16* __restrict__ hb,       // (E, 512)
    const __hip_bfloat16* __restrict__ wa1,      // (512, 512)
    const float* __restrict__ ba1,               // (512,)
    const __hip_bfloat16* __restrict__ wv1,
    const float* __restrict__ bv1,
    __hip_bfloat16* __restrict__ adv1,           // (E, 512)
    __hip_bfloat16* __restrict__ val1, int E) {
    constexpr int NRF = RT / 16;
    constexpr int LDP = 17;
    __shared__ float s_p[4][RT][LDP];

    const bool is_val = blockIdx.x >= AH / 16;
    const int n0 = (blockIdx.x % (AH / 16)) * 16;
    const __hip_bfloat16* W = is_val ? wv1 : wa1;
    const float* bias = is_val ? bv1 : ba1;
    __hip_bfloat16* out = is_val ? val1 : adv1;
    const int r0 = blockIdx.y * RT;
    const int rows = min(E - r0, RT);

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid & (WAVE - 1);
    const int frow = lane & 15;
    const int kseg = (lane >> 4) * 8;
    const int kq = wave * (AH / 4);

    const __hip_bfloat16* wp = W + (long)(n0 + frow) * AH + kq + kseg;
    f32x4 acc[NRF] = {};
#pragma unroll
    for (int k0 = 0; k0 < AH / 4; k0 += 32) {
        const bf16x8 b = load_bf16x8(wp + k0);
#pragma unroll
        for (int i = 0; i < NRF; ++i) {
            if (i * 16 >= rows) continue;
            const int row = i * 16 + frow;
            const bf16x8 a = (row < rows)
                ? load_bf16x8(hb + (long)(r0 + row) * AH + kq + kseg + k0)
                : zero_bf16x8();
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i],
                                                             0, 0, 0);
        }
    }
    {
        const int crow = (lane >> 4) * 4;
#pragma unroll
        for (int i = 0; i < NRF; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s_p[wave][i * 16 + crow + r][frow] = acc[i][r];
    }
    __syncthreads();
    for (int p = tid; p < RT * 16; p += 256) {
        const int row = p / 16, c = p % 16;
        if (row >= rows) continue;
        float v = ((s_p[0][row][c] + s_p[1][row][c])
                   + (s_p[2][row][c] + s_p[3][row][c])) + bias[n0 + c];
        v = fmaxf(v, 0.f);
        *reinterpret_cast<__bf16*>(out + (long)(r0 + row) * AH + n0 + c) =
            (__bf16)v;
    }
}

// ---------------------------------------------------------------------------
// head_out_step: one workgroup per 16 rows.  Wave w runs k-quarter w of three
// column fragments: advantage rows 0..15 and 16..31 of wa2t, value rows
// 0..15 of wv2t (row 0 is V).  Epilogue: 16 lanes per row, two advantage
// columns per lane; dueling combine and first-index argmax by 16-lane
// butterflies.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_out_step_kernel(
    const __hip_bfloat16* __restrict__ adv1,     // (E, 512)
    const __hip_bfloat16* __restrict__ val1,     // (E, 512)
    const __hip_bfloat16* __restrict__ wa2,      // (32, 512)
    const float* __restrict__ ba2,               // (32,)
    const __hip_bfloat16* __restrict__ wv2,      // (32, 512)
    const float* __restrict__ bv2,               // (32,)
    float* __restrict__ q,                       // (E, A)
    int* __restrict__ greedy,                    // (E,)
    int E, int A) {
    constexpr int LDP = 49;
    __shared__ float s_p[4][16][LDP];

    const int r0 = blockIdx.x * 16;
    const int rows = min(E - r0, 16);
    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid & (WAVE - 1);
    const int frow = lane & 15;
    const int kseg = (lane >> 4) * 8;
    const int kq = wave * (AH / 4);

    const long ao = (long)(r0 + frow) * AH + kq + kseg;
    const long wo = (long)frow * AH + kq + kseg;
    f32x4 acc[3] = {};
#pragma unroll
    for (int k0 = 0; k0 < AH / 4; k0 += 32) {
        bf16x8 aa = zero_bf16x8(), av = zero_bf16x8();
        if (frow < rows) {
            aa = load_bf16x8(adv1 + ao + k0);
            av = load_bf16x8(val1 + ao + k0);
        }
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            aa, load_bf16x8(wa2 + wo + k0), acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            aa, load_bf16x8(wa2 + wo + 16 * AH + k0), acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            av, load_bf16x8(wv2 + wo + k0), acc[2], 0, 0, 0);
    }
    {
        const int crow = (lane >> 4) * 4;
#pragma unroll
        for (int f = 0; f < 3; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s_p[wave][crow + r][f * 16 + frow] = acc[f][r];
    }
    __syncthreads();

    // every thread stays active through the butterflies; stores are masked
    const int row = tid >> 4, l = tid & 15;
    auto sum4 = [&](int c) {
        return (s_p[0][row][c] + s_p[1][row][c])
               + (s_p[2][row][c] + s_p[3][row][c]);
    };
    const float a0 = sum4(l) + ba2[l];
    const float a1 = sum4(16 + l) + ba2[16 + l];
    const float v = sum4(32) + bv2[0];
    const bool ok0 = l < A, ok1 = l + 16 < A;
    float s = (ok0 ? a0 : 0.f) + (ok1 ? a1 : 0.f);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);
    s /= (float)A;
    const float q0 = (v + a0) - s, q1 = (v + a1) - s;

    // first index of the row maximum (a NaN counts as the maximum, as in
    // numpy.argmax); candidates past A carry index 64 and lose every tie
    float bv = ok0 ? q0 : -INFINITY;
    int bi = ok0 ? l : 64;
    auto better = [](float x, int xi, float y, int yi) {
        const bool xn = x != x, yn = y != y;
        if (xn != yn) return xn;
        if (!xn && x != y) return x > y;
        return xi < yi;
    };
    if (ok1 && better(q1, l + 16, bv, bi)) { bv = q1; bi = l + 16; }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (row < rows) {
        const long gr = r0 + row;
        if (ok0) q[gr * A + l] = q0;
        if (ok1) q[gr * A + 16 + l] = q1;
        if (l == 0) greedy[gr] = bi;
    }
}

// ---------------------------------------------------------------------------
// Host wrappers.  Every operand is validated before anything launches: a bad
// operand raises and the outputs stay untouched.
// ---------------------------------------------------------------------------
void step_check(const torch::Tensor& t, const char* name,
                c10::ScalarType dtype, std::initializer_list<int64_t> shape) {
    TORCH_CHECK(t.defined() && t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ",
                t.scalar_type());
    TORCH_CHECK(t.sizes() == c10::IntArrayRef(shape.begin(), shape.size()),
                name, " must have shape ",
                c10::IntArrayRef(shape.begin(), shape.size()), ", got ",
                t.sizes());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

bool overlaps(const torch::Tensor& a, const torch::Tensor& b) {
    const char* a0 = static_cast<const char*>(a.data_ptr());
    const char* b0 = static_cast<const char*>(b.data_ptr());
    return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
}

// no output may share memory with an input (other workgroups still read it)
// or with another output
void check_no_alias(std::initializer_list<const torch::Tensor*> outs,
                    std::initializer_list<const torch::Tensor*> ins,
                    const char* what) {
    for (auto it = outs.begin(); it != outs.end(); ++it) {
        for (const torch::Tensor* i : ins)
            TORCH_CHECK(!overlaps(**it, *i), what,
                        ": an output aliases an input");
        for (auto jt = outs.begin(); jt != it; ++jt)
            TORCH_CHECK(!overlaps(**it, **jt), what,
                        ": two outputs alias each other");
    }
}

void same_device(std::initializer_list<const torch::Tensor*> ts,
                 const char* what) {
    const auto dev = (*ts.begin())->device();
    for (const torch::Tensor* t : ts)
        TORCH_CHECK(t->device() == dev, what,
                    ": operands must share one device");
}

const __hip_bfloat16* bfp(const torch::Tensor& t) {
    return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
__hip_bfloat16* bfp_mut(torch::Tensor& t) {
    return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

}  // namespace

// Tile choice (units per workgroup, rows per tile): units / rows = 0 selects
// the default, 8 units x 16 rows at every E — the fastest or within 4 % of it
// at E = 5, 64 and 256 on MI355X (docs/KERNELS.md has the table).  The other
// instantiations stay selectable for comparison; all compute the same bits.
void lstm_cell_step(torch::Tensor latent, torch::Tensor last_action,
                    torch::Tensor last_reward, torch::Tensor h0,
                    torch::Tensor c0, torch::Tensor wih_t,
                    torch::Tensor whh_t, torch::Tensor lstm_bias,
                    torch::Tensor h1, torch::Tensor c1, torch::Tensor hb,
                    int64_t units, int64_t rows) {
    TORCH_CHECK(latent.defined() && latent.dim() == 2,
                "latent must be (E, 512)");
    TORCH_CHECK(last_action.defined() && last_action.dim() == 2,
                "last_action must be (E, A)");
    TORCH_CHECK(wih_t.defined() && wih_t.dim() == 2,
                "wih_t must be (2048, kin_pad)");
    const int64_t E = latent.size(0), A = last_action.size(1);
    const int64_t KP = wih_t.size(1);
    TORCH_CHECK(E >= 1, "lstm_cell_step needs E >= 1, got ", E);
    TORCH_CHECK(A >= 1 && A <= APAD_HEAD, "lstm_cell_step needs 1 <= A <= ",
                APAD_HEAD, ", got ", A);
    TORCH_CHECK(KP % 32 == 0 && AH + A + 1 <= KP && KP <= AKP_MAX,
                "kin_pad must be a multiple of 32 with 512 + A + 1 <= "
                "kin_pad <= ", AKP_MAX, ", got ", KP);
    step_check(latent, "latent", torch::kBFloat16, {E, AH});
    step_check(last_action, "last_action", torch::kFloat32, {E, A});
    step_check(last_reward, "last_reward", torch::kFloat32, {E});
    step_check(h0, "h0", torch::kFloat32, {E, AH});
    step_check(c0, "c0", torch::kFloat32, {E, AH});
    step_check(wih_t, "wih_t", torch::kBFloat16, {4 * AH, KP});
    step_check(whh_t, "whh_t", torch::kBFloat16, {4 * AH, AH});
    step_check(lstm_bias, "lstm_bias", torch::kFloat32, {4 * AH});
    step_check(h1, "h1", torch::kFloat32, {E, AH});
    step_check(c1, "c1", torch::kFloat32, {E, AH});
    step_check(hb, "hb", torch::kBFloat16, {E, AH});
    same_device({&latent, &last_action, &last_reward, &h0, &c0, &wih_t,
                 &whh_t, &lstm_bias, &h1, &c1, &hb}, "lstm_cell_step");
    check_no_alias({&h1, &c1, &hb},
                   {&latent, &last_action, &last_reward, &h0, &c0, &wih_t,
                    &whh_t, &lstm_bias}, "lstm_cell_step");
    if (units == 0) units = 8;
    if (rows == 0) rows = 16;
    TORCH_CHECK((units == 8 || units == 16)
                && (rows == 16 || rows == 32 || rows == 64),
                "lstm_cell_step tiles: units in {8, 16}, rows in {16, 32, "
                "64}; got ", units, ", ", rows);

    auto stream = at::cuda::getCurrentCUDAStream(latent.device().index());
    dim3 grid((unsigned)(AH / units), (unsigned)cdiv(E, rows));
#define CELL(U, RT)                                                           \
    hipLaunchKernelGGL((lstm_cell_step_kernel<U, RT>), grid, dim3(256), 0,    \
                       stream.stream(), bfp(latent),                          \
                       last_action.data_ptr<float>(),                         \
                       last_reward.data_ptr<float>(), h0.data_ptr<float>(),   \
                       c0.data_ptr<float>(), bfp(wih_t), bfp(whh_t),          \
                       lstm_bias.data_ptr<float>(), h1.data_ptr<float>(),     \
                       c1.data_ptr<float>(), bfp_mut(hb), (int)E, (int)A,     \
                       (int)KP)
    if (units == 8) {
        if (rows == 16) CELL(8, 16); else if (rows == 32) CELL(8, 32);
        else CELL(8, 64);
    } else {
        if (rows == 16) CELL(16, 16); else if (rows == 32) CELL(16, 32);
        else CELL(16, 64);
    }
#undef CELL
}

void head_hidden_step(torch::Tensor hb, torch::Tensor wa1t, torch::Tensor ba1,
                      torch::Tensor wv1t, torch::Tensor bv1,
                      torch::Tensor adv1, torch::Tensor val1, int64_t rows) {
    TORCH_CHECK(hb.defined() && hb.dim() == 2, "hb must be (E, 512)");
    const int64_t E = hb.size(0);
    TORCH_CHECK(E >= 1, "head_hidden_step needs E >= 1, got ", E);
    step_check(hb, "hb", torch::kBFloat16, {E, AH});
    step_check(wa1t, "wa1t", torch::kBFloat16, {AH, AH});
    step_check(ba1, "ba1", torch::kFloat32, {AH});
    step_check(wv1t, "wv1t", torch::kBFloat16, {AH, AH});
    step_check(bv1, "bv1", torch::kFloat32, {AH});
    step_check(adv1, "adv1", torch::kBFloat16, {E, AH});
    step_check(val1, "val1", torch::kBFloat16, {E, AH});
    same_device({&hb, &wa1t, &ba1, &wv1t, &bv1, &adv1, &val1},
                "head_hidden_step");
    check_no_alias({&adv1, &val1}, {&hb, &wa1t, &ba1, &wv1t, &bv1},
                   "head_hidden_step");
    if (rows == 0) rows = 16;
    TORCH_CHECK(rows == 16 || rows == 64,
                "head_hidden_step tiles: rows in {16, 64}; got ", rows);

    auto stream = at::cuda::getCurrentCUDAStream(hb.device().index());
    dim3 grid(2 * AH / 16, (unsigned)cdiv(E, rows));
#define HID(RT)                                                               \
    hipLaunchKernelGGL((head_hidden_step_kernel<RT>), grid, dim3(256), 0,     \
                       stream.stream(), bfp(hb), bfp(wa1t),                   \
                       ba1.data_ptr<float>(), bfp(wv1t),                      \
                       bv1.data_ptr<float>(), bfp_mut(adv1), bfp_mut(val1),   \
                       (int)E)
    if (rows == 16) HID(16); else HID(64);
#undef HID
}

void head_out_step(torch::Tensor adv1, torch::Tensor val1, torch::Tensor wa2t,
                   torch::Tensor ba2, torch::Tensor wv2t, torch::Tensor bv2,
                   torch::Tensor q, torch::Tensor greedy) {
    TORCH_CHECK(adv1.defined() && adv1.dim() == 2, "adv1 must be (E, 512)");
    TORCH_CHECK(q.defined() && q.dim() == 2, "q must be (E, A)");
    const int64_t E = adv1.size(0), A = q.size(1);
    TORCH_CHECK(E >= 1, "head_out_step needs E >= 1, got ", E);
    TORCH_CHECK(A >= 1 && A <= APAD_HEAD, "head_out_step needs 1 <= A <= ",
                APAD_HEAD, ", got ", A);
    step_check(adv1, "adv1", torch::kBFloat16, {E, AH});
    step_check(val1, "val1", torch::kBFloat16, {E, AH});
    step_check(wa2t, "wa2t", torch::kBFloat16, {APAD_HEAD, AH});
    step_check(ba2, "ba2", torch::kFloat32, {APAD_HEAD});
    step_check(wv2t, "wv2t", torch::kBFloat16, {APAD_HEAD, AH});
    step_check(bv2, "bv2", torch::kFloat32, {APAD_HEAD});
    step_check(q, "q", torch::kFloat32, {E, A});
    step_check(greedy, "greedy", torch::kInt32, {E});
    same_device({&adv1, &val1, &wa2t, &ba2, &wv2t, &bv2, &q, &greedy},
                "head_out_step");
    check_no_alias({&q, &greedy}, {&adv1, &val1, &wa2t, &ba2, &wv2t, &bv2},
                   "head_out_step");

    auto stream = at::cuda::getCurrentCUDAStream(adv1.device().index());
    hipLaunchKernelGGL(head_out_step_kernel, dim3((unsigned)cdiv(E, 16)),
                       dim3(256), 0, stream.stream(), bfp(adv1), bfp(val1),
                       bfp(wa2t), ba2.data_ptr<float>(), bfp(wv2t),
                       bv2.data_ptr<float>(), q.data_ptr<float>(),
                       greedy.data_ptr<int>(), (int)E, (int)A);
}
