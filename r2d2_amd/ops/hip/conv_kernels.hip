// Implicit-GEMM MFMA convolution kernels for the Nature-CNN encoder (gfx950).
//
// Replaces MIOpen's conv paths, which on this workload fall back to naive
// f64-accumulation kernels + 261k per-image im2col launches (see
// profiles/r01_eager_step_kernel_stats.csv: 65% of all GPU time).
//
// Layout: NHWC, bf16 activations (uint8 input for conv1 with fused /255
// dequant).  K-order is (ky, kx, c), so a lane's 8 consecutive k-elements
// are 8 CONTIGUOUS input bytes/bf16 (x-then-c is memory-contiguous in NHWC
// and KW*CIN % 8 == 0 for all three convs) — A fragments load straight from
// global, no im2col materialization.  Weights are prepacked (COUT, K) for
// forward / wgrad and (CIN, TAPS*COUT) per tap-class for dgrad.
//
// Structure: the three layers are described once, as types (Conv1<CIN>,
// Conv2, Conv3); every kernel takes one of them as its only geometry
// parameter and the host dispatcher (dispatch_layer) maps (conv_id, cin) to
// it.  Nothing else is instantiated: a call that matches no layer raises.
//
// Forward:  out(M=N*OH*OW, COUT) = act(patch(M,K) @ Wt^T + bias); classic
//           (global patch reads) and band (whole image in LDS; weights in
//           LDS for conv1, in registers for the 64-output layers).
// Dgrad:    dX from the dense, pre-masked dY via uniform taps (stride-2
//           convs split into parity classes so every row in a tile has the
//           same taps; no divergence).  Dense: one launch per parity class,
//           tap table passed in, out-of-range taps dropped by a bounds
//           check on global gathers.  Band (what the engine runs): one
//           launch per layer, the image's dY staged once in LDS inside a
//           zero halo for all classes, weights in registers, dX stored
//           through LDS; bit-equal to dense.
// Wgrad:    dWt(COUT,K) = dY^T @ patch in 32-row tiles, register
//           accumulators flushed once per workgroup: with f32 atomics into
//           fresh zeros, or (_into) as a slab of partial sums that
//           wgrad_reduce_kernel sums into .grad in torch layout; optional
//           fused ReLU mask (empty act = dY pre-masked) + bias grad; chunked
//           (patch tiles copied from global memory) and band (whole image +
//           its dY in LDS, fragments gathered straight from the image).
//           Both run WgradTile.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

// dequantize 8 uint8 bytes (two little-endian dwords) to bf16/255
__device__ __forceinline__ bf16x8 dequant8(unsigned lo, unsigned hi) {
    bf16x8 r;
    const float inv = 1.f / 255.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[i] = (__bf16)(((lo >> (8 * i)) & 0xff) * inv);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[4 + i] = (__bf16)(((hi >> (8 * i)) & 0xff) * inv);
    return r;
}

// load 8 uint8 bytes (8-byte aligned) and dequantize to bf16/255
__device__ __forceinline__ bf16x8 load_dequant8(const unsigned char* p) {
    uint2 raw = *reinterpret_cast<const uint2*>(p);
    return dequant8(raw.x, raw.y);
}

// ---------------------------------------------------------------------------
// Patch-row loads, selected on CIN.  A lane's 8 k-elements are one
// contiguous run of the NHWC image starting at element
//   ((n*INH + oy*S + dy)*INW + ox*S)*CIN + rem.
// CIN == 4 (frame stack): ox*S*CIN = 16*ox and INW*CIN = 336 = 16*21, so the
// run is 16-byte aligned in u8 and in bf16 — one 8-byte global load, one
// 16-byte LDS read.
// CIN == 1 (single frame): the run starts at 4*ox + 84*row elements, i.e.
// only 4-byte aligned as u8 in global memory and only 8-byte aligned as bf16
// in LDS.  A wider access through a cast would assert an alignment the
// address does not have (off-alignment b128 LDS reads replay, and nothing
// guarantees the compiler splits them), so the access is issued at the
// alignment it really has: two 4-byte global loads, two 8-byte LDS reads.
// Restaging the image so the wide read is aligned would need a second,
// 4-element-shifted LDS copy for odd ox; K is only 64 here, the split read
// is the simpler choice.  Whole-image staging stays on the wide helpers:
// 84*84 = 8*882 bytes per image keeps every image base 8-byte aligned.
// ---------------------------------------------------------------------------
template <int CIN>
__device__ __forceinline__ bf16x8 load_patch_u8(const unsigned char* p) {
    if constexpr (CIN == 1) {
        const unsigned* q = reinterpret_cast<const unsigned*>(p);
        return dequant8(q[0], q[1]);
    } else {
        return load_dequant8(p);
    }
}

template <int CIN>
__device__ __forceinline__ bf16x8 lds_patch_row(const __hip_bfloat16* p) {
    if constexpr (CIN == 1) {
        const uint2* q = reinterpret_cast<const uint2*>(p);
        uint2 lo = q[0], hi = q[1];
        bf16x8_u r;
        r.u = uint4{lo.x, lo.y, hi.x, hi.y};
        return r.v;
    } else {
        return *reinterpret_cast<const bf16x8*>(p);
    }
}

// ---------------------------------------------------------------------------
// Layer geometry, stated once.  Square or not, everything a kernel or a host
// check needs derives from these eight facts per layer.
// ---------------------------------------------------------------------------
template <int KH_, int KW_, int CIN_, int S_, int INH_, int INW_, int COUT_,
          bool IN_U8_>
struct ConvGeom {
    static constexpr int KH = KH_, KW = KW_, CIN = CIN_, S = S_;
    static constexpr int INH = INH_, INW = INW_, COUT = COUT_;
    static constexpr bool IN_U8 = IN_U8_;       // u8 input, fused /255
    static constexpr int OH = (INH - KH) / S + 1;
    static constexpr int OW = (INW - KW) / S + 1;
    static constexpr int K = KH * KW * CIN;     // GEMM reduction extent
    static constexpr int KWC = KW * CIN;        // one kernel row (contiguous)
    static constexpr int NPIX = OH * OW;        // output pixels per image
    static constexpr int IMG = INH * INW * CIN; // input elements per image
    // dgrad: taps per stride-parity class, and that class's dX grid.  For
    // every layer S | INH, so the grid is the same for every parity offset.
    static constexpr int TAPS = (KH / S) * (KW / S);
    static constexpr int CLS_H = INH / S, CLS_W = INW / S;
    static_assert(KWC % 8 == 0 && K % 32 == 0 && IMG % 8 == 0,
                  "8-element lane runs / 32-wide MFMA k-tiles");
    static_assert(KH % S == 0 && KW % S == 0 && INH % S == 0 && INW % S == 0,
                  "uniform dgrad parity classes");
};

// conv1: 8x8 s4 over the 84x84 u8 frames, CIN 1 (single frame) or 4 (stack);
// conv2: 4x4 s2; conv3: 3x3 s1.  Each layer's input is the one below's output.
template <int CIN>
using Conv1 = ConvGeom<8, 8, CIN, 4, 84, 84, 32, true>;
using Conv2 = ConvGeom<4, 4, Conv1<4>::COUT, 2, Conv1<4>::OH, Conv1<4>::OW,
                       64, false>;
using Conv3 = ConvGeom<3, 3, Conv2::COUT, 1, Conv2::OH, Conv2::OW, 64, false>;

// ---------------------------------------------------------------------------
// Shared device pieces
// ---------------------------------------------------------------------------

// Warp-tile coordinates of a 256-thread workgroup, each wave a 32x32 tile of
// 2x2 MFMA fragments.  NCOL == 32 (e.g. conv1 COUT=32): the 4 waves stack on
// the M dim (128 rows) so no wave computes guarded-away columns; else the
// classic 2x2 (64 rows x 64 cols).
template <int NOUT>
constexpr int tile_ncol = NOUT <= 32 ? 32 : 64;

template <int NCOL>
struct WarpTile {
    static constexpr int ROWS = NCOL == 32 ? 128 : 64;
    int lane, wr, wc;
    int frow;   // fragment row/col this lane loads
    int kseg;   // its 8-element k segment within a 32-wide k-tile
    __device__ __forceinline__ WarpTile() {
        int wave = threadIdx.x / WAVE;
        lane = threadIdx.x & (WAVE - 1);
        wr = (NCOL == 32) ? wave : (wave >> 1);
        wc = (NCOL == 32) ? 0 : (wave & 1);
        frow = lane & 15;
        kseg = (lane >> 4) * 8;
    }
    __device__ __forceinline__ long row0() const {
        return (long)blockIdx.x * ROWS + wr * 32;
    }
    __device__ __forceinline__ long col0() const {
        return (long)blockIdx.y * 64 + wc * 32;
    }
};

// Walk a wave's MFMA accumulators: acc[i][j] is the 16x16 fragment at
// (16*i, 16*j) of the wave tile, of which a lane holds column lane&15, rows
// 4*(lane>>4) .. +3.  Calls f(row, col, value) with tile-relative coordinates.
template <int NI, int NJ, class F>
__device__ __forceinline__ void for_each_acc(const f32x4 (&acc)[NI][NJ],
                                             int lane, F&& f) {
    int ccol = lane & 15;
    int crow = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                f(i * 16 + crow + r, j * 16 + ccol, acc[i][j][r]);
}

// Element offset of the patch origin of GEMM row r = (n, oy, ox).
// 32-bit index math: M <= B*T*84*84 < 2^31, and the divisors are constants,
// so the divisions lower to multiply-shift.
template <class G>
__device__ __forceinline__ long patch_origin(unsigned r) {
    unsigned n = r / (unsigned)G::NPIX;
    unsigned p = r % (unsigned)G::NPIX;
    int oy = p / (unsigned)G::OW, ox = p % (unsigned)G::OW;
    return (((long)n * G::INH + (long)oy * G::S) * G::INW + (long)ox * G::S)
           * G::CIN;
}

// 8 k-elements of a patch row from the global image, at element offset off
template <class G>
__device__ __forceinline__ bf16x8 load_patch_row(const void* in, long off) {
    if constexpr (G::IN_U8)
        return load_patch_u8<G::CIN>(
            reinterpret_cast<const unsigned char*>(in) + off);
    else
        return load_bf16x8(reinterpret_cast<const __hip_bfloat16*>(in) + off);
}

// LDS layouts of a staged image: element (y, x, c) lives at y*RS + x*PS + c.
// DenseImage is plain NHWC.
template <class G>
struct DenseImage {
    static constexpr int PS = G::CIN, RS = G::INW * G::CIN, SIZE = G::IMG;
    __device__ __forceinline__ static int offset(int e) { return e; }
};

// GatherImage pads pixels and rows for the wgrad's transpose-read gather,
// which reads the same 32-byte k-run of 8 consecutive OUTPUT pixels per
// 32-lane half: the stride between output pixels, S*PS elements, is made
// 8 * odd banks (S*PS = 16 mod 32 elements; dense conv2/conv3 have 128 B =
// 32 banks, every other pixel on the same banks), and the row pad makes the
// step from the last pixel of an output row to the first of the next equal
// to that stride modulo all 64 banks (128 elements), so the 8 pixels may
// straddle output rows.  conv1's stride (32 B with four channels, 8 B with
// one, where a k-run is 16 B) needs no pad, and 4*84*CIN is already right.
template <class G>
struct GatherImage {
    static constexpr int pixel_stride() {
        if (G::S * G::CIN < 32) return G::CIN;
        int ps = G::CIN;
        while ((G::S * ps) % 32 != 16) ps += 8;
        return ps;
    }
    static constexpr int PS = pixel_stride();
    static constexpr int row_stride() {
        int rs = G::INW * PS;
        while ((G::S * rs - G::OW * G::S * PS) % 128 != 0) rs += 4;
        return rs;
    }
    static constexpr int RS = row_stride();
    static constexpr int SIZE = G::INH * RS;
    static constexpr bool DENSE = PS == G::CIN && RS == G::INW * G::CIN;
    // 8-element staging chunks stay inside a pixel and 16-byte aligned;
    // every gathered piece (4 elements of one pixel's k-run) 8-byte aligned
    static_assert(DENSE || (G::CIN % 8 == 0 && PS % 8 == 0 && RS % 8 == 0));
    static_assert((G::S * PS) % 4 == 0 && RS % 4 == 0 && G::KWC % 4 == 0);
    __device__ __forceinline__ static int offset(int e) {
        if constexpr (DENSE) return e;
        int r = e % (G::INW * G::CIN);
        return e / (G::INW * G::CIN) * RS + r / G::CIN * PS + r % G::CIN;
    }
};

// Stage image n whole into LDS in layout L (one global read + one dequant
// per element).  The caller owns the barriers around it.
template <class G, class L = DenseImage<G>>
__device__ __forceinline__ void stage_image(__hip_bfloat16* s_img,
                                            const void* in, long n) {
    const long gbase = n * G::IMG;
    for (int e = threadIdx.x * 8; e < G::IMG; e += blockDim.x * 8) {
        bf16x8 v;
        if constexpr (G::IN_U8)
            v = load_dequant8(
                reinterpret_cast<const unsigned char*>(in) + gbase + e);
        else
            v = load_bf16x8(
                reinterpret_cast<const __hip_bfloat16*>(in) + gbase + e);
        *reinterpret_cast<bf16x8*>(&s_img[L::offset(e)]) = v;
    }
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
template <class G, bool RELU>
__global__ __launch_bounds__(256) void conv_fwd_kernel(
    const void* __restrict__ in,            // (N, INH, INW, CIN)
    const __hip_bfloat16* __restrict__ Wt,  // (COUT, K)
    const float* __restrict__ bias,         // (COUT,)
    __hip_bfloat16* __restrict__ out,       // (M, COUT)
    int M) {
    constexpr int K = G::K, COUT = G::COUT;
    const WarpTile<tile_ncol<COUT>> wt;
    const long row0 = wt.row0(), col0 = wt.col0();

    // per-lane patch base addresses for its two A rows
    long abase[2];
    bool avalid[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned r = (unsigned)row0 + i * 16 + wt.frow;
        avalid[i] = r < (unsigned)M;
        abase[i] = avalid[i] ? patch_origin<G>(r) : 0;
    }

    f32x4 acc[2][2] = {};
    for (int k0 = 0; k0 < K; k0 += 32) {
        int k = k0 + wt.kseg;
        int dy = k / G::KWC;
        int rem = k % G::KWC;
        long off = (long)dy * G::INW * G::CIN + rem;
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = avalid[i] ? load_patch_row<G>(in, abase[i] + off)
                             : zero_bf16x8();
            long c = col0 + i * 16 + wt.frow;
            b[i] = (c < COUT) ? load_bf16x8(Wt + c * K + k) : zero_bf16x8();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[i], b[j], acc[i][j], 0, 0, 0);
    }

    for_each_acc(acc, wt.lane, [&](int r, int c, float v) {
        long rr = row0 + r;
        long cc = col0 + c;
        if (rr < M && cc < COUT) {
            v += bias[cc];
            if (RELU) v = fmaxf(v, 0.f);
            out[rr * COUT + cc] = f2bf(v);
        }
    });
}

// ---------------------------------------------------------------------------
// Dgrad of layer G from the DENSE (unpadded, pre-masked) upstream gradient:
//   dX[n, y, x, ci] = sum_t sum_co dY[n, (y-dy_t)/S, (x-dx_t)/S, co] *
//                     Wd[ci][t*COUT + co]
// Launched per stride-parity class (y0, x0); rows enumerate the class's
// (n, yy, xx) grid with y = y0 + yy*S, so every row has the same TAPS taps.
// Taps landing outside [0,OH)x[0,OW) contribute zero via a bounds check
// instead of a zero-padded staging copy.  OUT_MASK applies the ReLU mask of
// the conv BELOW ((act_x > 0) at the dX address) on store, so the next
// layer's dgrad and wgrad consume a pre-masked tensor directly.
// All geometry is compile-time: the per-lane row->(n,y,x) and k->(tap,co)
// divisions lower to mul-shift (the kernel is otherwise VALU-bound on
// address math).
// ---------------------------------------------------------------------------
template <class G, bool OUT_MASK>
__global__ __launch_bounds__(256) void conv_dgrad_dense_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (N, OH, OW, COUT)
    const __hip_bfloat16* __restrict__ Wd,   // (CIN, TAPS*COUT)
    const __hip_bfloat16* __restrict__ actx, // (N, INH, INW, CIN) or null
    __hip_bfloat16* __restrict__ dX,         // (N, INH, INW, CIN)
    const int* __restrict__ taps,            // (TAPS, 2): dy, dx
    int Mc, int y0, int x0) {
    constexpr int S = G::S, OH = G::OH, OW = G::OW, COUT = G::COUT;
    constexpr int XH = G::INH, XW = G::INW, CIN = G::CIN;
    constexpr int K = G::TAPS * COUT;
    constexpr unsigned XX = G::CLS_W, YX = G::CLS_H * G::CLS_W;
    const WarpTile<tile_ncol<CIN>> wt;
    const long row0 = wt.row0(), col0 = wt.col0();

    // class row -> (n, y, x)
    auto pixel = [&](unsigned r, unsigned& n, int& y, int& x) {
        n = r / YX;
        unsigned p = r % YX;
        y = y0 + (int)(p / XX) * S;
        x = x0 + (int)(p % XX) * S;
    };

    long nbase[2];
    int yv[2], xv[2];
    bool avalid[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned r = (unsigned)row0 + i * 16 + wt.frow;
        avalid[i] = r < (unsigned)Mc;
        unsigned n;
        pixel(avalid[i] ? r : 0, n, yv[i], xv[i]);
        nbase[i] = (long)n * OH * OW;
    }

    f32x4 acc[2][2] = {};
    for (int k0 = 0; k0 < K; k0 += 32) {
        int k = k0 + wt.kseg;
        int t = (unsigned)k / (unsigned)COUT;
        int co = (unsigned)k % (unsigned)COUT;
        int dy = taps[2 * t], dx = taps[2 * t + 1];
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // parity class guarantees S | (yv-dy); bounds replace padding
            int ny = yv[i] - dy, nx = xv[i] - dx;
            int oy = ny / S, ox = nx / S;
            bool ok = avalid[i] && ny >= 0 && nx >= 0 && oy < OH && ox < OW;
            a[i] = ok
                ? load_bf16x8(dY + (nbase[i] + (long)oy * OW + ox) * COUT + co)
                : zero_bf16x8();
            long c = col0 + i * 16 + wt.frow;
            b[i] = (c < CIN) ? load_bf16x8(Wd + c * K + k) : zero_bf16x8();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[i], b[j], acc[i][j], 0, 0, 0);
    }

    for_each_acc(acc, wt.lane, [&](int r, int c, float v) {
        long rr = row0 + r;
        long cc = col0 + c;
        if (rr < Mc && cc < CIN) {
            unsigned n;
            int y, x;
            pixel((unsigned)rr, n, y, x);
            long addr = (((long)n * XH + y) * XW + x) * CIN + cc;
            if (OUT_MASK)
                v = (bf2f(actx[addr]) > 0.f) ? v : 0.f;
            dX[addr] = f2bf(v);
        }
    });
}

// ---------------------------------------------------------------------------
// Wgrad: dWt(COUT, K) += sum_rows relu_mask(dY)[row][co] * patch[row][k]
// The FULL K extent (<= 576) and full COUT (<= 64) are covered per 32-row
// tile, so dY and the patches are each read exactly once; per-wave
// accumulators cover all k-tiles and are flushed once per workgroup (atomics
// or slab, see flush / flush_slab).  Optional fused ReLU mask; bias grad.
//
// WgradTile is everything the chunked and the band kernel share: the wave
// split, the accumulators, the dY staging, one 32-row MFMA step, the bias
// column sum and the two flushes.  The kernels differ only in where a
// B fragment comes from (a patch tile copied from global memory vs a gather
// straight out of the LDS image) and in their outer loop.
//
// Both operands are gathered with transpose-reads (common.h).  The 32 GEMM
// rows of a step are dealt to the lanes in 4-row blocks so that the eight
// rows one 32-lane half reads at a time are CONSECUTIVE: lane group g
// (lane / 16) takes block 4*(g/2) + (g%2) with its first read and the block
// two further on with its second, i.e. rows row_lo + {0, 8}.  Consecutive
// rows have one stride, so a row stride of 8 * odd banks spreads a half's
// eight 32-byte pieces over all 64 banks.
// ---------------------------------------------------------------------------
template <class G>
struct WgradTile {
    static constexpr int K = G::K, COUT = G::COUT;
    // NCOT = co tiles of 32 (1 when COUT<=32): waves split K 4/NCOT ways so
    // no wave computes guarded-away co columns
    static constexpr int NCOT = COUT / 32;
    static constexpr int NKW = 4 / NCOT;              // k splits
    static constexpr int KHALF = K / NKW;             // per-wave k extent
    static constexpr int KFRAG = KHALF / 16;          // 16-col frags per wave
    static_assert(COUT % 32 == 0 && 256 % COUT == 0 && KHALF % 16 == 0,
                  "waves own whole 32-co tiles and whole 16-column k frags");
    // padded LDS rows, in elements: 96 B / 160 B for dY and K*2 + 32 B for
    // the patch tile are all 8 * odd banks (see above) and keep 16-byte rows
    static constexpr int LD_DY = COUT + 16, LD_A = K + 16;
    static_assert((LD_DY / 2) % 16 == 8 && (LD_A / 2) % 16 == 8,
                  "row strides of 8 * odd banks");
    typedef __hip_bfloat16 PatchTile[32][LD_A];

    int lane;
    int wr;     // co tile
    int wc;     // k split
    int row_lo; // tile row of this lane's first piece; the second is 8 on
    int pcol;   // column of the piece inside a 16-column fragment
    // co extent per wave is always 32 (2 fragments of 16)
    f32x4 acc[2][KFRAG] = {};
    float bias_acc = 0.f;

    __device__ __forceinline__ WgradTile() {
        int wave = threadIdx.x / WAVE;
        lane = threadIdx.x & (WAVE - 1);
        wr = (NCOT == 1) ? 0 : (wave >> 1);
        wc = (NCOT == 1) ? wave : (wave & 1);
        int g = lane >> 4, i15 = lane & 15;
        row_lo = 16 * (g >> 1) + 4 * (g & 1) + (i15 >> 2);
        pcol = 4 * (i15 & 3);
    }

    // first k column of this lane's piece of the wave's kf-th fragment
    __device__ __forceinline__ int frag_k(int kf) const {
        return wc * KHALF + kf * 16 + pcol;
    }

    // Stage `rows` rows of dY with 16-byte loads: GEMM rows gm0 ..
    // gm0+nvalid-1, zero rows after them.  MASK applies the forward output's
    // ReLU (act > 0) on the way; without it dY arrives pre-masked (the
    // engine's dgrads mask on store) and act is never read.
    // The caller owns the barriers around it.
    template <bool MASK>
    __device__ __forceinline__ static void stage_dy(
        __hip_bfloat16* s_dy,                    // [rows][LD_DY]
        const __hip_bfloat16* __restrict__ dY,   // (M, COUT)
        const __hip_bfloat16* __restrict__ act,  // (M, COUT) forward output
        long gm0, int nvalid, int rows) {
        constexpr int C8 = COUT / 8;
        for (int e8 = threadIdx.x; e8 < rows * C8; e8 += 256) {
            int mrow = e8 / C8;
            int col = (e8 % C8) * 8;
            bf16x8 v = zero_bf16x8();
            if (mrow < nvalid) {
                long off = (gm0 + mrow) * COUT + col;
                v = load_bf16x8(dY + off);
                if constexpr (MASK) {
                    bf16x8 m = load_bf16x8(act + off);
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        v[e] = ((float)m[e] > 0.f) ? v[e] : (__bf16)0.f;
                }
            }
            *reinterpret_cast<bf16x8*>(&s_dy[mrow * LD_DY + col]) = v;
        }
    }

    // One MFMA step over the 32 staged dY rows at s_dy.  frag_b(kf) returns
    // the lane's B fragment of the wave's kf-th 16 k columns: elements 0..3
    // from tile row row_lo, 4..7 from row_lo + 8, piece column frag_k(kf).
    template <class FragB>
    __device__ __forceinline__ void mma(const __hip_bfloat16* s_dy,
                                        FragB&& frag_b) {
        bf16x8 fa[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const __hip_bfloat16* p =
                s_dy + row_lo * LD_DY + wr * 32 + i * 16 + pcol;
            fa[i] = lds_tr_frag8(p, p + 8 * LD_DY);
        }
#pragma unroll
        for (int kf = 0; kf < KFRAG; ++kf) {
            bf16x8 fb = frag_b(kf);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                acc[i][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    fa[i], fb, acc[i][kf], 0, 0, 0);
        }
    }

    // bias grad: column sums of `rows` staged rows, 256 / COUT threads each
    __device__ __forceinline__ void bias_rows(const __hip_bfloat16* s_dy,
                                              int rows) {
        int c = threadIdx.x % COUT;
        for (int mr = threadIdx.x / COUT; mr < rows; mr += 256 / COUT)
            bias_acc += bf2f(s_dy[mr * LD_DY + c]);
    }

    // s_red: 256 floats of LDS that nothing else uses any more.  The bias
    // partials of a column are summed there first: one atomic per column
    // and workgroup (all workgroups hit the same COUT addresses).
    __device__ __forceinline__ void flush(float* __restrict__ dWt,  // (COUT, K)
                                          float* __restrict__ db,   // (COUT,)
                                          float* s_red) {
        for_each_acc(acc, lane, [&](int r, int c, float v) {
            long co = wr * 32 + r;
            long kk = wc * KHALF + c;
            atomicAdd(&dWt[co * K + kk], v);
        });
        __syncthreads();
        s_red[threadIdx.x] = bias_acc;
        __syncthreads();
        if (threadIdx.x < COUT) {
            float s = 0.f;
            for (int i = threadIdx.x; i < 256; i += COUT) s += s_red[i];
            atomicAdd(&db[threadIdx.x], s);
        }
    }

    // Slab flush: the workgroup's partial sums go to its own slot of a
    // workspace with plain stores, no atomics; wgrad_reduce_kernel sums the
    // slots afterwards.  A slot is SLOT floats: the COUT*K accumulators in
    // FRAGMENT order -- the f32x4 of (wave, i, kf) and lane at float4 index
    // ((wave*2 + i)*KFRAG + kf)*64 + lane, so every wave-instruction stores
    // one contiguous KiB -- then 64 floats of bias partials (COUT used, the
    // rest zero).  slab_coord() maps a slot index back to (co, k).
    static constexpr int SLOT = COUT * K + 64;

    __device__ __forceinline__ void flush_slab(float* __restrict__ slot,
                                               float* s_red) {
        int wave = threadIdx.x / WAVE;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int kf = 0; kf < KFRAG; ++kf)
                *reinterpret_cast<f32x4*>(
                    slot + ((((wave * 2 + i) * KFRAG + kf) * 64 + lane) << 2)) =
                    acc[i][kf];
        __syncthreads();
        s_red[threadIdx.x] = bias_acc;
        __syncthreads();
        if (threadIdx.x < 64) {
            float s = 0.f;
            if (threadIdx.x < COUT)
                for (int i = threadIdx.x; i < 256; i += COUT) s += s_red[i];
            slot[COUT * K + threadIdx.x] = s;
        }
    }

    // (co, k) of float e < COUT*K of a slot: the inverse of flush_slab's
    // order and for_each_acc's fragment layout
    __device__ __forceinline__ static void slab_coord(int e, int& co, int& k) {
        int r = e & 3, ln = (e >> 2) & 63, f = e >> 8;
        int kf = f % KFRAG, i = f / KFRAG % 2, wave = f / (2 * KFRAG);
        int wr_ = (NCOT == 1) ? 0 : (wave >> 1);
        int wc_ = (NCOT == 1) ? wave : (wave & 1);
        co = wr_ * 32 + i * 16 + (ln >> 4) * 4 + r;
        k = wc_ * KHALF + kf * 16 + (ln & 15);
    }
};

// ---------------------------------------------------------------------------
// Reducer of the slab flush.  ws holds `parts` slots of WgradTile<G>::SLOT
// floats; element e of the result is slot 0's e + slot 1's e + ... summed in
// an order fixed by the code alone: thread group g of 16 adds slots g, g + 16,
// g + 32, ... in turn, then one thread adds the 16 group sums from 0 up.  So
// two launches on the same slots give the same bits.  A workgroup owns 64
// consecutive floats of the slot (256 B per slot, four slots per wave load)
// and stores them where they belong: the weight gradient in torch layout
// (COUT, CIN, KH, KW), the last 64 floats' first COUT into db.  Destination
// elements are OVERWRITTEN, not added to.
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(
    const float* __restrict__ ws,   // (parts, SLOT)
    int parts,
    float* __restrict__ dW,         // (COUT, CIN, KH, KW)
    float* __restrict__ db) {       // (COUT,)
    using Tile = WgradTile<G>;
    __shared__ __attribute__((aligned(16))) float s_part[16][64];
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const float* p = ws + (long)g * Tile::SLOT + blockIdx.x * 64 + q * 4;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = g; s < parts; s += 16, p += 16L * Tile::SLOT)
        sum += *reinterpret_cast<const f32x4*>(p);
    *reinterpret_cast<f32x4*>(&s_part[g][q * 4]) = sum;
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) v += s_part[i][threadIdx.x];
        int e = blockIdx.x * 64 + threadIdx.x;
        if (e < G::COUT * G::K) {
            int co, k;
            Tile::slab_coord(e, co, k);
            int ky = k / G::KWC, kx = k % G::KWC / G::CIN, c = k % G::CIN;
            dW[((co * G::CIN + c) * G::KH + ky) * G::KW + kx] = v;
        } else if (e - G::COUT * G::K < G::COUT) {
            db[e - G::COUT * G::K] = v;
        }
    }
}

// chunked wgrad: a workgroup owns rows_per_chunk GEMM rows; each 32-row tile
// of patches is copied from the global image into s_a, one barrier pair per
// tile.
// MASK: see stage_dy.  SLAB: dWt is the partial-sum workspace and the
// workgroup stores its slot there (flush_slab); else the atomic flush.
template <class G, bool MASK, bool SLAB>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (M, COUT)
    const __hip_bfloat16* __restrict__ act,  // (M, COUT) forward output
    const void* __restrict__ in,             // (N, INH, INW, CIN)
    float* __restrict__ dWt,                 // (COUT, K) f32, or the slabs
    float* __restrict__ db,                  // (COUT,) f32 (atomic flush)
    int M, int rows_per_chunk) {
    using Tile = WgradTile<G>;
    constexpr int K = G::K;
    __shared__ __attribute__((aligned(16)))
        __hip_bfloat16 s_dy[32 * Tile::LD_DY];
    __shared__ __attribute__((aligned(16))) typename Tile::PatchTile s_a;
    Tile tile;
    long mstart = (long)blockIdx.x * rows_per_chunk;
    long mend = min((long)M, mstart + rows_per_chunk);

    for (long m0 = mstart; m0 < mend; m0 += 32) {
        int nvalid = (int)min(32L, mend - m0);
        __syncthreads();
        Tile::template stage_dy<MASK>(s_dy, dY, act, m0, nvalid, 32);
        for (int e8 = threadIdx.x; e8 < 32 * (K / 8); e8 += 256) {
            int mrow = e8 / (K / 8);
            int k = (e8 % (K / 8)) * 8;
            bf16x8 w = zero_bf16x8();
            if (mrow < nvalid) {
                long base = patch_origin<G>((unsigned)(m0 + mrow));
                int dy_ = k / G::KWC, rem = k % G::KWC;
                w = load_patch_row<G>(
                    in, base + (long)dy_ * G::INW * G::CIN + rem);
            }
            *reinterpret_cast<bf16x8*>(&s_a[mrow][k]) = w;
        }
        __syncthreads();
        tile.mma(s_dy, [&](int kf) {
            const __hip_bfloat16* p = &s_a[tile.row_lo][tile.frag_k(kf)];
            return lds_tr_frag8(p, p + 8 * Tile::LD_A);
        });
        tile.bias_rows(s_dy, 32);
    }
    if constexpr (SLAB)
        tile.flush_slab(dWt + (long)blockIdx.x * Tile::SLOT,
                        reinterpret_cast<float*>(s_dy));
    else
        tile.flush(dWt, db, reinterpret_cast<float*>(s_dy));
}

// ---------------------------------------------------------------------------
// conv_fwd_band: per-image forward.  The whole input image AND the full
// prepacked weight matrix fit in LDS for every Nature-CNN conv, so the
// patch field reads LDS (one global read + one dequant per input element
// instead of one per patch overlap: conv1 557 MB u8 re-dequant -> 154 MB,
// conv3 9x re-read -> 1x).  Fused bias + ReLU as in conv_fwd_kernel.
// ---------------------------------------------------------------------------
// BAND_COLS: output columns of the LDS weight slab.  Only conv1 (32 outputs)
// runs this kernel in the engine; the 64-output layers keep their weights in
// registers (conv_fwd_band64_kernel below) and stage each image once.
constexpr int BAND_COLS = 32;

// Default grids of the per-image kernels, in workgroups: 512 = the 2 per CU
// that LDS (conv1) or VGPRs (register-resident weights) allow, times 256
// CUs, one resident round with no tail.  Measured at 5440 images, medians of
// two rounds, us, for 256 / 512 / 768 / 1024 / 2048 workgroups:
//   conv1 fwd (4 ch) 246-248 / 149 / 198 / 160-161 / 160-162
//   conv2 fwd        123-124 / 77-78 / 107 / 88-92 / 96-97
//   conv3 fwd        72 / 48 / 57 / 53-54 / 63
//   conv3 dgrad      70 / 53 / 62-63 / 58 / 67-68
//   conv2 dgrad      101 / 72-73 / 90-91 / 75 / 78-82
constexpr int BAND_WGS = 512;

template <class G>
__global__ __launch_bounds__(256) void conv_fwd_band_kernel(
    const void* __restrict__ in,            // (N, INH, INW, CIN)
    const __hip_bfloat16* __restrict__ Wt,  // (COUT, K)
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,       // (N*NPIX, COUT)
    int N, int imgs_per_wg, int co0) {
    constexpr int K = G::K, NPIX = G::NPIX;
    constexpr int NB = 2;                          // B frags = 32 cols/wave

    __shared__ __hip_bfloat16 s_img[G::IMG];
    __shared__ __hip_bfloat16 s_w[BAND_COLS][K + 8];

    const WarpTile<BAND_COLS> wt;                  // 4 waves stack rows

    for (int e = threadIdx.x * 8; e < BAND_COLS * K; e += blockDim.x * 8) {
        int c = e / K, k = e % K;
        *reinterpret_cast<bf16x8*>(&s_w[c][k]) =
            load_bf16x8(Wt + (long)(co0 + c) * K + k);
    }

    const long n0 = (long)blockIdx.x * imgs_per_wg;
    const long n1 = min((long)N, n0 + imgs_per_wg);
    for (long n = n0; n < n1; ++n) {
        __syncthreads();
        stage_image<G>(s_img, in, n);
        __syncthreads();

        for (int p0 = wt.wr * 32; p0 < NPIX; p0 += wt.ROWS) {
            int pbase[2];
            bool pval[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int pp = p0 + i * 16 + wt.frow;
                pval[i] = pp < NPIX;
                int oy = pp / G::OW, ox = pp % G::OW;
                pbase[i] = ((oy * G::S) * G::INW + ox * G::S) * G::CIN;
            }
            f32x4 acc[2][NB] = {};
            for (int k0 = 0; k0 < K; k0 += 32) {
                int k = k0 + wt.kseg;
                int dy = k / G::KWC;
                int rem = k % G::KWC;
                int off = dy * G::INW * G::CIN + rem;
                bf16x8 a[2], b[NB];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    a[i] = pval[i]
                        ? lds_patch_row<G::CIN>(&s_img[pbase[i] + off])
                        : zero_bf16x8();
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    b[j] = load_bf16x8(&s_w[wt.wc * 32 + j * 16 + wt.frow][k]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[i], b[j], acc[i][j], 0, 0, 0);
            }
            for_each_acc(acc, wt.lane, [&](int r, int c, float v) {
                int pp = p0 + r;
                int cc = wt.wc * 32 + c;
                if (pp < NPIX) {
                    v += bias[co0 + cc];
                    out[(n * NPIX + pp) * G::COUT + co0 + cc] =
                        f2bf(fmaxf(v, 0.f));
                }
            });
        }
    }
}

// ---------------------------------------------------------------------------
// conv_wgrad_band: per-image wgrad.  The WHOLE input image fits in LDS for
// every Nature-CNN conv (conv1 84x84x4 u8->bf16 56 KB, conv2 20x20x32
// 26 KB, conv3 9x9x64 10 KB), and so does the image's whole masked dY
// (rounded up to a multiple of 32 zero rows: 39 / 15 / 10 KB; four-channel
// conv1 takes it in two halves, see ROWS).  A workgroup
// stages both ONCE per image (single dequant per input element instead of
// one per patch overlap; conv1: 557 MB -> 154 MB per step) and then runs
// the image's 32-row tiles with no barrier between them: the B fragments
// are gathered straight out of the image — tile row q of a fragment is the
// patch of output pixel p0 + q, a transpose-read takes one address per lane,
// and a lane's 4 k-elements lie inside one kernel row (KWC % 4 == 0) — so
// no im2col tile is ever written.  Rows past the image's last pixel gather
// that last pixel against zero dY rows (pad, don't mask: the read needs
// every lane active).  Each image's contribution accumulates in registers,
// with ONE flush per workgroup.
// ---------------------------------------------------------------------------
template <class G, bool MASK, bool SLAB>
__global__ __launch_bounds__(256) void conv_wgrad_band_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (M=N*NPIX, COUT)
    const __hip_bfloat16* __restrict__ act,  // (M, COUT) forward out (mask)
    const void* __restrict__ in,             // (N, INH, INW, CIN)
    float* __restrict__ dWt,                 // (COUT, K) f32, or the slabs
    float* __restrict__ db,                  // (COUT,) f32 (atomic flush)
    int N, int imgs_per_wg) {
    using Tile = WgradTile<G>;
    using Img = GatherImage<G>;
    constexpr int NPIX = G::NPIX;
    // dY rows staged at a time: the whole image, except where image + dY
    // would pass half a CU's 160 KB of LDS (conv1 with four channels, 94 KB)
    // and leave one workgroup per CU with nothing to overlap its staging
    // with; there dY goes in two halves of 7 tiles (76 KB)
    constexpr int TILES = (NPIX + 31) / 32;
    constexpr bool WHOLE =
        (Img::SIZE + TILES * 32 * Tile::LD_DY) * 2 <= 80 * 1024;
    constexpr int ROWS = (WHOLE ? TILES : (TILES + 1) / 2) * 32;
    static_assert((Img::SIZE + ROWS * Tile::LD_DY) * 2 <= 80 * 1024);
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_img[Img::SIZE];
    __shared__ __attribute__((aligned(16)))
        __hip_bfloat16 s_dy[ROWS * Tile::LD_DY];
    Tile tile;

    // image offset of this lane's piece of each k fragment, from the patch
    // origin: k = (dy, kx, c)
    int koff[Tile::KFRAG];
#pragma unroll
    for (int kf = 0; kf < Tile::KFRAG; ++kf) {
        int k = tile.frag_k(kf);
        int rem = k % G::KWC;
        koff[kf] = k / G::KWC * Img::RS + rem / G::CIN * Img::PS
                   + rem % G::CIN;
    }
    // patch origin of output pixel pp, clamped into the image
    auto origin = [](int pp) {
        pp = min(pp, NPIX - 1);
        return (pp / G::OW * Img::RS + pp % G::OW * Img::PS) * G::S;
    };

    const long n0 = (long)blockIdx.x * imgs_per_wg;
    const long n1 = min((long)N, n0 + imgs_per_wg);
    for (long n = n0; n < n1; ++n) {
        for (int r0 = 0; r0 < NPIX; r0 += ROWS) {
            __syncthreads();    // the tiles staged before are done
            if (r0 == 0) stage_image<G, Img>(s_img, in, n);
            Tile::template stage_dy<MASK>(s_dy, dY, act, n * NPIX + r0,
                                          NPIX - r0, ROWS);
            __syncthreads();
            tile.bias_rows(s_dy, ROWS);
            for (int p0 = r0; p0 < min(r0 + ROWS, NPIX); p0 += 32) {
                const __hip_bfloat16* lo = s_img + origin(p0 + tile.row_lo);
                const __hip_bfloat16* hi =
                    s_img + origin(p0 + tile.row_lo + 8);
                tile.mma(s_dy + (p0 - r0) * Tile::LD_DY, [&](int kf) {
                    return lds_tr_frag8(lo + koff[kf], hi + koff[kf]);
                });
            }
        }
    }
    if constexpr (SLAB)
        tile.flush_slab(dWt + (long)blockIdx.x * Tile::SLOT,
                        reinterpret_cast<float*>(s_dy));
    else
        tile.flush(dWt, db, reinterpret_cast<float*>(s_dy));
}

// ---------------------------------------------------------------------------
// Register-resident B operand.  A 64-column layer's weights are 64-74 KB: as
// an LDS slab they crowd out the images and are refilled by every workgroup.
// Split over the waves instead, a wave's 32 columns of the whole K extent
// are K/32 * 2 fragments = at most 144 VGPRs, loaded ONCE per workgroup and
// never re-read; the k loop is fully unrolled around them.
//   b[ks][j] = W[(col0 + 16*j + lane%16) * K + 32*ks + 8*(lane/16) .. +7]
// ---------------------------------------------------------------------------
template <int KSTEPS>
__device__ __forceinline__ void load_b_regs(bf16x8 (&b)[KSTEPS][2],
                                            const __hip_bfloat16* W, int col0,
                                            int lane) {
    const __hip_bfloat16* p =
        W + (long)(col0 + (lane & 15)) * (KSTEPS * 32) + (lane >> 4) * 8;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            b[ks][j] = load_bf16x8(p + (long)j * 16 * (KSTEPS * 32) + ks * 32);
}

// ---------------------------------------------------------------------------
// conv_fwd_band for the 64-output layers: ONE launch, each image staged once
// for both column halves.  Waves are 2 (row halves of the image's output
// pixels) x 2 (32-column halves); the weights live in registers
// (load_b_regs), so LDS holds only the image, in the GatherImage layout whose
// output-pixel stride of 160 B keeps the 16-byte patch reads of 16
// consecutive pixels off each other's banks.  The k order per output element
// is conv_fwd_band_kernel's, so the outputs are bit-equal to it.
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(256, 2) void conv_fwd_band64_kernel(
    const void* __restrict__ in,            // (N, INH, INW, CIN)
    const __hip_bfloat16* __restrict__ Wt,  // (COUT, K)
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,       // (N*NPIX, COUT)
    int N, int imgs_per_wg) {
    using Img = GatherImage<G>;
    constexpr int K = G::K, NPIX = G::NPIX, KSTEPS = K / 32;
    constexpr int NI = ((NPIX + 15) / 16 + 1) / 2;  // row frags per wave
    static_assert(G::COUT == 64 && !G::IN_U8 && G::CIN % 32 == 0);
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_img[Img::SIZE];

    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    const int wr = wave >> 1, col0 = (wave & 1) * 32;
    const int frow = lane & 15, kseg = (lane >> 4) * 8;

    bf16x8 b[KSTEPS][2];
    load_b_regs<KSTEPS>(b, Wt, col0, lane);
    float bias_c[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bias_c[j] = bias[col0 + j * 16 + frow];

    // patch origin of this lane's row in each fragment, clamped into the
    // image: rows past the last pixel compute a copy that is never stored
    int pbase[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        int pp = min((wr * NI + i) * 16 + frow, NPIX - 1);
        pbase[i] = (pp / G::OW * Img::RS + pp % G::OW * Img::PS) * G::S + kseg;
    }

    const long n0 = (long)blockIdx.x * imgs_per_wg;
    const long n1 = min((long)N, n0 + imgs_per_wg);
    for (long n = n0; n < n1; ++n) {
        __syncthreads();
        stage_image<G, Img>(s_img, in, n);
        __syncthreads();

        f32x4 acc[NI][2] = {};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            // k = (ky, kx, c) of the step's first element: a compile-time
            // offset; the lane's kseg (in pbase) stays inside its pixel
            constexpr int CIN = G::CIN;
            const int rem = ks * 32 % G::KWC;
            const int off = ks * 32 / G::KWC * Img::RS + rem / CIN * Img::PS
                            + rem % CIN;
            bf16x8 a[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                a[i] = *reinterpret_cast<const bf16x8*>(
                    &s_img[pbase[i] + off]);
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[i], b[ks][j], acc[i][j], 0, 0, 0);
        }
        for_each_acc(acc, lane, [&](int r, int c, float v) {
            int pp = wr * NI * 16 + r;
            if (pp < NPIX) {
                v += bias_c[c / 16];
                out[(n * NPIX + pp) * G::COUT + col0 + c] =
                    f2bf(fmaxf(v, 0.f));
            }
        });
    }
}

// ---------------------------------------------------------------------------
// conv1_fwd_dual: conv1 of TWO networks (online and target) from one staging
// of each frame.  The networks differ only in a (32, K) weight matrix and a
// bias, so the u8 read, the dequant and the LDS image are shared and only
// the MFMAs and the stores double.
//   W    both networks' weights in registers (load_b_regs, 2 x K/32 x 2
//        fragments: 128 VGPRs at four channels, 32 at one); no LDS slab.
//        Every wave holds both networks and the waves split the image's 25
//        row fragments 7/6/6/6, so an A fragment is read from LDS once and
//        feeds four MFMAs.  The k order per output element is
//        conv_fwd_band_kernel's: outputs are bit-equal to it.
//   in   the next image's u8 bytes are loaded into registers (8 bytes per
//        lane and load, the alignment the frames really have) before the
//        MFMA loop and dequantised into the LDS image after the barrier that
//        ends it; two barriers per image.
//   out  a wave's 32 x 32 tile (bias + ReLU applied) goes through a private
//        LDS scratch and leaves as 16-byte stores contiguous over the wave:
//        an output row is 64 B, a 16-row fragment one 1 KB run.  The scratch
//        row stride of 80 B spreads the four rows a 2-byte write instruction
//        touches over disjoint banks.
// ---------------------------------------------------------------------------
template <class G>
struct Conv1Dual {
    static constexpr int CHUNKS = G::IMG / 8;             // 8-byte u8 chunks
    static constexpr int NPRE = (CHUNKS + 255) / 256;     // per thread
    static constexpr int NFRAG = G::NPIX / 16;            // 25 row fragments
    static constexpr int PER_WAVE = NFRAG / 4;            // wave 0: one more
    static constexpr int SCR_LD = G::COUT + 8;            // 80 B rows
    static constexpr int SCR = 32 * SCR_LD;               // per wave
    // LDS offset of k-step ks = ks * KS_STEP + a per-lane constant
    static constexpr int KS_STEP = 32 / G::KWC * G::INW * G::CIN;
    static_assert(G::NPIX % 16 == 0 && NFRAG % 4 == 1 && PER_WAVE % 2 == 0,
                  "whole fragments: pairs per wave, wave 0 one single more");
    static_assert(G::COUT == 32 && G::IN_U8 && 32 % G::KWC == 0);
    static_assert((G::IMG + 4 * SCR) * 2 <= 80 * 1024);
};

template <class G>
__global__ __launch_bounds__(256, 2) void conv1_fwd_dual_kernel(
    const unsigned char* __restrict__ in,    // (N, INH, INW, CIN) u8
    const __hip_bfloat16* __restrict__ Wt0,  // (COUT, K) network 0
    const float* __restrict__ bias0,
    const __hip_bfloat16* __restrict__ Wt1,  // (COUT, K) network 1
    const float* __restrict__ bias1,
    __hip_bfloat16* __restrict__ out0,       // (N*NPIX, COUT)
    __hip_bfloat16* __restrict__ out1,
    int N, int imgs_per_wg) {
    using D = Conv1Dual<G>;
    constexpr int NPIX = G::NPIX, COUT = G::COUT, KSTEPS = G::K / 32;
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_img[G::IMG];
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_scr[4 * D::SCR];

    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    const int frow = lane & 15, kseg = (lane >> 4) * 8;
    __hip_bfloat16* scr = s_scr + wave * D::SCR;

    bf16x8 b[2][KSTEPS][2];
    load_b_regs<KSTEPS>(b[0], Wt0, 0, lane);
    load_b_regs<KSTEPS>(b[1], Wt1, 0, lane);
    float bias_c[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        bias_c[0][j] = bias0[j * 16 + frow];
        bias_c[1][j] = bias1[j * 16 + frow];
    }
    // this lane's k segment inside the patch: kernel row, then its run
    const int klane = kseg / G::KWC * G::INW * G::CIN + kseg % G::KWC;

    auto load_image = [&](uint2 (&pre)[D::NPRE], long n) {
        const uint2* g = reinterpret_cast<const uint2*>(in + n * G::IMG);
#pragma unroll
        for (int c = 0; c < D::NPRE; ++c) {
            int e8 = threadIdx.x + c * 256;
            if (e8 < D::CHUNKS) pre[c] = g[e8];
        }
    };

    // row fragments f0 .. f0 + NI - 1 of image n, both networks
    auto tile = [&](auto ni, int f0, long n) {
        constexpr int NI = decltype(ni)::value;
        int pbase[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int pp = (f0 + i) * 16 + frow;
            pbase[i] = (pp / G::OW * G::INW + pp % G::OW) * G::S * G::CIN
                       + klane;
        }
        f32x4 acc[2][NI][2] = {};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            bf16x8 a[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                a[i] = lds_patch_row<G::CIN>(
                    &s_img[pbase[i] + ks * D::KS_STEP]);
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[q][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[i], b[q][ks][j], acc[q][i][j], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            for_each_acc(acc[q], lane, [&](int r, int c, float v) {
                v += bias_c[q][c / 16];
                scr[r * D::SCR_LD + c] = f2bf(fmaxf(v, 0.f));
            });
            // the scratch is this wave's own: order its writes before the
            // other lanes' reads, and those before the next tile's writes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __hip_bfloat16* go =
                (q ? out1 : out0) + (n * NPIX + f0 * 16) * COUT + lane * 8;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                *reinterpret_cast<bf16x8*>(go + i * 16 * COUT) =
                    *reinterpret_cast<const bf16x8*>(
                        &scr[(i * 16 + lane / 4) * D::SCR_LD + lane % 4 * 8]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };

    const long n0 = (long)blockIdx.x * imgs_per_wg;
    const long n1 = min((long)N, n0 + imgs_per_wg);
    if (n0 >= n1) return;
    const int f0 = wave == 0 ? 0 : 1 + wave * D::PER_WAVE;
    uint2 pre[D::NPRE];
    load_image(pre, n0);
    for (long n = n0; n < n1; ++n) {
        __syncthreads();    // every read of the previous image is done
#pragma unroll
        for (int c = 0; c < D::NPRE; ++c) {
            int e8 = threadIdx.x + c * 256;
            if (e8 < D::CHUNKS)
                *reinterpret_cast<bf16x8*>(&s_img[e8 * 8]) =
                    dequant8(pre[c].x, pre[c].y);
        }
        __syncthreads();
        if (n + 1 < n1) load_image(pre, n + 1);

        for (int t = 0; t < D::PER_WAVE; t += 2)
            tile(std::integral_constant<int, 2>{}, f0 + t, n);
        if (wave == 0)
            tile(std::integral_constant<int, 1>{}, D::PER_WAVE, n);
    }
}

// ---------------------------------------------------------------------------
// conv_dgrad_band: per-image dgrad, one launch per layer.  Same sums as
// conv_dgrad_dense_kernel — k runs tap-major, co-minor, 32 per MFMA step, in
// the parity class's tap order, out-of-image taps issued as zero fragments —
// so the result is bit-equal to it; what changes is where the operands come
// from and how dX leaves:
//   dY  the image's dense pre-masked gradient is staged ONCE in LDS inside a
//       zero halo (TH-1 / TW-1 pixels per side), so the tap of class row
//       (yy, xx) is the 16-byte LDS read at pixel (yy - jy, xx - jx) with a
//       compile-time tap offset and no bounds check.  The staged grid is the
//       same for every parity class: all S*S classes run on one staged dY.
//       Pixel stride 160 B and the row strides below were enumerated on the
//       host over the ds_read_b128 lane groups for every 16-row fragment of
//       both layers, row wraps included: no bank is hit twice.
//   W   in registers (load_b_regs).  conv3 (one class): waves are 2 row
//       halves x 2 column halves of 32.  conv2 (four classes of 32 columns):
//       wave w owns class w, 64 VGPRs of weights.
//   dX  the accumulators are assembled as the image's bf16 dX in LDS (the
//       four classes interleave into whole rows), then masked by the layer
//       below's ReLU and stored with 16-byte coalesced accesses.
// The next image's dY and this image's mask are loaded into registers before
// the MFMA loop; two barriers per image.
// ---------------------------------------------------------------------------
template <class G>
struct DgradBand {
    static constexpr int S = G::S, NCLS = S * S;
    static constexpr int TH = G::KH / S, TW = G::KW / S;   // taps per class
    static constexpr int HY = TH - 1, HX = TW - 1;         // halo
    static constexpr int SH = G::OH + 2 * HY, SW = G::OW + 2 * HX;
    static constexpr int PS = G::COUT + 16;                // 160 B
    static constexpr int RS = NCLS == 1 ? 976 : 928;       // see above
    static constexpr int DY_SIZE = SH * RS;
    static constexpr int PSX = G::CIN + 8;                 // dX pixel stride
    static constexpr int DX_SIZE = G::INH * G::INW * PSX;
    static constexpr int K = G::TAPS * G::COUT, KSTEPS = K / 32;
    static constexpr int NROWS = G::CLS_H * G::CLS_W;      // rows per class
    static constexpr int NFRAG = (NROWS + 15) / 16;
    // one class: 2 x 2 waves; four classes: one wave each, all its rows
    static constexpr int NI = NCLS == 1 ? (NFRAG + 1) / 2 : NFRAG;
    static constexpr int DY_CHUNKS = G::NPIX * G::COUT / 8;
    static constexpr int DX_CHUNKS = G::IMG / 8;
    static constexpr int NDY = (DY_CHUNKS + 255) / 256;
    static constexpr int NDX = (DX_CHUNKS + 255) / 256;
    static_assert(G::COUT == 64 && RS >= SW * PS && RS % 8 == 0);
    static_assert((NCLS == 1 && G::CIN == 64) || (NCLS == 4 && G::CIN == 32),
                  "wave split: 2x2 over 64 columns, or one class per wave");
    static_assert((DY_SIZE + DX_SIZE) * 2 <= 64 * 1024);
};

template <class G, bool OUT_MASK>
__global__ __launch_bounds__(256, 2) void conv_dgrad_band_kernel(
    const __hip_bfloat16* __restrict__ dY,   // (N, OH, OW, COUT)
    const __hip_bfloat16* __restrict__ Wd,   // (NCLS, CIN, TAPS*COUT)
    const __hip_bfloat16* __restrict__ actx, // (N, INH, INW, CIN) or null
    __hip_bfloat16* __restrict__ dX,         // (N, INH, INW, CIN)
    int N, int imgs_per_wg) {
    using D = DgradBand<G>;
    constexpr int COUT = G::COUT, CIN = G::CIN;
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_dy[D::DY_SIZE];
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_dx[D::DX_SIZE];

    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    const int cls = D::NCLS == 1 ? 0 : wave;
    const int frag0 = D::NCLS == 1 ? (wave >> 1) * D::NI : 0;
    const int col0 = D::NCLS == 1 ? (wave & 1) * 32 : 0;
    const int py = cls / G::S, px = cls % G::S;
    const int frow = lane & 15, kseg = (lane >> 4) * 8;

    bf16x8 b[D::KSTEPS][2];
    load_b_regs<D::KSTEPS>(b, Wd + (long)cls * CIN * D::K, col0, lane);

    // staged-dY offset of this lane's class row in each fragment, at tap
    // (0, 0); rows past the class grid read its last row and are not stored
    int abase[D::NI];
#pragma unroll
    for (int i = 0; i < D::NI; ++i) {
        int q = min((frag0 + i) * 16 + frow, D::NROWS - 1);
        abase[i] = (q / G::CLS_W + D::HY) * D::RS
                   + (q % G::CLS_W + D::HX) * D::PS + kseg;
    }
    // where this thread's 16-byte chunks of dY land in the halo'd image
    int dyoff[D::NDY];
#pragma unroll
    for (int c = 0; c < D::NDY; ++c) {
        int e8 = min((int)threadIdx.x + c * 256, D::DY_CHUNKS - 1);
        int pix = e8 / (COUT / 8);
        dyoff[c] = (pix / G::OW + D::HY) * D::RS
                   + (pix % G::OW + D::HX) * D::PS + e8 % (COUT / 8) * 8;
    }
    auto load_dy = [&](bf16x8 (&pre)[D::NDY], long n) {
        const __hip_bfloat16* g = dY + n * (G::NPIX * COUT);
#pragma unroll
        for (int c = 0; c < D::NDY; ++c) {
            int e8 = threadIdx.x + c * 256;
            if (e8 < D::DY_CHUNKS) pre[c] = load_bf16x8(g + e8 * 8);
        }
    };

    const long n0 = (long)blockIdx.x * imgs_per_wg;
    const long n1 = min((long)N, n0 + imgs_per_wg);
    if (n0 >= n1) return;
    bf16x8 pre[D::NDY];
    load_dy(pre, n0);
    for (int e = threadIdx.x * 8; e < D::DY_SIZE; e += 256 * 8)
        *reinterpret_cast<bf16x8*>(&s_dy[e]) = zero_bf16x8();
    __syncthreads();    // halo zeroed before anyone stages into the image

    for (long n = n0; n < n1; ++n) {
#pragma unroll
        for (int c = 0; c < D::NDY; ++c)
            if ((int)threadIdx.x + c * 256 < D::DY_CHUNKS)
                *reinterpret_cast<bf16x8*>(&s_dy[dyoff[c]]) = pre[c];
        __syncthreads();    // dY staged; the previous image's dX is stored
        if (n + 1 < n1) load_dy(pre, n + 1);
        bf16x8 mask[D::NDX];
        if (OUT_MASK) {
#pragma unroll
            for (int c = 0; c < D::NDX; ++c) {
                int e8 = threadIdx.x + c * 256;
                if (e8 < D::DX_CHUNKS)
                    mask[c] = load_bf16x8(actx + n * G::IMG + e8 * 8);
            }
        }

        f32x4 acc[D::NI][2] = {};
#pragma unroll
        for (int ks = 0; ks < D::KSTEPS; ++ks) {
            constexpr int PER_TAP = COUT / 32;
            const int t = ks / PER_TAP;
            const int off = -((t / D::TW) * D::RS + (t % D::TW) * D::PS)
                            + (ks % PER_TAP) * 32;
            bf16x8 a[D::NI];
#pragma unroll
            for (int i = 0; i < D::NI; ++i)
                a[i] = *reinterpret_cast<const bf16x8*>(&s_dy[abase[i] + off]);
#pragma unroll
            for (int i = 0; i < D::NI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[i], b[ks][j], acc[i][j], 0, 0, 0);
        }

        for_each_acc(acc, lane, [&](int r, int c, float v) {
            int q = frag0 * 16 + r;
            if (q < D::NROWS) {
                int y = py + q / G::CLS_W * G::S, x = px + q % G::CLS_W * G::S;
                s_dx[(y * G::INW + x) * D::PSX + col0 + c] = f2bf(v);
            }
        });
        __syncthreads();    // dX assembled; every read of s_dy is done

        __hip_bfloat16* gx = dX + n * G::IMG;
#pragma unroll
        for (int c = 0; c < D::NDX; ++c) {
            int e8 = threadIdx.x + c * 256;
            if (e8 < D::DX_CHUNKS) {
                bf16x8 v = *reinterpret_cast<const bf16x8*>(
                    &s_dx[e8 / (CIN / 8) * D::PSX + e8 % (CIN / 8) * 8]);
                if (OUT_MASK) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        v[e] = ((float)mask[c][e] > 0.f) ? v[e] : (__bf16)0.f;
                }
                *reinterpret_cast<bf16x8*>(gx + e8 * 8) = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

// conv_id: 1 = Conv1<cin1> (cin1 taken from the input's channel dimension),
//          2 = Conv2, 3 = Conv3.  Calls f with a value of the layer's type.
template <class F>
static void dispatch_layer(int64_t conv_id, int cin1, const char* who, F&& f) {
    if (conv_id == 1 && cin1 == 1) f(Conv1<1>{});
    else if (conv_id == 1 && cin1 == 4) f(Conv1<4>{});
    else if (conv_id == 2) f(Conv2{});
    else if (conv_id == 3) f(Conv3{});
    else TORCH_CHECK(false, who, ": unknown conv_id ", conv_id);
}

// conv1 input guard.  The kernels index the frames as a dense (N, INH, INW,
// CIN) u8 array and load them `wide` bytes at a time from data_ptr, so a
// strided view or a base pointer off that alignment must raise here, before
// any launch.  Returns CIN (1 = single frame, 4 = frame stack), 0 for the
// other layers; `wide1` / `wide4` are the widest global load the chosen
// kernel issues per variant.
static int conv1_cin(int64_t conv_id, const torch::Tensor& in, int64_t N,
                     int wide1, int wide4, const char* who) {
    if (conv_id != 1) return 0;
    constexpr int64_t INH = Conv1<4>::INH, INW = Conv1<4>::INW;
    TORCH_CHECK(in.is_cuda() && in.dtype() == torch::kUInt8, who,
                ": conv1 input must be a uint8 device tensor");
    TORCH_CHECK(in.dim() == 4 && in.size(0) == N && in.size(1) == INH
                && in.size(2) == INW, who,
                ": conv1 input must be (N, H, W, C) = (", N, ", ", INH, ", ",
                INW, ", C), got ", in.sizes());
    int64_t C = in.size(3);
    TORCH_CHECK(C == 1 || C == 4, who,
                ": conv1 is instantiated for 1 or 4 input channels, got ", C);
    TORCH_CHECK(in.is_contiguous(), who, ": conv1 input must be contiguous");
    int wide = (C == 1) ? wide1 : wide4;
    TORCH_CHECK(reinterpret_cast<uintptr_t>(in.data_ptr()) % wide == 0, who,
                ": conv1 input data_ptr must be ", wide, "-byte aligned");
    return (int)C;
}

// the bf16 layers take the previous layer's (N*NPIX, COUT) output as their
// (N, INH, INW, CIN) input: same elements, so only the count is checked
template <class G>
static void check_input(const torch::Tensor& in, int64_t N, const char* who) {
    if (G::IN_U8) return;                      // conv1_cin has checked it
    TORCH_CHECK(in.is_cuda() && in.dtype() == torch::kBFloat16
                && in.is_contiguous() && in.numel() == N * G::IMG, who,
                ": input must be a contiguous bf16 device tensor of ", N, " x ",
                G::INH, " x ", G::INW, " x ", G::CIN, " elements");
}

template <class G>
static void check_weights(const torch::Tensor& Wt, const char* who) {
    TORCH_CHECK(Wt.dim() == 2 && Wt.size(0) == G::COUT && Wt.size(1) == G::K,
                who, ": weights must be (", G::COUT, ", ", G::K, "), got ",
                Wt.sizes());
}

template <class G>
static void check_grads(const torch::Tensor& dY, const torch::Tensor& act,
                        int64_t N, const char* who) {
    // an empty act = no mask: dY is pre-masked (as gemm_dgrad's convention)
    bool has_m = act.defined() && act.numel() > 0;
    TORCH_CHECK(N > 0 && dY.numel() == N * G::NPIX * G::COUT
                && (!has_m || act.numel() == dY.numel()), who,
                ": dY and a non-empty act must be (N*", G::NPIX, ", ", G::COUT,
                "), got ", dY.sizes(), " and ", act.sizes());
    // rows are staged with 16-byte loads
    for (const torch::Tensor* t : {&dY, &act})
        TORCH_CHECK((t == &act && !has_m)
                    || (t->is_cuda() && t->dtype() == torch::kBFloat16
                        && t->is_contiguous()
                        && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0),
                    who, ": dY/act must be contiguous, 16-byte aligned bf16 "
                    "device tensors");
}

// Destination of the slab path: the partial-sum workspace (at least `parts`
// slots) and the .grad views the reducer overwrites, in torch layout.
template <class G>
static void check_wgrad_dest(const torch::Tensor& ws, const torch::Tensor& dW,
                             const torch::Tensor& db, int parts,
                             const char* who) {
    constexpr long SLOT = WgradTile<G>::SLOT;
    TORCH_CHECK(ws.is_cuda() && ws.dtype() == torch::kFloat32
                && ws.is_contiguous()
                && reinterpret_cast<uintptr_t>(ws.data_ptr()) % 16 == 0
                && ws.numel() >= parts * SLOT, who,
                ": the workspace must be a contiguous, 16-byte aligned f32 "
                "device tensor of at least ", parts, " x ", SLOT,
                " elements, got ", ws.numel());
    TORCH_CHECK(dW.is_cuda() && dW.dtype() == torch::kFloat32
                && dW.is_contiguous() && dW.dim() == 4
                && dW.size(0) == G::COUT && dW.size(1) == G::CIN
                && dW.size(2) == G::KH && dW.size(3) == G::KW, who,
                ": dW must be a contiguous f32 device tensor (", G::COUT, ", ",
                G::CIN, ", ", G::KH, ", ", G::KW, "), got ", dW.sizes());
    TORCH_CHECK(db.is_cuda() && db.dtype() == torch::kFloat32
                && db.is_contiguous() && db.dim() == 1
                && db.size(0) == G::COUT, who,
                ": db must be a contiguous f32 device tensor (", G::COUT, ")");
}

template <class G>
static void launch_wgrad_reduce(const torch::Tensor& ws, int parts,
                                const torch::Tensor& dW,
                                const torch::Tensor& db) {
    hipLaunchKernelGGL(
        (wgrad_reduce_kernel<G>), dim3(WgradTile<G>::SLOT / 64), dim3(256), 0,
        at::cuda::getCurrentCUDAStream().stream(), ws.data_ptr<float>(), parts,
        dW.data_ptr<float>(), db.data_ptr<float>());
}

// the geometry arguments of the classic entry points must name the layer
template <class G>
static void check_geometry(int64_t INH, int64_t INW, int64_t OH, int64_t OW,
                           int64_t COUT, int64_t K, const char* who) {
    TORCH_CHECK(INH == G::INH && INW == G::INW && OH == G::OH && OW == G::OW
                && COUT == G::COUT && K == G::K, who,
                ": this layer is ", G::INH, "x", G::INW, " -> ", G::OH, "x",
                G::OW, ", COUT ", G::COUT, ", K ", G::K, "; got ", INH, "x",
                INW, " -> ", OH, "x", OW, ", COUT ", COUT, ", K ", K);
}

torch::Tensor conv_fwd(torch::Tensor in, torch::Tensor Wt, torch::Tensor bias,
                       int64_t conv_id, int64_t N, int64_t INH, int64_t INW,
                       int64_t OH, int64_t OW, bool relu) {
    const char* who = "conv_fwd";
    torch::Tensor out;
    int cin1 = conv1_cin(conv_id, in, N, 4, 8, who);
    dispatch_layer(conv_id, cin1, who, [&](auto g) {
        using G = decltype(g);
        check_weights<G>(Wt, who);
        check_geometry<G>(INH, INW, OH, OW, Wt.size(0), Wt.size(1), who);
        check_input<G>(in, N, who);
        long M = N * G::NPIX;
        out = torch::empty({M, G::COUT}, in.options().dtype(torch::kBFloat16));
        dim3 grid(cdiv(M, WarpTile<tile_ncol<G::COUT>>::ROWS),
                  cdiv(G::COUT, 64));
        hipLaunchKernelGGL(
            (conv_fwd_kernel<G, true>), grid, dim3(256), 0,
            at::cuda::getCurrentCUDAStream().stream(), in.data_ptr(),
            reinterpret_cast<const __hip_bfloat16*>(Wt.data_ptr()),
            bias.data_ptr<float>(),
            reinterpret_cast<__hip_bfloat16*>(out.data_ptr()), (int)M);
    });
    return out;
}

// dense-input dgrad: dY is the UNPADDED, PRE-MASKED upstream gradient
// (N, OH, OW, COUT); actx (optional) fuses the ReLU mask of the conv below
// into the dX store.  Instantiated for conv3 and conv2 (conv1 has no dX).
template <class G>
static bool dgrad_dense_is(int64_t OH, int64_t OW, int64_t COUT, int64_t XH,
                           int64_t XW, int64_t CIN, int64_t S) {
    return OH == G::OH && OW == G::OW && COUT == G::COUT && XH == G::INH
           && XW == G::INW && CIN == G::CIN && S == G::S;
}

template <class G>
static void dgrad_dense_launch(const torch::Tensor& dY, const torch::Tensor& Wd,
                               const torch::Tensor& taps,
                               const torch::Tensor& actx, int64_t N,
                               int64_t y0, int64_t x0, torch::Tensor& dX) {
    const char* who = "conv_dgrad_dense";
    TORCH_CHECK(taps.dtype() == torch::kInt32 && taps.dim() == 2
                && taps.size(0) == G::TAPS && taps.size(1) == 2, who,
                ": taps must be int32 (", G::TAPS, ", 2), got ", taps.sizes());
    TORCH_CHECK(Wd.dim() == 2 && Wd.size(0) == G::CIN
                && Wd.size(1) == G::TAPS * G::COUT, who, ": Wd must be (",
                G::CIN, ", ", G::TAPS * G::COUT, "), got ", Wd.sizes());
    TORCH_CHECK(dY.numel() == N * G::NPIX * G::COUT && dX.numel() == N * G::IMG,
                who, ": dY must hold N*", G::NPIX * G::COUT, " and dX N*",
                G::IMG, " elements for N = ", N);
    TORCH_CHECK(y0 >= 0 && y0 < G::S && x0 >= 0 && x0 < G::S, who,
                ": parity offsets must lie in [0, ", G::S, ")");
    bool has_m = actx.defined() && actx.numel() > 0;
    if (has_m) TORCH_CHECK(actx.numel() == dX.numel());
    long Mc = N * G::CLS_H * G::CLS_W;
    dim3 grid(cdiv(Mc, WarpTile<tile_ncol<G::CIN>>::ROWS), cdiv(G::CIN, 64));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(
            kernel, grid, dim3(256), 0,
            at::cuda::getCurrentCUDAStream().stream(),
            reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr()),
            reinterpret_cast<const __hip_bfloat16*>(Wd.data_ptr()),
            has_m ? reinterpret_cast<const __hip_bfloat16*>(actx.data_ptr())
                  : nullptr,
            reinterpret_cast<__hip_bfloat16*>(dX.data_ptr()),
            taps.data_ptr<int>(), (int)Mc, (int)y0, (int)x0);
    };
    if (has_m) launch(conv_dgrad_dense_kernel<G, true>);
    else launch(conv_dgrad_dense_kernel<G, false>);
}

torch::Tensor conv_dgrad_dense(torch::Tensor dY, torch::Tensor Wd,
                               torch::Tensor taps, torch::Tensor actx,
                               int64_t N, int64_t OH, int64_t OW, int64_t COUT,
                               int64_t XH, int64_t XW, int64_t CIN,
                               int64_t y0, int64_t x0, int64_t S,
                               torch::Tensor dX) {
    if (dgrad_dense_is<Conv3>(OH, OW, COUT, XH, XW, CIN, S))
        dgrad_dense_launch<Conv3>(dY, Wd, taps, actx, N, y0, x0, dX);
    else if (dgrad_dense_is<Conv2>(OH, OW, COUT, XH, XW, CIN, S))
        dgrad_dense_launch<Conv2>(dY, Wd, taps, actx, N, y0, x0, dX);
    else
        TORCH_CHECK(false, "conv_dgrad_dense: only conv3 (", Conv3::OH, "x",
                    Conv3::OW, "x", Conv3::COUT, " -> ", Conv3::INH, "x",
                    Conv3::INW, "x", Conv3::CIN, ", stride ", Conv3::S,
                    ") and conv2 (", Conv2::OH, "x", Conv2::OW, "x",
                    Conv2::COUT, " -> ", Conv2::INH, "x", Conv2::INW, "x",
                    Conv2::CIN, ", stride ", Conv2::S,
                    ") are instantiated; got ", OH, "x", OW, "x", COUT, " -> ",
                    XH, "x", XW, "x", CIN, ", stride ", S);
    return dX;
}

// images per workgroup and grid for the per-image kernels: `wgs` workgroups
// at the most, every one with the same run of images but the last
static void band_grid(int64_t N, int64_t wgs, int& imgs, int& grid) {
    imgs = cdiv(N, std::max<int64_t>(1, wgs));
    grid = cdiv(N, imgs);
}

// per-image band forward.  N = number of images (B*T).  max_wgs > 0 caps the
// grid (tests push several images through one workgroup with it).
torch::Tensor conv_fwd_band(torch::Tensor in, torch::Tensor Wt,
                            torch::Tensor bias, int64_t conv_id, int64_t N,
                            int64_t max_wgs) {
    const char* who = "conv_fwd_band";
    torch::Tensor out;
    TORCH_CHECK(N > 0 && max_wgs >= 0, who, ": N must be positive and max_wgs "
                "non-negative");
    // whole-image staging loads 8 bytes per lane for both conv1 variants
    int cin1 = conv1_cin(conv_id, in, N, 8, 8, who);
    dispatch_layer(conv_id, cin1, who, [&](auto g) {
        using G = decltype(g);
        check_weights<G>(Wt, who);
        check_input<G>(in, N, who);
        TORCH_CHECK(Wt.is_cuda() && Wt.dtype() == torch::kBFloat16
                    && Wt.is_contiguous()
                    && reinterpret_cast<uintptr_t>(Wt.data_ptr()) % 16 == 0
                    && bias.is_cuda() && bias.dtype() == torch::kFloat32
                    && bias.is_contiguous() && bias.numel() == G::COUT, who,
                    ": weights must be contiguous, 16-byte aligned bf16 and "
                    "bias ", G::COUT, " f32, both on the device");
        out = torch::empty({N * G::NPIX, G::COUT},
                           in.options().dtype(torch::kBFloat16));
        int imgs, grid;
        auto stream = at::cuda::getCurrentCUDAStream().stream();
        auto wt = reinterpret_cast<const __hip_bfloat16*>(Wt.data_ptr());
        auto op = reinterpret_cast<__hip_bfloat16*>(out.data_ptr());
        if constexpr (G::COUT == 64) {
            // one launch for both column halves, weights in registers
            band_grid(N, max_wgs > 0 ? max_wgs : BAND_WGS, imgs, grid);
            hipLaunchKernelGGL(
                (conv_fwd_band64_kernel<G>), dim3(grid), dim3(256), 0, stream,
                in.data_ptr(), wt, bias.data_ptr<float>(), op, (int)N, imgs);
        } else {
            // one-channel conv1 (14 KB images, 5 KB slab) keeps its 2048:
            // 62 us there and at 1024, 72-73 us at 512, 113 at 256
            band_grid(N, max_wgs > 0 ? max_wgs : (G::CIN == 1 ? 2048 : BAND_WGS),
                      imgs, grid);
            for (int co0 = 0; co0 < G::COUT; co0 += BAND_COLS)
                hipLaunchKernelGGL(
                    (conv_fwd_band_kernel<G>), dim3(grid), dim3(256), 0,
                    stream, in.data_ptr(), wt, bias.data_ptr<float>(), op,
                    (int)N, imgs, co0);
        }
    });
    return out;
}

// conv1 of two networks on the same frames (see conv1_fwd_dual_kernel):
// returns {out0, out1}, each bit-equal to conv_fwd_band with that network's
// weights.  Default grids, measured at 5440 images: see docs/KERNELS.md.
constexpr int DUAL_WGS_4CH = 512, DUAL_WGS_1CH = 2048;

std::vector<torch::Tensor> conv1_fwd_dual(torch::Tensor in, torch::Tensor Wt0,
                                          torch::Tensor bias0,
                                          torch::Tensor Wt1,
                                          torch::Tensor bias1, int64_t N,
                                          int64_t max_wgs) {
    const char* who = "conv1_fwd_dual";
    torch::Tensor out0, out1;
    TORCH_CHECK(N > 0 && max_wgs >= 0, who, ": N must be positive and max_wgs "
                "non-negative");
    // the frames are loaded 8 bytes per lane for both channel counts
    int cin1 = conv1_cin(1, in, N, 8, 8, who);
    dispatch_layer(1, cin1, who, [&](auto g) {
        using G = decltype(g);
        if constexpr (G::IN_U8) {
            for (const torch::Tensor* w : {&Wt0, &Wt1}) {
                TORCH_CHECK(w->is_cuda() && w->dtype() == torch::kBFloat16
                            && w->is_contiguous()
                            && reinterpret_cast<uintptr_t>(w->data_ptr()) % 16
                                   == 0, who, ": weights must be contiguous, "
                            "16-byte aligned bf16 device tensors");
                check_weights<G>(*w, who);
            }
            for (const torch::Tensor* b : {&bias0, &bias1})
                TORCH_CHECK(b->is_cuda() && b->dtype() == torch::kFloat32
                            && b->is_contiguous() && b->numel() == G::COUT,
                            who, ": each bias must be ", G::COUT,
                            " contiguous f32 on the device");
            auto opts = in.options().dtype(torch::kBFloat16);
            out0 = torch::empty({N * G::NPIX, G::COUT}, opts);
            out1 = torch::empty({N * G::NPIX, G::COUT}, opts);
            int imgs, grid;
            band_grid(N, max_wgs > 0 ? max_wgs
                         : (G::CIN == 1 ? DUAL_WGS_1CH : DUAL_WGS_4CH),
                      imgs, grid);
            hipLaunchKernelGGL(
                (conv1_fwd_dual_kernel<G>), dim3(grid), dim3(256), 0,
                at::cuda::getCurrentCUDAStream().stream(),
                reinterpret_cast<const unsigned char*>(in.data_ptr()),
                reinterpret_cast<const __hip_bfloat16*>(Wt0.data_ptr()),
                bias0.data_ptr<float>(),
                reinterpret_cast<const __hip_bfloat16*>(Wt1.data_ptr()),
                bias1.data_ptr<float>(),
                reinterpret_cast<__hip_bfloat16*>(out0.data_ptr()),
                reinterpret_cast<__hip_bfloat16*>(out1.data_ptr()), (int)N,
                imgs);
        }
    });
    return {out0, out1};
}

// per-image band dgrad (see conv_dgrad_band_kernel).  dY is the dense,
// pre-masked upstream gradient; Wd holds every parity class's (CIN,
// TAPS*COUT) slab, class (py, px) at index py*S + px; actx (optional) fuses
// the ReLU mask of the conv below into the dX store.  conv2 and conv3 only.
torch::Tensor conv_dgrad_band(torch::Tensor dY, torch::Tensor Wd,
                              torch::Tensor actx, int64_t conv_id, int64_t N,
                              int64_t max_wgs) {
    const char* who = "conv_dgrad_band";
    torch::Tensor dX;
    TORCH_CHECK(conv_id == 2 || conv_id == 3, who,
                ": only conv2 and conv3 have a dgrad, got conv_id ", conv_id);
    TORCH_CHECK(N > 0 && max_wgs >= 0, who, ": N must be positive and max_wgs "
                "non-negative");
    dispatch_layer(conv_id, 0, who, [&](auto g) {
        using G = decltype(g);
        if constexpr (!G::IN_U8) {
            using D = DgradBand<G>;
            bool has_m = actx.defined() && actx.numel() > 0;
            TORCH_CHECK(dY.numel() == N * G::NPIX * G::COUT, who,
                        ": dY must hold N*", G::NPIX * G::COUT, " elements");
            TORCH_CHECK(Wd.dim() >= 2 && Wd.numel() == D::NCLS * G::CIN * D::K
                        && Wd.size(-1) == D::K && Wd.size(-2) == G::CIN, who,
                        ": Wd must be (", D::NCLS, ", ", G::CIN, ", ", D::K,
                        "), got ", Wd.sizes());
            if (has_m)
                TORCH_CHECK(actx.numel() == N * G::IMG, who,
                            ": the mask must hold N*", G::IMG, " elements");
            for (const torch::Tensor* t : {&dY, &Wd, &actx})
                TORCH_CHECK((t == &actx && !has_m)
                            || (t->is_cuda() && t->dtype() == torch::kBFloat16
                                && t->is_contiguous()
                                && reinterpret_cast<uintptr_t>(t->data_ptr())
                                       % 16 == 0), who,
                            ": dY, Wd and the mask must be contiguous, 16-byte "
                            "aligned bf16 device tensors");
            dX = torch::empty({N, G::INH, G::INW, G::CIN}, dY.options());
            int imgs, grid;
            band_grid(N, max_wgs > 0 ? max_wgs : BAND_WGS, imgs, grid);
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(
                    kernel, dim3(grid), dim3(256), 0,
                    at::cuda::getCurrentCUDAStream().stream(),
                    reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr()),
                    reinterpret_cast<const __hip_bfloat16*>(Wd.data_ptr()),
                    has_m ? reinterpret_cast<const __hip_bfloat16*>(
                                actx.data_ptr()) : nullptr,
                    reinterpret_cast<__hip_bfloat16*>(dX.data_ptr()), (int)N,
                    imgs);
            };
            if (has_m) launch(conv_dgrad_band_kernel<G, true>);
            else launch(conv_dgrad_band_kernel<G, false>);
        }
    });
    return dX;
}


// ---------------------------------------------------------------------------
// Wgrad entry points.  Each kernel has two: the returning one (fresh zeros,
// atomic flush, {dWt (COUT, K) packed, db}) and the _into one (slab flush
// into the caller's workspace, then wgrad_reduce_kernel OVERWRITES dW in
// torch layout and db; no zeros, no temporaries, bitwise reproducible).  An
// empty act selects MASK = false in both.  WgradDest is null for the first.
// ---------------------------------------------------------------------------
struct WgradDest {
    const torch::Tensor &ws, &dW, &db;
};

// grid of the band wgrad.  512 workgroups = the 2 per CU that VGPRs
// (conv2/conv3) or LDS (conv1) allow, times 256 CUs: one resident round with
// no tail, and every workgroup fewer is COUT*K flushed floats fewer.
// Measured for 5440 images, atomic flush, 1024 / 512 / 256 workgroups: conv3
// 162 / 122 / 121 us, conv2 170 / 129 / 145, conv1 (4 ch) 217 / 193 / 334.
static void wgrad_band_grid(int64_t N, int64_t max_wgs, int& imgs, int& grid) {
    band_grid(N, max_wgs > 0 ? max_wgs : BAND_WGS, imgs, grid);
}

static std::vector<torch::Tensor> wgrad_band_run(
    const char* who, const torch::Tensor& dY, const torch::Tensor& act,
    const torch::Tensor& in, int64_t conv_id, int64_t N, int64_t max_wgs,
    const WgradDest* dest) {
    torch::Tensor dWt, db;
    TORCH_CHECK(N > 0 && max_wgs >= 0, who, ": N must be positive and max_wgs "
                "non-negative");
    // whole-image staging loads 8 bytes per lane for both conv1 variants
    int cin1 = conv1_cin(conv_id, in, N, 8, 8, who);
    dispatch_layer(conv_id, cin1, who, [&](auto g) {
        using G = decltype(g);
        check_input<G>(in, N, who);
        check_grads<G>(dY, act, N, who);
        int imgs, grid;
        wgrad_band_grid(N, max_wgs, imgs, grid);
        if (dest) check_wgrad_dest<G>(dest->ws, dest->dW, dest->db, grid, who);
        bool mask = act.numel() > 0;
        auto launch = [&](auto kernel, float* w, float* b) {
            hipLaunchKernelGGL(
                kernel, dim3(grid), dim3(256), 0,
                at::cuda::getCurrentCUDAStream().stream(),
                reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr()),
                mask ? reinterpret_cast<const __hip_bfloat16*>(act.data_ptr())
                     : nullptr,
                in.data_ptr(), w, b, (int)N, imgs);
        };
        if (dest) {
            float* w = dest->ws.data_ptr<float>();
            if (mask) launch(conv_wgrad_band_kernel<G, true, true>, w, nullptr);
            else launch(conv_wgrad_band_kernel<G, false, true>, w, nullptr);
            launch_wgrad_reduce<G>(dest->ws, grid, dest->dW, dest->db);
        } else {
            auto f32 = dY.options().dtype(torch::kFloat32);
            dWt = torch::zeros({G::COUT, G::K}, f32);
            db = torch::zeros({G::COUT}, f32);
            float *w = dWt.data_ptr<float>(), *b = db.data_ptr<float>();
            if (mask) launch(conv_wgrad_band_kernel<G, true, false>, w, b);
            else launch(conv_wgrad_band_kernel<G, false, false>, w, b);
        }
    });
    return {dWt, db};
}

// per-image band wgrad (see conv_wgrad_band_kernel).  N = number of images;
// max_wgs > 0 caps the grid (tests push several images through a workgroup).
std::vector<torch::Tensor> conv_wgrad_band(torch::Tensor dY, torch::Tensor act,
                                           torch::Tensor in, int64_t conv_id,
                                           int64_t N, int64_t max_wgs) {
    return wgrad_band_run("conv_wgrad_band", dY, act, in, conv_id, N, max_wgs,
                          nullptr);
}

void conv_wgrad_band_into(torch::Tensor dY, torch::Tensor act,
                          torch::Tensor in, int64_t conv_id, int64_t N,
                          torch::Tensor ws, torch::Tensor dW, torch::Tensor db,
                          int64_t max_wgs) {
    WgradDest dest{ws, dW, db};
    wgrad_band_run("conv_wgrad_band_into", dY, act, in, conv_id, N, max_wgs,
                   &dest);
}

// GEMM rows per workgroup of the chunked wgrad: about 1024 workgroups, whole
// 32-row tiles
static long wgrad_chunk_rows(long M) {
    long target_chunks = 1024;
    long rows = std::max(32L, (M + target_chunks - 1) / target_chunks);
    return ((rows + 31) / 32) * 32;
}

static std::vector<torch::Tensor> wgrad_chunked_run(
    const char* who, const torch::Tensor& dY, const torch::Tensor& act,
    const torch::Tensor& in, int64_t conv_id, int64_t N, int64_t INH,
    int64_t INW, int64_t OH, int64_t OW, int64_t COUT, int64_t K,
    const WgradDest* dest) {
    torch::Tensor dWt, db;
    TORCH_CHECK(N > 0, who, ": N must be positive");
    int cin1 = conv1_cin(conv_id, in, N, 4, 8, who);
    dispatch_layer(conv_id, cin1, who, [&](auto g) {
        using G = decltype(g);
        check_geometry<G>(INH, INW, OH, OW, COUT, K, who);
        check_input<G>(in, N, who);
        check_grads<G>(dY, act, N, who);
        long M = N * G::NPIX;
        long rows_per_chunk = wgrad_chunk_rows(M);
        int grid = cdiv(M, rows_per_chunk);
        if (dest) check_wgrad_dest<G>(dest->ws, dest->dW, dest->db, grid, who);
        bool mask = act.numel() > 0;
        auto launch = [&](auto kernel, float* w, float* b) {
            hipLaunchKernelGGL(
                kernel, dim3(grid), dim3(256), 0,
                at::cuda::getCurrentCUDAStream().stream(),
                reinterpret_cast<const __hip_bfloat16*>(dY.data_ptr()),
                mask ? reinterpret_cast<const __hip_bfloat16*>(act.data_ptr())
                     : nullptr,
                in.data_ptr(), w, b, (int)M, (int)rows_per_chunk);
        };
        if (dest) {
            float* w = dest->ws.data_ptr<float>();
            if (mask) launch(conv_wgrad_kernel<G, true, true>, w, nullptr);
            else launch(conv_wgrad_kernel<G, false, true>, w, nullptr);
            launch_wgrad_reduce<G>(dest->ws, grid, dest->dW, dest->db);
        } else {
            auto f32 = dY.options().dtype(torch::kFloat32);
            dWt = torch::zeros({G::COUT, G::K}, f32);
            db = torch::zeros({G::COUT}, f32);
            float *w = dWt.data_ptr<float>(), *b = db.data_ptr<float>();
            if (mask) launch(conv_wgrad_kernel<G, true, false>, w, b);
            else launch(conv_wgrad_kernel<G, false, false>, w, b);
        }
    });
    return {dWt, db};
}

std::vector<torch::Tensor> conv_wgrad(torch::Tensor dY, torch::Tensor act,
                                      torch::Tensor in, int64_t conv_id,
                                      int64_t N, int64_t INH, int64_t INW,
                                      int64_t OH, int64_t OW, int64_t COUT,
                                      int64_t K) {
    return wgrad_chunked_run("conv_wgrad", dY, act, in, conv_id, N, INH, INW,
                             OH, OW, COUT, K, nullptr);
}

void conv_wgrad_into(torch::Tensor dY, torch::Tensor act, torch::Tensor in,
                     int64_t conv_id, int64_t N, int64_t INH, int64_t INW,
                     int64_t OH, int64_t OW, int64_t COUT, int64_t K,
                     torch::Tensor ws, torch::Tensor dW, torch::Tensor db) {
    WgradDest dest{ws, dW, db};
    wgrad_chunked_run("conv_wgrad_into", dY, act, in, conv_id, N, INH, INW, OH,
                      OW, COUT, K, &dest);
}

// floats of workspace an _into entry point needs for N images at its default
// grid: band = conv_wgrad_band_into, else conv_wgrad_into
int64_t conv_wgrad_ws_floats(int64_t conv_id, int64_t cin1, int64_t N,
                             bool band) {
    int64_t n = 0;
    TORCH_CHECK(N > 0, "conv_wgrad_ws_floats: N must be positive");
    dispatch_layer(conv_id, (int)cin1, "conv_wgrad_ws_floats", [&](auto g) {
        using G = decltype(g);
        int imgs, grid;
        wgrad_band_grid(N, 0, imgs, grid);
        if (!band) grid = cdiv(N * G::NPIX, wgrad_chunk_rows(N * G::NPIX));
        n = (int64_t)grid * WgradTile<G>::SLOT;
    });
    return n;
}
