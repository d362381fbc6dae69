// Fused persistent LSTM kernels (gfx950) — SURVEY.md §2.3 K6, the hard one.
//
// Replaces nn.LSTM + pack_padded_sequence (reference model.py:95-100,136-141;
// 87k hipBLASLt launches per profile) with ONE kernel per direction.
//
// Structure (forward):
// - X = rin @ W_ih^T + b precomputed for all (B, T) steps by the MFMA GEMM.
// - Persistent launch, one workgroup per 16 hidden units x 32-row batch
//   group (x2 networks in one launch = 128 workgroups at 64 rows; 32 rows
//   and fewer run 8-unit slices over one 64-row group).  W_hh slice and
//   the cell state c stay LDS-resident for all T steps; each step
//   bulk-stages the previous h into LDS with coalesced 16 B loads, runs
//   the gate GEMM entirely out of LDS, and advances h/c with vectorized
//   stores.
// - ONE kernel template per direction.  A batch above 64 rows is cut into
//   passes of 64 or 128 rows inside the same launch (lstm_fwd_multi /
//   lstm_bwd_multi); the 64-row entry points are its one-pass case.
// - NO global barrier: the time index makes the h exchange naturally
//   double-buffered, so each step is synchronized by PRODUCER FLAGS only
//   (HIP guide §6 G16 recipe R1: the handed-off bytes ONLY — the h slice
//   forward, dgates[t] backward — go out first, as 16-byte write-through
//   (sc1) stores -> per-wave vmcnt drain -> __syncthreads -> one relaxed
//   agent counter add, with NO release fence; c and the gate stash are
//   read after the launch only and are stored after the publish.  The
//   consumer polls relaxed, ONE agent acquire, that lane's vmcnt wait,
//   __syncthreads, then plain loads).  Loads that do not depend on the
//   recurrence (X[t]; dHext, stash, Cout) are issued BEFORE the await.
//   Flag words are zeroed by a tiny kernel before every launch (a
//   CAPTURED hipMemsetAsync replays a garbage fill value — see
//   zero_gridbar_kernel); max skew
//   between workgroups is self-limiting (each wg is both producer and
//   consumer).  Spins are bounded; a poison word aborts the launch.
// - Per-sample length masks replace pack_padded semantics: masked steps
//   copy h/c through unchanged.
//
// Backward (online net): reverse recurrence with the same counter protocol
// on the dgates stream — one workgroup per 16 hidden units x 16-row batch
// QUARTER (128 workgroups; measured faster than batch halves — the backward
// is CU-coverage bound; 33..48 rows run two 32-row halves); the recurrent
// GEMM streams dgates_{t+1} through a 4-deep register prefetch ring with
// the 4H reduction split across waves.
// The bulk weight gradients (dW_hh, dW_ih, db) and dX are plain GEMMs
// outside the kernel (gemm_wgrad / gemm_dgrad over B*T rows).
//
// Gate order matches torch.nn.LSTM: [i, f, g, o] chunks of H.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

__device__ __forceinline__ void lstore8(__hip_bfloat16* p, bf16x8 v) {
    bf16x8_u r;
    r.v = v;
    *reinterpret_cast<uint4*>(p) = r.u;
}

__device__ __forceinline__ float sigmoidf_(float x) {
    return 1.f / (1.f + __expf(-x));
}

// ---------------------------------------------------------------------------
// Producer-flag hand-off.  flags[slice] counts published time indices of that
// producer slice.  publish: called by ALL threads after the slice stores.
// await: wave 0 polls `nflags` flag words lane-parallel (relaxed), one
// acquire fence, __syncthreads.  Returns false on bounded-spin timeout.
// ---------------------------------------------------------------------------
#define LSTM_MAX_FLAGS 256

__device__ __forceinline__ void publish_slice(unsigned* flag, unsigned value) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(flag, value, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ bool await_slices(unsigned* flags, int nflags,
                                             unsigned value, unsigned* poison) {
    __shared__ unsigned ok_s;
    if (threadIdx.x < WAVE) {
        int lane = threadIdx.x;
        unsigned ok = 1;
        long spins = 0;
        for (;;) {
            unsigned f1 = (lane < nflags)
                ? __hip_atomic_load(&flags[lane], __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT) : ~0u;
            unsigned f2 = (lane + WAVE < nflags)
                ? __hip_atomic_load(&flags[lane + WAVE], __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT) : ~0u;
            if (__all(f1 >= value && f2 >= value)) break;
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (long)2e8) {
                if (lane == 0)
                    __hip_atomic_store(poison, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                ok = 0;
                break;
            }
            if (__hip_atomic_load(poison, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT)) {
                ok = 0;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (lane == 0) ok_s = ok;
    }
    __syncthreads();
    return ok_s != 0;
}

// ---------------------------------------------------------------------------
// Counter-aggregated hand-off (the production protocol): ONE atomic counter
// per (net, batch-half) group on its own cacheline.  publish = drain of the
// write-through payload stores + atomicAdd(1) (the release-fence form
// survives in handoff_counter_bench_kernel, which prices it with nothing
// dirty); await = poll until counter >= nprod * value.  The
// protocol's self-limiting skew (a producer cannot be >1 step ahead of the
// slowest in its group — it must await the whole group before advancing)
// makes the sum threshold equivalent to per-producer flags, at ~2/3 the
// per-step cost (tools/lstm_handoff_bench.py: 2.4 vs 3.4 us at 64 wgs).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void publish_count(unsigned* ctr) {
    // R1 publish: the payload went out as 16-byte sc1 (write-through) stores,
    // so there is NO release fence.  Every wave drains its own stores, the
    // barrier collects the waves, one lane signals.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool await_count(unsigned* ctr, unsigned target,
                                            unsigned* poison) {
    __shared__ unsigned ok_c;
    if (threadIdx.x == 0) {
        unsigned ok = 1;
        long spins = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (long)2e8) {
                __hip_atomic_store(poison, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                ok = 0;
                break;
            }
            if (__hip_atomic_load(poison, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT)) {
                ok = 0;
                break;
            }
        }
        // ONE agent acquire after the match; this lane waits for the
        // invalidate before the barrier lets the other waves load
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ok_c = ok;
    }
    __syncthreads();
    return ok_c != 0;
}

// layout of the workspace (int32 words): [0..255] counters/flags (group g
// uses word g*32 — one cacheline apart), [256] poison
struct GridBar {
    unsigned flags[LSTM_MAX_FLAGS];
    unsigned poison;
};

// ---------------------------------------------------------------------------
// The persistent kernels: one template per direction, any batch in ONE
// launch.
//
// The batch is cut into passes of P = ngroups * BROWS rows.  A workgroup
// owns one (net, UNITS-wide slice, row group) of a pass and, after the T
// steps of pass p, moves on to pass p+1 with its W_hh slice still in LDS —
// a host loop of 64-row launches would reload all 128 x 66 KB of weights
// and run a workspace reset per chunk.  Only the per-pass state is
// re-initialised (s_c / Hout[:,0] forward, s_dh / s_dc backward).  A 64-row
// launch (lstm_fwd / lstm_bwd) is the npasses == 1 case; every pass of a
// larger batch, a partial last one included, runs the layout a 64-row
// launch uses (forward BROWS=32, backward BROWS=16 / KSPLIT=4) with the
// same per-element accumulation order, so every full 64-row chunk is
// bit-equal to lstm_fwd / lstm_bwd on those rows.
//
// Handoff invariant.  The counters are zeroed once per launch and only ever
// grow.  Each workgroup publishes T+1 times per pass (once after the pass
// init, once per step), so when it awaits step t of pass p it has itself
// published  n = p*(T+1) + t + 1  times (backward: p*(T+1) + T - t), and
// the await target is WGS * n.  No workgroup of the group can publish more
// than n times without first passing this same await (the pass-init
// publish follows the last step's publish without an await in between, but
// the NEXT await is again at the publisher's own count).  So while any
// workgroup is still waiting for n, every count is <= n, and the sum
// reaches WGS * n only when ALL counts equal n — the sum threshold stays
// equivalent to per-producer flags across pass boundaries.  The pass-init
// publish releases only rows of the new pass (Hout[:, 0]), which nobody
// reads before passing an await of that pass.
//
// Row groups past the end of the batch (Bl <= 0) write nothing but still
// await and publish, like the empty quarters of a small batch.
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
// BROWS: batch rows per workgroup.  64 = the whole batch in one row group
// (B <= 32).  32 = batch-split: twice the workgroups, half the LDS staging
// per step, counter groups per (net, row group).
// UNITS: hidden units per workgroup.  8 goes with BROWS=64; 16 halves the
// workgroup count (half the handoff producers per counter group AND half
// the total h re-read traffic) at twice the per-wg MFMA work — the per-step
// cost is latency-dominated, so fewer/fatter workgroups win (measured;
// VERDICT r1 item 7).
template <int H, int BROWS, int UNITS>
__global__ __launch_bounds__(256, 1) void lstm_fwd_kernel(
    const __hip_bfloat16* __restrict__ X0,    // (B, T, 4H)
    const __hip_bfloat16* __restrict__ X1,    // or null
    const __hip_bfloat16* __restrict__ Whh0,  // (4H, H) row-major
    const __hip_bfloat16* __restrict__ Whh1,
    const float* __restrict__ init0,          // (2, B, H): h0, c0
    const float* __restrict__ init1,
    const int* __restrict__ lens,             // (B,)
    __hip_bfloat16* __restrict__ Hout0,       // (B, T+1, H)
    __hip_bfloat16* __restrict__ Hout1,
    float* __restrict__ Cout0,                // (B, T+1, H)
    float* __restrict__ Cout1,
    __hip_bfloat16* __restrict__ stash0,      // (B, T, 4H) post-nonlin gates
    GridBar* bar, int B, int T, int ngroups, int npasses) {
    constexpr int WGS = H / UNITS;            // producers per counter group
    constexpr int GCOLS = 4 * UNITS;          // gate columns per wg
    const int wgs_per_net = WGS * ngroups;
    const int net = blockIdx.x / wgs_per_net;
    const int rem = blockIdx.x % wgs_per_net;
    const int grp = rem / WGS;
    const int wid = rem % WGS;
    const int u0 = wid * UNITS;
    const int P = ngroups * BROWS;            // rows per pass

    const __hip_bfloat16* X = net ? X1 : X0;
    const __hip_bfloat16* Whh = net ? Whh1 : Whh0;
    const float* init = net ? init1 : init0;
    __hip_bfloat16* Hout = net ? Hout1 : Hout0;
    float* Cout = net ? Cout1 : Cout0;
    __hip_bfloat16* stash = net ? nullptr : stash0;
    unsigned* ctr = &bar->flags[(net * ngroups + grp) * 32];

    __shared__ __hip_bfloat16 s_whh[GCOLS][H + 8];
    __shared__ __hip_bfloat16 s_h[BROWS][H + 8];
    __shared__ float s_gates[BROWS][GCOLS + 4];
    __shared__ float s_c[BROWS][UNITS];
    __shared__ __hip_bfloat16 s_hrow[BROWS][UNITS];
    __shared__ int s_len[BROWS];

    // loaded ONCE for all passes
    for (int e = threadIdx.x * 8; e < GCOLS * H; e += blockDim.x * 8) {
        int c = e / H;
        int k = e % H;
        int g = c / UNITS, j = c % UNITS;
        lstore8(&s_whh[c][k],
                load_bf16x8(Whh + (long)(g * H + u0 + j) * H + k));
    }

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    // wave tiling over (BROWS rows x GCOLS cols):
    //   GCOLS=32: 2x2 waves of 16x16xNFRAG; GCOLS=64: 4 col-waves, rows
    //   split into BROWS/16 fragments per wave.
    constexpr int NCW = GCOLS / 16;            // col fragments total
    constexpr int NFRAG = (NCW == 4) ? BROWS / 16 : BROWS / 32;
    const int wrow0 = (NCW == 4) ? 0 : (wave >> 1) * 16 * NFRAG;
    const int wcol0 = (NCW == 4) ? wave * 16 : (wave & 1) * 16;
    const int frow = lane & 15;
    const int kseg = (lane >> 4) * 8;

    constexpr int CHUNKS = (BROWS * H) / 8;

    // descriptor of this net's whole Hout for the write-through h stores
    const __amdgpu_buffer_rsrc_t hout_rsrc =
        make_store_rsrc(Hout, (long)B * (T + 1) * H * 2);
    // (row, gate) work that is NOT the handoff — the X loads and the stash
    // stores — goes to the upper waves where the row group has up to 32
    // rows: wave 0 stores the h slice and polls the counter, and a poll
    // waits for everything its wave still has in flight.
    const int xtid = (threadIdx.x + 128) & 255;

    for (int pass = 0; pass < npasses; ++pass) {
        const int b0 = pass * P + grp * BROWS;
        const int Bl = min(B - b0, BROWS);    // <= 0: empty row group
        const unsigned base_pub = (unsigned)pass * (unsigned)(T + 1);
        // the last step's c and stash stores read s_c / s_gates after its
        // publish: let them finish before the pass init rewrites s_c
        if (pass > 0) __syncthreads();
        // The handed-off payload: this wg's (Bl x UNITS) slice of h at time
        // index tt, from s_hrow, as 16-byte write-through stores.
        auto store_h_slice = [&](int tt) {
            constexpr int H8 = UNITS / 8;        // 16-B pieces per h row
            int tid = threadIdx.x;
            if (tid < BROWS * H8) {
                int b = tid / H8, piece = tid % H8;
                if (b < Bl) {
                    long off = ((long)(b0 + b) * (T + 1) + tt) * H + u0
                               + piece * 8;
                    store_bf16x8_sc1(hout_rsrc, off,
                                     *reinterpret_cast<bf16x8*>(
                                         &s_hrow[b][piece * 8]));
                }
            }
        };
        // h0 -> Hout[:,0] (this wg's slice); c0 -> LDS-resident cell state
        for (int p = threadIdx.x; p < Bl * UNITS; p += blockDim.x) {
            int bl = p / UNITS, j = p % UNITS;
            int b = b0 + bl;
            int u = u0 + j;
            s_hrow[bl][j] = f2bf(init[(long)b * H + u]);
            Cout[((long)b * (T + 1)) * H + u] = init[((long)B + b) * H + u];
            s_c[bl][j] = init[((long)B + b) * H + u];
        }
        // the rows' lengths, read once per pass
        if (threadIdx.x < BROWS)
            s_len[threadIdx.x] =
                ((int)threadIdx.x < Bl) ? lens[b0 + threadIdx.x] : 0;
        __syncthreads();
        store_h_slice(0);
        publish_count(ctr);

        for (int t = 0; t < T; ++t) {
            // X[b, t] does not depend on the recurrence: issue this thread's
            // (row, gate) loads BEFORE the await so that the cold-memory
            // latency passes while the workgroup waits for its group
            const int xrow = xtid / 4;
            const int xg = xtid % 4;
            bf16x8 xpre[UNITS / 8];
            if (xrow < Bl) {
#pragma unroll
                for (int j8 = 0; j8 < UNITS; j8 += 8)
                    xpre[j8 / 8] = load_bf16x8(
                        X + ((long)(b0 + xrow) * T + t) * 4 * H + xg * H + u0
                        + j8);
            }
            if (!await_count(ctr, (unsigned)WGS * (base_pub + t + 1),
                             &bar->poison))
                return;
            // bulk-stage this group's h_prev (Bl x H) into LDS
            {
                // All loads first, branch-free (a row past Bl re-reads row
                // Bl-1 and is zeroed on the way into LDS): a branch per
                // load made each of them wait for the one before.
                const long base = (long)t * H;
                constexpr int NST = CHUNKS / 256;
                static_assert(CHUNKS % 256 == 0, "staging pieces per thread");
                bf16x8 hv[NST];
                if (Bl > 0) {
#pragma unroll
                    for (int i = 0; i < NST; ++i) {
                        int e = threadIdx.x + i * 256;
                        int row = min(e / (H / 8), Bl - 1);
                        int k8 = (e % (H / 8)) * 8;
                        hv[i] = load_bf16x8(Hout + ((long)(b0 + row) * (T + 1))
                                            * H + base + k8);
                    }
                }
#pragma unroll
                for (int i = 0; i < NST; ++i) {
                    int e = threadIdx.x + i * 256;
                    int row = e / (H / 8);
                    int k8 = (e % (H / 8)) * 8;
                    lstore8(&s_h[row][k8],
                            (row < Bl) ? hv[i] : zero_bf16x8());
                }
            }
            __syncthreads();

            // gates = h_prev @ Whh_slice^T  (all-LDS MFMA)
            f32x4 acc[NFRAG] = {};
#pragma unroll
            for (int k0 = 0; k0 < H; k0 += 32) {
                bf16x8 bfr = load_bf16x8(&s_whh[wcol0 + frow][k0 + kseg]);
#pragma unroll
                for (int i = 0; i < NFRAG; ++i) {
                    bf16x8 afr =
                        load_bf16x8(&s_h[wrow0 + i * 16 + frow][k0 + kseg]);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        afr, bfr, acc[i], 0, 0, 0);
                }
            }
            {
                int ccol = lane & 15;
                int crow = (lane >> 4) * 4;
#pragma unroll
                for (int i = 0; i < NFRAG; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s_gates[wrow0 + i * 16 + crow + r][wcol0 + ccol] =
                            acc[i][r];
            }
            __syncthreads();
            // + X[t] (vectorized), then nonlinearities + state advance
            if (xrow < Bl) {
#pragma unroll
                for (int j8 = 0; j8 < UNITS; j8 += 8)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        s_gates[xrow][xg * UNITS + j8 + j] +=
                            (float)xpre[j8 / 8][j];
            }
            __syncthreads();
            for (int p = threadIdx.x; p < Bl * UNITS; p += blockDim.x) {
                int b = p / UNITS, j = p % UNITS;
                bool active = t < s_len[b];
                float i_ = 0.f, f_ = 0.f, g_ = 0.f, o_ = 0.f;
                float c = s_c[b][j], h;
                if (active) {
                    i_ = sigmoidf_(s_gates[b][0 * UNITS + j]);
                    f_ = sigmoidf_(s_gates[b][1 * UNITS + j]);
                    g_ = tanhf(s_gates[b][2 * UNITS + j]);
                    o_ = sigmoidf_(s_gates[b][3 * UNITS + j]);
                    c = f_ * c + i_ * g_;
                    h = o_ * tanhf(c);
                } else {
                    h = (float)*(const __bf16*)&s_h[b][u0 + j];
                }
                s_c[b][j] = c;
                *(__bf16*)&s_hrow[b][j] = (__bf16)h;
                s_gates[b][0 * UNITS + j] = i_;
                s_gates[b][1 * UNITS + j] = f_;
                s_gates[b][2 * UNITS + j] = g_;
                s_gates[b][3 * UNITS + j] = o_;
            }
            __syncthreads();
            // Only the h slice is handed off: publish it FIRST (write-through
            // stores, drain, barrier, counter add; no release fence).  c and
            // the gate stash are read after the launch only, so their plain
            // stores follow the publish, off the serial chain.
            store_h_slice(t + 1);
            publish_count(ctr);
            {
                int tid = threadIdx.x;
                if (tid >= 128) {
                    // c writers: threads [128, 256) cover BROWS rows x C4
                    // float4 pieces (BROWS*C4 <= 128 for both layouts)
                    int t2 = tid - 128;
                    constexpr int C4 = UNITS / 4;  // float4 pieces per c row
                    static_assert(BROWS * C4 <= 128, "c-writer thread budget");
                    int b = t2 / C4, ch = t2 % C4;
                    if (b < Bl) {
                        long off = ((long)(b0 + b) * (T + 1) + t + 1) * H + u0
                                   + ch * 4;
                        *reinterpret_cast<float4*>(Cout + off) =
                            *reinterpret_cast<float4*>(&s_c[b][ch * 4]);
                    }
                }
            }
            if (stash) {
                int row = xtid / 4;
                int g = xtid % 4;
                if (row < Bl) {
#pragma unroll
                    for (int j8 = 0; j8 < UNITS; j8 += 8) {
                        bf16x8 v;
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            v[j] = (__bf16)s_gates[row][g * UNITS + j8 + j];
                        lstore8(stash + ((long)(b0 + row) * T + t) * 4 * H
                                + g * H + u0 + j8, v);
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Backward (online net).  H/16 wgs per row group, each 16 hidden units;
// W_hh^T slice in LDS; dgates_{t+1} streamed from global through a register
// ring; counter hand-off on the dgates stream.
// ---------------------------------------------------------------------------
// BROWS: 16 = batch quarters, all four waves on one 16-row tile, each with
// a quarter of the recurrent GEMM's 4H reduction (KSPLIT 4).  32 = batch
// halves: waves tile (row half x K half) (KSPLIT 2).
template <int H, int BROWS, int UNITS>
__global__ __launch_bounds__(256, 1) void lstm_bwd_kernel(
    const __hip_bfloat16* __restrict__ stash,  // (B, T, 4H) i,f,g,o
    const float* __restrict__ Cout,            // (B, T+1, H)
    const float* __restrict__ dHext,           // (B, T, H) upstream
    const __hip_bfloat16* __restrict__ Whh_bwd,// (H, 4H): W_hh^T row-major
    const int* __restrict__ lens,
    __hip_bfloat16* __restrict__ dgates,       // (B, T, 4H) out
    GridBar* bar, int B, int T, int ngroups, int npasses) {
    static_assert(UNITS == 16 && (BROWS == 16 || BROWS == 32),
                  "one 16-col MFMA tile; 4 waves = BROWS/16 row tiles x KSPLIT");
    constexpr int WGS = H / UNITS;
    constexpr int KSPLIT = 64 / BROWS;
    constexpr int NEL = BROWS * UNITS / 256;   // (row, unit) elements per thread
    const int grp = blockIdx.x / WGS;
    const int wid = blockIdx.x % WGS;
    const int u0 = wid * UNITS;
    const int P = ngroups * BROWS;             // rows per pass

    __shared__ __hip_bfloat16 s_wb[UNITS][4 * H + 8];
    __shared__ float s_dh[BROWS][UNITS + 1];
    __shared__ float s_dc[BROWS][UNITS + 1];
    __shared__ float s_rec[KSPLIT][BROWS][UNITS + 1];
    __shared__ __hip_bfloat16 s_dgout[BROWS][4 * UNITS + 8];

    unsigned* ctr = &bar->flags[grp * 32];

    // loaded ONCE for all passes
    for (int e = threadIdx.x * 8; e < UNITS * 4 * H; e += blockDim.x * 8) {
        int c = e / (4 * H);
        int k = e % (4 * H);
        lstore8(&s_wb[c][k], load_bf16x8(Whh_bwd + (long)(u0 + c) * 4 * H + k));
    }

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wrow0 = (KSPLIT == 4) ? 0 : (wave & 1) * 16;
    const int wk = (KSPLIT == 4) ? wave : (wave >> 1);  // this wave's K part
    const int frow = lane & 15;
    const int kseg = (lane >> 4) * 8;
    constexpr int NCHUNK = 4 * H / 32;
    const int c0 = wk * (NCHUNK / KSPLIT);
    const int cN = c0 + NCHUNK / KSPLIT;

    // descriptor of the whole dgates for the write-through stores
    const __amdgpu_buffer_rsrc_t dg_rsrc =
        make_store_rsrc(dgates, (long)B * T * 4 * H * 2);

    for (int pass = 0; pass < npasses; ++pass) {
        const int b0 = pass * P + grp * BROWS;
        const int Bl = min(B - b0, BROWS);     // <= 0: empty row group
        const unsigned base_pub = (unsigned)pass * (unsigned)(T + 1);
        for (int p = threadIdx.x; p < BROWS * UNITS; p += blockDim.x) {
            s_dh[p / UNITS][p % UNITS] = 0.f;
            s_dc[p / UNITS][p % UNITS] = 0.f;
        }
        // this thread's (row, unit) elements keep their rows for the whole
        // pass: the rows' lengths are read once
        int len_r[NEL];
#pragma unroll
        for (int e = 0; e < NEL; ++e) {
            int p = threadIdx.x + e * 256;
            len_r[e] = (p < Bl * UNITS) ? lens[b0 + p / UNITS] : 0;
        }
        publish_count(ctr);

        for (int t = T - 1; t >= 0; --t) {
            // Everything the pointwise step reads from global is a product
            // of the forward or of the heads, none of it written in this
            // launch: issue the loads BEFORE the await, so that they land
            // while the workgroup waits for its group.  Rows past Bl are
            // not read, nor is the stash at t + 1 = T.
            struct {
                float ext, c_next, c_prev;
                __hip_bfloat16 i, f, g, o, f_next;
            } pre[NEL];
#pragma unroll
            for (int e = 0; e < NEL; ++e) {
                int p = threadIdx.x + e * 256;
                if (p >= Bl * UNITS) break;
                int bg = b0 + p / UNITS;
                int u = u0 + p % UNITS;
                long so = ((long)bg * T + t) * 4 * H + u;
                long co = ((long)bg * (T + 1) + t) * H + u;
                pre[e].ext = dHext[((long)bg * T + t) * H + u];
                pre[e].i = stash[so];
                pre[e].f = stash[so + H];
                pre[e].g = stash[so + 2 * H];
                pre[e].o = stash[so + 3 * H];
                pre[e].c_prev = Cout[co];
                pre[e].c_next = Cout[co + H];
                if (t + 1 < T) pre[e].f_next = stash[so + 4 * H + H];
            }
            unsigned need = (unsigned)(T - t);  // pieces published for t+1
            if (!await_count(ctr, (unsigned)WGS * (base_pub + need),
                             &bar->poison))
                return;
            // rec(B,UNITS) = dgates_{t+1}(B,4H) @ s_wb^T with a 4-deep register
            // prefetch ring on the dgates stream (loads stay in flight across
            // MFMAs; no per-piece barriers)
            if (t < T - 1) {
                const int arow_l = wrow0 + frow;
                const __hip_bfloat16* dgrow =
                    dgates + ((long)(b0 + arow_l) * T + t + 1) * 4 * H;
                const bool rvalid = arow_l < Bl;
                f32x4 acc = {};
                bf16x8 a0 = rvalid ? load_bf16x8(dgrow + (c0 + 0) * 32 + kseg)
                    : zero_bf16x8();
                bf16x8 a1 = rvalid ? load_bf16x8(dgrow + (c0 + 1) * 32 + kseg)
                    : zero_bf16x8();
                bf16x8 a2 = rvalid ? load_bf16x8(dgrow + (c0 + 2) * 32 + kseg)
                    : zero_bf16x8();
                bf16x8 a3 = rvalid ? load_bf16x8(dgrow + (c0 + 3) * 32 + kseg)
                    : zero_bf16x8();
#pragma unroll 4
                for (int kc = c0; kc < cN; kc += 4) {
                    bf16x8 w0 = load_bf16x8(&s_wb[frow][(kc + 0) * 32 + kseg]);
                    bf16x8 w1 = load_bf16x8(&s_wb[frow][(kc + 1) * 32 + kseg]);
                    bf16x8 w2 = load_bf16x8(&s_wb[frow][(kc + 2) * 32 + kseg]);
                    bf16x8 w3 = load_bf16x8(&s_wb[frow][(kc + 3) * 32 + kseg]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, w0, acc, 0, 0, 0);
                    if (kc + 4 < cN)
                        a0 = rvalid ? load_bf16x8(dgrow + (kc + 4) * 32 + kseg)
                            : zero_bf16x8();
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, w1, acc, 0, 0, 0);
                    if (kc + 5 < cN)
                        a1 = rvalid ? load_bf16x8(dgrow + (kc + 5) * 32 + kseg)
                            : zero_bf16x8();
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, w2, acc, 0, 0, 0);
                    if (kc + 6 < cN)
                        a2 = rvalid ? load_bf16x8(dgrow + (kc + 6) * 32 + kseg)
                            : zero_bf16x8();
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, w3, acc, 0, 0, 0);
                    if (kc + 7 < cN)
                        a3 = rvalid ? load_bf16x8(dgrow + (kc + 7) * 32 + kseg)
                            : zero_bf16x8();
                }
                int ccol = lane & 15;
                int crow = (lane >> 4) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s_rec[wk][wrow0 + crow + r][ccol] = acc[r];
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < NEL; ++e) {
                int p = threadIdx.x + e * 256;
                if (p >= Bl * UNITS) break;
                int b = p / UNITS, jl = p % UNITS;
                float dh, dc_in;
                bool last = (t == T - 1);
                bool active_next = !last && ((t + 1) < len_r[e]);
                float ext = pre[e].ext;
                float rec = s_rec[0][b][jl];
#pragma unroll
                for (int kk = 1; kk < KSPLIT; ++kk) rec += s_rec[kk][b][jl];
                if (last) {
                    dh = ext;
                    dc_in = 0.f;
                } else if (active_next) {
                    float f_next = bf2f(pre[e].f_next);
                    dh = ext + rec;
                    dc_in = s_dc[b][jl] * f_next;
                } else {
                    dh = ext + s_dh[b][jl];
                    dc_in = s_dc[b][jl];
                }
                bool active = t < len_r[e];
                float di = 0.f, df = 0.f, dg = 0.f, do_ = 0.f;
                if (active) {
                    float i_ = bf2f(pre[e].i);
                    float f_ = bf2f(pre[e].f);
                    float g_ = bf2f(pre[e].g);
                    float o_ = bf2f(pre[e].o);
                    float tc = tanhf(pre[e].c_next);
                    float c_prev = pre[e].c_prev;
                    float dc = dc_in + dh * o_ * (1.f - tc * tc);
                    di = dc * g_ * i_ * (1.f - i_);
                    df = dc * c_prev * f_ * (1.f - f_);
                    dg = dc * i_ * (1.f - g_ * g_);
                    do_ = dh * tc * o_ * (1.f - o_);
                    s_dh[b][jl] = dh;
                    s_dc[b][jl] = dc;
                } else {
                    s_dh[b][jl] = dh;
                    s_dc[b][jl] = dc_in;
                }
                *(__bf16*)&s_dgout[b][0 * UNITS + jl] = (__bf16)di;
                *(__bf16*)&s_dgout[b][1 * UNITS + jl] = (__bf16)df;
                *(__bf16*)&s_dgout[b][2 * UNITS + jl] = (__bf16)dg;
                *(__bf16*)&s_dgout[b][3 * UNITS + jl] = (__bf16)do_;
            }
            __syncthreads();
            // dgates[t] is the whole handed-off payload: thread (b, g) ->
            // UNITS/8 x 16 B write-through stores, then drain, barrier and
            // counter add (no release fence)
            {
                int tid = threadIdx.x;
                int b = tid / 4;
                int g = tid % 4;
                if (b < Bl) {
#pragma unroll
                    for (int rep = 0; rep < UNITS / 8; ++rep) {
                        long off = ((long)(b0 + b) * T + t) * 4 * H + g * H + u0
                                   + rep * 8;
                        store_bf16x8_sc1(dg_rsrc, off,
                                         *reinterpret_cast<bf16x8*>(
                                             &s_dgout[b][g * UNITS + rep * 8]));
                    }
                }
            }
            publish_count(ctr);
        }
    }
}

// counter-aggregated handoff microbench: ONE atomic counter per group —
// publish = single atomicAdd, await = poll one word until nblocks*(t+1).
__global__ void handoff_counter_bench_kernel(GridBar* bar, int steps,
                                             int nblocks) {
    unsigned* ctr = &bar->flags[0];
    for (int t = 0; t < steps; ++t) {
        __syncthreads();
        if (threadIdx.x == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0) {
            long spins = 0;
            while (__hip_atomic_load(ctr, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT)
                   < (unsigned)(nblocks * (t + 1))) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (long)2e8) return;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
    }
}

// The counter handoff under the kernels' real conditions.  Before every
// publish each block stores `kb` KB of its own scratch region, 16 B per lane:
//   mode 0  plain stores, then the release-fence publish (what the LSTM paid
//           while Cout / stash were stored in front of the fence)
//   mode 1  write-through (sc1) stores, drain, barrier, counter add, NO
//           release fence (the publish the LSTM kernels use now)
// scratch holds nblocks * kb KB; block b writes only [b * kb KB, (b+1) * kb KB).
__global__ void handoff_payload_bench_kernel(GridBar* bar,
                                             __hip_bfloat16* scratch,
                                             long scratch_bytes, int steps,
                                             int nblocks, int kb, int mode) {
    unsigned* ctr = &bar->flags[0];
    const __amdgpu_buffer_rsrc_t rsrc = make_store_rsrc(scratch, scratch_bytes);
    const long base = (long)blockIdx.x * kb * 512;     // bf16 elements
    const int pieces = kb * 64;                        // 16-B pieces per block
    __shared__ int dead;
    if (threadIdx.x == 0) dead = 0;
    __syncthreads();
    for (int t = 0; t < steps; ++t) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)(float)(t + j);
        for (int p = threadIdx.x; p < pieces; p += blockDim.x) {
            if (mode == 1) store_bf16x8_sc1(rsrc, base + (long)p * 8, v);
            else lstore8(scratch + base + (long)p * 8, v);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            if (mode == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            long spins = 0;
            while (__hip_atomic_load(ctr, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT)
                   < (unsigned)(nblocks * (t + 1))) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (long)2e8) {
                    __hip_atomic_store(&bar->poison, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                    dead = 1;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (dead) return;          // uniform: every thread reads the LDS flag
    }
}

// ---------------------------------------------------------------------------
// assemble_rin: build the padded LSTM input rows (latent | one-hot action |
// reward | zero pad) in ONE launch (replaces a zeros fill + three slice
// copies per network per step).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assemble_rin_kernel(
    const __hip_bfloat16* __restrict__ latent,  // (M, 512)
    const float* __restrict__ la,               // (M, A)
    const float* __restrict__ lr,               // (M,)
    __hip_bfloat16* __restrict__ rin,           // (M, KP)
    int M, int A, int KP) {
    unsigned idx = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (idx >= (unsigned)M * KP) return;
    int k = (int)(idx % (unsigned)KP);
    unsigned m = idx / (unsigned)KP;
    if (k + 8 <= 512) {
        *reinterpret_cast<bf16x8*>(rin + idx) =
            load_bf16x8(latent + (long)m * 512 + k);
        return;
    }
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int kk = k + e;
        float f = 0.f;
        if (kk < 512) f = bf2f(latent[(long)m * 512 + kk]);
        else if (kk < 512 + A) f = la[(long)m * A + (kk - 512)];
        else if (kk == 512 + A) f = lr[m];
        v[e] = (__bf16)f;
    }
    *reinterpret_cast<bf16x8*>(rin + idx) = v;
}

// handoff-only microbench: prices one flag publish/await round at `nblocks`
__global__ void handoff_bench_kernel(GridBar* bar, int steps, int nblocks) {
    unsigned* flags = bar->flags;
    unsigned* myflag = &flags[blockIdx.x];
    if (threadIdx.x == 0)
        __hip_atomic_store(myflag, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    for (int t = 0; t < steps; ++t) {
        if (!await_slices(flags, nblocks, (unsigned)(t + 1), &bar->poison))
            return;
        publish_slice(myflag, (unsigned)(t + 2));
    }
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

// NOT hipMemsetAsync: a captured memset node replays with a garbage fill
// value from the second hipGraph replay onward (observed on ROCm 7.2,
// gpurun_out/graph_probe2.log — counters came back as <garbage>+increments
// and the poison word as the raw garbage).  A plain kernel replays
// correctly.
__global__ void zero_gridbar_kernel(unsigned* ws) {
    if (threadIdx.x < sizeof(GridBar) / 4) ws[threadIdx.x] = 0u;
}

static void zero_ws(torch::Tensor& ws, hipStream_t stream) {
    TORCH_CHECK(ws.numel() * ws.element_size() >= (long)sizeof(GridBar),
                "barrier workspace too small (need >= 256 int32)");
    hipLaunchKernelGGL(zero_gridbar_kernel, dim3(1), dim3(320), 0, stream,
                       reinterpret_cast<unsigned*>(ws.data_ptr()));
}

torch::Tensor assemble_rin(torch::Tensor latent, torch::Tensor la,
                           torch::Tensor lr, int64_t kin_pad) {
    long M = latent.size(0);
    long A = la.size(1);
    TORCH_CHECK(latent.dtype() == torch::kBFloat16 && latent.is_contiguous());
    TORCH_CHECK(la.dtype() == torch::kFloat32 && la.is_contiguous());
    TORCH_CHECK(kin_pad % 32 == 0 && 512 + A + 1 <= kin_pad);
    auto rin = torch::empty({M, kin_pad}, latent.options());
    long total = M * kin_pad / 8;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(assemble_rin_kernel,
                       dim3((int)((total + 255) / 256)), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const __hip_bfloat16*>(latent.data_ptr()),
                       la.data_ptr<float>(), lr.data_ptr<float>(),
                       reinterpret_cast<__hip_bfloat16*>(rin.data_ptr()),
                       (int)M, (int)A, (int)kin_pad);
    return rin;
}

void handoff_counter_bench(torch::Tensor barrier_ws, int64_t steps,
                           int64_t nblocks) {
    auto stream = at::cuda::getCurrentCUDAStream();
    zero_ws(barrier_ws, stream.stream());
    hipLaunchKernelGGL(handoff_counter_bench_kernel, dim3((int)nblocks),
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<GridBar*>(barrier_ws.data_ptr()),
                       (int)steps, (int)nblocks);
}

void handoff_payload_bench(torch::Tensor barrier_ws, torch::Tensor scratch,
                           int64_t steps, int64_t nblocks, int64_t kb,
                           int64_t mode) {
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous()
                && scratch.scalar_type() == torch::kBFloat16,
                "scratch must be a contiguous CUDA bf16 tensor");
    TORCH_CHECK(nblocks >= 1 && nblocks <= 256 && kb >= 0 && kb <= 64
                && steps >= 1 && (mode == 0 || mode == 1),
                "1 <= nblocks <= 256, 0 <= kb <= 64, mode 0 or 1");
    const long bytes = scratch.numel() * 2;
    TORCH_CHECK(bytes >= nblocks * kb * 1024 && bytes < (1L << 31),
                "scratch must hold nblocks * kb KB");
    auto stream = at::cuda::getCurrentCUDAStream();
    zero_ws(barrier_ws, stream.stream());
    hipLaunchKernelGGL(handoff_payload_bench_kernel, dim3((int)nblocks),
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<GridBar*>(barrier_ws.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(scratch.data_ptr()),
                       bytes, (int)steps, (int)nblocks, (int)kb, (int)mode);
}

void handoff_bench(torch::Tensor barrier_ws, int64_t steps, int64_t nblocks) {
    auto stream = at::cuda::getCurrentCUDAStream();
    zero_ws(barrier_ws, stream.stream());
    hipLaunchKernelGGL(handoff_bench_kernel, dim3((int)nblocks), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<GridBar*>(barrier_ws.data_ptr()),
                       (int)steps, (int)nblocks);
}

// Operand checks shared by the two LSTM wrappers: every one runs BEFORE the
// workspace reset and the launch, so a bad operand raises and nothing runs.
static void lstm_check(const torch::Tensor& t, const char* name,
                       c10::ScalarType dtype,
                       std::initializer_list<int64_t> shape) {
    TORCH_CHECK(t.defined() && t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ",
                t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.sizes() == c10::IntArrayRef(shape.begin(), shape.size()),
                name, " must have shape ",
                c10::IntArrayRef(shape.begin(), shape.size()), ", got ",
                t.sizes());
}


static void lstm_check_ws(const torch::Tensor& ws) {
    TORCH_CHECK(ws.defined() && ws.is_cuda() && ws.is_contiguous()
                && ws.scalar_type() == torch::kInt32
                && ws.numel() * 4 >= (long)sizeof(GridBar),
                "barrier_ws must be a contiguous CUDA int32 tensor of >= ",
                sizeof(GridBar) / 4, " words");
}

// ---------------------------------------------------------------------------
// Entry points.  lstm_fwd / lstm_bwd take 1 <= B <= 64 and run one pass of
// 64 rows.  lstm_fwd_multi / lstm_bwd_multi take 1 <= B <= 256; `rows` is
// their pass size P: 64 (128 workgroups, the 64-row grid) or 128 (256
// workgroups); 0 takes R2D2_LSTM_MULTI_ROWS, default
// LSTM_MULTI_ROWS_DEFAULT.  Each direction has ONE launch helper, which
// both of its entry points call.
// ---------------------------------------------------------------------------
#define LSTM_SINGLE_MAX_B 64
#define LSTM_MULTI_MAX_B 256
#define LSTM_MULTI_ROWS_DEFAULT 128

static int lstm_multi_rows(int64_t rows) {
    static const int rows_env = [] {
        const char* e = getenv("R2D2_LSTM_MULTI_ROWS");
        int v = e ? atoi(e) : LSTM_MULTI_ROWS_DEFAULT;
        return (v == 64 || v == 128) ? v : LSTM_MULTI_ROWS_DEFAULT;
    }();
    TORCH_CHECK(rows == 0 || rows == 64 || rows == 128,
                "rows per pass must be 64 or 128 (0 = default), got ", rows);
    return rows ? (int)rows : rows_env;
}

// `multi` says which entry point calls (`who` names it in messages); `rows`
// is read only for the multi-pass one.
static std::vector<torch::Tensor> lstm_fwd_launch(
    const char* who, bool multi, int64_t rows,
    torch::Tensor& X0, torch::Tensor& X1, torch::Tensor& Whh0,
    torch::Tensor& Whh1, torch::Tensor& init0, torch::Tensor& init1,
    torch::Tensor& lens, torch::Tensor& barrier_ws, bool want_stash) {
    TORCH_CHECK(X0.defined() && X0.dim() == 3, "X0 must be (B, T, 4H)");
    long B = X0.size(0), T = X0.size(1);
    long H4 = X0.size(2);
    long H = H4 / 4;
    TORCH_CHECK(H4 == 2048, who, " is instantiated for H=512");
    const long max_b = multi ? LSTM_MULTI_MAX_B : LSTM_SINGLE_MAX_B;
    TORCH_CHECK(B >= 1 && B <= max_b, "1 <= B <= ", max_b, " per ", who,
                " launch, got B = ", B);
    const int P = multi ? lstm_multi_rows(rows) : LSTM_SINGLE_MAX_B;
    bool two = X1.defined() && X1.numel() > 0;
    lstm_check(X0, "X0", torch::kBFloat16, {B, T, H4});
    lstm_check(Whh0, "Whh0", torch::kBFloat16, {H4, H});
    lstm_check(init0, "init0", torch::kFloat32, {2, B, H});
    lstm_check(lens, "lens", torch::kInt32, {B});
    if (two) {
        lstm_check(X1, "X1", torch::kBFloat16, {B, T, H4});
        lstm_check(Whh1, "Whh1", torch::kBFloat16, {H4, H});
        lstm_check(init1, "init1", torch::kFloat32, {2, B, H});
    }
    lstm_check_ws(barrier_ws);
    // the write-through h stores address Hout through a buffer descriptor
    TORCH_CHECK(B * (T + 1) * H * 2 < (1L << 31), who,
                ": Hout of 2 GiB or more (B * T too large)");

    auto bf = X0.options();
    auto f32 = X0.options().dtype(torch::kFloat32);
    auto H0 = torch::empty({B, T + 1, H}, bf);
    auto C0 = torch::empty({B, T + 1, H}, f32);
    auto H1 = two ? torch::empty({B, T + 1, H}, bf) : torch::Tensor();
    auto C1 = two ? torch::empty({B, T + 1, H}, f32) : torch::Tensor();
    auto stash = want_stash ? torch::empty({B, T, H4}, bf) : torch::Tensor();

    // lstm_fwd at B <= 32: the whole batch is ONE 64-row group of 8-unit
    // slices.  Everything else: 32-row groups of 16-unit slices (the
    // measured default: fewer/fatter workgroups, half the handoff producers
    // per counter and half the total h re-read).
    const bool whole = !multi && B <= 32;
    const int ngroups = whole ? 1 : P / 32;
    const int npasses = (int)((B + P - 1) / P);
    const int nblocks = (int)H / (whole ? 8 : 16) * ngroups * (two ? 2 : 1);
    static_assert(2 * (128 / 32) * 32 <= LSTM_MAX_FLAGS, "counter groups");
    auto kernel = whole ? lstm_fwd_kernel<512, 64, 8>
                        : lstm_fwd_kernel<512, 32, 16>;
    auto stream = at::cuda::getCurrentCUDAStream();
    zero_ws(barrier_ws, stream.stream());
    auto bp = [](torch::Tensor& t) {
        return t.defined()
            ? reinterpret_cast<__hip_bfloat16*>(t.data_ptr()) : nullptr;
    };
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, stream.stream(),
        reinterpret_cast<const __hip_bfloat16*>(X0.data_ptr()),
        two ? reinterpret_cast<const __hip_bfloat16*>(X1.data_ptr()) : nullptr,
        reinterpret_cast<const __hip_bfloat16*>(Whh0.data_ptr()),
        two ? reinterpret_cast<const __hip_bfloat16*>(Whh1.data_ptr()) : nullptr,
        init0.data_ptr<float>(),
        two ? init1.data_ptr<float>() : nullptr,
        lens.data_ptr<int>(), bp(H0), bp(H1),
        C0.data_ptr<float>(), two ? C1.data_ptr<float>() : nullptr,
        want_stash ? bp(stash) : nullptr,
        reinterpret_cast<GridBar*>(barrier_ws.data_ptr()),
        (int)B, (int)T, ngroups, npasses);

    std::vector<torch::Tensor> out = {H0, C0};
    out.push_back(two ? H1 : torch::Tensor());
    out.push_back(two ? C1 : torch::Tensor());
    out.push_back(want_stash ? stash : torch::Tensor());
    return out;
}

// Hout is part of the Python signature and is checked, but no kernel reads it.
static torch::Tensor lstm_bwd_launch(
    const char* who, bool multi, int64_t rows,
    torch::Tensor& stash, torch::Tensor& Cout, torch::Tensor& Hout,
    torch::Tensor& dHext, torch::Tensor& Whh_bwd, torch::Tensor& lens,
    torch::Tensor& barrier_ws) {
    TORCH_CHECK(stash.defined() && stash.dim() == 3,
                "stash must be (B, T, 4H)");
    long B = stash.size(0), T = stash.size(1), H4 = stash.size(2);
    long H = H4 / 4;
    TORCH_CHECK(H4 == 2048, who, " is instantiated for H=512");
    // rows past the last pass would come back unwritten from torch::empty
    const long max_b = multi ? LSTM_MULTI_MAX_B : LSTM_SINGLE_MAX_B;
    TORCH_CHECK(B >= 1 && B <= max_b, "1 <= B <= ", max_b, " per ", who,
                " launch, got B = ", B);
    const int P = multi ? lstm_multi_rows(rows) : LSTM_SINGLE_MAX_B;
    lstm_check(stash, "stash", torch::kBFloat16, {B, T, H4});
    lstm_check(Cout, "Cout", torch::kFloat32, {B, T + 1, H});
    lstm_check(Hout, "Hout", torch::kBFloat16, {B, T + 1, H});
    lstm_check(dHext, "dHext", torch::kFloat32, {B, T, H});
    lstm_check(Whh_bwd, "Whh_bwd", torch::kBFloat16, {H, H4});
    lstm_check(lens, "lens", torch::kInt32, {B});
    lstm_check_ws(barrier_ws);
    // the write-through dgates stores address it through a buffer descriptor
    TORCH_CHECK(B * T * H4 * 2 < (1L << 31), who,
                ": dgates of 2 GiB or more (B * T too large)");
    auto dgates = torch::empty({B, T, H4}, stash.options());

    // Batch QUARTERS (16-row groups, KSPLIT 4; 128 wgs per 64 rows) are the
    // default: measured 0.71 vs 0.95 ms against halves at 64 rows (the
    // backward is CU-coverage bound); with B <= 32 the quarters past the
    // batch hold no rows.  lstm_bwd at 33 <= B <= 48 runs two 32-row halves
    // (KSPLIT 2) instead.
    const bool halves = !multi && B > 32 && B <= 48;
    const int ngroups = P / (halves ? 32 : 16);
    const int npasses = (int)((B + P - 1) / P);
    const int nblocks = (int)H / 16 * ngroups;
    static_assert((128 / 16) * 32 <= LSTM_MAX_FLAGS, "counter groups");
    auto kernel = halves ? lstm_bwd_kernel<512, 32, 16>
                         : lstm_bwd_kernel<512, 16, 16>;
    auto stream = at::cuda::getCurrentCUDAStream();
    zero_ws(barrier_ws, stream.stream());
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, stream.stream(),
        reinterpret_cast<const __hip_bfloat16*>(stash.data_ptr()),
        Cout.data_ptr<float>(), dHext.data_ptr<float>(),
        reinterpret_cast<const __hip_bfloat16*>(Whh_bwd.data_ptr()),
        lens.data_ptr<int>(),
        reinterpret_cast<__hip_bfloat16*>(dgates.data_ptr()),
        reinterpret_cast<GridBar*>(barrier_ws.data_ptr()),
        (int)B, (int)T, ngroups, npasses);
    return dgates;
}

std::vector<torch::Tensor> lstm_fwd(
    torch::Tensor X0, torch::Tensor X1, torch::Tensor Whh0, torch::Tensor Whh1,
    torch::Tensor init0, torch::Tensor init1, torch::Tensor lens,
    torch::Tensor barrier_ws, bool want_stash) {
    return lstm_fwd_launch("lstm_fwd", false, 0, X0, X1, Whh0, Whh1, init0,
                           init1, lens, barrier_ws, want_stash);
}

std::vector<torch::Tensor> lstm_fwd_multi(
    torch::Tensor X0, torch::Tensor X1, torch::Tensor Whh0, torch::Tensor Whh1,
    torch::Tensor init0, torch::Tensor init1, torch::Tensor lens,
    torch::Tensor barrier_ws, bool want_stash, int64_t rows) {
    return lstm_fwd_launch("lstm_fwd_multi", true, rows, X0, X1, Whh0, Whh1,
                           init0, init1, lens, barrier_ws, want_stash);
}

torch::Tensor lstm_bwd(torch::Tensor stash, torch::Tensor Cout,
                       torch::Tensor Hout, torch::Tensor dHext,
                       torch::Tensor Whh_bwd, torch::Tensor lens,
                       torch::Tensor barrier_ws) {
    return lstm_bwd_launch("lstm_bwd", false, 0, stash, Cout, Hout, dHext,
                           Whh_bwd, lens, barrier_ws);
}

torch::Tensor lstm_bwd_multi(torch::Tensor stash, torch::Tensor Cout,
                             torch::Tensor Hout, torch::Tensor dHext,
                             torch::Tensor Whh_bwd, torch::Tensor lens,
                             torch::Tensor barrier_ws, int64_t rows) {
    return lstm_bwd_launch("lstm_bwd_multi", true, rows, stash, Cout, Hout,
                           dHext, Whh_bwd, lens, barrier_ws);
}
