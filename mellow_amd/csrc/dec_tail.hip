// Decode step: its tail -- the lm_head (fp32 / e4m3 and the streaming f32x3 form), the arg-max with the step epilogue, the
// log-sum-exp tap, the row repack and the row load -- and the plain arg-max of mellow_argmax.
// The design comment of the decode step, the shared device helpers and the launchers' variant dispatcher: dec_common.h; the step epilogue: step_tail.h.
#include "dec_common.h"
#include "step_tail.h"

namespace mellow {

void set_dec_tail_debug_buffer(uint64_t* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_kdbg), &p, sizeof(p)); }

// ----------------------------------------------------------------------------------------------------
// (measured and not kept: two 32-column tiles per workgroup sharing the x registers, 768 workgroups: 38.9 vs 36.7 us)
// K4  full-K projection (lm_head).  grid (n-tiles, 1, RB), 4 waves x 18 k-tiles, all 36 loads of a
//     wave in flight; X in F32-layout.  Writes row-major logits (optional) + fused arg-max candidates per tile.
// ----------------------------------------------------------------------------------------------------
enum { OUT_LOGITS = 1 };
#ifndef MELLOW_LM_WAVES
#define MELLOW_LM_WAVES 8     // 8 x 9 k-tiles: 53.45 vs 54.35 ms of decode per 63 steps with 4 x 18 (6 / 9 / 12 waves: 54.1 / 54.1 / 53.7)
#endif
constexpr int LM_WAVES = MELLOW_LM_WAVES;
// LSE (log-probs of the generated tokens, DecArgs::cand_sum): the tile maximum found for the arg-max candidate goes back to the 256
// epilogue threads through the same LDS; thread (row mm, q = tid / 32) sums exp(v - max) over its four columns 4 q .. 4 q + 3 in
// ascending order, and the thread that writes the row's candidate adds the eight partial sums in ascending q.
template <int OUT, bool BLK, int W8, bool LSE = false>
__global__ __launch_bounds__(LM_WAVES * 64) void dec_fullk_kernel(const float* __restrict__ Wp, const float* __restrict__ XF, int K8p,
                                                        int N, const DecArgs a, const float* __restrict__ wscale) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[LM_WAVES * 16 * 64];
    constexpr int KPW = 72 / LM_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x, rb = blockIdx.z;
    MELLOW_BLK_EXIT(rb)
    const int k8_0 = wave * KPW;
    const int64_t wslot = ((int64_t)nt * K8p + k8_0) * 64 + lane;
    const float4* xp = reinterpret_cast<const float4*>(XF) + ((int64_t)rb * 72 + k8_0) * 64 + lane;
    WFrag<KPW, W8> w;
    float4 x[KPW];
    const bool dbg = tid == 0 && nt == 0 && rb == 0;
    const int dslot = 5;
    kstamp(dslot, 0, dbg);
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        w.t[i] = w.load(Wp, wslot + i * 64);
        x[i] = xp[i * 64];
    }
    __builtin_amdgcn_sched_barrier(0);
    kstamp(dslot, 1, dbg);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = slice_mma32<KPW, W8>(acc, w, x);
    kstamp(dslot, 2, dbg && acc[0] == acc[0]);
    reduce_store(MELLOW_LDS(red) + wave * 16 * 64 + lane, acc);
    __syncthreads();
    kstamp(dslot, 3, dbg);
    const bool epi = tid < 256;             // the epilogue is 256 threads wide (more waves only with MELLOW_LM_WAVES > 4)
    const int mm = tid & 31, n = epi_col(nt, tid);
    float4 v4 = reduce32<LM_WAVES>(MELLOW_LDS(red), tid);
    {
        if (W8) v4 = f4scale(v4, wscale + n);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        const int64_t row = (int64_t)rb * 32 + mm;
        if (epi && a.logits && n < N) *reinterpret_cast<float4*>(a.logits + row * N + n) = v4;
        // best (value, lowest index) of this 32-column tile per row (torch.argmax tie rule)
        __syncthreads();
        float bv = v[0];
        int bi = n;
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (arg_better(v[j], n + j, bv, bi)) { bv = v[j]; bi = n + j; }
        if (epi) {
            red[tid] = bv;
            reinterpret_cast<int*>(red)[256 + tid] = bi;
        }
        __syncthreads();
        if (tid < 32) {
            float best = red[tid];
            int idx = reinterpret_cast<int*>(red)[256 + tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) {
                const float ov = red[tid + 32 * q];
                const int oi = reinterpret_cast<int*>(red)[256 + tid + 32 * q];
                if (arg_better(ov, oi, best, idx)) { best = ov; idx = oi; }
            }
            const int64_t o = ((int64_t)rb * 32 + tid) * (N >> 5) + nt;          // N / 32 = gridDim.x (a dispatch-packet read in the tail otherwise)
            a.cand_val[o] = best;
            a.cand_idx[o] = idx;
            if constexpr (LSE) red[512 + tid] = best;
        }
        if constexpr (LSE) {
            __syncthreads();
            const float tmax = red[512 + mm];
            float ps = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) ps += expf(v[j] - tmax);
            if (epi) red[768 + tid] = ps;
            __syncthreads();
            if (tid < 32) {
                float ssum = red[768 + tid];
#pragma unroll
                for (int q = 1; q < 8; ++q) ssum += red[768 + tid + 32 * q];      // fixed order
                a.cand_sum[((int64_t)rb * 32 + tid) * (N >> 5) + nt] = ssum;
            }
        }
    }
    kspan(a.dbg_seq, 1);
}


// ----------------------------------------------------------------------------------------------------
// K4y  lm_head, f32x3 form, as a streaming GEMM: one WAVE owns a 32-row n-tile over the WHOLE K = 576 (no split-K, no LDS
//      reduction), a workgroup = H3_NW waves = H3_NW consecutive n-tiles, and the pre-split activations (F3-32, written by the
//      final norm) of up to G row blocks sit in LDS, shared by the waves.  The weights are
//      streamed ONCE per step whatever the batch (the fp32 kernel above re-reads them per row block and every 32-row tile
//      re-reads x: at B = 128 that is 4 x 113 MB of weights and 0.45 GB of activations through the L2s), split to bf16 triples
//      in registers once per chunk and used for all G row blocks.  Rows beyond G blocks: further passes.
//      The arg-max candidates of a tile are formed from the accumulators directly (a wave holds all 32 columns of its rows).
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_H3_NW
#define MELLOW_H3_NW 8
#endif
#ifndef MELLOW_H3R_D1
#define MELLOW_H3R_D1 1           // weight chunks in flight per wave at 1 / 2 / >= 3 row blocks (2 and 3 measured slower)
#endif
#ifndef MELLOW_H3R_D2
#define MELLOW_H3R_D2 1
#endif
#ifndef MELLOW_H3R_D4
#define MELLOW_H3R_D4 1
#endif
constexpr int H3_NW = MELLOW_H3_NW, H3_CP = 3, H3_NC = 36 / H3_CP;
//      Activations RESIDENT in LDS: the G row blocks' fragments of 36 / G k-pairs fill the 108 KiB stage once per phase (G
//      phases), and inside a phase the waves run without any barrier -- each streams its own n-tile's weights D chunks ahead
//      (D = 1: deeper register prefetch measured slower) and reads the fragments it needs from LDS.  (A first form refilled a small
//      stage every chunk -- one barrier + one L2 round trip per chunk: tools/experiments/r05_dec_head3_kernel.hip.txt.)
//      LSE (DecArgs::cand_sum): after the exchange below both lanes of a pair know the tile's maximum; each sums exp(acc - max)
//      over its 16 accumulators in register order (columns 8 q + 4 h + j: q, then j, ascending), the halves are exchanged the same
//      way and the h == 0 lane stores (its own sum) + (its partner's).
template <int G, int D, bool BLK, bool LSE = false>
__global__ __launch_bounds__(H3_NW * 64) void dec_head3r_kernel(const float* __restrict__ Wp, const i32x4* __restrict__ X3, int K8p, int N,
                                                                int RB_p, const DecArgs a) {
    kspan(a.dbg_seq, 0);
    extern __shared__ __attribute__((aligned(16))) i32x4 xs[];        // [G][PPH][3][64]
    constexpr int PPH = 36 / G, NCH = PPH / H3_CP;                     // pairs / chunks per phase
    constexpr int STAGE = G * PPH * 3 * 64;                            // = 36 * 192 slots = 108 KiB
    static_assert(PPH * G == 36 && NCH * H3_CP == PPH && H3_NC % D == 0 && NCH % D == 0, "phases hold whole chunks");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x * H3_NW + wave;
    const float4* wbase = reinterpret_cast<const float4*>(Wp) + (int64_t)nt * K8p * 64 + lane;
    for (int rb0 = 0; rb0 < RB_p; rb0 += G) {
        const int gn = min(G, RB_p - rb0);
        f32x16 acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
        float4 wn[D][2 * H3_CP];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int i = 0; i < 2 * H3_CP; ++i) wn[d][i] = ldg_nt(wbase + (d * 2 * H3_CP + i) * 64);
        for (int ph = 0; ph < G; ++ph) {
            if (ph || rb0) __syncthreads();               // every wave has read the previous phase's fragments
            // fill: slot i = (g, pair pp of the phase, piece, lane) <- X3[((rb0 + g) * 36 + ph * PPH + pp) * 3 + piece][lane]
            {
                constexpr int FILL = (STAGE + H3_NW * 64 - 1) / (H3_NW * 64);      // all loads of a thread in flight together
                i32x4 t[FILL];
#pragma unroll
                for (int j = 0; j < FILL; ++j) {
                    const int i = tid + j * H3_NW * 64;
                    if (i < STAGE) {
                        const int g = i / (PPH * 3 * 64), rest = i % (PPH * 3 * 64);
                        t[j] = X3[(((int64_t)(rb0 + (g < gn ? g : 0)) * 36 + ph * PPH) * 3) * 64 + rest];
                    }
                }
#pragma unroll
                for (int j = 0; j < FILL; ++j) {
                    const int i = tid + j * H3_NW * 64;
                    if (i < STAGE) xs[i] = t[j];
                }
            }
            __syncthreads();
            for (int c0 = 0; c0 < NCH; c0 += D) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int cc = c0 + d, c = ph * NCH + cc;      // chunk of the phase / of the whole K
                    float4 w[2 * H3_CP];
#pragma unroll
                    for (int i = 0; i < 2 * H3_CP; ++i) w[i] = wn[d][i];
                    if (c + D < H3_NC) {
#pragma unroll
                        for (int i = 0; i < 2 * H3_CP; ++i) wn[d][i] = ldg_nt(wbase + ((c + D) * 2 * H3_CP + i) * 64);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    i32x4 wp[H3_CP][3];
#pragma unroll
                    for (int p = 0; p < H3_CP; ++p) {
                        pair_natural(w[2 * p], w[2 * p + 1]);
                        split_pair(w[2 * p], w[2 * p + 1], wp[p][0], wp[p][1], wp[p][2]);
                    }
                    const i32x4* st = xs + (cc * H3_CP) * 3 * 64 + lane;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        if (g < gn) {
#pragma unroll
                            for (int p = 0; p < H3_CP; ++p) {
                                const i32x4 xq[3] = {st[((g * PPH + p) * 3 + 0) * 64], st[((g * PPH + p) * 3 + 1) * 64], st[((g * PPH + p) * 3 + 2) * 64]};
                                acc[g] = mma6(acc[g], wp[p], xq);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        const int m = lane & 31, h = lane >> 5;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g < gn && !(BLK && a.blk_live[rb0 + g] == 0)) {
                const int64_t row = (int64_t)(rb0 + g) * 32 + m;
                float bv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = nt * 32 + 8 * q + 4 * h;
                    if (a.logits) *reinterpret_cast<float4*>(a.logits + row * N + n) = make_float4(acc[g][4 * q], acc[g][4 * q + 1], acc[g][4 * q + 2], acc[g][4 * q + 3]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (arg_better(acc[g][4 * q + j], n + j, bv, bi)) { bv = acc[g][4 * q + j]; bi = n + j; }
                }
                auto rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(bv), __float_as_uint(bv), false, false);
                auto ri = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
                const float ov = __uint_as_float(h ? rv[0] : rv[1]);
                const int oi = (int)(h ? ri[0] : ri[1]);
                if (arg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                if (h == 0) {
                    const int64_t o = row * (N >> 5) + nt;
                    a.cand_val[o] = bv;
                    a.cand_idx[o] = bi;
                }
                if constexpr (LSE) {
                    float ps = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) ps += expf(acc[g][r] - bv);
                    auto rs = __builtin_amdgcn_permlane32_swap(__float_as_uint(ps), __float_as_uint(ps), false, false);
                    const float os = __uint_as_float(h ? rs[0] : rs[1]);
                    if (h == 0) a.cand_sum[row * (N >> 5) + nt] = ps + os;
                }
            }
        }
    }
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// row-parallel helpers (one workgroup per batch row)
// ----------------------------------------------------------------------------------------------------
// arg-max over the lm_head's per-tile candidates, fused with the loop bookkeeping of reference wrapper.py:232-249:
// record the token at column (*d_pos - T0 + 1), track stop ids, and gather its embedding row (embed_tokens,
// wrapper.py:237) as the next step's residual stream (row-major + F32-layout).
// LSE (LoopArgs::out_logprob): the chosen token is the row maximum M = `best`, so its log-prob is -log S with S merged from the
// head's (cand_val, cand_sum) partials by dec_lse_sum (common.h): written where the token is.
template <bool LSE>
__global__ __launch_bounds__(256) void dec_argmax_kernel(const float* __restrict__ cand_val_p, const int32_t* __restrict__ cand_idx_p, int n,
                                                         const DecArgs a, int32_t* __restrict__ tokens,
                                                         const float* __restrict__ embed, int write_x, const LoopArgs lp) {
    kspan(a.dbg_seq, 0);
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int tok_s;
    __shared__ float lse_sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(lp.row_of_slot, lp.blk_snap, b);      // a dead slot still takes part in the step's arrival count
    float best = -INFINITY;
    int idx = 0x7fffffff;
    if (!dead) {
        for (int i = tid; i < n; i += 256) {
            const float v = cand_val_p[(int64_t)b * n + i];
            const int id = cand_idx_p[(int64_t)b * n + i];
            if (arg_better(v, id, best, idx)) { best = v; idx = id; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(idx, off, 64);
            if (arg_better(ov, oi, best, idx)) { best = ov; idx = oi; }
        }
        if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
    }
    __syncthreads();
    float S = 0.f;
    if constexpr (LSE) {
        if (!dead) {            // (workgroup-uniform)
            float M = bv[0];
            int mi = bi[0];
            for (int w = 1; w < 4; ++w)
                if (arg_better(bv[w], bi[w], M, mi)) { M = bv[w]; mi = bi[w]; }
            S = dec_lse_sum(cand_val_p + (int64_t)b * n, a.cand_sum + (int64_t)b * n, n, M, lse_sh);
            S = (M - M == 0.f) ? S : __builtin_nanf("");
        }
    }
    if (tid == 0) {
        if (!dead) {
            for (int w = 1; w < 4; ++w)
                if (arg_better(bv[w], bi[w], best, idx)) { best = bv[w]; idx = bi[w]; }
            idx = min(max(idx, 0), n * 32 - 1);       // always a valid row of the embedding table (n tiles x 32 ids = vocab)
            tokens[b] = idx;
            tok_s = idx;
        }
        if (lp.out_tokens) {
            if (!dead) {
                if constexpr (LSE) step_record(lp, a, b, row, idx, [S] { return -dec_lse_log(S); });
                else step_record(lp, a, b, row, idx);
            }
            step_publish(lp, [n_seen = lp.n_seen] { return atomicAdd(n_seen, 0); });
        }
    }
    if (dead) return;
    if (write_x) {
        __syncthreads();
        if (tid < 144) step_embed_gather(embed, tok_s, a, b, tid);
    }
    kspan(a.dbg_seq, 1);
}

// numeric tap of the same merge on caller rows (mellow_debug_dec_head_lse): the row maximum from the tile maxima, then dec_lse_sum
__global__ __launch_bounds__(256) void dec_lse_tap_kernel(const float* __restrict__ cand_val_p, const float* __restrict__ cand_sum_p, int n,
                                                          float* __restrict__ out_lse, float* __restrict__ out_max) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    const float M = dec_lse_max(cand_val_p + (int64_t)b * n, n, sh);
    const float S = dec_lse_sum(cand_val_p + (int64_t)b * n, cand_sum_p + (int64_t)b * n, n, M, sh);
    if (threadIdx.x == 0) {
        out_lse[b] = dec_lse_value(M, S);
        out_max[b] = M;
    }
}

// Row migration (reference stop rule, more than one 32-row block).  One workgroup, after the step's arg-max: the rows that
// have not produced the stop id yet are counted; if they fit into fewer 32-row blocks than are live, they are packed (stable)
// into the lowest slots: their next-step residual rows move, row_of_slot is rewritten, the emptied blocks' live words are
// cleared.  A row's arithmetic does not depend on its slot (MFMA rows are independent, every reduction is per row), so the
// tokens are unchanged; rows that had already stopped are dropped (their texts are cut at the stop id anyway).
__global__ __launch_bounds__(1024) void dec_compact_kernel(const DecArgs a, int B, const LoopArgs lp) {
    __shared__ int src_of[1024];           // new slot -> old slot
    __shared__ int row_new[1024];
    __shared__ int wsum[16];
    __shared__ int n_act_s, n_live_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (B + 31) >> 5;
    int row = -1, active = 0;
    if (tid < B) {
        row = lp.row_of_slot[tid];
        active = row >= 0 && lp.blk_live[tid >> 5] != 0 && lp.seen_stop[row] == 0;
    }
    // exclusive prefix sum of `active` over the slots: ballot inside a wave, then over the 16 waves
    const unsigned long long m = __ballot(active);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    if (tid == 0) {
        int live = 0;
        for (int k = 0; k < nblk; ++k) live += lp.blk_live[k] != 0;
        n_live_s = live;
    }
    src_of[tid] = -1;
    row_new[tid] = -1;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < 16; ++w) n += wsum[w];
        n_act_s = n;
    }
    __syncthreads();
    const int n_act = n_act_s;
    if ((n_act + 31) / 32 >= n_live_s) return;            // repacking would not empty a block (workgroup-uniform)
    if (active) { src_of[base + before] = tid; row_new[base + before] = row; }
    __syncthreads();
    // move the residual rows, 7 destination slots (7 x 144 float4 = 1008 threads) at a time in increasing order: a destination
    // is never above its source and sources only grow, so a chunk can only overwrite sources of chunks already done
    float4* x = reinterpret_cast<float4*>(a.xmidF);
    for (int d0 = 0; d0 < n_act; d0 += 7) {
        const int d = d0 + tid / 144, c = tid % 144;
        const bool mv = tid < 1008 && d < n_act && src_of[d] != d;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (mv) v = x[f32_idx(src_of[d] >> 5, 72, src_of[d] & 31, c * 4)];
        __syncthreads();
        if (mv) x[f32_idx(d >> 5, 72, d & 31, c * 4)] = v;
        __syncthreads();
    }
    if (tid < B) lp.row_of_slot[tid] = row_new[tid];
    if (tid < 32) {
        const int left = tid < nblk ? min(max(n_act - 32 * tid, 0), 32) : 0;
        lp.blk_left[tid] = left;
        lp.blk_live[tid] = left > 0;
    }
    if (tid == 0) *lp.n_compactions += 1;
}
void launch_dec_compact(const DecArgs& a, int B, const LoopArgs& loop, hipStream_t s) {
    hipLaunchKernelGGL(dec_compact_kernel, dim3(1), dim3(1024), 0, s, a, B, loop);
}

// rows -> residual stream (row-major + F32-layout): src row b = in[row_of(b)]
__global__ __launch_bounds__(192) void dec_load_rows_kernel(const DecArgs a, const float* __restrict__ in, int64_t ld,
                                                            const int32_t* __restrict__ row_ids, int T_last, int n_src) {
    const int b = blockIdx.x, tid = threadIdx.x;
    // caller-supplied ids are clamped to the table (an out-of-range id must not become a wild read; the Python
    // binding rejects it with an IndexError before it gets here)
    const int64_t src = row_ids ? (int64_t)min(max(row_ids[b], 0), n_src - 1) : (int64_t)b * T_last + (T_last - 1);
    if (tid < 144) step_store_x(a.xmidF, b, tid, reinterpret_cast<const float4*>(in + src * ld)[tid]);
}

// ---- launchers -------------------------------------------------------------------------------------------
// true when the streaming f32x3 lm_head (dec_head3r_kernel) tiles this vocabulary: only then may the final norm hand its output
// over pre-split (DecArgs::xn3, which aliases xnF) -- engine_lm.cpp: ensure_lm
bool dec_head3r_fits(int vocab) { return vocab % 32 == 0 && (vocab / 32) % H3_NW == 0; }
// its dynamic LDS and the instantiation that serves `rb` row blocks, as with_qkv2x3 / with_gateup3 of dec_gemv.hip: for the launcher and
// for dec_tail_prepare_lds alike
constexpr size_t dec_head3r_lds() { return (size_t)36 * 3 * 64 * 16; }
template <class F> static inline void with_head3r(int rb, bool blk, bool lse, F&& f) {
    with_int<1, 2, 4>(rb, [&](auto g) { with_bool(blk, [&](auto b) { with_bool(lse, [&](auto l) {
        constexpr int G = g.value, D = G == 1 ? MELLOW_H3R_D1 : G == 2 ? MELLOW_H3R_D2 : MELLOW_H3R_D4;      // weight chunks in flight
        f(&dec_head3r_kernel<G, D, b.value, l.value>, dec_head3r_lds());
    }); }); });
}
void launch_dec_lm_head(const DecArgs& a, const float* Wp, int K8p, int vocab, hipStream_t s, const float* wscale) {
    if ((a.x3 & DEC_X3_HEAD) && !wscale && a.xn3 && (vocab / 32) % H3_NW == 0) {
        // f32x3 mode, activations pre-split by the final norm: the streaming form (weights read once for every row block)
        const i32x4* X3 = reinterpret_cast<const i32x4*>(a.xn3);
        with_head3r(a.RB, a.blk_live != nullptr, a.cand_sum != nullptr, [&](auto* kernel, size_t lds) {
            set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds);
            hipLaunchKernelGGL(kernel, dim3(vocab / 32 / H3_NW), dim3(H3_NW * 64), lds, s, Wp, X3, K8p, vocab, a.RB, a);
        });
        return;
    }
    // (fp32 rows in xnF -- taps on caller rows, or a vocabulary the streaming form does not tile: the exact fp32 kernel below)
    with_blk_w8(a, wscale, [&](auto blk, auto w8) { with_bool(a.cand_sum != nullptr, [&](auto lse) {
        hipLaunchKernelGGL((dec_fullk_kernel<OUT_LOGITS, blk.value, w8.value, lse.value>), dim3(vocab / 32, 1, a.RB), dim3(LM_WAVES * 64), 0, s, Wp,
                           (const float*)a.xnF, K8p, vocab, a, wscale);
    }); });
}
// this file's share of dec_prepare_lds_attributes (engine.cpp): every instantiation the lm_head launcher can pick
void dec_tail_prepare_lds() {
    const auto raise = [](auto* kernel, size_t lds) { set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds); };
    for (const int rb : {1, 2, 4})
        for (const bool blk : {false, true})
            for (const bool lse : {false, true}) with_head3r(rb, blk, lse, raise);
}
void launch_dec_argmax(const DecArgs& a, int B, int n_tiles, int32_t* tokens, const float* embed, int write_x,
                       const LoopArgs& loop, hipStream_t s) {
    // the log-prob record needs the head's partial sums: both set (mellow_generate_scored) or neither
    with_bool(loop.out_logprob != nullptr && a.cand_sum != nullptr, [&](auto lse) {
        hipLaunchKernelGGL(dec_argmax_kernel<lse.value>, dim3(B), dim3(256), 0, s, (const float*)a.cand_val, (const int32_t*)a.cand_idx, n_tiles, a,
                           tokens, embed, write_x, loop);
    });
}
void launch_dec_lse_tap(const DecArgs& a, int B, int n_tiles, float* out_lse, float* out_max, hipStream_t s) {
    hipLaunchKernelGGL(dec_lse_tap_kernel, dim3(B), dim3(256), 0, s, (const float*)a.cand_val, (const float*)a.cand_sum, n_tiles, out_lse, out_max);
}
void launch_dec_load_rows(const DecArgs& a, int B, const float* in, int64_t ld, const int32_t* row_ids, int T_last,
                          int n_src, hipStream_t s) {
    hipLaunchKernelGGL(dec_load_rows_kernel, dim3(B), dim3(192), 0, s, a, in, ld, row_ids, T_last, n_src);
}

// ---- full-row arg-max (mellow_argmax tap): torch.argmax tie rule, float4 loads --------------------------------
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ logits, int V, int64_t ld,
                                                      int32_t* __restrict__ tokens) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float4* row = reinterpret_cast<const float4*>(logits + (int64_t)b * ld);
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = tid; i < (V >> 2); i += 1024) {
        const float4 v = row[i];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (arg_better(vv[j], 4 * i + j, best, idx)) { best = vv[j]; idx = 4 * i + j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (arg_better(ov, oi, best, idx)) { best = ov; idx = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (arg_better(bv[w], bi[w], best, idx)) { best = bv[w]; idx = bi[w]; }
        tokens[b] = min(max(idx, 0), V - 1);
    }
}
void launch_argmax(const float* logits, int B, int V, int64_t ld, int32_t* tokens, hipStream_t s) {
    hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(1024), 0, s, logits, V, ld, tokens);
}

}  // namespace mellow
