// Decode step: the GEMV launches of a layer -- q/k/v, gate/up, down, the fused down + q/k/v, their f32x3 forms -- and the final
// norm.  The design comment of the decode step, the shared device helpers and the launchers' variant dispatcher: dec_common.h.
#include "dec_common.h"

namespace mellow {

void set_dec_gemv_debug_buffer(uint64_t* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_kdbg), &p, sizeof(p)); }

// ----------------------------------------------------------------------------------------------------
// K1  qkv projection, split-K.  grid (30 n-tiles, DEC_KC_QKV, RB) = 240 workgroups, 3 waves x 3 k-tiles (+1 epilogue wave).
//     X = baseF + sum_{s<KCD} dslabF[s]  (residual stream, un-normalised; norm weight folded into W)
//     out: pq[kc][row][960] row-major slabs (consumer = attention, row-parallel)
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_QKV_WAVES
#define MELLOW_QKV_WAVES 9     // 9 x 1 k-tile: 53.0 vs 53.6 ms of decode per 63 steps with 3 x 3
#endif
constexpr int QW = MELLOW_QKV_WAVES;                 // compute waves: 3 x 3 k-tiles or 9 x 1
constexpr int QKV_THREADS = QW * 64 < 256 ? 256 : QW * 64;
template <int KCD, bool BLK, bool FIRST, int W8>      // W8: 0 fp32 weights, 1 e4m3 weights widened, 2 e4m3 weights and activations (fp8 MFMA)
__global__ __launch_bounds__(QKV_THREADS) void dec_qkv_kernel(const float* __restrict__ Wp, const float* __restrict__ xmidF_p,
                                                              const float* __restrict__ dslabF_p, int K8p, const DecArgs a,
                                                              const float* __restrict__ wscale) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[QW * 16 * 64];
    __shared__ float ssq_s[QW * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x, kc = blockIdx.y, rb = blockIdx.z;
    constexpr int KPW = 72 / (DEC_KC_QKV * QW);   // k-tiles per compute wave (with QW = 3, wave 3 only helps the epilogue)
    // The first kernel of a step (a.first): advance the position word (nothing of the previous step reads it any more)
    // and stage this position's RoPE row at a fixed address, so that no attention kernel of the step has to chase
    // pos -> table row (two dependent round trips).  One half-wave: the loads of *d_pos precede the store in program order.
    if (FIRST && nt == 29 && kc == 0 && rb == 0 && tid < 32) {     // FIRST: compile-time, like BLK
        const int p = *a.d_pos + a.inc_pos;
        const float c = a.rope_cos[(int64_t)p * 32 + tid], sn = a.rope_sin[(int64_t)p * 32 + tid];
        a.rope_cur[tid] = c;
        a.rope_cur[32 + tid] = sn;
        if (tid == 0 && a.inc_pos) *a.d_pos = p;
    }
    MELLOW_BLK_EXIT(rb)      // every row of this block has stopped (workgroup-uniform)
    if (wave < QW) {
        const int k8_0 = (kc * QW + wave) * KPW;
        const int64_t wslot = ((int64_t)nt * K8p + k8_0) * 64 + lane;
        const float4* xb = reinterpret_cast<const float4*>(xmidF_p) + ((int64_t)rb * 72 + k8_0) * 64 + lane;
        const float4* sb = reinterpret_cast<const float4*>(dslabF_p) + ((int64_t)rb * 72 + k8_0) * 64 + lane;
        WFrag<KPW, W8> w;
        float4 x[KPW], sl[KPW][KCD > 0 ? KCD : 1];
#pragma unroll
        for (int i = 0; i < KPW; ++i) {
            w.t[i] = w.load(Wp, wslot + i * 64);
            x[i] = xb[i * 64];
#pragma unroll
            for (int s = 0; s < KCD; ++s) sl[i][s] = sb[(int64_t)s * a.slabF_stride4 + i * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float ssp = 0.f;
#pragma unroll
        for (int i = 0; i < KPW; ++i) {
#pragma unroll
            for (int s = 0; s < KCD; ++s) x[i] = f4add(x[i], sl[i][s]);
            // side jobs of two n-tiles (the workgroups of one k-chunk see every row of x_new on these 72 columns):
            //   nt == 0: partial sum of squares per row (the attention's RMS statistic)
            //   nt == 1: x_new row-major (the o_proj's residual operand)
            if (nt == 0) ssp += f4ssq(x[i]);
            if (nt == 1)
                *reinterpret_cast<float4*>(a.xnewR + ((int64_t)rb * 32 + (lane & 31)) * 576 + (k8_0 + i) * 8 + (lane >> 5) * 4) = x[i];
        }
        acc = slice_mma32<KPW, W8>(acc, w, x);
        if (nt == 0) {
            ssp = half_sum(ssp);                 // the two k-halves of a row sit in lanes m and m + 32
            if (lane < 32) ssq_s[wave * 32 + lane] = ssp;
        }
        reduce_store(MELLOW_LDS(red) + wave * 16 * 64 + lane, acc);
    }
    __syncthreads();
    if (nt == 0 && tid < 32)
    {
        float ssum = ssq_s[tid & 31];
#pragma unroll
        for (int wv = 1; wv < QW; ++wv) ssum += ssq_s[wv * 32 + (tid & 31)];
        a.ssq1[((int64_t)rb * 32 + tid) * DEC_KC_QKV + kc] = ssum;
    }
    if (tid >= 256) return;                              // (QW = 9 only) the epilogue is 256 threads wide; no barrier follows
    const int mm = tid & 31, n = epi_col(nt, tid);
    float4 v = reduce32<QW>(MELLOW_LDS(red), tid);
    if (W8) v = f4scale(v, wscale + n);
    if (n < 960) *reinterpret_cast<float4*>(a.pq + ((int64_t)kc * a.rows + rb * 32 + mm) * 960 + n) = v;
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// f32x3 forms of the two big GEMM launches of a decode layer, for batches of MORE than one 32-row block (north_star's batch 64,
// BASELINE configs[3] / [4]): the same workgroup -> weight-tile mapping, slab outputs and consumers as dec_qkv2_kernel /
// dec_gateup16_kernel, but
//   * ONE workgroup serves every row block: its weight fragments are loaded once and split to bf16 triples once (the fp32
//     kernels replicate the grid per row block: weights re-read, fp32 MFMA time per block),
//   * the activations arrive pre-split from their producer (F3 layouts above: o_proj writes x_mid, gate/up writes h), so a
//     row block costs 3 x 16-byte loads and six bf16 MFMAs per k-pair and no VALU,
//   * RBM row blocks are accumulated in registers per pass, one LDS reduction across the waves per pass.
// ----------------------------------------------------------------------------------------------------
#define MELLOW_BF16S(W, X, ACC) ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, W), __builtin_bit_cast(bf16x8, X), ACC, 0, 0, 0)
__device__ __forceinline__ f32x4 mma6s(f32x4 acc, const i32x4 (&w)[3], const i32x4 (&x)[3]) {
    MELLOW_BF16S(w[2], x[0], acc);
    MELLOW_BF16S(w[0], x[2], acc);
    MELLOW_BF16S(w[1], x[1], acc);
    MELLOW_BF16S(w[1], x[0], acc);
    MELLOW_BF16S(w[0], x[1], acc);
    MELLOW_BF16S(w[0], x[0], acc);
    return acc;
}
// One wave's share of a 32-row weight tile: NP k-pairs of W (fp32, P-layout, tiles k8_0 ..) against the same pairs of every
// row block's F3-32 activations.  acc[g] += W . x[rb0 + g] for g < gn.
template <int NP, int NPA>
__device__ __forceinline__ void x3_load(i32x4 (&xq)[NPA][3], const i32x4* __restrict__ x3, int64_t off) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[p][c] = x3[off + (p * 3 + c) * 64];
}
// xq[0] holds the fragments of block rb0 on entry (requested by the caller together with the weights)
template <int NP, int RBM, int NPA>
__device__ __forceinline__ void x3_tile_job(const i32x4 (&wp)[NPA][3], i32x4 (&xq)[2][NPA][3], const i32x4* __restrict__ x3 /* (rb 0, pair T0, piece 0, lane) */,
                                            int64_t rb_stride, int rb0, int gn, f32x16 (&acc)[RBM]) {
#pragma unroll
    for (int g = 0; g < RBM; ++g) {
        if (g < gn) {
            if (g + 1 < RBM && g + 1 < gn) x3_load<NP, NPA>(xq[(g + 1) & 1], x3, (int64_t)(rb0 + g + 1) * rb_stride);
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[g] = mma6(acc[g], wp[p], xq[g & 1][p]);
        }
    }
}
#ifndef MELLOW_Q3_WAVES
#define MELLOW_Q3_WAVES 6
#endif
constexpr int Q3W = MELLOW_Q3_WAVES;
// K5+K1 (f32x3, any number of row blocks): see dec_qkv2_kernel for the algebra and the workgroup types.  xmid3 = x_mid in F3-32
// (36 pairs per row block), h3 = h in F3-32 (96 pairs).
// One workgroup's job for either type (NP k-pairs per wave): weights + the first block's fragments requested together, weights
// split once, RBM row blocks accumulated per pass, one LDS reduction per pass, slabs out.
template <int NP, int RBM, bool BLK>
__device__ __forceinline__ void q3_body(const float4* __restrict__ wp4, const i32x4* __restrict__ xsrc, int64_t rb_stride, int nt, int slab,
                                        bool side, int RB_p, const DecArgs& a, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    i32x4 wp[NP][3];
    i32x4 xq[2][NP][3];
    constexpr bool ALL = RBM <= 2;            // a pass's fragments fit the registers: request all of them at once (no dependent second round trip)
    {
        float4 w[2 * NP];
#pragma unroll
        for (int i = 0; i < 2 * NP; ++i) w[i] = ldg_nt(wp4 + i * 64);
        x3_load<NP, NP>(xq[0], xsrc, 0);
        if (ALL && RBM == 2 && RB_p > 1) x3_load<NP, NP>(xq[1], xsrc, rb_stride);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            pair_natural(w[2 * p], w[2 * p + 1]);
            split_pair(w[2 * p], w[2 * p + 1], wp[p][0], wp[p][1], wp[p][2]);
        }
    }
    for (int rb0 = 0; rb0 < RB_p; rb0 += RBM) {
        const int gn = min(RBM, RB_p - rb0);
        f32x16 acc[RBM];
#pragma unroll
        for (int g = 0; g < RBM; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
        if (rb0) {
            x3_load<NP, NP>(xq[0], xsrc, (int64_t)rb0 * rb_stride);
            if (ALL && RBM == 2 && gn > 1) x3_load<NP, NP>(xq[1], xsrc, (int64_t)(rb0 + 1) * rb_stride);
        }
        if constexpr (ALL && RBM == 2) {
            if (gn > 1) {               // two row blocks = two independent accumulator chains, interleaved term by term
#pragma unroll
                for (int p = 0; p < NP; ++p) {
#define MELLOW_Q3_TERM(PW, PX) MELLOW_BF16(wp[p][PW], xq[0][p][PX], acc[0]); MELLOW_BF16(wp[p][PW], xq[1][p][PX], acc[1]);
                    MELLOW_Q3_TERM(2, 0) MELLOW_Q3_TERM(0, 2) MELLOW_Q3_TERM(1, 1) MELLOW_Q3_TERM(1, 0) MELLOW_Q3_TERM(0, 1) MELLOW_Q3_TERM(0, 0)
#undef MELLOW_Q3_TERM
                }
            } else {
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[0] = mma6(acc[0], wp[p], xq[0][p]);
            }
        } else if constexpr (ALL) {
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[0] = mma6(acc[0], wp[p], xq[0][p]);
        } else {
            x3_tile_job<NP, RBM, NP>(wp, xq, xsrc, rb_stride, rb0, gn, acc);
        }
        if (rb0) __syncthreads();                 // the previous pass's epilogue has read `red`
#pragma unroll
        for (int g = 0; g < RBM; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[((wave * RBM + g) * 16 + r) * 64 + lane] = acc[g][r];
        __syncthreads();
        if (tid < 256) {
            const int mm = tid & 31, hh = (tid >> 5) & 1, gq = tid >> 6;
            const int n = nt * 32 + 8 * gq + 4 * hh;
            for (int g = 0; g < gn; ++g) {
                const int rb = rb0 + g;
                if (BLK && a.blk_live[rb] == 0) continue;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = 4 * gq + j;
                    float sacc = red[((0 * RBM + g) * 16 + q) * 64 + mm + 32 * hh];
#pragma unroll
                    for (int wv = 1; wv < Q3W; ++wv) sacc += red[((wv * RBM + g) * 16 + q) * 64 + mm + 32 * hh];      // fixed order
                    v[j] = sacc;
                }
                const float4 o = make_float4(v[0], v[1], v[2], v[3]);
                if (side) *(reinterpret_cast<float4*>(a.dslabF) + (int64_t)slab * a.slabF_stride4 + f32_idx(rb, 72, mm, n)) = o;
                else *reinterpret_cast<float4*>(a.pq + ((int64_t)slab * a.rows + rb * 32 + mm) * 960 + n) = o;
            }
        }
    }
}
template <bool BLK, int RBM>
__global__ __launch_bounds__(Q3W * 64) void dec_qkv2x3_kernel(const float* __restrict__ Wx, const float* __restrict__ Wh,
                                                              const float* __restrict__ Wd, const i32x4* __restrict__ xmid3,
                                                              const i32x4* __restrict__ h3, int K8x, int K8h, int RB_p, const DecArgs a) {
    kspan(a.dbg_seq, 0);
    extern __shared__ __attribute__((aligned(16))) float red_dyn[];        // [Q3W][RBM][16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    constexpr int XP = 18 / Q3W, HP = (96 / Q2_HC) / Q3W;                    // k-pairs per wave
    static_assert(XP * Q3W == 18 && HP * Q3W * Q2_HC == 96 && Q3W * 64 >= 256, "waves must divide the k-chunks into whole pairs; the epilogue is 256 threads wide");
    if (b < 60) {              // x part (workgroup-uniform branch; each side is its own straight-line body)
        const int nt = b % 30, slab = b / 30;
        const int T0 = slab * 18 + wave * XP;
        q3_body<XP, RBM, BLK>(reinterpret_cast<const float4*>(Wx) + ((int64_t)nt * K8x + 2 * T0) * 64 + lane, xmid3 + (int64_t)T0 * 3 * 64 + lane,
                              (int64_t)36 * 3 * 64, nt, slab, false, RB_p, a, red_dyn);
    } else {                   // h part
        const int idx = b - 60, hc = idx / 48, nt = idx % 48;
        const bool side = nt >= 30;
        const int T0 = hc * (96 / Q2_HC) + wave * HP;
        const float4* wp4 = side ? reinterpret_cast<const float4*>(Wd) + ((int64_t)(nt - 30) * 192 + 2 * T0) * 64 + lane
                                 : reinterpret_cast<const float4*>(Wh) + ((int64_t)nt * K8h + 2 * T0) * 64 + lane;
        q3_body<HP, RBM, BLK>(wp4, h3 + (int64_t)T0 * 3 * 64 + lane, (int64_t)96 * 3 * 64, side ? nt - 30 : nt, side ? hc : 2 + hc, side, RB_p, a, red_dyn);
    }
    kspan(a.dbg_seq, 1);
}

#ifndef MELLOW_GU3_WAVES
#define MELLOW_GU3_WAVES 6
#endif
constexpr int GU3W = MELLOW_GU3_WAVES;
// K4b (f32x3, any number of row blocks): see dec_gateup16_kernel.  x3 = x_mid in F3-16 (18 pairs x 2 row halves per block).
// Writes h both as fp32 (guF: the last layer's fp32 down projection reads it) and pre-split (h3, F3-32 with 96 pairs).
template <bool BLK, int RBM>
__global__ __launch_bounds__(GU3W * 64) void dec_gateup3_kernel(const float* __restrict__ Wp16, const i32x4* __restrict__ x3,
                                                                const float* __restrict__ ssq_in, int RB_p, const DecArgs a) {
    kspan(a.dbg_seq, 0);
    extern __shared__ __attribute__((aligned(16))) float red_dyn[];        // [GU3W][RBM][8][64]
    float* red = red_dyn;
    constexpr int NP = 18 / GU3W;
    static_assert(NP * GU3W == 18, "waves must divide the 18 k-pairs");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x;
    const int T0 = wave * NP;
    i32x4 wp[NP][3];
    i32x4 xq[2][NP][2][3];
    const i32x4* xsrc = x3 + (int64_t)T0 * 2 * 3 * 64 + lane;
    constexpr int64_t RBS = (int64_t)18 * 2 * 3 * 64;          // slots per row block
    {
        // P16N: [n16-tile][pair T][half][lane][4 floats]: lane (n, q) holds k = 32 T + 8 q + 4 half .. + 3 (1 KiB per wave load)
        const float4* wp4 = reinterpret_cast<const float4*>(Wp16) + ((int64_t)nt * 18 + T0) * 128 + lane;
        float4 w[2 * NP];
#pragma unroll
        for (int i = 0; i < 2 * NP; ++i) w[i] = ldg_nt(wp4 + i * 64);
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int c = 0; c < 6; ++c) xq[0][p][c / 3][c % 3] = xsrc[(p * 6 + c) * 64];          // block 0, requested with the weights
        if (RBM == 2 && RB_p > 1) {              // a two-block pass: both blocks' fragments at once
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int c = 0; c < 6; ++c) xq[1][p][c / 3][c % 3] = xsrc[RBS + (p * 6 + c) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < NP; ++p) split_pair(w[2 * p], w[2 * p + 1], wp[p][0], wp[p][1], wp[p][2]);
    }
    for (int rb0 = 0; rb0 < RB_p; rb0 += RBM) {
        const int gn = min(RBM, RB_p - rb0);
        // the epilogue's RMS statistic (36 partial sums per row, written by the o_proj): requested with the operands, not after
        // the reduction barrier.  Epilogue thread e = tid (+ a second round when gn * 64 > the block): row block e / 64, row (e % 64) / 2
        float4 s4[2][9];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = tid + k * GU3W * 64;
            if (e < gn * 64 && (k == 0 || RBM * 64 > GU3W * 64)) {
                const float4* sq = reinterpret_cast<const float4*>(ssq_in + ((int64_t)(rb0 + (e >> 6)) * 32 + ((e & 63) >> 1)) * 40);
#pragma unroll
                for (int j = 0; j < 9; ++j) s4[k][j] = sq[j];
            }
        }
        f32x4 acc0[RBM], acc1[RBM];
        if (rb0) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int c = 0; c < 6; ++c) xq[0][p][c / 3][c % 3] = xsrc[(int64_t)rb0 * RBS + (p * 6 + c) * 64];
            if (RBM == 2 && gn > 1) {
#pragma unroll
                for (int p = 0; p < NP; ++p)
#pragma unroll
                    for (int c = 0; c < 6; ++c) xq[1][p][c / 3][c % 3] = xsrc[(int64_t)(rb0 + 1) * RBS + (p * 6 + c) * 64];
            }
        }
#pragma unroll
        for (int g = 0; g < RBM; ++g) {
            acc0[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc1[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (g < gn) {
                if (RBM > 2 && g + 1 < RBM && g + 1 < gn) {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int c = 0; c < 6; ++c) xq[(g + 1) & 1][p][c / 3][c % 3] = xsrc[(int64_t)(rb0 + g + 1) * RBS + (p * 6 + c) * 64];
                }
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    // the two row halves are independent accumulator chains: term by term, alternating (a dependent MFMA waits ~2x its issue time)
#define MELLOW_G3_TERM(PW, PX) MELLOW_BF16S(wp[p][PW], xq[g & 1][p][0][PX], acc0[g]); MELLOW_BF16S(wp[p][PW], xq[g & 1][p][1][PX], acc1[g]);
                    MELLOW_G3_TERM(2, 0) MELLOW_G3_TERM(0, 2) MELLOW_G3_TERM(1, 1) MELLOW_G3_TERM(1, 0) MELLOW_G3_TERM(0, 1) MELLOW_G3_TERM(0, 0)
#undef MELLOW_G3_TERM
                }
            }
        }
        if (rb0) __syncthreads();
#pragma unroll
        for (int g = 0; g < RBM; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                red[((wave * RBM + g) * 8 + r) * 64 + lane] = acc0[g][r];
                red[((wave * RBM + g) * 8 + 4 + r) * 64 + lane] = acc1[g][r];
            }
        __syncthreads();
        // thread (g, m, q): as the epilogue of dec_gateup16_kernel, 64 threads per row block
        static_assert(RBM * 64 <= 2 * GU3W * 64, "two epilogue rounds cover a pass");
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = tid + k * GU3W * 64;
            if (e >= gn * 64 || (k == 1 && RBM * 64 <= GU3W * 64)) continue;
            const int g = e >> 6, t = e & 63, rb = rb0 + g;
            if (BLK && a.blk_live[rb] == 0) continue;
            const int m = t >> 1, q = t & 1;
            const int gl = (m & 15) + 16 * q, ul = gl + 32, rbase = (m >> 4) * 4;
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 9; ++j) ss += (s4[k][j].x + s4[k][j].y) + (s4[k][j].z + s4[k][j].w);
            const float r2 = 1.0f / sqrtf(ss / 576.0f + a.eps);
            float h[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float gv = red[((0 * RBM + g) * 8 + rbase + r) * 64 + gl], uv = red[((0 * RBM + g) * 8 + rbase + r) * 64 + ul];
#pragma unroll
                for (int wv = 1; wv < GU3W; ++wv) {                       // fixed order
                    gv += red[((wv * RBM + g) * 8 + rbase + r) * 64 + gl];
                    uv += red[((wv * RBM + g) * 8 + rbase + r) * 64 + ul];
                }
                h[r] = __fmul_rn(siluf_(gv * r2), uv * r2);
            }
            const float4 hv = as_stored(make_float4(h[0], h[1], h[2], h[3]));
            *(reinterpret_cast<float4*>(a.guF) + ((int64_t)rb * 192 + nt) * 64 + m + 32 * q) = hv;
            const F3Quad hq = f3_split4(hv), ho = f3_partner(hq);     // threads (q = 0, q = 1) of a row hold the halves of one slot
            if (q == 0) f3_store8(a.h3, f3_32_slot(rb, 96, m, 8 * nt), hq, ho);
        }
    }
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// K4b gate/up projection + SwiGLU on 16-row weight tiles.  grid (192 n16-tiles, RB), 4 waves x 9 k16-tiles,
//     v_mfma_f32_16x16x4_f32; W = folded gate/up in P16-layout, tile t = gate[8t..8t+7] | up[8t..8t+7];
//     X = x_mid in F16-layout.  192 workgroups x (36 KB of W + 72 KB of X).
//     epilogue: r2[m] = rsqrt(mean(x_mid[m]^2) + eps) from the o_proj's per-tile sums;
//     h = silu(r2 g) * (r2 u)  ->  hF[rb][hidden/8][lane][4]  (F32-layout B operand of the down projection)
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_GU_WAVES
#define MELLOW_GU_WAVES 4
#endif
constexpr int GU_WAVES = MELLOW_GU_WAVES;
template <bool BLK, int W8>
__global__ __launch_bounds__(GU_WAVES * 64) void dec_gateup16_kernel(const float* __restrict__ Wp16, const float* __restrict__ xF16,
                                                                     const float* __restrict__ ssq_in, const DecArgs a,
                                                                     const float* __restrict__ wscale) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[GU_WAVES * 8 * 64];
    constexpr int K16 = 36, TPW = K16 / GU_WAVES;
    static_assert(TPW * GU_WAVES == K16, "waves must divide the 36 k16-tiles");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x, rb = blockIdx.y;
    MELLOW_BLK_EXIT(rb)
    const int t0 = wave * TPW;
    const int64_t wslot = ((int64_t)nt * K16 + t0) * 64 + lane;
    const float4* xp = reinterpret_cast<const float4*>(xF16) + (((int64_t)rb * 36 + t0) * 2) * 64 + lane;
    // epilogue thread (m = tid>>1, q = tid&1), tid < 64: its row's 36 sum-of-squares partials, issued up front
    const float4* sq = reinterpret_cast<const float4*>(ssq_in + ((int64_t)rb * 32 + ((tid >> 1) & 31)) * 40);
    WFrag<TPW, W8> w;
    float4 x0[TPW], x1[TPW], s4[9];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        w.t[i] = w.load(Wp16, wslot + i * 64);
        x0[i] = xp[(i * 2) * 64];
        x1[i] = xp[(i * 2 + 1) * 64];
    }
    if (tid < 64) {
#pragma unroll
        for (int j = 0; j < 9; ++j) s4[j] = sq[j];
    }
    __builtin_amdgcn_sched_barrier(0);
    // rows 0..15 (x0) and 16..31 (x1) of the block against the same weight fragment
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 acc0 = slice_mma16<TPW, W8>(zero, w, x0), acc1 = slice_mma16<TPW, W8>(zero, w, x1);
    reduce_store(MELLOW_LDS(red) + wave * 8 * 64 + lane, acc0);
    reduce_store(MELLOW_LDS(red) + (wave * 8 + 4) * 64 + lane, acc1);
    __syncthreads();
    if (tid < 64) {
        // D[i = tile row 4*(lane>>4) + r][j = batch row lane&15], accumulator (m>>4).  Tile rows 0..7 = gate of hidden
        // units 8nt..8nt+7, rows 8..15 = up of the same units: thread (m, q) combines gate rows 4q..4q+3 (lane group q)
        // with up rows 8+4q.. (lane group q+2).
        const int m = tid >> 1, q = tid & 1;
        const int gl = (m & 15) + 16 * q, ul = gl + 32, rbase = (m >> 4) * 4;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) ss += (s4[j].x + s4[j].y) + (s4[j].z + s4[j].w);
        const float r2 = 1.0f / sqrtf(ss / 576.0f + a.eps);
        float h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float gv = red_sum<GU_WAVES, 8>(MELLOW_LDS(red), rbase + r, gl), uv = red_sum<GU_WAVES, 8>(MELLOW_LDS(red), rbase + r, ul);
            if (W8) { gv *= wscale[nt * 16 + 4 * q + r]; uv *= wscale[nt * 16 + 8 + 4 * q + r]; }     // packed tile rows
            h[r] = __fmul_rn(siluf_(gv * r2), uv * r2);
        }
        // hidden unit k = 8*nt + 4*q + r: down k-tile nt, F32-layout lane' = m + 32*q
        *(reinterpret_cast<float4*>(a.guF) + ((int64_t)rb * 192 + nt) * 64 + m + 32 * q) = make_float4(h[0], h[1], h[2], h[3]);
    }
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// K5  down projection, split-K.  grid (18 n-tiles, DEC_KC_DOWN, RB), 6 waves x 4 k-tiles.
//     X = h (SwiGLU output of K4b, F32-layout);  out: down slabs in F32-layout (next layer's qkv / final norm)
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_DOWN_WAVES
#define MELLOW_DOWN_WAVES 4
#endif
// waves per workgroup: 4 x 6 k-tiles (one wave per SIMD, a 4-way LDS reduction): 52.2 ms of decode per 63 steps against
// 53.0-53.2 with 6 x 4, 8 x 3 or 12 x 2 (same box, tools/ab_build.sh)
constexpr int DN_WAVES = MELLOW_DOWN_WAVES;
static_assert(DN_WAVES >= 4 && 192 % (8 * DN_WAVES) == 0, "the epilogue needs 256 threads; waves must divide the k-tiles");
template <bool BLK, int W8>
__global__ __launch_bounds__(DN_WAVES * 64) void dec_down_kernel(const float* __restrict__ Wp, const float* __restrict__ guF_p, int K8p,
                                                                 const DecArgs a, const float* __restrict__ wscale) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[DN_WAVES * 16 * 64];
    constexpr int KPW = 192 / (DEC_KC_DOWN * DN_WAVES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x, kc = blockIdx.y, rb = blockIdx.z;
    MELLOW_BLK_EXIT(rb)
    const int k8_0 = (kc * DN_WAVES + wave) * KPW;
    const int64_t wslot = ((int64_t)nt * K8p + k8_0) * 64 + lane;
    const float4* hp = reinterpret_cast<const float4*>(guF_p) + ((int64_t)rb * 192 + k8_0) * 64 + lane;
    const bool dbg = tid == 0 && nt == 0 && kc == 0 && rb == 0;
    kstamp(4, 0, dbg);
    WFrag<KPW, W8> w;
    float4 h4[KPW];
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        w.t[i] = w.load(Wp, wslot + i * 64);
        h4[i] = hp[i * 64];
    }
    __builtin_amdgcn_sched_barrier(0);
    kstamp(4, 1, dbg);
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    acc = slice_mma32<KPW, W8>(acc, w, h4);
    kstamp(4, 2, dbg && acc[0] == acc[0]);
    reduce_store(MELLOW_LDS(red) + wave * 16 * 64 + lane, acc);
    __syncthreads();
    kstamp(4, 3, dbg);
    if (tid < 256) {
        const int mm = tid & 31, n = epi_col(nt, tid);
        float4 v = reduce32<DN_WAVES>(MELLOW_LDS(red), tid);
        if (W8) v = f4scale(v, wscale + n);
        reinterpret_cast<float4*>(a.dslabF)[(int64_t)kc * a.slabF_stride4 + f32_idx(rb, 72, mm, n)] = v;
    }
    kstamp(4, 4, dbg);
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// K5+K1  the down projection of layer l and the q/k/v projection of layer l+1 in ONE launch (no kernel boundary between them).
//     qkv_{l+1} = W' x_new with x_new = x_mid + Wd h is linear in (x_mid, h):  W' x_mid + (W' Wd) h.  The product Q = W' Wd
//     (960 x 1536) is formed once at load time in fp64 and rounded to fp32 (engine_weights.cpp), and stored behind W' in one P-layout
//     matrix Wq2 [30 n-tiles][72 + 192 k-tiles].  The residual stream itself still goes through Wd (the "side" tiles), so the
//     composed weights only ever feed the next RMS-scaled projection, never the residual.
//     Workgroup types (grid.x):   [0, 60)              x part: n-tile b % 30, k-chunk b / 30 (2 chunks of 36 k-tiles of x_mid)
//                                 [60, 60 + 48 Q2_HC)  h part: k-chunk hc of h (192 / Q2_HC k-tiles);
//                                                      n-tile < 30: Q rows -> pq slab 2 + hc;  n-tile >= 30: Wd rows -> down slab hc
//     Consumer: dec_attn_kernel<FUSED> sums the Q2_NPQ pq slabs and forms x_new = x_mid + sum of the Q2_HC down slabs.
// ----------------------------------------------------------------------------------------------------
// Q2W = waves per workgroup (chosen per launch: 4 for one row block, Q2W otherwise)
// Operands: Wx = W' (P-layout, K8x k-tiles per n-tile), Wh = W' Wd (K8h k-tiles per n-tile), Wd = the down weight (192 k-tiles).
//   fp32 (W8 == 0): Wx and Wh are the two column ranges of ONE matrix [30][72 + 192] (K8x = K8h = Q2_K8)
//   e4m3 (W8 != 0): three separately quantised matrices (the q/k/v copy of the unfused layer, the composed one, the down copy),
//                   one scale per packed row each: sc_x, sc_h, sc_d; W8 == 2 also quantises x_mid / h per wave slice (see WFrag)
template <bool BLK, int Q2W, int W8>
__global__ __launch_bounds__(Q2W * 64) void dec_qkv2_kernel(const float* __restrict__ Wx, const float* __restrict__ Wh,
                                                            const float* __restrict__ Wd, const float* __restrict__ xmidF_p,
                                                            const float* __restrict__ guF_p, int K8x, int K8h, const DecArgs a,
                                                            const float* __restrict__ sc_x, const float* __restrict__ sc_h,
                                                            const float* __restrict__ sc_d) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[Q2W * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, rb = blockIdx.y;
    MELLOW_BLK_EXIT(rb)
    const bool dbg = tid == 0 && b == 60 && rb == 0;          // an h-part workgroup (the longest kind)
    kstamp(7, 0, dbg);
    constexpr int XT = 36 / Q2W, HT = (192 / Q2_HC) / Q2W;      // k-tiles per wave
    static_assert(XT * Q2W == 36 && HT * Q2W * Q2_HC == 192, "waves must divide the k-chunks");
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    int nt, slab;
    bool side = false;
    const float* wsc = sc_x;
    if (b < 60) {              // x part (workgroup-uniform branch; each side keeps its loads straight-line)
        nt = b % 30; slab = b / 30;
        const int k8_0 = slab * 36 + wave * XT;
        const int64_t wslot = ((int64_t)nt * K8x + k8_0) * 64 + lane;
        const float4* xb = reinterpret_cast<const float4*>(xmidF_p) + ((int64_t)rb * 72 + k8_0) * 64 + lane;
        WFrag<XT, W8> w;
        float4 x[XT];
#pragma unroll
        for (int i = 0; i < XT; ++i) {
            w.t[i] = w.load(Wx, wslot + i * 64);
            x[i] = xb[i * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = slice_mma32<XT, W8>(acc, w, x);
    } else {                   // h part
        const int idx = b - 60, hc = idx / 48;
        nt = idx % 48;
        side = nt >= 30;
        slab = side ? hc : 2 + hc;
        wsc = side ? sc_d : sc_h;
        const int k8_0 = hc * (192 / Q2_HC) + wave * HT;
        const float* wbase = side ? Wd : Wh;
        const int64_t wslot = side ? ((int64_t)(nt - 30) * 192 + k8_0) * 64 + lane : ((int64_t)nt * K8h + k8_0) * 64 + lane;
        const float4* hp = reinterpret_cast<const float4*>(guF_p) + ((int64_t)rb * 192 + k8_0) * 64 + lane;
        WFrag<HT, W8> w;
        float4 h4[HT];
#pragma unroll
        for (int i = 0; i < HT; ++i) {
            w.t[i] = w.load(wbase, wslot + i * 64);
            h4[i] = hp[i * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        kstamp(7, 1, dbg);
        acc = slice_mma32<HT, W8>(acc, w, h4);
        kstamp(7, 2, dbg && acc[0] == acc[0]);
        if (side) nt -= 30;
    }
    reduce_store(MELLOW_LDS(red) + wave * 16 * 64 + lane, acc);
    __syncthreads();
    kstamp(7, 3, dbg);
    if (tid < 256) {
        const int mm = tid & 31, n = epi_col(nt, tid);
        float4 o = reduce32<Q2W>(MELLOW_LDS(red), tid);
        if (W8) o = f4scale(o, wsc + n);
        if (side) *(reinterpret_cast<float4*>(a.dslabF) + (int64_t)slab * a.slabF_stride4 + f32_idx(rb, 72, mm, n)) = o;
        else *reinterpret_cast<float4*>(a.pq + ((int64_t)slab * a.rows + rb * 32 + mm) * 960 + n) = o;
    }
    kstamp(7, 4, dbg);
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// row-parallel helpers (one workgroup per batch row)
// ----------------------------------------------------------------------------------------------------
// final RMSNorm: xn = w * ((x_mid + sum down slabs) * rsqrt(mean^2 + eps)) -> F32-layout operand of the lm_head
template <int KCD, bool BLK>
__global__ __launch_bounds__(192) void dec_final_norm_kernel(const float* __restrict__ norm_w, const float* __restrict__ xmidF_p,
                                                             const float* __restrict__ dslabF_p, int64_t stride4_p, const DecArgs a) {
    kspan(a.dbg_seq, 0);
    __shared__ float part[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (BLK && b == 0 && tid < 32) a.blk_snap[tid] = a.blk_live[tid];      // for this step's arg-max (kernels.h)
    MELLOW_BLK_EXIT(b >> 5)
    const int xi = tid < 144 ? tid : 0;
    const int64_t fi = f32_idx(b >> 5, 72, b & 31, xi * 4);
    float4 v = reinterpret_cast<const float4*>(xmidF_p)[fi];
    float4 xs[KCD > 0 ? KCD : 1];
#pragma unroll
    for (int s = 0; s < KCD; ++s) xs[s] = reinterpret_cast<const float4*>(dslabF_p)[(int64_t)s * stride4_p + fi];
    const float4 wv = reinterpret_cast<const float4*>(norm_w)[xi];
#pragma unroll
    for (int s = 0; s < KCD; ++s) v = f4add(v, xs[s]);
    float ss = tid < 144 ? f4ssq(v) : 0.f;
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    const float r = 1.0f / sqrtf((part[0] + part[1] + part[2]) / 576.0f + a.eps);
    if (tid < 144) {
        float4 y;
        y.x = __fmul_rn(wv.x, __fmul_rn(v.x, r)); y.y = __fmul_rn(wv.y, __fmul_rn(v.y, r));
        y.z = __fmul_rn(wv.z, __fmul_rn(v.z, r)); y.w = __fmul_rn(wv.w, __fmul_rn(v.w, r));
        if (!a.xn3) reinterpret_cast<float4*>(a.xnF)[fi] = y;
    }
    if (a.xn3) {                       // f32x3 lm_head: pre-split, F3-32; threads 2i, 2i + 1 hold the halves of one slot
        float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < 144) {
            y.x = __fmul_rn(wv.x, __fmul_rn(v.x, r)); y.y = __fmul_rn(wv.y, __fmul_rn(v.y, r));
            y.z = __fmul_rn(wv.z, __fmul_rn(v.z, r)); y.w = __fmul_rn(wv.w, __fmul_rn(v.w, r));
        }
        const F3Quad mine = f3_split4(y), other = f3_partner(mine);
        if (tid < 144 && !(tid & 1)) f3_store8(a.xn3, f3_32_slot(b >> 5, 36, b & 31, tid * 4), mine, other);
    }
    kspan(a.dbg_seq, 1);
}

// ---- launchers -------------------------------------------------------------------------------------------
void launch_dec_qkv(const DecArgs& a, const float* Wp, int K8p, int kcd, hipStream_t s, const float* wscale) {
    const dim3 grid(30, DEC_KC_QKV, a.RB);
    // the first qkv launch of a step (a.first) always starts from a materialised x (kcd == 0); later ones sum the down slabs
    with_int<0, DEC_KC_DOWN>(kcd, [&](auto kcd_c) { with_bool(a.first != 0, [&](auto first) { with_blk_w8(a, wscale, [&](auto blk, auto w8) {
        hipLaunchKernelGGL((dec_qkv_kernel<kcd_c.value, blk.value, first.value, w8.value>), grid, dim3(QKV_THREADS), 0, s, Wp, (const float*)a.xmidF,
                           (const float*)a.dslabF, K8p, a, wscale);
    }); }); });
}
// fp32 form: Wq2 = [30][Q2_K8] (W' | W' Wd);  e4m3 form (sc_x != null): three separately quantised matrices (kernel comment)
static void launch_dec_qkv2_any(const DecArgs& a, const float* Wx, int K8x, const float* Wh, int K8h, const float* Wd,
                                const float* sc_x, const float* sc_h, const float* sc_d, hipStream_t s) {
    // waves per workgroup: 4 x (9 | 12) k-tiles when there is one row block (a 4-way instead of a 12-way LDS reduction: 49.55 vs
    // 49.98 ms of decode per 63 steps at B = 32), 12 x (3 | 4) otherwise (B = 64: 76.3 vs 77.2 ms); -DMELLOW_Q2_WAVES=n forces one
    const dim3 grid(Q2_BLOCKS, a.RB);
#ifdef MELLOW_Q2_WAVES_FORCED
    bool few = false;
#else
    bool few = a.RB == 1;
#endif
    // (activations on the fp8 pipe: a wave's k-slice is the unit of the activation scale, so the wave count must not depend on
    //  the batch size -- a row's tokens would otherwise change with the number of row blocks around it)
    if (w8_mode(a, sc_x) == 2) few = false;
    with_bool(few, [&](auto few_c) { with_blk_w8(a, sc_x, [&](auto blk, auto w8) {
        constexpr int WV = few_c.value ? 4 : Q2_WAVES;
        hipLaunchKernelGGL((dec_qkv2_kernel<blk.value, WV, w8.value>), grid, dim3(WV * 64), 0, s, Wx, Wh, Wd, (const float*)a.xmidF,
                           (const float*)a.guF, K8x, K8h, a, sc_x, sc_h, sc_d);
    }); });
}
// The kernels with dynamic LDS: one function per family states the byte count, and one hands f(kernel, bytes) the instantiation
// that serves `rb` row blocks (>= 1; RBM / G = 1, 2, or 4 for every larger count) -- to the launcher and to
// dec_gemv_prepare_lds alike (the lm_head's: dec_tail.hip).
constexpr size_t dec_qkv2x3_lds(int rbm) { return (size_t)Q3W * rbm * 16 * 64 * 4; }
constexpr size_t dec_gateup3_lds(int rbm) { return (size_t)GU3W * rbm * 8 * 64 * 4; }
template <class F> static inline void with_qkv2x3(int rb, bool blk, F&& f) {
    with_int<1, 2, 4>(rb, [&](auto rbm) { with_bool(blk, [&](auto b) { f(&dec_qkv2x3_kernel<b.value, rbm.value>, dec_qkv2x3_lds(rbm.value)); }); });
}
template <class F> static inline void with_gateup3(int rb, bool blk, F&& f) {
    with_int<1, 2, 4>(rb, [&](auto rbm) { with_bool(blk, [&](auto b) { f(&dec_gateup3_kernel<b.value, rbm.value>, dec_gateup3_lds(rbm.value)); }); });
}
void launch_dec_qkv2x3(const DecArgs& a, const float* Wq2, const float* Wd, hipStream_t s) {
    const float* Wh = Wq2 + (size_t)72 * 64 * 4;
    const i32x4 *x3 = reinterpret_cast<const i32x4*>(a.xmid3_32), *h3 = reinterpret_cast<const i32x4*>(a.h3);
    with_qkv2x3(a.RB, a.blk_live != nullptr, [&](auto* kernel, size_t lds) {
        set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds);
        hipLaunchKernelGGL(kernel, dim3(Q2_BLOCKS), dim3(Q3W * 64), lds, s, Wq2, Wh, Wd, x3, h3, Q2_K8, Q2_K8, a.RB, a);
    });
}
void launch_dec_gateup3(const DecArgs& a, const float* Wp16, hipStream_t s) {
    const i32x4* x3 = reinterpret_cast<const i32x4*>(a.xmid3_16);
    with_gateup3(a.RB, a.blk_live != nullptr, [&](auto* kernel, size_t lds) {
        set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds);      // (beyond 64 KiB only with more waves: MELLOW_GU3_WAVES)
        hipLaunchKernelGGL(kernel, dim3(192), dim3(GU3W * 64), lds, s, Wp16, x3, (const float*)a.ssq, a.RB, a);
    });
}
void launch_dec_qkv2(const DecArgs& a, const float* Wq2, const float* Wd, hipStream_t s) {
    launch_dec_qkv2_any(a, Wq2, Q2_K8, Wq2 + (size_t)72 * 64 * 4, Q2_K8, Wd, nullptr, nullptr, nullptr, s);
}
void launch_dec_qkv2_w8(const DecArgs& a, const float* Wx8, const float* sc_x, const float* Wh8, const float* sc_h,
                        const float* Wd8, const float* sc_d, hipStream_t s) {
    launch_dec_qkv2_any(a, Wx8, 72, Wh8, 192, Wd8, sc_x, sc_h, sc_d, s);
}
void launch_dec_gateup(const DecArgs& a, const float* Wp16, hipStream_t s, const float* wscale) {
    with_blk_w8(a, wscale, [&](auto blk, auto w8) {
        hipLaunchKernelGGL((dec_gateup16_kernel<blk.value, w8.value>), dim3(192, a.RB), dim3(GU_WAVES * 64), 0, s, Wp16, a.xmidF16, a.ssq, a, wscale);
    });
}
void launch_dec_down(const DecArgs& a, const float* Wp, int K8p, hipStream_t s, const float* wscale) {
    with_blk_w8(a, wscale, [&](auto blk, auto w8) {
        hipLaunchKernelGGL((dec_down_kernel<blk.value, w8.value>), dim3(18, DEC_KC_DOWN, a.RB), dim3(DN_WAVES * 64), 0, s, Wp, (const float*)a.guF,
                           K8p, a, wscale);
    });
}
void launch_dec_final_norm(const DecArgs& a, const float* norm_w, int kcd, hipStream_t s) {
    with_int<0, DEC_KC_DOWN>(kcd, [&](auto kcd_c) { with_bool(a.blk_live != nullptr, [&](auto blk) {
        hipLaunchKernelGGL((dec_final_norm_kernel<kcd_c.value, blk.value>), dim3(a.rows), dim3(192), 0, s, norm_w, (const float*)a.xmidF,
                           (const float*)a.dslabF, a.slabF_stride4, a);
    }); });
}
// this file's share of dec_prepare_lds_attributes (engine.cpp): every instantiation the two launchers above can pick
void dec_gemv_prepare_lds() {
    const auto raise = [](auto* kernel, size_t lds) { set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds); };
    for (const int rb : {1, 2, 4})
        for (const bool blk : {false, true}) {
            with_qkv2x3(rb, blk, raise);
            with_gateup3(rb, blk, raise);
        }
}

}  // namespace mellow
