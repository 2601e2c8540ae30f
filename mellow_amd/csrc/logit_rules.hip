// Repetition controls inside the decode step (include/mellow_hip.h, mellow_generate_rules states the exact definition; DESIGN.md 6m
// where the launch sits): one launch between the lm_head and whichever kernel picks the token (arg-max, sampler, beam select).
//
// One 1024-thread workgroup per batch slot, in the sampler's tiling (48 values per thread, coalesced float4 loads):
//   1. the row's history h[0 .. s) is staged in LDS.  Plain calls read it from the token record (it is indexed by EXAMPLE, so a
//      row that migrated to another slot still finds its own); beam rows first build it from their parent's copy in a ping-pong
//      buffer plus the token the last selection gave them; the tap reads the caller's rows;
//   2. two LDS bitmaps of one bit per token: `pen` = the tokens of the history (repetition penalty: once per DISTINCT token), `ban` =
//      the tokens that would complete a repeated n-gram, plus the stop id while s < min_new_tokens.  Marked with atomicOr, threads
//      strided over the history positions: a bitmap is a set, so the result does not depend on which thread gets there first;
//   3. every thread applies penalty, bias and bans, in that order, to its own 48 values and stores the float4 groups that changed;
//   4. the per-32-column partials the greedy arg-max and the LSE merges read instead of the logits (cand_val / cand_idx in arg_better
//      order, cand_sum = sum exp(l - cand_val), exactly 0 for a tile whose maximum is -inf) are formed anew from the processed values:
//      a tile is the eight float4 groups of eight neighbouring lanes, reduced by three butterfly steps in one fixed order.
// No float atomics and no arrival order anywhere: the bits depend on the inputs only.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

__device__ __forceinline__ void mark(uint32_t* map, int t) {
    if ((unsigned)t < (unsigned)SAMPLE_MAX_V) atomicOr(&map[t >> 5], 1u << (t & 31));      // (an id outside the vocabulary marks nothing)
}

__global__ __launch_bounds__(ROW_THREADS) void dec_logit_rules_kernel(const RulesArgs g) {
    __shared__ int32_t hist[RULES_MAX_HIST];
    __shared__ uint32_t pen[ROW_TILES], ban[ROW_TILES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(g.row_of_slot, g.blk_snap, b);
    if (dead) return;

    const float theta = __uint_as_float(g.prm[RUL_THETA]);
    const int n = (int)g.prm[RUL_NGRAM], min_new = (int)g.prm[RUL_MIN_NEW], stop_id = (int)g.prm[RUL_STOP];
    const bool bias_on = g.prm[RUL_BIAS_ON] != 0;

    // ---- 1. the history ---------------------------------------------------------------------------------------------------------
    int s;
    if (g.hist_len) {                                                 // tap: caller rows, a length per row
        s = min(max(g.hist_len[b], 0), min(g.hist_ld, RULES_MAX_HIST));
        const int32_t* __restrict__ h = g.hist + (int64_t)b * g.hist_ld;
        for (int i = tid; i < s; i += ROW_THREADS) hist[i] = h[i];
    } else {
        const int max_len = min(g.params[0], RULES_MAX_HIST);
        s = min(max(*g.d_pos - g.T0 + 1, 0), max_len);
        if (g.beam_hist) {
            // row r continues beam parent_tab[s - 1][r] of its example: that row's history before the last selection (the other half of
            // the ping-pong buffer: no row reads what a row of this launch writes) plus the token the selection gave r
            if (s >= 1) {
                const int pr = row / g.k * g.k + min(max(g.parent_tab[(int64_t)(s - 1) * g.N + row], 0), g.k - 1);
                const int32_t* __restrict__ src = g.beam_hist + ((int64_t)((s - 1) & 1) * g.N + pr) * g.hist_ld;
                int32_t* __restrict__ dst = g.beam_hist + ((int64_t)(s & 1) * g.N + row) * g.hist_ld;
                for (int i = tid; i < s; i += ROW_THREADS) {
                    const int32_t t = i < s - 1 ? src[i] : g.token_tab[(int64_t)(s - 1) * g.N + row];
                    hist[i] = t;
                    dst[i] = t;
                }
            }
        } else {
            const int32_t* __restrict__ h = g.hist + (int64_t)row * g.params[0];      // the token record: columns [0, s) are written
            for (int i = tid; i < s; i += ROW_THREADS) hist[i] = h[i];
        }
    }
    for (int i = tid; i < ROW_TILES; i += ROW_THREADS) { pen[i] = 0u; ban[i] = 0u; }
    __syncthreads();

    // ---- 2. the two sets --------------------------------------------------------------------------------------------------------
    for (int i = tid; i < s; i += ROW_THREADS) mark(pen, hist[i]);
    if (n > 0 && s >= n - 1) {
        // position i starts an (n - 1)-gram equal to the last n - 1 tokens: the token after it would repeat an n-gram
        for (int i = tid; i <= s - n; i += ROW_THREADS) {
            bool eq = true;
            for (int j = 0; j < n - 1 && eq; ++j) eq = hist[i + j] == hist[s - n + 1 + j];
            if (eq) mark(ban, hist[i + n - 1]);
        }
    }
    if (tid == 0 && s < min_new && stop_id >= 0) mark(ban, stop_id);
    __syncthreads();

    // ---- 3. apply, 4. tile partials ---------------------------------------------------------------------------------------------
    float* __restrict__ lrow = g.logits + (int64_t)b * g.ld;
    const int64_t cbase = (int64_t)b * ROW_TILES;
#pragma unroll 2
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + tid;
        const float4 v4 = reinterpret_cast<const float4*>(lrow)[i4];
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias_on) b4 = reinterpret_cast<const float4*>(g.bias)[i4];
        const uint32_t pb = pen[i4 >> 3] >> ((i4 & 7) * 4), bb = ban[i4 >> 3] >> ((i4 & 7) * 4);
        const float in[4] = {v4.x, v4.y, v4.z, v4.w}, bi[4] = {b4.x, b4.y, b4.z, b4.w};
        float v[4];
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = in[j];
            if ((pb >> j) & 1u) x = x < 0.f ? __fmul_rn(x, theta) : __fdiv_rn(x, theta);
            if (bias_on) x = __fadd_rn(x, bi[j]);
            if ((bb >> j) & 1u) x = -INFINITY;
            v[j] = x;
            changed |= __float_as_uint(x) != __float_as_uint(in[j]);
        }
        if (changed) reinterpret_cast<float4*>(lrow)[i4] = make_float4(v[0], v[1], v[2], v[3]);
        const auto [bv, bx] = tile_best(v, i4);
        if (g.cand_sum) {
            // a tile whose maximum is -inf (banned whole) sums to exactly 0: no exp(-inf - -inf)
            float ps = 0.f;
            if (bv > -INFINITY || bv != bv) ps = tile_exp4(v, bv);
            ps = tile_sum8(ps);
            if ((tid & 7) == 0) g.cand_sum[cbase + (i4 >> 3)] = ps;
        }
        if ((tid & 7) == 0) {
            g.cand_val[cbase + (i4 >> 3)] = bv;
            g.cand_idx[cbase + (i4 >> 3)] = bx;
        }
    }
}

}  // namespace

void launch_dec_logit_rules(const RulesArgs& g, int B, hipStream_t s) {
    if (B <= 0 || g.ld != SAMPLE_MAX_V) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(dec_logit_rules_kernel, dim3(B), dim3(ROW_THREADS), 0, s, g);
}

}  // namespace mellow
