// The k likeliest tokens of a decode step's row (include/mellow_hip.h, mellow_generate_top_logprobs states the exact definition;
// DESIGN.md 6o where the launch sits): one launch between the rules launch and whichever kernel picks the token, so it sees exactly
// the row the token is chosen from.  It reads the row and its tile partials and writes the record only.
//
// One 1024-thread workgroup per batch slot, in the sampler's tiling (48 values per thread, coalesced float4 loads):
//   1. the row's log-sum-exp is merged from the (cand_val, cand_sum) partials by dec_lse_max / dec_lse_sum / dec_lse_value
//      (common.h), the functions and the order dec_sample_kernel<true> uses: the same bits;
//   2. every thread turns its 48 values into order-preserving u32 keys (-0 counts as +0) and keeps them in registers, slot s = 4 q + j
//      of a thread being index 4 * (q * 1024 + tid) + j: a thread's slots ascend with the index.  The order (value descending, index
//      ascending) is (key descending, index ascending), and no two elements are equal in it;
//   3. k rounds of a block maximum.  Every thread offers the first of its elements it has not given away yet (it keeps its two
//      first ones at hand and looks through its 48 keys again, past a bit mask of those given away, only when both are gone); a
//      wave finds the largest key and then the lowest index among the lanes that hold it with DPP steps, the sixteen wave results
//      meet in LDS (two buffers in turn: one barrier per round) and every 16-lane row reduces them the same way.  Integer compares
//      only: the selection is exact and depends on no arrival order;
//   4. threads 0 .. k - 1 read the winners' logits back from the row and record (id, l[id] - lse).
// No atomics: the result depends on the inputs only.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

constexpr int TL_SLOTS = 4 * ROW_NV4;                       // values per thread (48)
static_assert(ROW_WAVES == 16, "the wave results are reduced by one 16-lane DPP row");

// the order key of a raw logit: these come straight from the head and may be -0, which has to rank as +0 does (+ 0.0f turns it)
__device__ __forceinline__ uint32_t tl_key(float z) { return order_key(z + 0.0f); }

// 16-lane and 64-lane all-reduces of u32 without LDS traffic (common.h has the float forms and says what the DPP controls do)
template <int CTRL>
__device__ __forceinline__ uint32_t tl_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
template <bool MAX>
__device__ __forceinline__ uint32_t tl_pick(uint32_t a, uint32_t b) { return MAX ? max(a, b) : min(a, b); }
template <bool MAX>
__device__ __forceinline__ uint32_t tl_row16(uint32_t v) {
    v = tl_pick<MAX>(v, tl_dpp<0xB1>(v));
    v = tl_pick<MAX>(v, tl_dpp<0x4E>(v));
    v = tl_pick<MAX>(v, tl_dpp<0x141>(v));
    v = tl_pick<MAX>(v, tl_dpp<0x140>(v));
    return v;
}
template <bool MAX>
__device__ __forceinline__ uint32_t tl_wave(uint32_t v) {
    v = tl_row16<MAX>(v);
    v = tl_pick<MAX>(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F));
    auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return tl_pick<MAX>((uint32_t)r[0], (uint32_t)r[1]);
}

__global__ __launch_bounds__(ROW_THREADS) void dec_top_logprobs_kernel(const TopArgs g) {
    __shared__ float lse_sh[4];
    __shared__ uint32_t red_k[2][ROW_WAVES], red_i[2][ROW_WAVES];
    __shared__ int win[TOP_LOGPROBS_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(g.row_of_slot, g.blk_snap, b);
    if (dead) return;
    int step = 0, max_len = 1;                                        // the tap: one step, [B][k]
    if (g.d_pos) {
        max_len = g.params[0];
        step = *g.d_pos - g.T0 + 1;
        if (step < 0 || step >= max_len) return;                      // workgroup-uniform
    }
    const int k = min(max(g.k, 1), TOP_LOGPROBS_MAX_K);

    // ---- 1. the row's log-sum-exp ------------------------------------------------------------------------------------------------
    const int n = (int)(g.ld >> 5);
    const float M = dec_lse_max(g.cand_val + (int64_t)b * n, n, lse_sh);
    const float lse = dec_lse_value(M, dec_lse_sum(g.cand_val + (int64_t)b * n, g.cand_sum + (int64_t)b * n, n, M, lse_sh));

    // ---- 2. the keys ---------------------------------------------------------------------------------------------------------------
    const float* __restrict__ lrow = g.logits + (int64_t)b * g.ld;
    uint32_t key[TL_SLOTS];
#pragma unroll
    for (int q = 0; q < ROW_NV4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(lrow)[q * ROW_THREADS + tid];
        key[4 * q + 0] = tl_key(v.x); key[4 * q + 1] = tl_key(v.y); key[4 * q + 2] = tl_key(v.z); key[4 * q + 3] = tl_key(v.w);
    }
    // the thread's two first elements among the slots `gone` does not mark: (k1, s1) before (k2, s2); a strict compare keeps the
    // lower slot among equal keys.  s2 = TL_SLOTS: there is no second.  (Key 0 is never taken: it stands for "none", and is the key
    // of one NaN pattern only; a row with a NaN reports NaN log-probs and its ids are only held inside the vocabulary.)
    uint32_t k1 = 0, k2 = 0;
    int s1 = 0, s2 = TL_SLOTS;
    unsigned long long gone = 0;
    auto first_two = [&](auto masked) {
        k1 = 0; k2 = 0; s1 = TL_SLOTS; s2 = TL_SLOTS;
#pragma unroll
        for (int s = 0; s < TL_SLOTS; ++s) {
            if (decltype(masked)::value && ((gone >> s) & 1ull)) continue;
            const uint32_t x = key[s];
            const bool c1 = x > k1, c2 = x > k2;
            k2 = c1 ? k1 : (c2 ? x : k2); s2 = c1 ? s1 : (c2 ? s : s2);
            k1 = c1 ? x : k1; s1 = c1 ? s : s1;
        }
        if (s1 == TL_SLOTS) s1 = 0;          // (a thread gives away at most k <= 20 of its 48: only if every other key is 0)
    };
    first_two(std::false_type());

    // ---- 3. k rounds ---------------------------------------------------------------------------------------------------------------
    for (int r = 0; r < k; ++r) {
        const uint32_t idx = (uint32_t)(((s1 >> 2) * ROW_THREADS + tid) * 4 + (s1 & 3));
        const uint32_t wk = tl_wave<true>(k1);
        const uint32_t wi = tl_wave<false>(k1 == wk ? idx : 0xFFFFFFFFu);
        if ((tid & 63) == 0) { red_k[r & 1][tid >> 6] = wk; red_i[r & 1][tid >> 6] = wi; }
        __syncthreads();                     // (round r + 1 writes the other buffers; round r + 2 comes after the next barrier)
        const uint32_t ok = red_k[r & 1][tid & 15], oi = red_i[r & 1][tid & 15];
        const uint32_t K = tl_row16<true>(ok);
        const uint32_t I = tl_row16<false>(ok == K ? oi : 0xFFFFFFFFu);
        if (tid == 0) win[r] = (int)min(I, (uint32_t)(SAMPLE_MAX_V - 1));
        if (k1 == K && idx == I) {           // the one thread that owned the winner
            gone |= 1ull << s1;
            if (s2 != TL_SLOTS) { k1 = k2; s1 = s2; s2 = TL_SLOTS; }
            else first_two(std::true_type());
        }
    }
    __syncthreads();

    // ---- 4. the record -------------------------------------------------------------------------------------------------------------
    if (tid < k) {
        const int id = win[tid];
        const int64_t o = ((int64_t)row * max_len + step) * k + tid;
        g.out_ids[o] = id;
        g.out_lp[o] = lrow[id] - lse;
    }
}

}  // namespace

void launch_dec_top_logprobs(const TopArgs& g, int B, hipStream_t s) {
    if (B <= 0 || g.ld != SAMPLE_MAX_V || g.k < 1 || g.k > TOP_LOGPROBS_MAX_K) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(dec_top_logprobs_kernel, dim3(B), dim3(ROW_THREADS), 0, s, g);
}

}  // namespace mellow
