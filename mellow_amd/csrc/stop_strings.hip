// Stop strings inside the decode step (include/mellow_hip.h, mellow_generate_stop_strings states the exact definition; DESIGN.md 6ze
// where the launch sits): one launch after the constraint launch and before the top log-probs and whichever kernel picks the token.
//
// One 1024-thread workgroup per batch slot, in the tiling of the rules and the constraint kernels:
//   1. the slot rule gives the row; a dead slot returns;
//   2. the row's state is a hit flag, a tail length and the last 63 bytes of its generated text.  The loop keeps it in a ping-pong
//      buffer indexed by EXAMPLE (a row that migrated to another slot still finds its own): step s reads half (s - 1) & 1 of the
//      parent row -- the row itself, or under beams the row the last selection made it continue -- appends the bytes of the ONE
//      token that selection gave the row and writes half s & 1; no row reads what a row of this launch writes.  The tap has no
//      buffer: it advances the empty text once per history token;
//   3. the match is parallel, not a walk: the tail, the token's bytes (two dependent loads: its offsets, then its bytes) and the
//      string table are in LDS, and the threads share the (start offset, string) pairs -- at most 319 x 16 -- each a direct
//      comparison of at most 64 bytes.  The verdict is one LDS word that a matching thread sets with a plain store of 1: the same
//      value whoever stores it, so it does not depend on arrival order;
//   4. a row that is not hit returns here without touching its logits or its partials.  A hit row becomes the one-hot row of the
//      stop id -- 0.0 there, -inf elsewhere -- and its per-32-column partials are formed anew from those values with the tile
//      helpers of the constraint kernel: the stop id's tile gets (0.0, stop id, sum 1.0), every other (-inf, its lowest index, 0).
// No float atomics and no arrival order anywhere: the bits depend on the inputs only.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

constexpr int STS_TEXT = (STS_TAIL + STS_MAX_TOKEN_BYTES + 3) / 4 * 4;      // bytes of LDS for tail | token bytes
constexpr int STS_STR_BYTES = STS_MAX_STRINGS * STS_MAX_STR_LEN;
static_assert(STS_STR_BYTES / 4 + STS_MAX_STRINGS + 1 <= ROW_THREADS && STS_MAX_TOKEN_BYTES <= ROW_THREADS, "one thread per staged word / byte");
static_assert(STS_OFF + STS_MAX_STRINGS + 1 <= STS_WORDS && STS_TAIL + 1 == 4 * (STS_ROW_WORDS - 2), "block and state layout");

// the strings of the call in LDS
struct StsTable {
    const uint8_t* bytes;        // [STS_STR_BYTES]
    const int32_t* off;          // [STS_MAX_STRINGS + 1]
    int n;
};

// One step of the definition, by the whole workgroup: text[0 .. len) is the row's tail; token t's bytes are appended and every stop
// string is looked for in the whole.  len and t are workgroup-uniform; every thread returns the same hit << 8 | new tail length,
// and the new tail is at text[0 ..).  `verdict` = one word of LDS, free again on return.
__device__ __forceinline__ int sts_advance(const StopStrArgs& g, const StsTable& tb, uint8_t* text, int len, int t, int32_t* verdict) {
    const int tid = threadIdx.x;
    int n = 0, o0 = 0;
    if ((unsigned)t < (unsigned)SAMPLE_MAX_V) {                       // (a column that holds no token appends nothing)
        o0 = g.tok_off[t];
        n = o0 < 0 ? 0 : min(max(g.tok_off[t + 1] - o0, 0), STS_MAX_TOKEN_BYTES);
    }
    if (tid == 0) *verdict = 0;
    if (tid < n) text[len + tid] = g.tok_bytes[(int64_t)o0 + tid];
    __syncthreads();
    const int L = len + n;
    for (int p = tid; p < L * tb.n; p += ROW_THREADS) {
        const int start = p / tb.n, j = p - start * tb.n;
        const int s0 = min(max(tb.off[j], 0), STS_STR_BYTES - STS_MAX_STR_LEN);
        const int m = min(max(tb.off[j + 1] - tb.off[j], 1), STS_MAX_STR_LEN);
        if (start + m > L) continue;
        bool eq = true;
        for (int i = 0; i < m && eq; ++i) eq = text[start + i] == tb.bytes[s0 + i];
        if (eq) *verdict = 1;                                         // (a plain store of 1: idempotent)
    }
    __syncthreads();
    const int hit = *verdict;
    const int nl = min(L, STS_TAIL);
    uint8_t c = 0;
    if (tid < nl) c = text[L - nl + tid];
    __syncthreads();
    if (tid < nl) text[tid] = c;
    __syncthreads();                                                  // (text and verdict are rewritten by the next step)
    return hit << 8 | nl;
}

__global__ __launch_bounds__(ROW_THREADS) void dec_stop_strings_kernel(const StopStrArgs g) {
    __shared__ uint32_t text_w[STS_TEXT / 4];
    __shared__ uint32_t str_w[STS_STR_BYTES / 4];
    __shared__ int32_t str_off[STS_MAX_STRINGS + 1];
    __shared__ int32_t verdict;
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(g.row_of_slot, g.blk_snap, b);
    if (dead) return;

    uint8_t* text = reinterpret_cast<uint8_t*>(text_w);
    const int stop_id = (int)g.blk[STS_STOP];
    const StsTable tb{reinterpret_cast<const uint8_t*>(str_w), str_off, min(max((int)g.blk[STS_COUNT], 0), STS_MAX_STRINGS)};
    if (tid < STS_STR_BYTES / 4) str_w[tid] = g.blk[STS_WORDS + tid];
    else if (tid < STS_STR_BYTES / 4 + STS_MAX_STRINGS + 1) str_off[tid - STS_STR_BYTES / 4] = (int32_t)g.blk[STS_OFF + tid - STS_STR_BYTES / 4];

    // ---- 2., 3. the state, advanced ---------------------------------------------------------------------------------------------
    int hit = 0, len = 0;
    if (g.hist_len) {                                                 // tap: the empty text advanced once per token of the caller's row
        const int s = min(max(g.hist_len[b], 0), g.hist_ld);
        const int32_t* __restrict__ h = g.hist + (int64_t)b * g.hist_ld;
        for (int i = 0; i < s && !hit; ++i) {                         // (sticky: nothing after a hit changes it)
            const int r = sts_advance(g, tb, text, len, h[i], &verdict);
            hit = r >> 8; len = r & 0xff;
        }
        if (tid == 0 && g.out_hit) g.out_hit[b] = hit;
    } else {
        const int max_len = g.params[0];
        const int s = min(max(*g.d_pos - g.T0 + 1, 0), max_len);
        if (tid < STS_ROW_WORDS - 2) text_w[tid] = 0u;
        if (s >= 1) {
            int pr = row, t;
            if (g.parent_tab) {      // row r continues beam parent_tab[s - 1][r] of its example, with the token the selection gave r
                pr = row / g.k * g.k + min(max(g.parent_tab[(int64_t)(s - 1) * g.N + row], 0), g.k - 1);
                t = g.token_tab[(int64_t)(s - 1) * g.N + row];
            } else {
                t = g.hist[(int64_t)row * max_len + s - 1];           // the token record: column s - 1 is written
            }
            const uint32_t* __restrict__ st = g.state + ((int64_t)((s - 1) & 1) * STS_STATE_ROWS + pr) * STS_ROW_WORDS;
            hit = st[0] != 0u;
            len = (int)min(st[1], (uint32_t)STS_TAIL);
            if (tid < STS_ROW_WORDS - 2) text_w[tid] = st[2 + tid];
            __syncthreads();                                          // (the token's bytes go behind the tail, into the same words)
            if (!hit) {
                const int r = sts_advance(g, tb, text, len, t, &verdict);
                hit = r >> 8; len = r & 0xff;
            }
        }
        uint32_t* __restrict__ dst = g.state + ((int64_t)(s & 1) * STS_STATE_ROWS + row) * STS_ROW_WORDS;
        if (tid < STS_ROW_WORDS - 2) dst[2 + tid] = text_w[tid];
        else if (tid == STS_ROW_WORDS - 2) dst[0] = (uint32_t)hit;
        else if (tid == STS_ROW_WORDS - 1) dst[1] = (uint32_t)len;
    }

    // ---- 4. a hit row becomes the one-hot row of the stop id ---------------------------------------------------------------------
    if (!hit || (unsigned)stop_id >= (unsigned)SAMPLE_MAX_V) return;  // the common case: the row stays as the earlier launches left it
    float* __restrict__ lrow = g.logits + (int64_t)b * g.ld;
    const int64_t cbase = (int64_t)b * ROW_TILES;
#pragma unroll 2
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + tid;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 4 * i4 + j == stop_id ? 0.f : -INFINITY;
        reinterpret_cast<float4*>(lrow)[i4] = make_float4(v[0], v[1], v[2], v[3]);
        const auto [bv, bx] = tile_best(v, i4);
        if (g.cand_sum) {
            // a tile whose maximum is -inf sums to exactly 0: no exp(-inf - -inf)
            float ps = 0.f;
            if (bv > -INFINITY) ps = tile_exp4(v, bv);
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

void launch_dec_stop_strings(const StopStrArgs& g, int B, hipStream_t s) {
    if (B <= 0 || g.ld != SAMPLE_MAX_V) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(dec_stop_strings_kernel, dim3(B), dim3(ROW_THREADS), 0, s, g);
}

}  // namespace mellow
