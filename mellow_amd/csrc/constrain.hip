// Constrained decoding inside the decode step (include/mellow_hip.h, mellow_generate_constraint states the exact definition; DESIGN.md 6zd
// where the launch sits): one launch after the rules launch and before the top log-probs and whichever kernel picks the token.
//
// One 1024-thread workgroup per batch slot, in the tiling of the rules kernel (48 values per thread, coalesced float4 loads):
//   1. the slot rule gives the row; a dead slot returns;
//   2. the row's state is ONE int, a node of the trie or DEAD / FREE / DONE.  The loop keeps it in a ping-pong buffer indexed by
//      EXAMPLE (a row that migrated to another slot still finds its own): step s reads half (s - 1) & 1 of the parent row -- the
//      row itself, or under beams the row the last selection made it continue -- advances it by the ONE token that selection gave
//      the row and writes half s & 1; no row reads what a row of this launch writes.  The tap has no buffer: it advances the root
//      once per history token.  A transition looks the token up among the node's edges with the threads strided over them; the
//      edges of a node are strictly ascending, so at most one thread matches and what lands in LDS does not depend on arrival order;
//   3. an LDS bitmap of one bit per token is marked with atomicOr over the node's edges (a node may have more edges than the
//      workgroup has threads), plus the stop bit: a bitmap is a set, so the result does not depend on which thread gets there first.
//      A row whose allowed set is everything (FREE) or empty returns before this without touching its logits or its partials;
//   4. every thread sets the values outside the set to -inf in its own 48 values, stores the float4 groups that changed, and the
//      per-32-column partials (cand_val / cand_idx in arg_better order, cand_sum = sum exp(l - cand_val), exactly 0 for a tile whose
//      maximum is -inf) are formed anew from the processed values, as in the rules kernel.
// No float atomics and no arrival order anywhere: the bits depend on the inputs only.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

// the arena sliced by the counts of the value block
struct Trie {
    const int32_t* __restrict__ first;
    const int32_t* __restrict__ flags;
    const int32_t* __restrict__ token;
    const int32_t* __restrict__ child;
    int n_nodes;
};

// One transition of the definition, by the whole workgroup: u and t are workgroup-uniform, every thread returns the same state.
// `match` = one word of LDS, free again on return.
__device__ __forceinline__ int con_advance(const Trie& tr, int u, int t, int stop_id, bool then_free, int32_t* match) {
    if (u < 0) return u;                                  // DEAD, FREE and DONE absorb
    const int tid = threadIdx.x;
    if (tid == 0) *match = -1;
    __syncthreads();
    const int e1 = tr.first[u + 1];
    for (int e = tr.first[u] + tid; e < e1; e += ROW_THREADS)
        if (tr.token[e] == t) *match = tr.child[e];       // (strictly ascending edges: at most one thread stores)
    __syncthreads();
    const int c = *match;
    __syncthreads();                                      // (match is rewritten by the next transition)
    if (c >= 0 && c < tr.n_nodes) return then_free && (tr.flags[c] & 1) ? CON_FREE : c;       // an edge wins over the stop rule
    if (t == stop_id && stop_id >= 0 && (tr.flags[u] & 1)) return CON_DONE;
    return CON_DEAD;
}

__global__ __launch_bounds__(ROW_THREADS) void dec_constrain_kernel(const ConstrainArgs g) {
    __shared__ uint32_t allow[ROW_TILES];
    __shared__ int32_t match;
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(g.row_of_slot, g.blk_snap, b);
    if (dead) return;

    const int stop_id = (int)g.prm[CON_STOP];
    const bool then_free = g.prm[CON_THEN_FREE] != 0;
    const int n_nodes = (int)g.prm[CON_NODES], n_edges = (int)g.prm[CON_EDGES];
    const Trie tr{g.trie, g.trie + n_nodes + 1, g.trie + 2 * n_nodes + 1, g.trie + 2 * n_nodes + 1 + n_edges, n_nodes};

    // ---- 2. the state ---------------------------------------------------------------------------------------------------------
    int u = g.row_root[row];
    if (g.hist_len) {                                                 // tap: the root advanced once per token of the caller's row
        const int s = min(max(g.hist_len[b], 0), g.hist_ld);
        const int32_t* __restrict__ h = g.hist + (int64_t)b * g.hist_ld;
        for (int i = 0; i < s; ++i) u = con_advance(tr, u, h[i], stop_id, then_free, &match);
        if (tid == 0 && g.out_state) g.out_state[b] = u;
    } else {
        const int max_len = g.params[0];
        const int s = min(max(*g.d_pos - g.T0 + 1, 0), max_len);
        if (s >= 1) {
            int pr = row, t;
            if (g.parent_tab) {      // row r continues beam parent_tab[s - 1][r] of its example, with the token the selection gave r
                pr = row / g.k * g.k + min(max(g.parent_tab[(int64_t)(s - 1) * g.N + row], 0), g.k - 1);
                t = g.token_tab[(int64_t)(s - 1) * g.N + row];
            } else {
                t = g.hist[(int64_t)row * max_len + s - 1];           // the token record: column s - 1 is written
            }
            u = g.state[((s - 1) & 1) * CON_STATE_ROWS + pr];
            if (u >= n_nodes) u = CON_DEAD;                           // (never: the state is a root or what an earlier launch wrote)
            u = con_advance(tr, u, t, stop_id, then_free, &match);
        }
        if (tid == 0) g.state[(s & 1) * CON_STATE_ROWS + row] = u;
    }

    // ---- 3. the allowed set ---------------------------------------------------------------------------------------------------
    if (u == CON_FREE) return;                                        // everything: the row stays as the head left it
    const int e0 = u >= 0 ? tr.first[u] : 0, e1 = u >= 0 ? tr.first[u + 1] : 0;
    const bool stop_ok = stop_id >= 0 && stop_id < SAMPLE_MAX_V && (u < 0 || (tr.flags[u] & 1));
    if (e1 <= e0 && !stop_ok) return;                                 // empty: it constrains nothing
    for (int i = tid; i < ROW_TILES; i += ROW_THREADS) allow[i] = 0u;
    __syncthreads();
    for (int e = e0 + tid; e < e1; e += ROW_THREADS) {
        const int t = tr.token[e];
        if ((unsigned)t < (unsigned)SAMPLE_MAX_V) atomicOr(&allow[t >> 5], 1u << (t & 31));
    }
    if (tid == 0 && stop_ok) atomicOr(&allow[stop_id >> 5], 1u << (stop_id & 31));
    __syncthreads();

    // ---- 4. apply, tile partials ----------------------------------------------------------------------------------------------
    float* __restrict__ lrow = g.logits + (int64_t)b * g.ld;
    const int64_t cbase = (int64_t)b * ROW_TILES;
#pragma unroll 2
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + tid;
        const float4 v4 = reinterpret_cast<const float4*>(lrow)[i4];
        const uint32_t ab = allow[i4 >> 3] >> ((i4 & 7) * 4);
        const float in[4] = {v4.x, v4.y, v4.z, v4.w};
        float v[4];
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (ab >> j) & 1u ? in[j] : -INFINITY;
            changed |= __float_as_uint(v[j]) != __float_as_uint(in[j]);
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

void launch_dec_constrain(const ConstrainArgs& g, int B, hipStream_t s) {
    if (B <= 0 || g.ld != SAMPLE_MAX_V) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(dec_constrain_kernel, dim3(B), dim3(ROW_THREADS), 0, s, g);
}

}  // namespace mellow
