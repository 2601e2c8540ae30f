// Beam search inside the decode step (include/mellow_hip.h, mellow_generate_beam states the definition; DESIGN.md 6k the launches).
//
// SELECT, two launches (kernels.h, launch_beam_select):
//   1. beam_rows_kernel: one 1024-thread workgroup per row holds the row's 49152 logits in registers (48 per thread, coalesced
//      float4 loads, the tiling of sample.hip).  It forms lse = M + log S in one fixed order (per thread ascending, a butterfly over
//      the wave, the 16 waves ascending: no atomics) and then the row's k best candidates c = cum + (l - lse) by k rounds of a
//      workgroup arg-max over one u64 key per element (order key of c | inverted index): round j takes the largest key below round
//      j - 1's.  A finished row writes its single candidate and returns at once.
//   2. beam_merge_kernel: one wave per example ranks the <= k * k survivors by (c desc, parent asc, token asc) -- every lane counts
//      the lanes that beat it -- and the k winners do what dec_argmax_kernel does at the end of a step: tables, cum / fin, the
//      embedding row of the next step, the finished count, and the last arrival publishes the progress word.
// Two launches and no arrival counter per example: the merge needs all k rows of its example, and a counter would make the last
// of k 1024-thread workgroups carry the merge and the publish on its tail while the others idle; a second launch of B waves costs
// a few microseconds of the step's ~130 launches and keeps both kernels free of inter-workgroup ordering (the only cross-workgroup
// words are the integer arrival / finished counts the arg-max kernel already uses).  The bits depend on the inputs only.
//
// REORDER, two launches (launch_beam_reorder): rows whose parent is another row gather positions [T, pos] of the parent's K and V
// pages into a staging buffer, then scatter them into their own pages -- a parent may itself be overwritten in the same step, so
// the copy is never done in place.  Fixed grids, grid-stride loops; the position and the parent table are read from device words.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

static_assert(BEAM_MAX_K * BEAM_MAX_K <= 64, "one wave ranks an example's survivors");

// order key of a candidate value (c carries no -0: the callers add +0).  Unlike the sampler, which has left before it forms a key, the
// select meets NaN candidates (a NaN logit makes the row's lse NaN): every NaN maps to the one largest key (the arg-max rule: a NaN is
// the maximum, ties go to the lowest index)
__device__ __forceinline__ uint32_t ckey(float c) { return c != c ? 0xFFFFFFFFu : order_key(c); }

__global__ __launch_bounds__(ROW_THREADS) void beam_rows_kernel(const BeamArgs g, const int32_t* __restrict__ params) {
    __shared__ float red_f[ROW_WAVES];
    __shared__ unsigned long long red_u[ROW_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float cum = g.cum_in[r];
    float* cc = g.cand_c + (int64_t)r * BEAM_MAX_K;
    float* cl = g.cand_lp + (int64_t)r * BEAM_MAX_K;
    int32_t* ct = g.cand_tok + (int64_t)r * BEAM_MAX_K;
    if (g.fin_in[r] != 0) {              // workgroup-uniform: a finished row offers (r, stop id) with increment 0 and stays finished
        if (tid == 0) {
            g.cand_n[r] = 1;
            cc[0] = cum + 0.0f; ct[0] = params ? params[1] : g.stop_id; cl[0] = 0.f;
        }
        return;
    }
    const float* __restrict__ lrow = g.logits + (int64_t)r * g.ld;
    float l[ROW_NV4][4];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) {
        const float4 v = reinterpret_cast<const float4*>(lrow)[k * ROW_THREADS + tid];
        l[k][0] = v.x; l[k][1] = v.y; l[k][2] = v.z; l[k][3] = v.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, l[k][j]);
    }
    const float M = block_reduce(m, [](float a, float b) { return fmaxf(a, b); }, red_f);
    // S = sum exp(l - M): thread-local in ascending (k, j), a butterfly over the wave (both partners form the same sum), the waves
    // in ascending order.  A NaN logit makes S, and with it lse and every candidate of the row, NaN.
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += expf(l[k][j] - M);
    const float S = block_reduce(s, [](float a, float b) { return a + b; }, red_f);
    const float lse = (M - M == 0.f) ? M + (float)log((double)S) : __builtin_nanf("");
    // k rounds: the largest key strictly below the previous round's.  key = ckey(c) << 32 | (0x7fffffff - index): c descending,
    // then index ascending; all keys of a row are distinct and below ~0.
    unsigned long long prev = ~0ull;
    if (tid == 0) g.cand_n[r] = g.k;
#pragma unroll 1
    for (int jr = 0; jr < g.k; ++jr) {
        // (a thread meets its indices in ascending order: of equal values the first one met stays)
        const uint32_t pkey = (uint32_t)(prev >> 32), pinv = (uint32_t)prev;
        uint32_t bkey = 0u, binv = 0u;
#pragma unroll
        for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = ckey(cum + (opaque(l[k][j]) - lse) + 0.0f);
                const uint32_t inv = (uint32_t)(0x7fffffff - (4 * (k * ROW_THREADS + tid) + j));
                if ((key < pkey || (key == pkey && inv < pinv)) && (key > bkey || (key == bkey && inv > binv))) { bkey = key; binv = inv; }
            }
        unsigned long long best = ((unsigned long long)bkey << 32) | binv;
        best = block_reduce(best, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; }, red_u);
        if (tid == 0) {
            int idx = 0x7fffffff - (int)(uint32_t)(best & 0xffffffffull);
            idx = min(max(idx, 0), SAMPLE_MAX_V - 1);
            const float lp = lrow[idx] - lse;               // the arithmetic of the key above: the same bits
            cc[jr] = cum + lp + 0.0f; ct[jr] = idx; cl[jr] = lp;
        }
        prev = best;
    }
}

// LOOP: the step's bookkeeping for the k new beams of the example: its own tables at the step's row, cum / fin and the finished
// count, then the publish and the embedding gather of the step epilogue (step_tail.h).  The tap (LOOP = false) writes the four
// outputs [N] and nothing else.
template <bool LOOP>
__global__ __launch_bounds__(64) void beam_merge_kernel(const BeamArgs g, const DecArgs a, int32_t* __restrict__ tokens,
                                                        const float* __restrict__ embed, const LoopArgs lp) {
    __shared__ int sel_par[BEAM_MAX_K], sel_tok[BEAM_MAX_K];
    __shared__ float sel_c[BEAM_MAX_K], sel_lp[BEAM_MAX_K];
    const int b = blockIdx.x, lane = threadIdx.x, k = g.k;
    const int par = lane / k, slot = lane - par * k;           // (lanes >= k * k: par >= k, never valid)
    bool valid = false;
    float c = 0.f, inc = 0.f;
    int tok = 0;
    if (par < k) {
        const int row = b * k + par;
        valid = slot < g.cand_n[row];
        if (valid) {
            c = g.cand_c[(int64_t)row * BEAM_MAX_K + slot];
            tok = g.cand_tok[(int64_t)row * BEAM_MAX_K + slot];
            inc = g.cand_lp[(int64_t)row * BEAM_MAX_K + slot];
        }
    }
    const uint32_t key = ckey(c);
    // rank = survivors that come before this one in (c desc, parent asc, token asc); (parent, token) pairs are distinct
    int rank = 0;
    for (int t = 0; t < k * k; ++t) {
        const uint32_t ok = __shfl(key, t, 64);
        const int ot = __shfl(tok, t, 64), ov = __shfl((int)valid, t, 64), op = t / k;
        const bool before = ok > key || (ok == key && (op < par || (op == par && ot < tok)));
        rank += (ov && before) ? 1 : 0;
    }
    if (valid && rank < k) { sel_par[rank] = par; sel_tok[rank] = tok; sel_c[rank] = c; sel_lp[rank] = inc; }
    __syncthreads();
    if constexpr (!LOOP) {
        if (lane < k) {
            const int row = b * k + lane;
            g.out_parent[row] = sel_par[lane]; g.out_token[row] = sel_tok[lane]; g.out_cum[row] = sel_c[lane]; g.out_lp[row] = sel_lp[lane];
        }
        return;
    } else {
        const int max_len = lp.params[0], stop_id = lp.params[1];
        const int step = *a.d_pos - lp.T0 + 1;
        int fin = 0;
        if (lane < k) {
            const int row = b * k + lane;
            fin = sel_tok[lane] == stop_id ? 1 : 0;
            g.cum_state[row] = sel_c[lane];
            g.fin_state[row] = fin;
            tokens[row] = min(max(sel_tok[lane], 0), SAMPLE_MAX_V - 1);
            if (step >= 0 && step < max_len) {
                const int64_t o = (int64_t)step * g.N + row;
                g.out_parent[o] = sel_par[lane]; g.out_token[o] = sel_tok[lane]; g.out_lp[o] = sel_lp[lane]; g.out_cum[o] = sel_c[lane];
            }
        }
        const int nfin = __popcll(__ballot(fin));
        if (lane == 0) {
            // the finished count of a step is formed anew (it can fall): every example adds its own, the last arrival takes the
            // total and leaves the word at 0 for the next step
            if (nfin) atomicAdd(lp.n_seen, nfin);
            step_publish(lp, [n_seen = lp.n_seen] { return atomicExch(n_seen, 0); });
        }
        // embed[token] of every new beam: the next step's residual row
        for (int j = 0; j < k; ++j) {
            const int row = b * k + j, t = min(max(sel_tok[j], 0), SAMPLE_MAX_V - 1);
            for (int i = lane; i < 144; i += 64) step_embed_gather(embed, t, a, row, i);
        }
    }
}

// Reorder, first half: row r whose parent row pr = (r / k) * k + parent[step][r] is another row copies positions [T0, pos] of pr's K
// and V pages [layer][Bp][3][Tmax][64] to its slice of the staging buffers [layer][N][3][max_len][64].  GATHER = false is the second
// half: the same elements from the staging slice into r's own pages.  A thread owns one float4 of K and of V; 64-bit indices (one
// layer of pages at 1024 rows is past 2^31 bytes).  Rows that keep their own page move nothing.
template <bool GATHER>
__global__ __launch_bounds__(256) void beam_kv_move_kernel(float4* __restrict__ kpages, float4* __restrict__ vpages, float4* __restrict__ kst,
                                                           float4* __restrict__ vst, const int32_t* __restrict__ parent_tab,
                                                           const int32_t* __restrict__ d_pos, const int32_t* __restrict__ params, int T0,
                                                           int layers, int N, int k, int Bp, int Tmax) {
    const int max_len = params[0], step = *d_pos - T0 + 1;        // positions T0 .. T0 + step - 1 were appended by steps 1 .. step
    if (step <= 0 || step >= max_len || T0 + step > Tmax) return;
    const int64_t c16 = (int64_t)step * 16, ML16 = (int64_t)max_len * 16, Tmax16 = (int64_t)Tmax * 16;
    const int64_t total = (int64_t)layers * N * 3 * c16;
    const int32_t* __restrict__ par = parent_tab + (int64_t)step * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pg = i / c16, q = i - pg * c16;          // staging page (l * N + r) * 3 + h, float4 inside its first `step` positions
        const int64_t lr = pg / 3, h = pg - lr * 3, l = lr / N;
        const int r = (int)(lr - l * N);
        const int pr = r / k * k + min(max(par[r], 0), k - 1);
        if (pr == r) continue;
        const int64_t st = pg * ML16 + q;
        if constexpr (GATHER) {
            const int64_t src = ((l * Bp + pr) * 3 + h) * Tmax16 + (int64_t)T0 * 16 + q;
            kst[st] = kpages[src];
            vst[st] = vpages[src];
        } else {
            const int64_t dst = ((l * Bp + r) * 3 + h) * Tmax16 + (int64_t)T0 * 16 + q;
            kpages[dst] = kst[st];
            vpages[dst] = vst[st];
        }
    }
}

}  // namespace

void launch_beam_select(const BeamArgs& g, int B, const DecArgs& a, int32_t* tokens, const float* embed, const LoopArgs* loop, hipStream_t s) {
    if (B <= 0 || g.k < 1 || g.k > BEAM_MAX_K || g.ld != SAMPLE_MAX_V) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(beam_rows_kernel, dim3(B * g.k), dim3(ROW_THREADS), 0, s, g, loop ? loop->params : nullptr);
    if (loop) hipLaunchKernelGGL(beam_merge_kernel<true>, dim3(B), dim3(64), 0, s, g, a, tokens, embed, *loop);
    else hipLaunchKernelGGL(beam_merge_kernel<false>, dim3(B), dim3(64), 0, s, g, a, tokens, embed, LoopArgs());
}

void launch_beam_reorder(float* k_pages, float* v_pages, float* k_stage, float* v_stage, const int32_t* parent_tab, const int32_t* d_pos,
                         const int32_t* params, int T0, int layers, int N, int k, int Bp, int Tmax, hipStream_t s) {
    if (layers <= 0 || N <= 0 || k < 2 || N % k != 0 || N > Bp) return;             // (k = 1: every row is its own parent)
    constexpr int blocks = 1024;      // fixed: the element count of a step is a device word
    hipLaunchKernelGGL(beam_kv_move_kernel<true>, dim3(blocks), dim3(256), 0, s, reinterpret_cast<float4*>(k_pages), reinterpret_cast<float4*>(v_pages),
                       reinterpret_cast<float4*>(k_stage), reinterpret_cast<float4*>(v_stage), parent_tab, d_pos, params, T0, layers, N, k, Bp, Tmax);
    hipLaunchKernelGGL(beam_kv_move_kernel<false>, dim3(blocks), dim3(256), 0, s, reinterpret_cast<float4*>(k_pages), reinterpret_cast<float4*>(v_pages),
                       reinterpret_cast<float4*>(k_stage), reinterpret_cast<float4*>(v_stage), parent_tab, d_pos, params, T0, layers, N, k, Bp, Tmax);
}

}  // namespace mellow
