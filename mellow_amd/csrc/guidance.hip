// Contrastive (classifier-free) guidance inside the decode step (include/mellow_hip.h, mellow_generate_guidance states the exact
// definition; DESIGN.md 6n where the launch sits): one launch between the lm_head and the rules launch / the kernel that picks the token.
//
// Rows 2p and 2p + 1 of the batch are the conditional and the negative row of pair p.  One 1024-thread workgroup per PAIR, in the
// sampler's / rules' row tiling (48 values per thread and row, coalesced float4 loads).  Both rows at once (2 x 48 floats per thread)
// do not fit the 128 VGPRs a lane of a 1024-thread workgroup has, so the rows are read twice:
//   pass 1, one row after the other: the row's 48 values per thread are held in registers, its maximum m and then its sum of
//           exp(l - m) are reduced over the workgroup: lse = m + log(sum);
//   pass 2 re-reads both rows (from L2: 2 x 196 KB per pair), forms g = b + s * (a - b) with a = l_c - lse_c, b = l_u - lse_u, stores g to
//           BOTH rows, and the eight neighbouring lanes that hold one 32-column tile form the tile's partials from g (cand_val /
//           cand_idx in arg_better order, cand_sum = sum exp(g - cand_val)), stored for both rows as well.
// Every reduction runs in one fixed order: a thread's own values ascending, then a butterfly over the wave, then the waves' results
// from LDS in wave order.  No float atomics and no arrival order anywhere: the bits depend on the inputs only, and the two rows of a
// pair leave the kernel bit-identical.  Logits are finite (they come from the head); +-inf inputs are outside the definition.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

// log-sum-exp of one row: m + log(sum exp(l - m)), m the row's maximum
__device__ __forceinline__ float gd_row_lse(const float* __restrict__ lrow, float* red) {
    const int tid = threadIdx.x;
    float4 v[ROW_NV4];
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) v[k] = reinterpret_cast<const float4*>(lrow)[k * ROW_THREADS + tid];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) m = fmaxf(fmaxf(fmaxf(fmaxf(m, v[k].x), v[k].y), v[k].z), v[k].w);
    m = block_reduce(m, [](float a, float b) { return fmaxf(a, b); }, red);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) {
        s += expf(v[k].x - m);
        s += expf(v[k].y - m);
        s += expf(v[k].z - m);
        s += expf(v[k].w - m);
    }
    s = block_reduce(s, [](float a, float b) { return a + b; }, red);
    return m + logf(s);
}

__global__ __launch_bounds__(ROW_THREADS) void dec_guidance_kernel(const GuideArgs g) {
    __shared__ float red[ROW_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    // (a guided call runs without row migration: no slot table, so not step_slot; a pair never straddles a row block)
    if (g.blk_snap && g.blk_snap[(2 * p) >> 5] == 0) return;         // workgroup-uniform; written by an EARLIER launch
    const float scale = __uint_as_float(g.prm[GDN_SCALE]);
    float* __restrict__ rc = g.logits + (int64_t)(2 * p) * g.ld;     // conditional row
    float* __restrict__ ru = rc + g.ld;                              // negative row

    // ---- pass 1 -----------------------------------------------------------------------------------------------------------------
    const float lse_c = gd_row_lse(rc, red);
    const float lse_u = gd_row_lse(ru, red);

    // ---- pass 2: combine, store to both rows, tile partials -----------------------------------------------------------------------
    const int64_t cb_c = (int64_t)(2 * p) * ROW_TILES, cb_u = cb_c + ROW_TILES;
#pragma unroll 2
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + tid;
        const float4 c4 = reinterpret_cast<const float4*>(rc)[i4];
        const float4 u4 = reinterpret_cast<const float4*>(ru)[i4];
        const float lc[4] = {c4.x, c4.y, c4.z, c4.w}, lu[4] = {u4.x, u4.y, u4.z, u4.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = __fsub_rn(lc[j], lse_c), b = __fsub_rn(lu[j], lse_u);
            v[j] = __fmaf_rn(scale, __fsub_rn(a, b), b);
        }
        const float4 o = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(rc)[i4] = o;
        reinterpret_cast<float4*>(ru)[i4] = o;
        const auto [bv, bx] = tile_best(v, i4);
        if (g.cand_sum) {
            const float ps = tile_sum8(tile_exp4(v, bv));            // (no -inf guard: g is finite)
            if ((tid & 7) == 0) {
                g.cand_sum[cb_c + (i4 >> 3)] = ps;
                g.cand_sum[cb_u + (i4 >> 3)] = ps;
            }
        }
        if ((tid & 7) == 0) {
            g.cand_val[cb_c + (i4 >> 3)] = bv;
            g.cand_val[cb_u + (i4 >> 3)] = bv;
            g.cand_idx[cb_c + (i4 >> 3)] = bx;
            g.cand_idx[cb_u + (i4 >> 3)] = bx;
        }
    }
}

}  // namespace

void launch_dec_guidance(const GuideArgs& g, int P, hipStream_t s) {
    if (P <= 0 || g.ld != SAMPLE_MAX_V) return;      // (the engine never asks for these)
    hipLaunchKernelGGL(dec_guidance_kernel, dim3(P), dim3(ROW_THREADS), 0, s, g);
}

}  // namespace mellow
