// The tail of a decode step, device side: what the kernels after the lm_head launch share (sample.hip, beam.hip, logit_rules.hip,
// guidance.hip, top_logprobs.hip and the arg-max of dec_tail.hip).  Everything here is inlined into its caller; the
// helpers return values and take closures that capture by value, because a result written through a reference, or a local whose
// address a closure holds, changed the instructions of the callers (DESIGN.md 6s has the per-kernel comparison).
//   - the row tiling of the 1024-thread row kernels;
//   - block_reduce, opaque, order_key;
//   - the per-tile partials (cand_val / cand_idx / cand_sum) of processed values;
//   - the slot rule;
//   - the step epilogue: step_record, step_publish, step_embed_gather.
#pragma once
#include "common.h"
#include "kernels.h"
#include <type_traits>

namespace mellow {

// ---- row tiling: one 1024-thread workgroup holds a row of SAMPLE_MAX_V values, 48 per thread as 12 coalesced float4 groups (group k of
// thread t is float4 k * 1024 + t of the row); a 32-column tile of the lm_head is the float4 groups of eight neighbouring lanes -------
constexpr int ROW_THREADS = 1024, ROW_WAVES = ROW_THREADS / 64;
constexpr int ROW_NV4 = SAMPLE_MAX_V / 4 / ROW_THREADS;     // float4 groups per thread (12)
constexpr int ROW_TILES = SAMPLE_MAX_V / 32;                // 32-column tiles of a row = words of a one-bit-per-token map (1536)
static_assert(ROW_NV4 * 4 * ROW_THREADS == SAMPLE_MAX_V, "row tiling");
static_assert(ROW_THREADS % 8 == 0 && ROW_TILES == ROW_NV4 * (ROW_THREADS / 8), "a tile is the float4 groups of eight neighbouring lanes");

// butterfly over the wave (both partners form the same value), then the waves' values from LDS in wave order: every thread of a
// ROW_THREADS workgroup returns the same bits.  `red` = ROW_WAVES values of LDS, free again on return.
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    T r = red[0];
    for (int w = 1; w < ROW_WAVES; ++w) r = op(r, red[w]);
    __syncthreads();            // (red is rewritten by the next reduction)
    return r;
}

// a copy of a register value the compiler cannot see through: keeps per-element arithmetic (keys, masses, indices) inside the loop
// that needs it.  Hoisted out, the 48 results of a thread's row slice would be live next to its 48 values: a lane of a 1024-thread
// workgroup has 128 VGPRs, the rest spills.
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
// the same for a thread index: an element's index is formed again where it is needed (seen through, the 48 index keys of a thread's
// slice are hoisted out of the sampler's index select and spilled; its filtered instantiation uses this and runs without them)
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}

// order-preserving key: a > b (as floats, no NaN) <=> order_key(a) > order_key(b); equal keys <=> equal bits, so a caller whose
// values can carry -0 adds +0.0f first
__device__ __forceinline__ uint32_t order_key(float z) {
    const uint32_t u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- the per-tile partials the greedy arg-max and every LSE merge read instead of the logits, formed anew by a kernel that edits
// a row: the same order as the head's own, so the same bits -------------------------------------------------------------------------
// v = the four processed values of float4 group i4.  The tile's best (value, lowest index) in arg_better order: own four in
// ascending index, then the eight lanes of the tile.
struct TileBest {
    float v;
    int idx;
};
__device__ __forceinline__ TileBest tile_best(const float (&v)[4], int i4) {
    float bv = v[0];
    int bx = 4 * i4;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (arg_better(v[j], 4 * i4 + j, bv, bx)) { bv = v[j]; bx = 4 * i4 + j; }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int ox = __shfl_xor(bx, off, 64);
        if (arg_better(ov, ox, bv, bx)) { bv = ov; bx = ox; }
    }
    return {bv, bx};
}
// sum exp(v - bv) of the tile in two halves, so that a caller can guard the first: a thread's four in ascending order ...
__device__ __forceinline__ float tile_exp4(const float (&v)[4], float bv) {
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ps += expf(v[j] - bv);
    return ps;
}
// ... then a butterfly over the eight lanes (both partners form the same sum)
__device__ __forceinline__ float tile_sum8(float ps) {
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) ps += __shfl_xor(ps, off, 64);
    return ps;
}

// ---- the slot rule: batch slot b holds example `row`; a slot whose whole 32-row block has stopped, or that is empty after a repack,
// computes nothing any more.  Workgroup-uniform; both tables were written by an EARLIER launch ---------------------------------------
struct StepSlot {
    int row;
    bool dead;
};
__device__ __forceinline__ StepSlot step_slot(const int32_t* row_of_slot, const int32_t* blk_snap, int b) {
    const int row = row_of_slot ? row_of_slot[b] : b;
    return {row, (blk_snap && blk_snap[b >> 5] == 0) || row < 0};
}

// ---- the step epilogue (reference wrapper.py:232-249): what one thread of the kernel that picked slot b's token does with it ----------
// record: the token (and, where the caller has one, its log-prob: `logprob()` is only evaluated for a column inside the record) at
// the step's column of example `row`; a row's first stop id is counted, and the row that brings its block's count to 0 clears the
// block's live word -- from the NEXT step on (this step's kernels read blk_snap).
struct NoLogprob {};
template <typename LpF = NoLogprob>
__device__ __forceinline__ void step_record(const LoopArgs& lp, const DecArgs& a, int b, int row, int idx, LpF logprob = {}) {
    const int max_len = lp.params[0], stop_id = lp.params[1];
    const int step = *a.d_pos - lp.T0 + 1;
    if (step >= 0 && step < max_len) lp.out_tokens[(int64_t)row * max_len + step] = idx;
    if constexpr (!std::is_same<LpF, NoLogprob>::value) {
        if (step >= 0 && step < max_len) lp.out_logprob[(int64_t)row * max_len + step] = logprob();
    }
    if (idx == stop_id && lp.seen_stop[row] == 0) {
        lp.seen_stop[row] = 1;
        atomicAdd(lp.n_seen, 1);
        if (lp.blk_left && atomicSub(lp.blk_left + (b >> 5), 1) == 1) lp.blk_live[b >> 5] = 0;
    }
}
// publish: every workgroup of the launch calls it once (one thread, dead slots included); the last to arrive publishes the step to
// the host: ticket = picker launches so far, low word = `count()`, the rows that have stopped (evaluated by that last arrival only).
// Ordering: the caller's n_seen / blk_left atomics must have been performed before its arrival is counted -- a drained vmcnt is
// enough for device-scope atomics (no cache write-back: a __threadfence() here cost ~3 us per step).  The last arrival resets
// `arrive` for the next step's launch, which stream order puts after this one.  The host reads only the progress word itself
// before the stream is synchronised, so its store needs no release.
template <typename CountF>
__device__ __forceinline__ void step_publish(const LoopArgs& lp, CountF count) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (atomicAdd(lp.arrive, 1) == (int)gridDim.x - 1) {
        *lp.arrive = 0;
        const int t = *lp.ticket + 1;
        *lp.ticket = t;
        const int ns = count();
        __hip_atomic_store(lp.host_progress, ((unsigned long long)(unsigned)t << 32) | (unsigned)ns, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// embed gather: float4 i (of 144) of a 576-wide row into the F32-layout residual row of a slot: the next step's input
__device__ __forceinline__ void step_store_x(float* xmidF, int slot, int i, float4 e) {
    reinterpret_cast<float4*>(xmidF)[f32_idx(slot >> 5, 72, slot & 31, i * 4)] = e;
}
__device__ __forceinline__ void step_embed_gather(const float* __restrict__ embed, int token, const DecArgs& a, int slot, int i) {
    step_store_x(a.xmidF, slot, i, reinterpret_cast<const float4*>(embed + (int64_t)token * 576)[i]);
}

}  // namespace mellow
