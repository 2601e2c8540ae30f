// KV-cached decode step (replaces the reference's full re-forward per generated token, wrapper.py:216-249;
// SURVEY.md §8a A15/A16).  B = 32 rows per row-block, fp32 everywhere, bit-reproducible (no atomics).
//
// What the profiles of the first two designs showed (profiles/): a decode step moves only
// 1.2 GB, so it is bound by (a) ~4 us per *dependent* launch (inter-kernel data crosses the XCD L2s via the
// memory side), (b) the per-CU vector-memory rate (64 B/clk/CU: a workgroup that gathers an activation matrix
// row by row spends >10k cycles just issuing loads) and (c) serialised round trips (a load behind a branch
// or a runtime-count loop is a full wait).  Hence this design:
//
//   * 5 launches per layer, each spread over 72..288 workgroups:
//       qkv  (split-K slabs) -> attn (row-parallel, key-split) -> o_proj (complete output) ->
//       gate/up (complete output) -> down (split-K slabs, consumed by the next layer's qkv/attn)
//   * every GEMM operand is read with fully coalesced 1 KiB-per-wave loads: weights in P-layout /
//     P16-layout (kernels.h), activations written by their PRODUCER in MFMA fragment order ("F-layout"):
//       F32[rb][k/8][lane][4],  lane = (m%32) + 32*((k%8)/4)   (B operand of v_mfma_f32_32x32x2_f32)
//       F16[rb][k/16][half][lane][4], lane = (m%16) + 16*((k%16)/4), half = (m%32)/16  (…16x16x4_f32)
//   * all loads of a wave are issued up front in straight-line code (compile-time slab counts, clamped
//     addresses instead of branches, sched_barrier between the load block and the math);
//   * the RMSNorm weight is folded into the qkv / gate-up weights at load time and the per-row scale
//     r = rsqrt(mean(x^2)+eps) is applied by the consumer (attention: q,k,v are linear in r; down: inside
//     the SwiGLU), so no normalisation launch exists; split-K partial sums ("slabs") are summed by their
//     consumers in a fixed order.
//
// This header: what more than one of dec_attn.hip, dec_gemv.hip and dec_tail.hip needs.  Device helpers first,
// the host-side variant dispatcher of the launchers at the end.
#pragma once
#include "common.h"
#include "kernels.h"
#include <type_traits>
#include <utility>

namespace mellow {

// developer instrumentation: when a debug buffer is set, workgroup 0 / thread 0 stamps s_memtime at phase points
// (compiled in only with -DMELLOW_KDEBUG: the stamps cost ~9 % of a decode step)
// (no relocatable device code: every file that includes this header has a g_kdbg of its own and a one-line setter for it;
//  set_kernel_debug_buffer, engine_dev.cpp, calls them all)
__device__ uint64_t* g_kdbg = nullptr;
#ifdef MELLOW_KDEBUG
__device__ __forceinline__ void kstamp(int slot, int idx, bool who) {
    if (g_kdbg && who) g_kdbg[slot * 8 + idx] = __builtin_readcyclecounter();
}
// span of a whole launch: earliest start / latest end over ALL its workgroups on the constant 100 MHz clock (s_memrealtime,
// one counter for the device), at g_kdbg[64 + 2 * seq (+1)]; seq = DecArgs::dbg_seq, set per launch by the host
__device__ __forceinline__ void kspan(int seq, int end) {
    if (g_kdbg && seq >= 0 && seq < 480 && threadIdx.x == 0) {
        const unsigned long long t = wall_clock64();
        if (end) atomicMax(reinterpret_cast<unsigned long long*>(g_kdbg) + 64 + 2 * seq + 1, t);
        else atomicMin(reinterpret_cast<unsigned long long*>(g_kdbg) + 64 + 2 * seq, t);
    }
}
#else
#define kstamp(slot, idx, who) ((void)0)
#define kspan(seq, end) ((void)0)
#endif

#define MELLOW_BLK_EXIT(RB) if (BLK) { if (a.blk_live[RB] == 0) return; }   // BLK: compile-time (a run-time null test costs 0.26 us per launch)
// streamed-once operands (weights, KV pages): non-temporal loads (`global_load_dwordx4 ... nt`).  Each of these lines is read
// by exactly one workgroup per step, so keeping it in L2 buys nothing, and the nt policy shortens issue -> landed by ~18 %
// on this part (MI355X_MICROARCH.md, row nt-weights)
__device__ __forceinline__ float4 ldg_nt(const float4* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
}
// Decode weights in e4m3 (BASELINE config 5, `W8` variants of the GEMM kernels): the SAME slot order as the fp32 layouts
// (one float4 slot = one 4-byte word of four e4m3 values), one scale per packed weight row, applied to the reduced output.
// W8 == 1: the values are widened to fp32 in registers and multiplied on the fp32 matrix pipe, the activations stay fp32
// (MELLOW_FP8_DECODE_ACT=0: the form the weight pin of the parity suite runs).
// W8 == 2 ("A8"), the mode's default: the e4m3 words go to the fp8 matrix pipe as they are (v_mfma_f32_32x32x16_fp8_fp8 /
// 16x16x32) and the ACTIVATIONS are quantised to e4m3 in the consumer's registers, right after the fp32 fragments have landed:
// one scale per (batch row, k-slice of the wave) = amax / 448 of the values the wave holds for that row, applied to the wave's
// accumulators before the cross-wave reduction -- finer than a per-row scale and free of any cross-workgroup statistic.  No
// repacking: a lane's e4m3 word of k-tile t and of k-tile t+1 form the 8-byte A operand, and the activation fragments of the same
// two tiles (same lane -> same k positions) the B operand; the contraction only needs A and B to agree on which k a byte holds.
//
// WFrag: a lane's weight words of N k-tiles in the mode's form -- fp32 quads (W8 == 0; W8 == 1: widened by the load) or the
// e4m3 words (W8 == 2).  load() fetches ONE k-tile: every kernel interleaves it with the activation loads of the same tile in a
// load block of its own (the o_proj clamps the slot per tile), and the products below take the fragment whole.
template <int N, int W8>
struct WFrag {
    using word = std::conditional_t<W8 == 2, uint32_t, float4>;
    word t[N];
    static __device__ __forceinline__ word load(const float* __restrict__ Wp, int64_t slot) {
        if constexpr (W8 == 0) {
            return ldg_nt(reinterpret_cast<const float4*>(Wp) + slot);
        } else {
            const uint32_t u = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(Wp) + slot);
            if constexpr (W8 == 2) {
                return u;
            } else {
                const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(u, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(u, true);
                return make_float4(lo[0], lo[1], hi[0], hi[1]);
            }
        }
    }
};
__device__ __forceinline__ float f4amax(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
__device__ __forceinline__ uint32_t q4_e4m3(float4 v, float inv) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * inv, v.y * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * inv, v.w * inv, w, true);
    return (uint32_t)w;
}
__device__ __forceinline__ long pk64(uint32_t lo, uint32_t hi) { return (long)(((uint64_t)hi << 32) | (uint64_t)lo); }
// N k-tiles of a wave on the fp8 pipe, two tiles per instruction (an odd last tile is paired with zeros)
template <int N>
__device__ __forceinline__ f32x16 mfma8_32(f32x16 acc, const uint32_t (&w)[N], const uint32_t (&x)[N]) {
#pragma unroll
    for (int i = 0; i < N; i += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(pk64(w[i], i + 1 < N ? w[i + 1] : 0u), pk64(x[i], i + 1 < N ? x[i + 1] : 0u), acc, 0, 0, 0);
    return acc;
}
template <int N>
__device__ __forceinline__ f32x4 mfma8_16(f32x4 acc, const uint32_t (&w)[N], const uint32_t (&x)[N]) {
#pragma unroll
    for (int i = 0; i < N; i += 2)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pk64(w[i], i + 1 < N ? w[i + 1] : 0u), pk64(x[i], i + 1 < N ? x[i + 1] : 0u), acc, 0, 0, 0);
    return acc;
}
// (amax of a row's slice) -> (1 / scale, scale); an all-zero slice quantises to zeros
__device__ __forceinline__ void a8_scales(float amax, float& inv, float& sc) {
    inv = amax > 0.f ? 448.0f / amax : 0.f;
    sc = amax * (1.0f / 448.0f);
}
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float f4ssq(float4 v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ f32x16 mfma4(f32x16 acc, float4 w, float4 x) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, x.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, x.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, x.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, x.w, acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x4 mfma4s(f32x4 acc, float4 w, float4 x) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, x.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, x.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, x.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, x.w, acc, 0, 0, 0);
    return acc;
}
// One wave's slice of a 32-row weight tile against its 32 batch rows: acc += W[:, slice] x[slice].  W8 == 2 quantises the slice
// of each batch row (lanes m and m + 32 hold it) and scales the WHOLE accumulator: acc holds nothing but this slice (zeros on entry).
template <int N, int W8>
__device__ __forceinline__ f32x16 slice_mma32(f32x16 acc, const WFrag<N, W8>& w, const float4 (&x)[N]) {
    if constexpr (W8 == 2) {
        float am = 0.f, inv, sc;
#pragma unroll
        for (int i = 0; i < N; ++i) am = fmaxf(am, f4amax(x[i]));
        a8_scales(half_max(am), inv, sc);
        uint32_t xq[N];
#pragma unroll
        for (int i = 0; i < N; ++i) xq[i] = q4_e4m3(x[i], inv);
        acc = mfma8_32<N>(acc, w.t, xq);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= sc;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) acc = mfma4(acc, w.t[i], x[i]);
    }
    return acc;
}
// The same for a 16-row weight tile and 16 batch rows (v_mfma_f32_16x16x4_f32 / 16x16x32 fp8): a batch row's values of the
// slice sit in the four lanes m + 16 q, hence the swz_xor16 step of the amax.
template <int N, int W8>
__device__ __forceinline__ f32x4 slice_mma16(f32x4 acc, const WFrag<N, W8>& w, const float4 (&x)[N]) {
    if constexpr (W8 == 2) {
        float am = 0.f, inv, sc;
#pragma unroll
        for (int i = 0; i < N; ++i) am = fmaxf(am, f4amax(x[i]));
        am = fmaxf(am, swz_xor16(am));
        a8_scales(half_max(am), inv, sc);
        uint32_t xq[N];
#pragma unroll
        for (int i = 0; i < N; ++i) xq[i] = q4_e4m3(x[i], inv);
        acc = mfma8_16<N>(acc, w.t, xq);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= sc;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) acc = mfma4s(acc, w.t[i], x[i]);
    }
    return acc;
}
// Cross-wave reduction through LDS, red[wave][row of ROWS][lane].  A wave parks its accumulators (register r of lane l = row
// r0 + r) with reduce_store; after the barrier red_sum adds one (row, lane) over the waves -- wave 0's partial first, then
// waves 1, 2, ... in ascending order: the summation order of every build.
typedef __attribute__((address_space(3))) float lds_f32;      // the helpers take `red` as an LDS pointer: through a generic one the
#define MELLOW_LDS(p) ((lds_f32*)(p))                         // index arithmetic is canonicalised in 64 bits and the reads pair worse
template <typename V>
__device__ __forceinline__ void reduce_store(lds_f32* row0_lane, V acc) {
#pragma unroll
    for (int r = 0; r < (int)(sizeof(V) / sizeof(float)); ++r) row0_lane[r * 64] = acc[r];
}
template <int WAVES, int ROWS>
__device__ __forceinline__ float red_sum(const lds_f32* red, int r, int lane) {
    float s = red[r * 64 + lane];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) s += red[(wv * ROWS + r) * 64 + lane];
    return s;
}
// The 256-thread epilogue of a 32 x 32 tile: thread (mm = tid % 32, hh = tid / 32 % 2, gq = tid / 64 % 4) owns batch row mm and
// the four columns epi_col .. + 3 of the tile (accumulator registers 4 gq .. 4 gq + 3 of lane mm + 32 hh).
template <int WAVES>
__device__ __forceinline__ float4 reduce32(const lds_f32* red, int tid) {
    const int mm = tid & 31, hh = (tid >> 5) & 1, gq = (tid >> 6) & 3;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {            // (red_sum's index with the parent's association: (row * 64 + mm) + 32 hh pairs the reads as before)
        const int r = 4 * gq + j;
        float sacc = red[r * 64 + mm + 32 * hh];
#pragma unroll
        for (int wv = 1; wv < WAVES; ++wv) sacc += red[(wv * 16 + r) * 64 + mm + 32 * hh];
        v[j] = sacc;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ int epi_col(int nt, int tid) { return nt * 32 + 8 * ((tid >> 6) & 3) + 4 * ((tid >> 5) & 1); }
// e4m3 weights: the scales of the four packed rows sc[0 .. 3] on a thread's four reduced values
__device__ __forceinline__ float4 f4scale(float4 v, const float* __restrict__ sc) { return make_float4(v.x * sc[0], v.y * sc[1], v.z * sc[2], v.w * sc[3]); }

// ----------------------------------------------------------------------------------------------------
// f32x3 mode (the engine's default): the decode GEMMs on the bf16 matrix pipe at fp32 accuracy.  Every fp32 operand value is
// the EXACT sum of three bf16 pieces (split3, common.h: the same split as the prefill GEMMs of gemm_bf16x3.hip), formed here
// IN REGISTERS right after the fp32 fragments have landed -- the weights stay 4 bytes per value in HBM, the activations stay
// fp32 between launches -- and the six largest partial products run on v_mfma_f32_32x32x16_bf16 (32 cycles per SIMD for
// K = 16 against 8 x 64 cycles of v_mfma_f32_32x32x2_f32 for the same K), smallest first, fp32 accumulation.  No repacking:
// a lane's float4 of k-tile t and of k-tile t + 1 are the eight k positions of its bf16 operand; A (weights, P-layout) and
// B (activations, F32-layout) agree on which k a slot holds (lane half h of tile t: k = 8t + 4h + j), which is all the
// contraction needs (the e4m3 form above pairs its tiles the same way).
// Row blocks: one workgroup serves EVERY 32-row block of the batch with the weight fragments it split once (the fp32 kernels
// above replicate the grid per row block and re-stream the weights).
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void split_pair(float4 a, float4 b, i32x4& p0, i32x4& p1, i32x4& p2) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split8(v, p0, p1, p2);
}
#define MELLOW_BF16(W, X, ACC) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, W), __builtin_bit_cast(bf16x8, X), ACC, 0, 0, 0)
// six of the nine partial products, smallest first (pieces: 0 = leading, 2 = trailing; dropped: (1,2), (2,1), (2,2) < 2^-23 |w x|)
__device__ __forceinline__ f32x16 mma6(f32x16 acc, const i32x4 (&w)[3], const i32x4 (&x)[3]) {
    MELLOW_BF16(w[2], x[0], acc);
    MELLOW_BF16(w[0], x[2], acc);
    MELLOW_BF16(w[1], x[1], acc);
    MELLOW_BF16(w[1], x[0], acc);
    MELLOW_BF16(w[0], x[1], acc);
    MELLOW_BF16(w[0], x[0], acc);
    return acc;
}

// Pre-split activations ("F3" layouts): where ONE launch produces an activation that MANY workgroups of the next launch
// multiply, the producer also stores it as bf16 triples in the consumer's fragment order, so that the split is paid once per
// value instead of once per consuming workgroup (the lm_head has 1536 of them).  6 bytes per value instead of 4.
//   F3-32 (B operand of v_mfma_f32_32x32x16_bf16; pairs T = K / 16):
//       16-byte slot ((rb * K/16 + T) * 3 + piece) * 64 + lane,  lane = m % 32 + 32 h;  element e of the slot: k = 16 T + 8 h + e
//   F3-16 (B operand of v_mfma_f32_16x16x32_bf16; pairs T = K / 32, row halves mh):
//       slot (((rb * K/32 + T) * 2 + mh) * 3 + piece) * 64 + lane,  lane = m % 16 + 16 q;  k = 32 T + 8 q + e
// Eight CONSECUTIVE k per slot: a producer thread owns four consecutive k of one row, its neighbour (lane ^ 1) the other four
// of the same slot, so the even thread of a pair collects both halves (one DPP step) and stores whole 16-byte slots -- no
// workgroup ever writes half a slot (half-slot stores from two workgroups on different XCDs cost 0.9 us per launch).
// The weight side agrees on the k order: a 32-row weight tile pair (P-layout: lane half h of tile t holds k = 8 t + 4 h + j) is
// brought to k = 16 T + 8 h + e with one v_permlane32_swap per value (pair_natural); the 16-row gate/up tiles have their own
// packed copy in that order (P16N, launch_pack_weight16n).
struct F3Quad { uint2 p[3]; };      // four consecutive k of one row as bf16 triples: p[piece] = 4 bf16
__device__ __forceinline__ F3Quad f3_split4(float4 y) {
    __bf16 h[4], m[4], l[4];
    split3(y.x, h[0], m[0], l[0]); split3(y.y, h[1], m[1], l[1]); split3(y.z, h[2], m[2], l[2]); split3(y.w, h[3], m[3], l[3]);
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    F3Quad q;
    q.p[0] = __builtin_bit_cast(uint2, bf16x4{h[0], h[1], h[2], h[3]});
    q.p[1] = __builtin_bit_cast(uint2, bf16x4{m[0], m[1], m[2], m[3]});
    q.p[2] = __builtin_bit_cast(uint2, bf16x4{l[0], l[1], l[2], l[3]});
    return q;
}
__device__ __forceinline__ unsigned dpp_xor1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true); }
// The quad as it goes to memory, for a producer that stores it as fp32 AND as triples.  __fmul_rn is a plain product to the compiler,
// and under the default contraction mode split3's `a - float(h)` may be fused with the product that formed a into an fma on the
// UNROUNDED product: the triple is then the split of a value that can differ from the stored fp32 word by its last bit (seen in
// dec_gateup3_kernel on the z / w elements).  An empty asm operand is opaque to that fusion and costs no instruction.
__device__ __forceinline__ float4 as_stored(float4 v) {
    asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
}
// the neighbour's quad (lane ^ 1).  Both threads of a pair must be active.
__device__ __forceinline__ F3Quad f3_partner(const F3Quad& q) {
    F3Quad o;
#pragma unroll
    for (int c = 0; c < 3; ++c) { o.p[c].x = dpp_xor1(q.p[c].x); o.p[c].y = dpp_xor1(q.p[c].y); }
    return o;
}
// whole slot (columns k .. k + 7, k % 8 == 0): lo = the quad of k .. k + 3, hi = of k + 4 .. k + 7
__device__ __forceinline__ void f3_store8(void* base, int64_t slot0, const F3Quad& lo, const F3Quad& hi) {
    uint4* p = reinterpret_cast<uint4*>(base) + slot0;
    p[0] = make_uint4(lo.p[0].x, lo.p[0].y, hi.p[0].x, hi.p[0].y);
    p[64] = make_uint4(lo.p[1].x, lo.p[1].y, hi.p[1].x, hi.p[1].y);
    p[128] = make_uint4(lo.p[2].x, lo.p[2].y, hi.p[2].x, hi.p[2].y);
}
// slot of piece 0 for (row m of block rb, columns k .. k + 7, k % 8 == 0)
__device__ __forceinline__ int64_t f3_32_slot(int rb, int KP, int m, int k) {
    return ((int64_t)rb * KP + (k >> 4)) * 3 * 64 + m + 32 * ((k >> 3) & 1);
}
__device__ __forceinline__ int64_t f3_16_slot(int rb, int KP, int m, int k) {
    return (((int64_t)rb * KP + (k >> 5)) * 2 + (m >> 4)) * 3 * 64 + (m & 15) + 16 * ((k >> 3) & 3);
}
// weight fragments of a tile pair (a = tile 2T, b = tile 2T + 1, P-layout) -> the slot order above: lane half 0 gets tile 2T's
// eight k, lane half 1 tile 2T + 1's
__device__ __forceinline__ void pair_natural(float4& a, float4& b) {
    float* pa = &a.x; float* pb = &b.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(pa[j]), __float_as_uint(pb[j]), false, false);
        pa[j] = __uint_as_float(r[0]);
        pb[j] = __uint_as_float(r[1]);
    }
}

// ---- host side: the variant dispatcher of the launchers ----------------------------------------------------
// Every decode kernel is a template over a few switches that the host knows only at run time.  These helpers turn one such value
// into a compile-time constant (a std::integral_constant) and hand it to a generic lambda, so that a launcher names its kernel, its
// grid and its arguments once.  A launcher nests them for the LEGAL combinations only: a kernel exists for what is spelled here.
template <class F> static inline void with_bool(bool v, F&& f) {
    if (v) f(std::true_type{}); else f(std::false_type{});
}
// one value out of a fixed list; the last entry also serves every value that is not listed (the `else` of a ladder)
template <int V0, int... Vs, class F> static inline void with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
    else if (v == V0) f(std::integral_constant<int, V0>{});
    else with_int<Vs...>(v, f);
}
// weight mode of a launch: 0 fp32, 1 e4m3 weights widened to fp32, 2 e4m3 weights and activations on the fp8 matrix pipe (a.a8)
static inline int w8_mode(const DecArgs& a, const float* wscale) { return wscale ? (a.a8 ? 2 : 1) : 0; }
// f(BLK, W8): BLK = per-row-block early exit compiled in (a.blk_live != null); W8 = the weight mode (wscale != null: e4m3 weights)
template <class F> static inline void with_blk_w8(const DecArgs& a, const float* wscale, F&& f) {
    with_bool(a.blk_live != nullptr, [&](auto blk) { with_int<2, 1, 0>(w8_mode(a, wscale), [&](auto w8) { f(blk, w8); }); });
}

}  // namespace mellow
