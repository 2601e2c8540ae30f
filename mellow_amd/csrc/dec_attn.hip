// Decode step: the attention (flash decoding over the K/V pages) and the o_proj that merges its key splits, plus the K/V page
// utilities (bf16 shadow, fan-out).  The design comment of the decode step, the shared device helpers and the launchers' variant
// dispatcher: dec_common.h.
#include "dec_common.h"

namespace mellow {

void set_dec_attn_debug_buffer(uint64_t* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_kdbg), &p, sizeof(p)); }

// ----------------------------------------------------------------------------------------------------
// K2  attention (flash decoding).  grid (3 kv heads, rows, key splits: DEC_TS at one row block, 1 from two on), 8 waves.
//     r1 = RMS scale of x_new from the qkv kernel's per-chunk sums;  q,k,v = r1 * sum_kc pq slabs;  RoPE; KV append;
//     per-wave online softmax over an interleaved set of 4-key groups; partial (m, l, o) per split.
//     Split sp owns key groups [sp*gs, (sp+1)*gs) (the last split: everything from sp*gs on, plus the new key).
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_DA_MINW
#define MELLOW_DA_MINW 4      // waves per SIMD the register allocation must allow: 4 = two 8-wave workgroups per CU (128 VGPRs), so that
#endif                        // the 384 workgroups of a 64-row batch are resident together instead of in two rounds
constexpr int DA_WAVES = 8;         // (4 and 16 waves: another summation order, no faster -- profiles/r06_decode_attn_ablation.txt)
constexpr int DA_G = 7;             // 4-key groups in flight per wave: one chunk covers 2 * DA_WAVES * DA_G * 4 = 448 keys
static_assert(DA_WAVES == 8, "the merge of the waves' partials reduces over 8-lane groups");
#ifndef MELLOW_DA_G1
#define MELLOW_DA_G1 5      // 5 of 7: 48.55 ms of decode per 63 steps; 2 / 3 / 4 / 7 (= everything up front): 49.35 / 49.15 / 49.0 / 49.75 (same box)
#endif
constexpr int DA_G1 = MELLOW_DA_G1 < DA_G ? MELLOW_DA_G1 : DA_G;    // key groups requested before the prologue
// bf16 pages (KV16, the fp8 mode): the SCORES on the matrix pipe.  Ablations of the vector form at B = 128 (same box, decode per 63
// steps): 75.5 ms; without the K/V loads 67.1; without the score / softmax / PV loop 60.3 (per 28 keys of a wave ~500 vector
// instructions: 84 of them the 16-lane DPP sums of 21 dot products, ~80 hazard s_nops, 63
// redundant exps).  Here a wave's chunk is ONE 32-key tile (~200 vector instructions): lane (key kk = lane % 32, half hf = lane / 32)
// loads the 64 contiguous bytes of its key's dims 32 hf .. 32 hf + 31 (four 16-byte loads = the B operands of four
// v_mfma_f32_32x32x16_bf16, k order: step s <-> dims 32 hf + 8 s ..), the A operand holds q as EXACT bf16 triples in rows
// 4 piece + head (rows are free: 32 of them, 9 used), so S = q . k is the fp32 dot product of the fp32 q with the bf16 key up to
// summation order, one value per (key lane, head) -- no cross-lane sums, 3 exps per key.  The weights go through 4 KiB of LDS
// (wave-private, in-order: no barrier) to the lanes of the unchanged P V accumulation (lane = key sub x dim quad).
// Same box, fp8 mode, decode per 63 steps: B = 128 75.9 -> 72.4 ms, B = 32 43.9 -> 41.7; with the loads compiled out the two forms
// cost the same (66.5 / 67.1): the loop is a dependent chain (scores -> max -> exp -> weights -> P V) more than an issue stream, and
// what the matrix form wins is the chain's length and the registers (116 instead of 218 at one row block).
constexpr int DA_GM = 8;            // key groups per wave and chunk of the matrix form: 32 keys = one MFMA tile
// Measured and dropped (profiles/r06_decode_attn_ablation.txt; the switch of the first is gone):
//   * the K tile loads non-temporal: a lane's four 16-byte pieces share a 64-byte segment that four instructions touch, and a
//     non-temporal line does not stay for the next one (same box, fp8 B = 128: 78.9 ms with nt, 72.5 without);
//   * the tile as 32 consecutive keys loaded in 1 KiB runs and turned into the operand order through a swizzled LDS image (72.8
//     against 72.5 ms: the LDS round trip costs what the coalescing gains).
// Physical waves (template parameter NW): the eight chunk streams of a workgroup ("virtual waves": own weights region, own
// partial in the merge) can run on 8 waves or, two after the other, on 4 -- the same arithmetic in the same order, so the
// results are bit-identical and four 256-thread workgroups share a CU (the 768 workgroups of B = 128 resident together instead
// of in 1.5 rounds).  Measured +-0 (fp8 B = 128, same box: 72.4 ms on 8 waves, 72.4-73.5 on 4): MELLOW_DA16_NW stays 8.
// (The parameter outlived DESIGN.md 6v: without the loop over virtual waves the compiler lays the publish tail of the matrix form
// out otherwise, 4 .. 5 instructions more; with it the kernel is the instruction stream the figures above were measured on.)
#ifndef MELLOW_DA16_MINW
#define MELLOW_DA16_MINW MELLOW_DA_MINW
#endif
#ifndef MELLOW_DA16_NW
#define MELLOW_DA16_NW 8            // physical waves of the matrix form from two row blocks on (4 = two virtual waves per wave)
#endif

// KV16 (fp8 mode): the decode step reads and extends a bf16 SHADOW of the K/V pages (engine_lm.cpp: converted from the fp32
// pages the prefill wrote, once per call): half the bytes of the step's largest stream.  The new key / value of the step itself
// are used in fp32 (from LDS) and appended rounded to nearest even.  Its loads are load_ktile / load_vgroup of the kernel; the
// fp32 pages of the vector form go through ld_kv.
__device__ __forceinline__ float4 ld_kv(const float* page, int64_t elem) { return ldg_nt(reinterpret_cast<const float4*>(page + elem)); }
template <bool KV16>
__device__ __forceinline__ void st_kv(float* page, int64_t elem, float v) {
    if constexpr (KV16) reinterpret_cast<__bf16*>(page)[elem] = static_cast<__bf16>(v);
    else page[elem] = v;
}
// FUSED: the producer was dec_qkv2_kernel (the previous layer's down projection and this layer's q/k/v in one launch): the
// projected values arrive as Q2_NPQ slabs, and x_new = x_mid + sum of the Q2_HC down slabs is formed HERE (the 144 float4 of the
// row, by every workgroup of the row: its sum of squares is the RMS statistic; the (kv head 0, split 0) workgroup also writes the
// row for the o_proj's residual).  !FUSED: the producer was dec_qkv_kernel (first layer of a step: 8 slabs + its own statistic).
// ONE: the launch has a single 32-row block (192 workgroups: one per CU, registers are free) -> the chunk loop in its plain form
//      (221 VGPRs, 0.7 ms of decode per 63 steps faster at B = 32); otherwise the first chunk is peeled by hand so that the kernel
//      fits 128 VGPRs and two workgroups share a CU (B = 64: 384 workgroups resident together, 73.7 -> 71.2 ms)
template <bool BLK, bool FUSED, bool ONE, bool KV16, int NW, int TS>
__global__ __launch_bounds__(NW * 64, ONE ? 2 : (KV16 ? MELLOW_DA16_MINW : MELLOW_DA_MINW)) void dec_attn_kernel(float* __restrict__ k_cache, float* __restrict__ v_cache,
                                                                  const int32_t* __restrict__ d_pos_p, const float* __restrict__ pq_p,
                                                                  const float* __restrict__ xmidF_p, int Tmax_p, int gs_p, int rows_p,
                                                                  const DecArgs a) {
    kspan(a.dbg_seq, 0);
    // (the leading scalar arguments repeat fields of `a`: the first 14 dwords of the argument block are preloaded into SGPRs
    //  by the command processor -- build.py, -amdgpu-kernarg-preload-count -- so the K/V and slab addresses do not wait for a
    //  scalar load from the argument buffer at the start of every launch)
    __shared__ float ssq_part[3];
    __shared__ __attribute__((aligned(16))) float qs[3 * 64];            // RoPE'd, pre-scaled q
    __shared__ __attribute__((aligned(16))) float knew[64], vnew[64];
    __shared__ __attribute__((aligned(16))) float xs[320];               // q (3 x 64) | k | v before RoPE, RMS-scaled
    __shared__ __attribute__((aligned(16))) float ored[DA_WAVES * 3 * 64];
    __shared__ float mred[DA_WAVES * 3], lred[DA_WAVES * 3];
    __shared__ float snew_s[3];
    constexpr bool MF = KV16;                                            // bf16 pages: scores on the matrix pipe (comment at DA_GM)
    __shared__ __attribute__((aligned(16))) float pl[MF ? DA_WAVES * 32 * 4 : 4];     // softmax weights [wave][key of the tile][head | pad]
    __shared__ __attribute__((aligned(16))) __bf16 qb[MF ? 10 * 64 : 8];               // q as bf16 triples [piece][head][dim] + a zero row
    constexpr int VPW = DA_WAVES / NW;                                   // virtual waves per physical wave (matrix form only)
    static_assert(DA_WAVES % NW == 0 && (MF || NW == DA_WAVES), "the vector form runs one chunk stream per wave");
    // key group of slot u in the chunk that starts at group g0: the interleaved groups of the vector form
    auto mf_group = [&](int g0, int u) { return g0 + u * DA_WAVES; };

    static_assert(TS == DEC_TS || !(ONE || KV16), "one row block and the bf16 pages always run DEC_TS key splits (kernels.h dec_key_splits)");
    const int g = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
    int row = b;                  // the example whose KV pages this slot reads and extends (slot == example unless rows migrate)
    if (BLK) {
        const int live = a.blk_live[b >> 5];
        if (a.row_of_slot) row = a.row_of_slot[b];
        if (live == 0 || row < 0) return;       // the block has stopped / the slot is empty (workgroup-uniform)
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Tmax = Tmax_p;
    // (KV16: the same element offsets into pages of 2-byte elements: half the float offset)
    float* kpage = k_cache + (((int64_t)row * 3 + g) * Tmax * 64 >> (KV16 ? 1 : 0));
    float* vpage = v_cache + (((int64_t)row * 3 + g) * Tmax * 64 >> (KV16 ? 1 : 0));
    const int sub = lane >> 4, quad = lane & 15;   // lane -> (key sub, dim quad): a wave instruction = 4 keys x 64 dims

    // ===== ONE round trip, every load independent and straight-line: position word, RMS partials, qkv slabs,
    //       the staged RoPE row and the first chunk of K/V (key ranges of the splits are fixed per launch, a.gs,
    //       so their addresses do not wait for the position; keys >= pos are masked after the loads land) =====
    const bool dbg = tid == 0 && g == 0 && b == 0 && sp == 0;
    kstamp(1, 0, dbg);
#ifdef MELLOW_POS_VECTOR_LOAD
    const int pos = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const volatile int*>(d_pos_p));
#else
    const int pos = *d_pos_p;        // keys 0..pos-1 are cached; the new key is key `pos`
#endif
    // prologue: the 320 projected values of this (row, kv head) -- q of 3 heads | k | v -- are the sums of the qkv kernel's
    // split-K slabs.  80 threads own one float4 of columns each (8 slab loads of 16 B; before: 512 threads x 16 dword loads),
    // scale by the RMS statistic and park the result in LDS; 192 threads then apply RoPE / append the new key and value.
    //   r <48: query head 3g + r/16, columns 4(r%16)..   r <64: key columns 4(r-48)..   r <80: value columns 4(r-64)..
    const int hsel = (tid >> 5) & 3, i = tid & 31;
    const int r = tid < 80 ? tid : 0;
    const int pcol = r < 48 ? (3 * g + (r >> 4)) * 64 + 4 * (r & 15) : r < 64 ? 576 + g * 64 + 4 * (r - 48) : 768 + g * 64 + 4 * (r - 64);
    const float* prow = pq_p + (int64_t)b * 960 + pcol;
    constexpr int NPQ = FUSED ? Q2_NPQ : DEC_KC_QKV;
    float4 sl4[NPQ], sq4[2];
    if (tid < 80) {
#pragma unroll
        for (int s = 0; s < NPQ; ++s)
            sl4[s] = float4(*reinterpret_cast<const float4*>(prow + (int64_t)s * rows_p * 960));      // (copied as a value: the loads keep their place between the address steps)
        if (!FUSED) {
            sq4[0] = reinterpret_cast<const float4*>(a.ssq1 + (int64_t)b * DEC_KC_QKV)[0];
            sq4[1] = reinterpret_cast<const float4*>(a.ssq1 + (int64_t)b * DEC_KC_QKV)[1];
        }
    }
    // FUSED: float4 c (columns 4c..4c+3) of the residual row, by thread c < 144: x_mid + the down slabs
    float4 xr4 = make_float4(0.f, 0.f, 0.f, 0.f), xd4[FUSED ? Q2_HC : 1];
    if (FUSED && tid < 144) {
        const int64_t fi = ((int64_t)(b >> 5) * 72 + (tid >> 1)) * 64 + (b & 31) + 32 * (tid & 1);      // f32_idx(rb, 72, m, 4 tid)
        xr4 = reinterpret_cast<const float4*>(xmidF_p)[fi];
#pragma unroll
        for (int s = 0; s < Q2_HC; ++s) xd4[s] = reinterpret_cast<const float4*>(a.dslabF)[(int64_t)s * a.slabF_stride4 + fi];
    }
    const float c = a.rope_cur[i], sn = a.rope_cur[32 + i];
    const int gbeg = sp * gs_p;                                   // groups of 4 keys
    const int gend_fixed = sp == TS - 1 ? 0x3fffffff : gbeg + gs_p;
    // The K/V stream of a workgroup (107 KB at 420 keys) is bound by what the memory side delivers per CU (~12 B/clk): a wave
    // that issues all 14 page loads up front sits in the issue queue for ~4 us, and the prologue's barriers wait for the
    // slowest wave.  So only the first DA_G1 key groups are requested before the prologue (enough bytes in flight to keep the
    // stream busy while it runs: slab sums, RoPE, two barriers); the rest is requested after it, and the score loop consumes
    // the groups in arrival order.
    const int kk = lane & 31, hf = lane >> 5;                     // matrix form: lane -> (key of the 32-key tile, half of its dims)
    i32x4 kq[4];
    u32x2 vq[DA_GM];
    auto load_ktile = [&](int g0) {
        const int gi = g0 + (kk >> 2) * DA_WAVES;
        const int tc = min(gi * 4 + (kk & 3), Tmax - 1);
        const i32x4* kp = reinterpret_cast<const i32x4*>(reinterpret_cast<const uint16_t*>(kpage) + (int64_t)tc * 64 + hf * 32);
#pragma unroll
        for (int st = 0; st < 4; ++st)
            kq[st] = kp[st];
    };
    auto load_vgroup = [&](int g0, int u) {
        const int gi = mf_group(g0, u);
        const int tc = min(gi * 4 + sub, Tmax - 1);
        vq[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(vpage) + (int64_t)tc * 64 + quad * 4));
    };
    float4 k4[MF ? 1 : DA_G], v4[MF ? 1 : DA_G];
    const int g_first = gbeg + wave;                              // the wave's first key group
    auto load_group = [&](int g0, int u) {                        // slot u of the chunk that starts at group g0 (vector form)
        const int gi = g0 + u * DA_WAVES;
        const int tc = min(gi * 4 + sub, Tmax - 1);               // inside the page; validity is decided later
        k4[u] = ld_kv(kpage, (int64_t)tc * 64 + quad * 4);
        v4[u] = ld_kv(vpage, (int64_t)tc * 64 + quad * 4);
    };
    if constexpr (MF) {
        load_ktile(g_first);
#pragma unroll
        for (int u = 0; u < DA_GM / 2; ++u) load_vgroup(g_first, u);
    } else {
#pragma unroll
        for (int u = 0; u < DA_G1; ++u) load_group(g_first, u);
    }
    __builtin_amdgcn_sched_barrier(0);
    kstamp(1, 1, dbg);

    const int ngroups = (pos + 3) >> 2;                           // groups of 4 cached keys
    const int gend = min(ngroups, gend_fixed);
    static_assert(DEC_KC_QKV == 8, "fixed summation order below");
    if (FUSED) {
        if (tid < 192) {                     // waves 0..2: the residual row and its sum of squares (threads 144..191 add zeros)
            float4 x = xr4;
#pragma unroll
            for (int s = 0; s < Q2_HC; ++s) x = f4add(x, xd4[s]);                // slab 0, then 1, ...
            const float ss = wave_sum(tid < 144 ? f4ssq(x) : 0.f);
            if (lane == 0) ssq_part[wave] = ss;
            if (g == 0 && sp == 0 && tid < 144) reinterpret_cast<float4*>(a.xnewR + (int64_t)b * 576)[tid] = x;
        }
        if (tid < 80) {
            float4 x = sl4[0];
#pragma unroll
            for (int s = 1; s < NPQ; ++s) x = f4add(x, sl4[s]);
            *reinterpret_cast<float4*>(xs + 4 * tid) = x;          // scaled by the RMS statistic after the barrier
        }
    } else if (tid < 80) {
        float4 x = sl4[0];
#pragma unroll
        for (int s = 1; s < DEC_KC_QKV; ++s) x = f4add(x, sl4[s]);           // slab 0, then 1, ... (the order of every build)
        const float ssum = ((sq4[0].x + sq4[0].y) + (sq4[0].z + sq4[0].w)) + ((sq4[1].x + sq4[1].y) + (sq4[1].z + sq4[1].w));
        const float rscale = 1.0f / sqrtf(ssum / 576.0f + a.eps);
        *reinterpret_cast<float4*>(xs + 4 * tid) = make_float4(x.x * rscale, x.y * rscale, x.z * rscale, x.w * rscale);
    }
    __syncthreads();
    kstamp(1, 2, dbg);
    const float rs2 = FUSED ? 1.0f / sqrtf(((ssq_part[0] + ssq_part[1]) + ssq_part[2]) / 576.0f + a.eps) : 1.0f;
    if (tid < 128) {
        const int base = hsel < 3 ? hsel * 64 : 192;
        const float x1 = xs[base + i] * rs2, x2 = xs[base + i + 32] * rs2;
        const float o1 = __fadd_rn(__fmul_rn(x1, c), __fmul_rn(-x2, sn));
        const float o2 = __fadd_rn(__fmul_rn(x2, c), __fmul_rn(x1, sn));
        if (hsel < 3) {
            qs[hsel * 64 + i] = o1 * 0.125f;        // head_dim^-0.5 = 1/8 exactly
            qs[hsel * 64 + i + 32] = o2 * 0.125f;
            if constexpr (MF) {                     // the same values as exact bf16 triples: the A operand of the score MFMAs
                __bf16 p0, p1, p2;
                split3(o1 * 0.125f, p0, p1, p2);
                qb[(0 * 3 + hsel) * 64 + i] = p0; qb[(1 * 3 + hsel) * 64 + i] = p1; qb[(2 * 3 + hsel) * 64 + i] = p2;
                split3(o2 * 0.125f, p0, p1, p2);
                qb[(0 * 3 + hsel) * 64 + i + 32] = p0; qb[(1 * 3 + hsel) * 64 + i + 32] = p1; qb[(2 * 3 + hsel) * 64 + i + 32] = p2;
            }
        } else {
            knew[i] = o1; knew[i + 32] = o2;
            if (sp == 0) { st_kv<KV16>(kpage, (int64_t)pos * 64 + i, o1); st_kv<KV16>(kpage, (int64_t)pos * 64 + i + 32, o2); }
        }
    } else if (tid < 192) {
        const float x1 = xs[256 + tid - 128] * rs2;
        vnew[tid - 128] = x1;
        if (sp == 0) st_kv<KV16>(vpage, (int64_t)pos * 64 + (tid - 128), x1);
    } else if (MF && tid < 256) {
        qb[9 * 64 + tid - 192] = static_cast<__bf16>(0.f);
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MF) {
#pragma unroll
        for (int u = DA_GM / 2; u < DA_GM; ++u) load_vgroup(g_first, u);
    } else {
#pragma unroll
        for (int u = DA_G1; u < DA_G; ++u) load_group(g_first, u);
    }
    __builtin_amdgcn_sched_barrier(0);
    kstamp(1, 3, dbg);

    if (wave < 3) {                      // score of the new key (q . k_new, both in LDS), consumed after the last barrier
        const float sn_ = wave_sum(qs[wave * 64 + lane] * knew[lane]);
        if (lane == 0) snew_s[wave] = sn_;
    }
    float4 q4[3];
    // matrix form: row 4 piece + head of the A operand in the k order of the key lanes (step s: dims 32 hf + 8 s ..); rows without
    // a (piece, head) read the zero row of qb.  Read from LDS per chunk: 16 registers less across the loop.
    const int aq_off = ((kk >> 2) < 3 && (kk & 3) < 3 ? (kk >> 2) * 3 + (kk & 3) : 9) * 64 + hf * 32;
    if constexpr (!MF) {
#pragma unroll
        for (int hh = 0; hh < 3; ++hh) q4[hh] = *reinterpret_cast<const float4*>(qs + hh * 64 + quad * 4);
    }
    float m_run[3] = {-INFINITY, -INFINITY, -INFINITY};
    float l_run[3] = {0.f, 0.f, 0.f};      // per-lane partial (this lane's keys only)
    float4 acc[3];
#pragma unroll
    for (int hh = 0; hh < 3; ++hh) acc[hh] = make_float4(0.f, 0.f, 0.f, 0.f);

    // one chunk = the DA_G key groups a wave holds in registers (masked by weight, exp(-inf) = 0: slots beyond the context hold
    // finite values, engine_lm.cpp clear_page_tails; the 16 dim-quads of a key are one DPP row).  The first chunk (every context
    // up to 448 keys per split) works on the registers loaded above; further chunks (longer contexts) reload and repeat.
    // Two code shapes around the same body (a macro, so that both are the literal source text):
    //   ONE   the plain loop; the compiler keeps a second set of K/V registers alive across the back edge (220 VGPRs)
    //   !ONE  the first chunk peeled by hand: 118 VGPRs, two workgroups per CU (DA_MINW)
#define MELLOW_DA_CHUNK(g0)                                                                                              \
    {                                                                                                                    \
        float sc[DA_G][3];                                                                                               \
        float cmax[3] = {-INFINITY, -INFINITY, -INFINITY};                                                               \
_Pragma("unroll")                                                                                                        \
        for (int u = 0; u < DA_G; ++u) {                                                                                 \
            const int gi = g0 + u * DA_WAVES;                                                                            \
            const int t = gi * 4 + sub;                                                                                  \
            const bool ok = gi < gend && t < pos;                                                                        \
_Pragma("unroll")                                                                                                        \
            for (int hh = 0; hh < 3; ++hh) {                                                                             \
                float sv = q4[hh].x * k4[u].x + q4[hh].y * k4[u].y + q4[hh].z * k4[u].z + q4[hh].w * k4[u].w;            \
                sv = row16_sum(sv);                                                                                      \
                sv = ok ? sv : -INFINITY;                                                                                \
                sc[u][hh] = sv;                                                                                          \
                cmax[hh] = fmaxf(cmax[hh], sv);                                                                          \
            }                                                                                                            \
        }                                                                                                                \
_Pragma("unroll")                                                                                                        \
        for (int hh = 0; hh < 3; ++hh) {                                                                                 \
            float cm = cmax[hh];                                                                                         \
            cm = fmaxf(cm, swz_xor16(cm));                                                                               \
            cm = half_max(cm);                                                                                           \
            const float m_new = fmaxf(m_run[hh], cm);                                                                    \
            const float alpha = fast_exp(m_run[hh] - m_new);                                                             \
            m_run[hh] = m_new;                                                                                           \
            float lsum = 0.f;                                                                                            \
            float4 o = make_float4(acc[hh].x * alpha, acc[hh].y * alpha, acc[hh].z * alpha, acc[hh].w * alpha);          \
_Pragma("unroll")                                                                                                        \
            for (int u = 0; u < DA_G; ++u) {                                                                             \
                const float p = fast_exp(sc[u][hh] - m_new);                                                             \
                lsum += p;                                                                                               \
                o.x += p * v4[u].x; o.y += p * v4[u].y; o.z += p * v4[u].z; o.w += p * v4[u].w;                          \
            }                                                                                                            \
            acc[hh] = o;                                                                                                 \
            l_run[hh] = l_run[hh] * alpha + lsum;                                                                        \
        }                                                                                                                \
    }
    const int g_stop = gend;
    // a later chunk's groups, all at once.  The text of load_group, written out: as a loop over load_group (a lambda, an always-inline
    // lambda, this macro around the lambda, a macro around a macro) every vector-form kernel comes out 7 .. 14 instructions
    // shorter with other waits in its FIRST chunk, and the one-row-block kernel takes 220 .. 221 VGPRs instead of 218
#define MELLOW_DA_RELOAD(g0)                                                                                             \
    {                                                                                                                    \
        _Pragma("unroll") for (int u = 0; u < DA_G; ++u) {                                                               \
            const int gi = (g0) + u * DA_WAVES;                                                                          \
            const int tc = min(gi * 4 + sub, Tmax - 1);                                                                  \
            k4[u] = ld_kv(kpage, (int64_t)tc * 64 + quad * 4);                                                           \
            v4[u] = ld_kv(vpage, (int64_t)tc * 64 + quad * 4);                                                           \
        }                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
    }
    // matrix form of a chunk (KV16): scores by four MFMAs, one softmax weight per (key lane, head), P V as above
    auto chunk_mf = [&](int vw, int g0) {
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const i32x4 aq = *reinterpret_cast<const i32x4*>(qb + aq_off + 8 * st);
            MELLOW_BF16(aq, kq[st], sacc);
        }
        // output lane (key kk, half hf'): rows 8 (r / 4) + 4 hf' + r % 4 -> piece 0 in r = head (hf' = 0), piece 1 in r = head (hf' = 1),
        // piece 2 in r = 4 + head (hf' = 0); rows 12 .. 14 (r = 4 + head, hf' = 1) are zero rows of A
        const int gi = mf_group(g0, kk >> 2), t = gi * 4 + (kk & 3);
        const bool ok = gi < gend && t < pos;
        float pw[3], alpha[3];
#pragma unroll
        for (int hh = 0; hh < 3; ++hh) {
            float sv = half_sum(sacc[hh] + sacc[4 + hh]);              // both halves of the wave hold the key's score
            sv = ok ? sv : -INFINITY;
            float cm = row16_max(sv);
            cm = fmaxf(cm, swz_xor16(cm));                            // max over the 32 keys of the tile (at least one is valid)
            const float m_new = fmaxf(m_run[hh], cm);
            alpha[hh] = fast_exp(m_run[hh] - m_new);
            m_run[hh] = m_new;
            pw[hh] = fast_exp(sv - m_new);
            l_run[hh] = l_run[hh] * alpha[hh] + pw[hh];               // per key lane; summed over the tile's lanes at the end
        }
        float4* plw = reinterpret_cast<float4*>(pl) + vw * 32;
        if (hf == 0) plw[kk] = make_float4(pw[0], pw[1], pw[2], 0.f);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // wave-private hand-over: LDS operations of a wave complete in order
#pragma unroll
        for (int hh = 0; hh < 3; ++hh) acc[hh] = make_float4(acc[hh].x * alpha[hh], acc[hh].y * alpha[hh], acc[hh].z * alpha[hh], acc[hh].w * alpha[hh]);
#pragma unroll
        for (int u = 0; u < DA_GM; ++u) {
            const float4 pp = plw[4 * u + sub];                        // the three heads' weights of key (u, sub): one address per 16 lanes
            const float4 v = bf16x4_f32(vq[u]);
            acc[0].x += pp.x * v.x; acc[0].y += pp.x * v.y; acc[0].z += pp.x * v.z; acc[0].w += pp.x * v.w;
            acc[1].x += pp.y * v.x; acc[1].y += pp.y * v.y; acc[1].z += pp.y * v.z; acc[1].w += pp.y * v.w;
            acc[2].x += pp.z * v.x; acc[2].y += pp.z * v.y; acc[2].z += pp.z * v.z; acc[2].w += pp.z * v.w;
        }
        asm volatile("" ::: "memory");                                 // the next chunk's weights are written after these reads
    };
    // reduce the 4 key-subs of the wave; publish (m, l, o) of the (virtual) wave vw
    auto publish = [&](int vw) {
#pragma unroll
        for (int hh = 0; hh < 3; ++hh) {
            float l = l_run[hh];                 // identical across the 16 quads of a sub; sum over the 4 subs
            if constexpr (MF) {                  // matrix form: one partial per key lane, the two halves of the wave hold the same 32
                l = row16_sum(l);
                l += swz_xor16(l);
            } else {
                l += swz_xor16(l);
                l = half_sum(l);
            }
            float4 o = acc[hh];
            o.x += swz_xor16(o.x); o.y += swz_xor16(o.y);
            o.z += swz_xor16(o.z); o.w += swz_xor16(o.w);
            o.x = half_sum(o.x); o.y = half_sum(o.y);
            o.z = half_sum(o.z); o.w = half_sum(o.w);
            if (sub == 0) *reinterpret_cast<float4*>(ored + (vw * 3 + hh) * 64 + quad * 4) = o;
            if (lane == 0) { mred[vw * 3 + hh] = m_run[hh]; lred[vw * 3 + hh] = l; }
        }
    };
    if constexpr (MF) {
        // virtual wave wave + NW j of this physical wave, one after the other on the same registers: its chunks
        // gbeg + vw + c * (DA_WAVES * DA_GM) below g_stop, then its partial; the first chunk of j = 0 was requested around the prologue
#pragma clang loop unroll(disable)
        for (int j = 0; j < VPW; ++j) {
            const int vw = wave + NW * j;
            if (j != 0) {
#pragma unroll
                for (int hh = 0; hh < 3; ++hh) { m_run[hh] = -INFINITY; l_run[hh] = 0.f; acc[hh] = make_float4(0.f, 0.f, 0.f, 0.f); }
            }
#pragma clang loop unroll(disable)
            for (int g0 = gbeg + vw; g0 < g_stop; g0 += DA_WAVES * DA_GM) {
                if (g0 != g_first) {             // every chunk but the first: load, then the same body
                    load_ktile(g0);
#pragma unroll
                    for (int u = 0; u < DA_GM; ++u) load_vgroup(g0, u);
                    __builtin_amdgcn_sched_barrier(0);
                }
                chunk_mf(vw, g0);
            }
            publish(vw);
        }
    } else if constexpr (ONE) {
        for (int g0 = g_first; g0 < g_stop; g0 += DA_WAVES * DA_G) {
            if (g0 != g_first) MELLOW_DA_RELOAD(g0)        // later chunks (only for contexts beyond 448 keys per split)
            MELLOW_DA_CHUNK(g0)
        }
    } else {
        if (g_first < g_stop) MELLOW_DA_CHUNK(g_first)
#pragma clang loop unroll(disable)
        for (int g0 = g_first + DA_WAVES * DA_G; g0 < g_stop; g0 += DA_WAVES * DA_G) {
            MELLOW_DA_RELOAD(g0)
            MELLOW_DA_CHUNK(g0)
        }
    }
#undef MELLOW_DA_CHUNK
#undef MELLOW_DA_RELOAD
    if constexpr (!MF) {
        // (the vector form keeps its own text: routing it through the lambda above changes the register allocation of the one-row-block
        //  kernel -- +128 v_mov, 7.9 -> 8.7 us per launch at B = 32, measured)
#pragma unroll
        for (int hh = 0; hh < 3; ++hh) {
            float l = l_run[hh];                 // identical across the 16 quads of a sub; sum over the 4 subs
            l += swz_xor16(l);
            l = half_sum(l);
            acc[hh].x += swz_xor16(acc[hh].x); acc[hh].y += swz_xor16(acc[hh].y);
            acc[hh].z += swz_xor16(acc[hh].z); acc[hh].w += swz_xor16(acc[hh].w);
            acc[hh].x = half_sum(acc[hh].x); acc[hh].y = half_sum(acc[hh].y);
            acc[hh].z = half_sum(acc[hh].z); acc[hh].w = half_sum(acc[hh].w);
            if (sub == 0) *reinterpret_cast<float4*>(ored + (wave * 3 + hh) * 64 + quad * 4) = acc[hh];
            if (lane == 0) { mred[wave * 3 + hh] = m_run[hh]; lred[wave * 3 + hh] = l; }
        }
    }
    kstamp(1, 4, dbg && l_run[0] == l_run[0]);
    __syncthreads();
    kstamp(1, 5, dbg);
#pragma unroll
    for (int it = tid; it < 384; it += NW * 64) {      // (whole 8-lane groups: 384 and NW * 64 are multiples of 8)
        // item -> (pair = (head hh, dim quad dq), wave w): the 8 waves' partials of a pair sit in 8 adjacent lanes and are
        // combined with three DPP steps (xor 1, xor 2, mirror of the 8-lane half-row) instead of a serial loop in 48 threads
        const int w = it & 7, pair = it >> 3, hh = pair >> 4, dq = pair & 15;
        const float mw = mred[w * 3 + hh];
        const float snew = snew_s[hh];
        float M = mw;
        M = fmaxf(M, dpp_mov<0xB1>(M));
        M = fmaxf(M, dpp_mov<0x4E>(M));
        M = fmaxf(M, dpp_mov<0x141>(M));
        if (sp == TS - 1) M = fmaxf(M, snew);          // the last split also owns the new key
        const float f = M > -INFINITY ? fast_exp(mw - M) : 0.f;      // waves without keys: m = -inf -> factor 0; an empty split: all 0
        const float4 ow = *reinterpret_cast<const float4*>(ored + (w * 3 + hh) * 64 + dq * 4);
        float L = lred[w * 3 + hh] * f;
        float4 O = make_float4(ow.x * f, ow.y * f, ow.z * f, ow.w * f);
#define MELLOW_R8(V) V += dpp_mov<0xB1>(V); V += dpp_mov<0x4E>(V); V += dpp_mov<0x141>(V)
        MELLOW_R8(L); MELLOW_R8(O.x); MELLOW_R8(O.y); MELLOW_R8(O.z); MELLOW_R8(O.w);
#undef MELLOW_R8
        if (w == 0) {
            if (sp == TS - 1 && M > -INFINITY) {
                const float pn = fast_exp(snew - M);
                const float4 vn = *reinterpret_cast<const float4*>(vnew + dq * 4);
                L += pn;
                O.x += pn * vn.x; O.y += pn * vn.y; O.z += pn * vn.z; O.w += pn * vn.w;
            }
            // F16-layout (B operand of the o_proj's 16x16x4 MFMA): column k = head*64 + 4*dq
            const int head = 3 * g + hh, k = head * 64 + dq * 4;
            const int rb = b >> 5, m = b & 31;
            const int64_t o4 = ((((int64_t)sp * a.RB + rb) * 36 + (k >> 4)) * 2 + (m >> 4)) * 64 + (m & 15) + 16 * ((k >> 2) & 3);
            *(reinterpret_cast<float4*>(a.attF16) + o4) = O;
            if (dq == 0)      // (m, l) of this split: [head][row][split] pairs, so that the o_proj reads both splits of a row with one 16-byte load
                *reinterpret_cast<float2*>(a.att_ml + (((int64_t)head * a.rows + b) * TS + sp) * 2) = make_float2(M, L);
        }
    }
    kstamp(1, 6, dbg);
    kspan(a.dbg_seq, 1);
}

// ----------------------------------------------------------------------------------------------------
// K3  o_proj with complete output.  grid (36 n16-tiles, 2 row halves x RB), 16 waves; v_mfma_f32_16x16x4_f32,
//     W in P16-layout.  A workgroup owns 16 rows x 16 columns and the whole K = 576 (one MFMA tile), so its
//     output is complete: x_mid = x_new + merge(attention splits) Wo^T.  Splitting the 32 batch rows into two
//     halves doubles the workgroups (72) and halves the activation bytes each CU has to pull.
//     writes x_mid row-major + F32-layout (next layer's qkv) + F16-layout (gate/up) + per-tile sum of squares
// ----------------------------------------------------------------------------------------------------
#ifndef MELLOW_OPROJ_WAVES
#define MELLOW_OPROJ_WAVES 12
#endif
// waves per workgroup: 12 x 3 k16-tiles = the 36 tiles exactly (16 x 3 left 12 empty slots whose loads were still issued:
// +1.1 ms of decode per 63 steps, measured on one box with tools/ab_build.sh)
constexpr int OP_WAVES = MELLOW_OPROJ_WAVES;
// rows per workgroup: 16 (two halves of a 32-row block, 72 workgroups) or 8 (four quarters, 144 workgroups: the MFMA tile still
// has 16 batch columns, eight of them zero, but a workgroup pulls half the attention partials -- its body is bound by the
// bytes one CU has to ingest)
// Chosen per launch: 8 rows for a single row block (B <= 32: 52.8 -> 52.2 ms of decode per 63 steps), 16 rows otherwise (at
// B = 64 the 288 eight-row workgroups no longer fit the 256 CUs: 76.3 -> 78.5 ms).  MELLOW_OPROJ_ROWS forces one form.
template <bool BLK, int W8, int OP_ROWS, int TS>
__global__ __launch_bounds__(OP_WAVES * 64) void dec_oproj_kernel(const float* __restrict__ Wp16, const float* __restrict__ attF16_p,
                                                                  const float* __restrict__ att_ml_p, const float* __restrict__ xnewR_p,
                                                                  int RB_p, int rows_p, const DecArgs a,
                                                                  const float* __restrict__ wscale) {
    kspan(a.dbg_seq, 0);
    __shared__ __attribute__((aligned(16))) float red[OP_WAVES * 4 * 64];   // [wave][acc reg][lane]
    constexpr int K16 = 36, TPW = (K16 + OP_WAVES - 1) / OP_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int PARTS = 32 / OP_ROWS;                     // workgroups per 32-row block
    const int nt = blockIdx.x, rb = blockIdx.y / PARTS, part = blockIdx.y % PARTS;
    const int mh = OP_ROWS == 16 ? part : part >> 1;        // which 16-row half the MFMA tile covers
    MELLOW_BLK_EXIT(rb)
    const int ml = lane & 15;
    const bool lrow = OP_ROWS == 16 || (ml >> 3) == (part & 1);          // this lane's batch row belongs to the workgroup
    const int64_t wslot = (int64_t)nt * K16 * 64 + lane;
    // epilogue operand issued up front: thread (m, nq) of the 16 x 16 tile owns 4 consecutive columns
    const int em = (tid >> 2) & 15, enq = tid & 3;
    const bool erow_ok = OP_ROWS == 16 || (em >> 3) == (part & 1);
    const int64_t erow = (int64_t)rb * 32 + mh * 16 + em;
    float4 xres = make_float4(0.f, 0.f, 0.f, 0.f);
    if (erow_ok) xres = *reinterpret_cast<const float4*>(xnewR_p + erow * 576 + nt * 16 + enq * 4);

    WFrag<TPW, W8> w;
    float4 os[TPW][TS];
    float ms[TPW][TS], ls[TPW][TS];
    const int64_t row = (int64_t)rb * 32 + mh * 16 + ml;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = wave + OP_WAVES * i, tc = t < K16 ? t : K16 - 1;     // clamped: out-of-range tiles get zero weights
        w.t[i] = w.load(Wp16, wslot + (int64_t)tc * 64);
        if (t >= K16) { if constexpr (W8 == 2) w.t[i] = 0u; else w.t[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
        const int h = tc >> 2;                                        // tile = 16 k of head h
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            ms[i][s] = 0.f; ls[i][s] = 1.f; os[i][s] = make_float4(0.f, 0.f, 0.f, 0.f);     // rows of another workgroup: x = 0
            if (lrow) os[i][s] = reinterpret_cast<const float4*>(attF16_p)[((((int64_t)s * RB_p + rb) * 36 + tc) * 2 + mh) * 64 + lane];
        }
        if (lrow) {
            const float* mlp = att_ml_p + ((int64_t)h * rows_p + row) * TS * 2;
            if constexpr (TS == 2) {                     // (m, l) of both splits of the row: one 16-byte load
                const float4 v = *reinterpret_cast<const float4*>(mlp);
                ms[i][0] = v.x; ls[i][0] = v.y; ms[i][1] = v.z; ls[i][1] = v.w;
            } else if constexpr (TS == 1) {
                const float2 v = *reinterpret_cast<const float2*>(mlp);
                ms[i][0] = v.x; ls[i][0] = v.y;
            } else {
#pragma unroll
                for (int s = 0; s < TS; ++s) { ms[i][s] = mlp[2 * s]; ls[i][s] = mlp[2 * s + 1]; }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 xm[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        // merge the key splits: x = sum_s f_s o_s / sum_s f_s l_s, f_s = exp(m_s - max m)
        float M = ms[i][0];
#pragma unroll
        for (int s = 1; s < TS; ++s) M = fmaxf(M, ms[i][s]);
        float L = 0.f;
        float4 O = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            const float f = fast_exp(ms[i][s] - M);
            L += ls[i][s] * f;
            O.x += os[i][s].x * f; O.y += os[i][s].y * f; O.z += os[i][s].z * f; O.w += os[i][s].w * f;
        }
        const float inv = 1.0f / L;
        xm[i] = make_float4(O.x * inv, O.y * inv, O.z * inv, O.w * inv);      // the merged activation
    }
    acc = slice_mma16<TPW, W8>(acc, w, xm);
    // D[i = n_local = 4*(lane>>4) + r][j = m_local = lane&15]
    reduce_store(MELLOW_LDS(red) + wave * 4 * 64 + lane, acc);
    __syncthreads();
    if (tid < 64 && erow_ok) {
        // columns n = 4*enq + r live in registers r = 0..3 of lane em + 16*enq
        const int src_lane = em + 16 * enq;
        const int k = nt * 16 + enq * 4;
        float4 v = make_float4(red_sum<OP_WAVES, 4>(MELLOW_LDS(red), 0, src_lane), red_sum<OP_WAVES, 4>(MELLOW_LDS(red), 1, src_lane), red_sum<OP_WAVES, 4>(MELLOW_LDS(red), 2, src_lane), red_sum<OP_WAVES, 4>(MELLOW_LDS(red), 3, src_lane));
        if (W8) v = f4scale(v, wscale + k);
        const float4 y = f4add(xres, v);
        *(reinterpret_cast<float4*>(a.xmidF) + f32_idx(rb, 72, mh * 16 + em, k)) = y;
        if (a.xmid3_32) {                  // f32x3 layer kernels: x_mid pre-split for the q/k/v part (F3-32) and for gate/up (F3-16)
            const F3Quad yq = f3_split4(y), yo = f3_partner(yq);      // threads (enq, enq ^ 1) hold the halves of one slot
            if (!(enq & 1)) {
                f3_store8(a.xmid3_32, f3_32_slot(rb, 36, mh * 16 + em, k), yq, yo);
                f3_store8(a.xmid3_16, f3_16_slot(rb, 18, mh * 16 + em, k), yq, yo);
            }
        } else
        *(reinterpret_cast<float4*>(a.xmidF16) + (((int64_t)rb * 36 + nt) * 2 + mh) * 64 + em + 16 * enq) = y;
        float ss = f4ssq(y);
        ss += dpp_mov<0xB1>(ss);             // sum over the quad (the 4 column groups of one row)
        ss += dpp_mov<0x4E>(ss);
        if (enq == 0) a.ssq[erow * 40 + nt] = ss;
    }
    kspan(a.dbg_seq, 1);
}

// fp32 K/V pages -> their bf16 shadow (KV16; round to nearest even), 8 values per thread
__global__ __launch_bounds__(256) void kv_to_bf16_kernel(const float4* __restrict__ src, uint4* __restrict__ dst, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const float4 a = src[2 * i], b = src[2 * i + 1];
        typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
        const bf16x8v o = {static_cast<__bf16>(a.x), static_cast<__bf16>(a.y), static_cast<__bf16>(a.z), static_cast<__bf16>(a.w),
                           static_cast<__bf16>(b.x), static_cast<__bf16>(b.y), static_cast<__bf16>(b.z), static_cast<__bf16>(b.w)};
        dst[i] = __builtin_bit_cast(uint4, o);
    }
}
void launch_kv_to_bf16(const float* src, void* dst, int64_t n, hipStream_t s) {
    const int64_t n8 = n >> 3;
    const int blocks = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);
    hipLaunchKernelGGL(kv_to_bf16_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(src), reinterpret_cast<uint4*>(dst), n8);
}
// Prefix K/V of B examples -> the decode pages of their n answers each (mellow_generate_n): for every layer l, kv head h and
// position t < T the 64 floats of K and of V of example b go to rows b * n .. b * n + n - 1.  src: [layer][B][3][Tp][64] (a
// buffer of its own: never the pages), dst: [layer][Bp][3][Tmax][64].  Pure bandwidth: a thread owns one float4 of the source
// (K and V), reads it ONCE and stores it n times -- HBM reads are 1 / n of the writes; for a fixed copy j consecutive threads
// store consecutive 16-byte words of one page.  Positions >= T of a page are not touched.  64-bit indices throughout: one layer
// of pages at 1024 rows is past 2^31 bytes.
__global__ __launch_bounds__(256) void kv_fanout_kernel(const float4* __restrict__ ksrc, const float4* __restrict__ vsrc,
                                                        float4* __restrict__ kdst, float4* __restrict__ vdst, int64_t total,
                                                        int B, int n, int Bp, int T16, int64_t Tp16, int64_t Tmax16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pg = i / T16, q = i - pg * T16;          // source page (l * B + b) * 3 + h, float4 inside its first T positions
        const int64_t lb = pg / 3, h = pg - lb * 3, l = lb / B, b = lb - l * B;
        const float4 k = ksrc[pg * Tp16 + q], v = vsrc[pg * Tp16 + q];
        int64_t d = ((l * Bp + b * n) * 3 + h) * Tmax16 + q;
        for (int j = 0; j < n; ++j, d += 3 * Tmax16) {
            kdst[d] = k;
            vdst[d] = v;
        }
    }
}
void launch_kv_fanout(const float* k_prefix, const float* v_prefix, float* k_pages, float* v_pages, int layers, int B, int n, int Bp,
                      int T, int Tp, int Tmax, hipStream_t s) {
    if (layers <= 0 || B <= 0 || n <= 0 || T <= 0 || T > Tp || T > Tmax || (int64_t)B * n > Bp) return;      // (the engine never asks for these)
    const int64_t total = (int64_t)layers * B * 3 * T * 16;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(kv_fanout_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(k_prefix),
                       reinterpret_cast<const float4*>(v_prefix), reinterpret_cast<float4*>(k_pages), reinterpret_cast<float4*>(v_pages),
                       total, B, n, Bp, T * 16, (int64_t)Tp * 16, (int64_t)Tmax * 16);
}

// ---- launchers -------------------------------------------------------------------------------------------
// false, and nothing launched: no instantiation serves a.ts key splits (the caller reports it)
bool launch_dec_attn(const DecArgs& a, float* k_cache, float* v_cache, bool fused, hipStream_t s) {
    const dim3 grid(3, a.rows, a.ts);
    const bool one = a.RB == 1 && !a.blk_live;
    if (a.ts != DEC_TS && (one || a.kv16 || a.ts != DEC_TS_MULTI)) return false;      // kernels.h dec_key_splits
    auto launch = [&](auto blk, auto one_c) { with_bool(fused, [&](auto fused_c) { with_bool(a.kv16 != 0, [&](auto kv16) {
        constexpr bool ONE = one_c.value, KV16 = kv16.value;
        // bf16 pages, matrix form: MELLOW_DA16_NW physical waves from two row blocks on -- kernel comment at DA_GM
        constexpr int NW = KV16 && !ONE ? MELLOW_DA16_NW : DA_WAVES;
        // the split count: ONE never meets another than DEC_TS, and the bf16 pages always run DEC_TS
        constexpr int TSM = ONE || KV16 ? DEC_TS : DEC_TS_MULTI;
        with_int<DEC_TS, TSM>(a.ts, [&](auto ts) {
            hipLaunchKernelGGL((dec_attn_kernel<blk.value, fused_c.value, ONE, KV16, NW, ts.value>), grid, dim3(NW * 64), 0, s, k_cache, v_cache,
                               (const int32_t*)a.d_pos, (const float*)a.pq, (const float*)a.xmidF, a.Tmax, a.gs, a.rows, a);
        });
    }); }); };
    // (the per-block early exit exists only with more than one row block, so <BLK, ONE> never meet)
    if (one) launch(std::false_type{}, std::true_type{});
    else with_bool(a.blk_live != nullptr, [&](auto blk) { launch(blk, std::false_type{}); });
    return true;
}
int dec_attn_chunk_groups(bool kv16) { return DA_WAVES * (kv16 ? DA_GM : DA_G); }
void launch_dec_oproj(const DecArgs& a, const float* Wp16, hipStream_t s, const float* wscale) {
#ifdef MELLOW_OPROJ_ROWS
    const int rows = MELLOW_OPROJ_ROWS;
#else
    const int rows = a.RB == 1 ? 8 : 16;
#endif
    with_int<8, 16>(rows, [&](auto rows_c) { with_int<1, DEC_TS>(a.ts, [&](auto ts) { with_blk_w8(a, wscale, [&](auto blk, auto w8) {
        constexpr int ROWS = rows_c.value, PARTS = ROWS == 8 ? 4 : 2;        // the two forms of the kernel: 8 rows x 4 parts, 16 rows x 2 parts
        hipLaunchKernelGGL((dec_oproj_kernel<blk.value, w8.value, ROWS, ts.value>), dim3(36, PARTS * a.RB), dim3(OP_WAVES * 64), 0, s, Wp16,
                           (const float*)a.attF16, (const float*)a.att_ml, (const float*)a.xnewR, a.RB, a.rows, a, wscale);
    }); }); });
}

}  // namespace mellow
