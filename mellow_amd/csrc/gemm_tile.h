// What the 128 x 128 tile GEMMs share (gemm_bf16x3.hip: the f32x3 kernels; gemm_fp8.hip: gemm_mx8_kernel), each once:
//   - glds16, the LDS-DMA load;
//   - the accumulator zeroing;
//   - the tile prologue: block index -> tile (tile_decode), the split-K k-range, the row scales of the norm-free chaining, the
//     idle-wave rule;
//   - the LDS-DMA stage descriptor ("waves 0, 1 carry A, waves 2, 3 carry W") and its issue step;
//   - host side: the rule of the XCD-ownership order and the tile grid.
// Everything here is inlined into its caller.  The helpers return values (a result written through a reference
// changed callers there, and the zeroing did here: it is a macro).
#pragma once
#include "common.h"
#include "kernels.h"

namespace mellow {

constexpr int TILE_M = 128, TILE_N = 128;           // a workgroup's output tile: 4 waves, 64 x 64 each (wm = wave >> 1, wn = wave & 1)

// 64 lanes x 16 bytes global -> LDS without registers: LDS address = lds_addr (wave-uniform, through m0) + lane * 16.  Issued from
// inline asm, which hipcc does not count: the callers' vmcnt waits are explicit.
__device__ __forceinline__ void glds16(const void* base, uint32_t voff, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_addr), "s"(base) : "memory");
}

// Accumulator zeroing: one f32x16, f32x16 [2], f32x16 [2][2].  Macros: as a function writing through a reference it moved a global
// load and two waits of the x3p loop.
#define TILE_ZERO_ACC(a) _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (a)[r_] = 0.f;
#define TILE_ZERO_ACC2(a) _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) TILE_ZERO_ACC((a)[j_])
#define TILE_ZERO_ACC22(a) _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) TILE_ZERO_ACC2((a)[i_])

// ---- block index -> output tile (pm, pn), tile = pm * gn + pn, and the split-K part of it ---------------------------------------
// Two orders.  xcd_remap (common.h): panel-major, tile = L % (gm gn), split = L / (gm gn); SPLITK = false is the launch without
// split-K (one workgroup per tile, no division by the tile count).
// ng (wide outputs: gn % 8 == 0, gn >= 16, no split-K; tile_ng below): weight-stationary per XCD (block b runs on XCD b % 8: observed,
// speed only).  XCD x owns the n-tiles [x gn/8, (x+1) gn/8) for EVERY row panel.  With the panel-major order an XCD walks ~12 row
// panels and needs ALL gn weight tiles for each: the LM's gate/up operand is 10.6 MB against a 4 MiB L2, so every panel re-fetched
// the whole weight -- measured 850 MB of reads per launch for 54 MB of operands, 45 % of the family's memory-side traffic, and the
// launch ran at the fabric's rate (profiles/r05_pmc_traffic_by_shape_*.txt).  In the ng order an XCD keeps gn / 8 weight tiles
// (1.3 MB) hot and every panel is read once per XCD: 8 x 43 + 10.6 MB.
struct TilePos {
    int pm, pn, tile, split;
};
template <bool SPLITK>
__device__ __forceinline__ TilePos tile_decode(int gm, int gn, int ks, int ng) {
    TilePos t;
    if (ng) {
        const int npx = gn >> 3, b = (int)blockIdx.x, j = b >> 3;
        t.pm = j / npx; t.pn = (b & 7) * npx + j % npx;
        t.tile = t.pm * gn + t.pn; t.split = 0;
    } else {
        const int tiles = gm * gn;
        const int L = xcd_remap((int)blockIdx.x, SPLITK ? tiles * ks : tiles);
        t.tile = SPLITK ? L % tiles : L; t.split = SPLITK ? L / tiles : 0;
        t.pm = t.tile / gn; t.pn = t.tile % gn;
    }
    return t;
}
// this workgroup's k steps of KTf: [kt0, kt0 + KT) (all of them without split-K)
struct KRange {
    int kt0, KT;
};
__device__ __forceinline__ KRange splitk_range(int KTf, int split, int ks) {
    const int kt0 = split * KTf / ks;
    return {kt0, (split + 1) * KTf / ks - kt0};
}

// norm-free chaining (kernels.h, rs_*): the scale of row pm * 128 + r.  A kernel forms its 128 row scales into LDS while its first
// LDS-DMA stages are in flight, so that the epilogue finds them there instead of starting with nine dependent loads per row.
__device__ __forceinline__ float rs_row_scale(const GemmArgs& g, int pm, int r) {
    int64_t m = (int64_t)pm * TILE_M + r;
    m = m < g.M ? m : g.M - 1;
    const float* sp = g.rs_ssq + m * g.rs_parts;
    float ss = 0.f;
    for (int q = 0; q < g.rs_parts; ++q) ss += sp[q];                 // fixed order
    return 1.0f / sqrtf(ss / g.rs_dim + g.rs_eps);
}

// A wave whose 64 columns lie entirely beyond the weight's rows (the second half of the last column tile when N is an odd multiple
// of 64: N = 576 -> 1 wave pair in 10, N = 960 -> 1 in 16) keeps its loading duty and its barriers but issues no MFMA: the matrix
// pipe it would have kept busy with zeros goes to the other workgroup of the CU.  Wave-uniform.
__device__ __forceinline__ bool wave_idle(int pn, int wn, int Nw) { return pn * TILE_N + wn * 64 >= Nw; }

// ---- LDS-DMA staging of a k step: both operands lie in HBM in the order the stage has in LDS, 2 * PIECES 1-KiB pieces per operand.
// Waves 0, 1 carry the A stage (pieces (wave & 1) * PIECES .. + PIECES - 1), waves 2, 3 the W stage; the A stages of the ring
// lie at lds_a, the W stages at lds_w (byte addresses).  base_a / base_w = the operand at this workgroup's first k step (base_a
// at this wave's first piece); a k step advances A by kstep_a bytes (contiguous pieces) and W by kstep_w; voff_w(c) = byte offset
// of this lane's 16 bytes of W piece c from base_w -- each kernel's own arithmetic (mx8 counts it from the weight's start).
template <int PIECES>
struct DmaStage {
    const char* base;       // wave-uniform
    uint32_t kstep;
    uint32_t voff[PIECES];
    uint32_t lds0;          // of this wave's first piece in stage 0
};
template <int PIECES, typename VoffW>
__device__ __forceinline__ DmaStage<PIECES> dma_stage(int wave, int lane, const char* base_a, const char* base_w, uint32_t kstep_a, uint32_t kstep_w,
                                                      uint32_t lds_a, uint32_t lds_w, VoffW voff_w) {
    DmaStage<PIECES> d;
    const bool isA = wave < 2;
    const int c0 = (wave & 1) * PIECES;
    d.base = isA ? base_a : base_w;
    d.kstep = isA ? kstep_a : kstep_w;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) d.voff[j] = isA ? (uint32_t)(j * 1024 + lane * 16) : voff_w(c0 + j);
    d.lds0 = (isA ? lds_a : lds_w) + (uint32_t)c0 * 1024u;
    return d;
}
// k step t (clamped to the last: the look-ahead issues behind the end re-load it) -> the stage at byte offset st_off of the ring
template <int PIECES>
__device__ __forceinline__ const char* dma_step_base(const DmaStage<PIECES>& d, int t, int KT) {
    const int t_ = t < KT ? t : KT - 1;
    return d.base + (int64_t)t_ * d.kstep;
}
template <int PIECES>
__device__ __forceinline__ void dma_piece(const DmaStage<PIECES>& d, const char* step_base, uint32_t st_off, int j) {
    glds16(step_base, d.voff[j], d.lds0 + (st_off + (uint32_t)(j * 1024)));
}
template <int PIECES>
__device__ __forceinline__ void dma_issue(const DmaStage<PIECES>& d, int t, int KT, uint32_t st_off) {
    const char* b_ = dma_step_base(d, t, KT);
#pragma unroll
    for (int j = 0; j < PIECES; ++j) dma_piece(d, b_, st_off, j);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// the ng order pays when an XCD's share of the weight is at least two tiles
inline bool tile_ng(int gn) { return gn % 8 == 0 && gn >= 16; }
// D = a kernel's argument struct {GemmArgs a; int gm, gn; ...}
template <typename D>
inline D tile_grid(const GemmArgs& a) {
    D d;
    d.a = a;
    d.gm = (a.M + TILE_M - 1) / TILE_M;
    d.gn = (a.Nw + TILE_N - 1) / TILE_N;
    return d;
}

}  // namespace mellow
