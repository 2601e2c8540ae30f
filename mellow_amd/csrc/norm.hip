// The norm kernels: the encoder's LayerNorm (plain / row-map gather, patch-merging gather) and the LM's RMSNorm, each as fp32 rows
// and as the pre-split image its consumer GEMM reads (APB for the x3q kernel, MXFP8 in AMX order for gemm_mx8_kernel: common.h).
// Every expression that decides a result bit stands ONCE here -- ln_stats, ln_affine, sumsq4, rms_scaled -- with contraction off
// inside it: written out per kernel the compiler contracted two copies of one sum in opposite orders, and
// tests/test_gpu_norm.py holds the image kernels to the plain kernels' rows word for word.
#include "common.h"
#include "kernels.h"

namespace mellow {

constexpr int LN_MAXV = 6;  // float4 per lane: one wave per row, row kept in registers (C <= 1536)

// The float4 quads of a row that a lane owns, v = lane, lane + 64, .. < nv (`lane` and `nv` are the caller's); the statements see q
// and v.  A macro: as a __forceinline__ function over a closure it gave other instructions in rmsnorm_kernel and in pass 1 of
// rmsnorm_apb_kernel, as one text it gives the streams they had with the loop written out.
#define ROW_QUADS(N, q, v, ...)                          \
    _Pragma("unroll") for (int q = 0; q < (N); ++q) {    \
        const int v = lane + 64 * q;                     \
        if (v < nv) { __VA_ARGS__ }                      \
    }

// x^2 + y^2 + z^2 + w^2 of one float4 in ONE pinned form, fma(x, x, y y) + fma(z, z, w w).  Written as a plain expression the compiler
// is free to contract it either way round, and it did: fma(x, x, y y) in rmsnorm_kernel, fma(y, y, x x) in rmsnorm_apb_kernel, so the
// two kernels' 1/rms differed in the last place on a few rows in a hundred (tests/test_gpu_norm.py).  This is the form rmsnorm_kernel
// and both LayerNorm kernels (on the centred values) compiled to before: their results are unchanged.
__device__ __forceinline__ float sumsq4(const float4& v) {
#pragma clang fp contract(off)
    const float yy = v.y * v.y, ww = v.w * v.w;
    return __builtin_fmaf(v.x, v.x, yy) + __builtin_fmaf(v.z, v.z, ww);
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
// The row statistic (biased variance, eps 1e-5) from the quads a lane holds; the only one in the tree.  Per quad (x + y) + (z + w) and
// sumsq4 of the centred quad, quads in the order of q, then the wave butterfly: two passes over registers.
template <int NQ>
__device__ __forceinline__ void ln_stats(const float4 (&x)[NQ], int lane, int nv, int C, float& mean, float& rstd) {
#pragma clang fp contract(off)
    float sum = 0.f;
    ROW_QUADS(NQ, q, v, sum += (x[q].x + x[q].y) + (x[q].z + x[q].w);)
    mean = wave_sum(sum) / (float)C;
    const float mu = mean;
    float sq = 0.f;
    ROW_QUADS(NQ, q, v, sq += sumsq4(make_float4(x[q].x - mu, x[q].y - mu, x[q].z - mu, x[q].w - mu));)
    rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + 1e-5f);
}
// (x - mean) rstd w + b.  The one freedom this leaves the compiler is the last step, which it fuses to fma((x - mean) rstd, w, b) at every
// site as it always did (the same count of fma and product instructions per kernel as before; the image == rows identities of the test).
__device__ __forceinline__ float4 ln_affine(const float4& x, float mean, float rstd, const float4& w, const float4& b) {
    return make_float4((x.x - mean) * rstd * w.x + b.x, (x.y - mean) * rstd * w.y + b.y, (x.z - mean) * rstd * w.z + b.z,
                       (x.w - mean) * rstd * w.w + b.w);
}

template <int MODE>  // 0: plain / row-map gather, 1: patch-merging gather
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        int64_t M, int C, const float* __restrict__ w,
                                                        const float* __restrict__ b,
                                                        const int32_t* __restrict__ row_map, int ntok, int R,
                                                        int Cin) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * 4 + wave;
    if (m >= M) return;
    const int nv = C >> 2;
    const float* src_row = nullptr;
    int64_t seg_base[4];
    if (MODE == 0) {
        int64_t src = m;
        if (row_map) src = (m / ntok) * ntok + row_map[m % ntok];
        src_row = in + src * C;
    } else {
        // output token (clip, i, j) of the (R/2)^2 grid gathers tokens (2i,2j), (2i+1,2j), (2i,2j+1), (2i+1,2j+1)
        // in that order (reference htsat.py:488-492)
        const int R2 = R >> 1;
        const int64_t clip = m / (R2 * R2);
        const int ij = (int)(m % (R2 * R2));
        const int i = ij / R2, j = ij % R2;
        const int64_t cb = clip * R * R;
        seg_base[0] = (cb + (int64_t)(2 * i) * R + 2 * j) * Cin;
        seg_base[1] = (cb + (int64_t)(2 * i + 1) * R + 2 * j) * Cin;
        seg_base[2] = (cb + (int64_t)(2 * i) * R + 2 * j + 1) * Cin;
        seg_base[3] = (cb + (int64_t)(2 * i + 1) * R + 2 * j + 1) * Cin;
    }
    float4 x[LN_MAXV] = {};
    ROW_QUADS(LN_MAXV, q, v,
        if (MODE == 0) {
            x[q] = reinterpret_cast<const float4*>(src_row)[v];
        } else {
            const int e = v * 4;
            const int seg = e / Cin, c = e % Cin;
            x[q] = *reinterpret_cast<const float4*>(in + seg_base[seg] + c);
        })
    float mean, rstd;
    ln_stats(x, lane, nv, C, mean, rstd);
    float4* dst = reinterpret_cast<float4*>(out + m * C);
    ROW_QUADS(LN_MAXV, q, v, dst[v] = ln_affine(x[q], mean, rstd, reinterpret_cast<const float4*>(w)[v], reinterpret_cast<const float4*>(b)[v]);)
}
void launch_layernorm(const float* in, float* out, int M, int C, const float* w, const float* b,
                      const int32_t* row_map, int ntok, hipStream_t s) {
    hipLaunchKernelGGL((layernorm_kernel<0>), dim3((M + 3) / 4), dim3(256), 0, s, in, out, (int64_t)M, C, w, b,
                       row_map, ntok, 0, 0);
}
void launch_merge_layernorm(const float* in, float* out, int n, int R, int C, const float* w, const float* b,
                            hipStream_t s) {
    const int64_t M = (int64_t)n * (R / 2) * (R / 2);
    hipLaunchKernelGGL((layernorm_kernel<1>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, in, out, M, 4 * C, w, b,
                       (const int32_t*)nullptr, 0, R, C);
}

// ---- the image kernels (*_apb) -----------------------------------------------------------------------------------------------------
// A workgroup owns 32 consecutive OUTPUT rows.  Pass 1 reads them one row per wave at a time (coalesced), with the plain kernel's
// lane -> column mapping, expressions and reduction order (the same statistic bit for bit), and stages them in LDS; a second pass
// over global memory in image order touches 32 cache lines per load instruction (22 us per launch at M = 12448; from LDS: see
// profiles/).  Row stride C + 4 floats: the sixteen lanes of a ds_read_b128 group then sit on sixteen different bank quads.
//
// Pass 2, the one image writer: the staged rows re-read with lane = (row % 32, k-half), the order of an APB slot run, so that every
// store instruction of a wave writes 1 KiB contiguous (a first version that stored from the row-per-wave mapping scattered 16-byte
// pieces 12 KiB apart and took 2.3x the time of the plain kernel).  FINISH(at, x) turns four staged columns into four results; it is
// all that distinguishes LayerNorm from RMSNorm.  AMX = false: the APB image of the x3q GEMM, a lane holds 8 columns per step.
// AMX = true (fp8 mode): the same values quantised to MXFP8 in the AMX image order of gemm_mx8_kernel (common.h: one scale per 32
// columns; a lane holds 16 consecutive columns, its partner lane the other 16 of the block; pad blocks up to a whole k64 step are
// written as zeros).
// A macro over the kernel's lane, wave, ml, m, C, KT, RS, out and sc, and FINISH a macro too whose `at` is the text `col + 4 * q`,
// to be written behind a pointer WITHOUT parentheses: the address is then (w + col) + 4 q as it always was.  w + (col + 4 q), which a
// closure over the column gives, is another instruction stream to the compiler, and as a __forceinline__ function the writer reads
// the staged quads with other LDS instructions; this text gives rmsnorm_apb_kernel the streams it had.
#define NORM_IMAGE_ROWS(AMX, rows_s, FINISH)                                                                       \
    do {                                                                                                           \
        constexpr int NQ2 = AMX ? 4 : 2; /* float4 per lane and step */                                            \
        const int kh = lane >> 5, KT64 = (C + 63) >> 6, KQ = (KT64 + 3) >> 2;                                      \
        for (int k = wave; k < (AMX ? 2 * KT64 : KT); k += 4) {                                                    \
            const int col = AMX ? k * 32 + kh * 16 : k * 16 + kh * 8;                                              \
            float y[4 * NQ2];                                                                                      \
            _Pragma("unroll") for (int q = 0; q < NQ2; ++q) {                                                      \
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                                                        \
                if (!AMX || col + 4 * q < C) {                                                                     \
                    const float4 x0 = *reinterpret_cast<const float4*>(rows_s + ml * RS + col + 4 * q);            \
                    v = FINISH(col + 4 * q, x0);                                                                   \
                }                                                                                                  \
                y[4 * q] = v.x; y[4 * q + 1] = v.y; y[4 * q + 2] = v.z; y[4 * q + 3] = v.w;                        \
            }                                                                                                      \
            if constexpr (AMX) amx_store16(out, sc, m, k, KT64, KQ, y, kh);                                        \
            else apb_store8(out, m, k * 2 + kh, KT, y);                                                            \
        }                                                                                                          \
    } while (0)
// one launch of an image kernel: 32 rows per workgroup, the rows' LDS stage, the kernel's cap on it
template <class... P, class... A>
static void launch_norm_image(void (*kernel)(P...), size_t lds_cap, int M, int C, hipStream_t s, A... args) {
    set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_cap);
    hipLaunchKernelGGL(kernel, dim3((M + 31) / 32), dim3(256), (size_t)32 * (C + 4) * sizeof(float), s, static_cast<P>(args)...);
}

// The row-map LayerNorm as an image.  Pass 1 keeps the wave's eight rows in registers (x[8][NQ]) for the two-pass variance;
// NQ = float4 per lane (C <= 256 NQ).
template <int NQ, bool AMX>
__global__ __launch_bounds__(256) void layernorm_apb_kernel(const float* __restrict__ in, i32x4* __restrict__ out, int64_t M, int C,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const int32_t* __restrict__ row_map, int ntok, uint8_t* __restrict__ sc) {
    extern __shared__ __attribute__((aligned(16))) float ln_rows_s[];
    __shared__ float mu_s[32], rs_s[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = C >> 2, KT = C >> 4, RS = C + 4;
    const int64_t m0 = (int64_t)blockIdx.x * 32;
    float4 x[8][NQ] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t m = m0 + wave * 8 + i;
        m = m < M ? m : M - 1;
        int64_t src = m;
        if (row_map) src = (m / ntok) * ntok + row_map[m % ntok];
        const float4* sp = reinterpret_cast<const float4*>(in + src * C);
        ROW_QUADS(NQ, q, v, x[i][q] = sp[v];)
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float4* dst = reinterpret_cast<float4*>(ln_rows_s + (wave * 8 + i) * RS);
        ROW_QUADS(NQ, q, v, dst[v] = x[i][q];)
        float mean, rstd;
        ln_stats(x[i], lane, nv, C, mean, rstd);
        if (lane == 0) { mu_s[wave * 8 + i] = mean; rs_s[wave * 8 + i] = rstd; }
    }
    __syncthreads();
    const int ml = lane & 31;
    const int64_t m = m0 + ml;
    if (m >= M) return;
    const float mean = mu_s[ml], rstd = rs_s[ml];
#define LN_FINISH(at, x4) ln_affine(x4, mean, rstd, *reinterpret_cast<const float4*>(w + at), *reinterpret_cast<const float4*>(b + at))
    NORM_IMAGE_ROWS(AMX, ln_rows_s, LN_FINISH);
#undef LN_FINISH
}
// C % 16 == 0, C <= 768 (98.8 KB of rows); out_apb holds roundup(M, 128) rows (rows >= M are left as they are: their products are
// never stored).  out_scales: AMX image + scale bytes (fp8 mode)
void launch_layernorm_apb(const float* in, void* out_apb, int M, int C, const float* w, const float* b, const int32_t* row_map,
                          int ntok, hipStream_t s, void* out_scales) {
    auto go = [&](auto kernel) { launch_norm_image(kernel, 100 * 1024, M, C, s, in, out_apb, (int64_t)M, C, w, b, row_map, ntok, out_scales); };
    if (out_scales) {
        if (C <= 256) go(layernorm_apb_kernel<1, true>); else if (C <= 512) go(layernorm_apb_kernel<2, true>); else go(layernorm_apb_kernel<3, true>);
    } else {
        if (C <= 256) go(layernorm_apb_kernel<1, false>); else if (C <= 512) go(layernorm_apb_kernel<2, false>); else go(layernorm_apb_kernel<3, false>);
    }
}

// ---- RMSNorm -----------------------------------------------------------------------------------------------------------------------
// w * (x * r) with each product rounded to fp32 on its own; the only RMS product in the tree.  It is not written with __fmul_rn: HIP's
// __fmul_rn is a plain product, so it may still be contracted with what consumes it.  split3's a - h (common.h) turned the last
// product into fma(w, x r, -h), and the three pieces then summed to the 48-bit product rounded another way -- one unit in the last
// place off the plain kernel's row in about 7 % of the elements.  With contraction off inside this function the product carries no
// contract flag and stays a product.
__device__ __forceinline__ float rms_scaled(float w, float x, float r) {
#pragma clang fp contract(off)
    const float xr = x * r;
    return w * xr;
}
__device__ __forceinline__ float4 rms_scaled4(const float4& w, const float4& x, float r) {
    return make_float4(rms_scaled(w.x, x.x, r), rms_scaled(w.y, x.y, r), rms_scaled(w.z, x.z, r), rms_scaled(w.w, x.w, r));
}
// LlamaRMSNorm (fp32): w * (x * rsqrt(mean(x^2) + eps))
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t M,
                                                      int C, const float* __restrict__ w, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * 4 + wave;
    if (m >= M) return;
    const int nv = C >> 2;
    const float4* src = reinterpret_cast<const float4*>(in + m * C);
    float4 x[LN_MAXV] = {};
    float ss = 0.f;
    ROW_QUADS(LN_MAXV, q, v, x[q] = src[v]; ss += sumsq4(x[q]);)
    const float r = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
    float4* dst = reinterpret_cast<float4*>(out + m * C);
    ROW_QUADS(LN_MAXV, q, v, dst[v] = rms_scaled4(reinterpret_cast<const float4*>(w)[v], x[q], r);)
}
void launch_rmsnorm(const float* in, float* out, int M, int C, const float* w, float eps, hipStream_t s) {
    hipLaunchKernelGGL(rmsnorm_kernel, dim3((M + 3) / 4), dim3(256), 0, s, in, out, (int64_t)M, C, w, eps);
}
// RMSNorm as an image.  Pass 1 streams the rows into LDS: all eight rows of the wave are loaded before the first reduction (rows past
// M: a clamped re-read, result unused).
template <bool AMX>
__global__ __launch_bounds__(256) void rmsnorm_apb_kernel(const float* __restrict__ in, i32x4* __restrict__ out, int64_t M,
                                                          int C, const float* __restrict__ w, float eps, uint8_t* __restrict__ sc) {
    extern __shared__ __attribute__((aligned(16))) float rows_s[];
    __shared__ float rs[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = C >> 2, KT = C >> 4, RS = C + 4;
    const int64_t m0 = (int64_t)blockIdx.x * 32;
    float ss[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t m = m0 + wave * 8 + i;
        m = m < M ? m : M - 1;
        const float4* src = reinterpret_cast<const float4*>(in + m * C);
        float4* dst = reinterpret_cast<float4*>(rows_s + (wave * 8 + i) * RS);
        ss[i] = 0.f;
        ROW_QUADS(LN_MAXV, q, v, const float4 x = src[v]; dst[v] = x; ss[i] += sumsq4(x);)
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float r = 1.0f / sqrtf(wave_sum(ss[i]) / (float)C + eps);
        if (lane == 0) rs[wave * 8 + i] = r;
    }
    __syncthreads();
    const int ml = lane & 31;
    const int64_t m = m0 + ml;
    if (m >= M) return;
    const float r = rs[ml];
#define RMS_FINISH(at, x4) rms_scaled4(*reinterpret_cast<const float4*>(w + at), x4, r)
    NORM_IMAGE_ROWS(AMX, rows_s, RMS_FINISH);
#undef RMS_FINISH
}
// C % 16 == 0, C <= 752 (96 KiB of rows; 74 KB at C = 576: two workgroups per CU)
void launch_rmsnorm_apb(const float* in, void* out_apb, int M, int C, const float* w, float eps, hipStream_t s, void* out_scales) {
    auto go = [&](auto kernel) { launch_norm_image(kernel, 96 * 1024, M, C, s, in, out_apb, (int64_t)M, C, w, eps, out_scales); };
    if (out_scales) go(rmsnorm_apb_kernel<true>); else go(rmsnorm_apb_kernel<false>);
}
#undef NORM_IMAGE_ROWS
#undef ROW_QUADS

}  // namespace mellow
