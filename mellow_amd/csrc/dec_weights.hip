// Load-time preparation of the decode weights: the fp64 composition W' Wd of the fused down + q/k/v launch, the P16 / P16N packings
// and the e4m3 copies with their row scales.  Nothing here runs in a decode step.
#include "common.h"
#include "kernels.h"

namespace mellow {

// C[M][N] (fp32) = A[M][K] . B[K][N] with fp64 products and accumulation, rounded once: the load-time composition of two
// weight matrices (W_qkv' . W_down) for dec_qkv2_kernel.  16 x 16 outputs per workgroup, operands staged through LDS.
__global__ __launch_bounds__(256) void compose_f64_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                                                          int M, int N, int K) {
    __shared__ double as[16][17], bs[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m = blockIdx.y * 16 + ty, n = blockIdx.x * 16 + tx;
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += 16) {
        as[ty][tx] = (m < M && k0 + tx < K) ? (double)A[(int64_t)m * K + k0 + tx] : 0.0;
        bs[ty][tx] = (k0 + ty < K && n < N) ? (double)B[(int64_t)(k0 + ty) * N + n] : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc += as[ty][kk] * bs[kk][tx];
        __syncthreads();
    }
    if (m < M && n < N) C[(int64_t)m * N + n] = (float)acc;
}
void launch_compose_f64(const float* A, const float* B, float* C, int M, int N, int K, hipStream_t s) {
    hipLaunchKernelGGL(compose_f64_kernel, dim3((N + 15) / 16, (M + 15) / 16), dim3(256), 0, s, A, B, C, M, N, K);
}
// fp32 packed decode weight (P-layout: 32 rows per tile, or P16: 16 rows per tile; `slots` float4 slots per tile) -> one
// 4-byte word of four e4m3 values per slot + one scale per packed row (amax / 448): one workgroup per tile
__global__ __launch_bounds__(256) void pack_dec_fp8_kernel(const float4* __restrict__ Wp, int slots, int rows, uint32_t* __restrict__ out,
                                                           float* __restrict__ scale) {
    __shared__ unsigned amax_s[32];
    __shared__ float inv_s[32];
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tid < 32) amax_s[tid] = 0u;
    __syncthreads();
    const float4* src = Wp + (int64_t)tile * slots;
    for (int i = tid; i < slots; i += 256) {
        const float4 v = src[i];
        const float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
        atomicMax(&amax_s[(i & 63) & (rows - 1)], __float_as_uint(m));          // non-negative floats order like their bit patterns
    }
    __syncthreads();
    if (tid < rows) {
        const float am = __uint_as_float(amax_s[tid]);
        const float sc = am > 0.f ? am / 448.0f : 1.0f;
        scale[(int64_t)tile * rows + tid] = sc;
        inv_s[tid] = 1.0f / sc;
    }
    __syncthreads();
    for (int i = tid; i < slots; i += 256) {
        const float4 v = src[i];
        const float inv = inv_s[(i & 63) & (rows - 1)];
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * inv, v.y * inv, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * inv, v.w * inv, w, true);
        out[(int64_t)tile * slots + i] = (uint32_t)w;
    }
}
void launch_pack_dec_fp8(const float* Wp, int tiles, int slots_per_tile, int rows_per_tile, void* out, float* scale, hipStream_t s) {
    hipLaunchKernelGGL(pack_dec_fp8_kernel, dim3(tiles), dim3(256), 0, s, reinterpret_cast<const float4*>(Wp), slots_per_tile,
                       rows_per_tile, reinterpret_cast<uint32_t*>(out), scale);
}

// P16 packing: out[nt][k16][lane][4] = W[nt*16 + (lane&15)][k16*16 + 4*(lane>>4) + j]
__global__ void pack_weight16_kernel(const float* __restrict__ w, int N, int K, float* __restrict__ out) {
    const int64_t total = (int64_t)(N / 16) * (K / 16) * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const int64_t tile = i >> 6;
        const int k16 = (int)(tile % (K / 16)), nt = (int)(tile / (K / 16));
        const int n = nt * 16 + (lane & 15), k0 = k16 * 16 + 4 * (lane >> 4);
        reinterpret_cast<float4*>(out)[i] = *reinterpret_cast<const float4*>(w + (int64_t)n * K + k0);
    }
}
// P16N packing (f32x3 gate/up): out[nt][T][half][lane][4] = W[nt*16 + (lane&15)][T*32 + 8*(lane>>4) + 4*half + j]
__global__ void pack_weight16n_kernel(const float* __restrict__ w, int N, int K, float* __restrict__ out) {
    const int64_t total = (int64_t)(N / 16) * (K / 32) * 128;            // float4 units
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63), half = (int)((i >> 6) & 1);
        const int64_t tile = i >> 7;
        const int T = (int)(tile % (K / 32)), nt = (int)(tile / (K / 32));
        const int n = nt * 16 + (lane & 15), k0 = T * 32 + 8 * (lane >> 4) + 4 * half;
        reinterpret_cast<float4*>(out)[i] = *reinterpret_cast<const float4*>(w + (int64_t)n * K + k0);
    }
}
void launch_pack_weight16n(const float* w, int N, int K, float* out, hipStream_t s) {
    const int64_t total = (int64_t)(N / 16) * (K / 32) * 128;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_weight16n_kernel, dim3(blocks), dim3(256), 0, s, w, N, K, out);
}
void launch_pack_weight16(const float* w, int N, int K, float* out, hipStream_t s) {
    const int64_t total = (int64_t)(N / 16) * (K / 16) * 64;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_weight16_kernel, dim3(blocks), dim3(256), 0, s, w, N, K, out);
}

}  // namespace mellow
