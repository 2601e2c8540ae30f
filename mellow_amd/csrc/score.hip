// Teacher-forced scoring (mellow_score / mellow_lm_score): the kernels around the fused LM head.
//   score_build_input_kernel  [prefix_b | embed(candidate)] rows of the LM input + the target ids of the scored positions
//   lse_merge_kernel          a row's per-64-column log-softmax partials (gemm_epilogue.h, EPI_LSE) -> log-prob, arg-max, lse, max
//   score_sum_kernel          per-candidate sum of the token log-probs
// The head itself is gemm_f32_kernel<..., EPI_LSE> (gemm_f32.hip): no [rows][vocab] tensor exists anywhere on this path.
#include "common.h"
#include "kernels.h"

namespace mellow {

__device__ __forceinline__ void flag_bad_id(unsigned long long* word, unsigned row, int id) {
    __hip_atomic_store(word, (1ull << 63) | ((unsigned long long)(row & 0x7fffffffu) << 32) | (unsigned)id, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(192) void score_build_input_kernel(const float* __restrict__ prefix, const float* __restrict__ embed,
                                                                const int32_t* __restrict__ cand_ids,
                                                                const int32_t* __restrict__ cand_len, int K, int L, int P, int vocab,
                                                                int row0, float* __restrict__ x, int32_t* __restrict__ targets,
                                                                unsigned long long* __restrict__ bad_word) {
    const int t = blockIdx.x, r = blockIdx.y, T = P + L - 1;
    const int64_t gr = (int64_t)row0 + r;           // row of [B][K]
    const float4* src;
    if (t < P) src = reinterpret_cast<const float4*>(prefix + ((gr / K) * P + t) * 576);
    else src = reinterpret_cast<const float4*>(embed + (int64_t)min(max(cand_ids[gr * L + (t - P)], 0), vocab - 1) * 576);
    if (threadIdx.x < 144) reinterpret_cast<float4*>(x + ((int64_t)r * T + t) * 576)[threadIdx.x] = src[threadIdx.x];
    if (t < L && threadIdx.x == 0) {                // (T >= L: the first L workgroups of a row also write its targets)
        const int id = cand_ids[gr * L + t];
        int tg = t < cand_len[gr] ? id : -1;
        if (t < cand_len[gr] && (id < 0 || id >= vocab)) { flag_bad_id(bad_word, (unsigned)gr, id); tg = -1; }
        targets[(int64_t)r * L + t] = tg;
    }
}
void launch_score_build_input(const float* prefix, const float* embed, const int32_t* cand_ids, const int32_t* cand_len, int K,
                              int L, int P, int vocab, int row0, int nr, float* x, int32_t* targets, unsigned long long* bad_word,
                              hipStream_t s) {
    hipLaunchKernelGGL(score_build_input_kernel, dim3(P + L - 1, nr), dim3(192), 0, s, prefix, embed, cand_ids, cand_len, K, L, P,
                       vocab, row0, x, targets, bad_word);
}

// One thread per row; partials are [group][row], so a wave reads consecutive rows of one group.  Two passes in ascending group
// order: the maximum with its lowest column (arg_better: NaN wins, lowest NaN column -- groups ascend, so do their columns),
// then the sum of the rescaled group sums.  A fixed order and no atomics: the result depends on the row's logits only.
__global__ __launch_bounds__(64) void lse_merge_kernel(const float2* __restrict__ part_ms, const int32_t* __restrict__ part_arg,
                                                       int64_t ld, int groups, int rows, const int32_t* __restrict__ targets,
                                                       const float* __restrict__ tgt_logit, int vocab,
                                                       float* __restrict__ out_logprob, int32_t* __restrict__ out_argmax,
                                                       float* __restrict__ out_lse, float* __restrict__ out_max,
                                                       unsigned long long* __restrict__ bad_word) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= rows) return;
    float M = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll 8                         // (the loads of eight groups in flight: one thread walks 768 of them)
    for (int g = 0; g < groups; ++g) {
        const float mg = part_ms[(int64_t)g * ld + m].x;
        const int ag = part_arg[(int64_t)g * ld + m];
        if (arg_better(mg, ag, M, arg)) { M = mg; arg = ag; }
    }
    float S = 0.f;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) {
        const float2 p = part_ms[(int64_t)g * ld + m];
        S += p.x == M ? p.y : p.y * expf(p.x - M);
    }
    const float lse = M + logf(S);
    int t = targets[m];
    if (t < -1 || t >= vocab) { flag_bad_id(bad_word, (unsigned)m, t); t = -1; }
    out_logprob[m] = t >= 0 ? tgt_logit[m] - lse : 0.f;
    if (out_argmax) out_argmax[m] = min(max(arg, 0), vocab - 1);
    if (out_lse) out_lse[m] = lse;
    if (out_max) out_max[m] = M;
}
void launch_lse_merge(const float2* part_ms, const int32_t* part_arg, int64_t ld, int groups, int rows, const int32_t* targets,
                      const float* tgt_logit, int vocab, float* out_logprob, int32_t* out_argmax, float* out_lse, float* out_max,
                      unsigned long long* bad_word, hipStream_t s) {
    hipLaunchKernelGGL(lse_merge_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, part_ms, part_arg, ld, groups, rows, targets,
                       tgt_logit, vocab, out_logprob, out_argmax, out_lse, out_max, bad_word);
}

__global__ __launch_bounds__(64) void score_sum_kernel(const float* __restrict__ logprob, const int32_t* __restrict__ cand_len,
                                                       int rows, int L, float* __restrict__ out_sum) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int n = min(cand_len[r], L);
    float s = 0.f;
    for (int j = 0; j < n; ++j) s += logprob[(int64_t)r * L + j];
    out_sum[r] = s;
}
void launch_score_sum(const float* logprob, const int32_t* cand_len, int rows, int L, float* out_sum, hipStream_t s) {
    hipLaunchKernelGGL(score_sum_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, logprob, cand_len, rows, L, out_sum);
}

}  // namespace mellow
