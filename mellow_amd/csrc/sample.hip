// Seeded nucleus (top-p) / temperature sampling inside the decode step (include/mellow_hip.h, mellow_generate_sampled).
//
// One 1024-thread workgroup per row holds the whole row in registers (48 values per thread, coalesced float4 loads):
//   1. z = l / T (fp32), row maximum m, first NaN index (a row with a NaN yields it: the greedy rule);
//   2. every token's softmax mass as a fixed-point integer q = rn(exp(z - m) * 2^31) and the row total S = sum q -- integer
//      sums, so the nucleus boundary depends on no summation or arrival order;
//   3. the boundary: token i is kept iff the mass strictly before it in the order (z desc, index asc) is <= top_p * S.  A
//      mass-weighted radix select over the order-preserving u32 key of z (4 passes of 8 bits, per-wave LDS histograms of
//      integer mass) finds the boundary key; ties on that key are cut by index with a second select over the index (counts);
//   4. Gumbel-max over the kept tokens: argmax (z + g), g = -log(-log u), u from Philox4x32-10 keyed by (seed) with counter
//      (index / 4, step, global row, 0); ties to the lowest index.  Noise is only formed for kept tokens.
// The loop variant then runs the step epilogue (step_tail.h) as dec_argmax_kernel (dec_tail.hip) does, which it replaces in the step.
//
// The filtered instantiation (FILT; include/mellow_hip.h, mellow_generate_filters) puts two more filters around step 3, in Hugging
// Face's order top_k, top_p, min_p:
//   3a. top_k = K: the same select with weight 1 per token and threshold K - 1 finds the K-th key and the count above it; a tie
//       group on that key larger than its share is cut by the index select.  T = the first K tokens of the order;
//   3b. the nucleus select runs over T only (every other token, the cut-off part of T's tie group included, is given z = -inf and
//       with it mass 0), so the first histogram's total is S_T and its tie counts are counts of participants;
//   3c. min_p: a token is kept iff q >= qmin = rn(min_p * 2^31); q is monotone in z, so the largest failing key is a boundary key.
// The kept set is a prefix of the order, so one (boundary key, index cut) pair describes it.  Neutral values
// (K = 0, qmin = 0) give the plain instantiation's draw, bit for bit.
#include "common.h"
#include "kernels.h"
#include "step_tail.h"

namespace mellow {

namespace {

// (the keys of this file are order_key(z) as it stands: z carries no -0, sample_row adds +0 where it forms z, and a row with a NaN
// has left before any key is formed)

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct SelScratch {
    unsigned long long hist[ROW_WAVES][256];   // per-wave histograms (integer adds: order-free)
    unsigned long long bin[256];
    uint32_t digit;
    unsigned long long above, mass;
};

// Mass-weighted radix select, descending: among the items whose key matches the prefix found so far, find the key K such
// that mass(key > K) <= thr < mass(key >= K), walking 8-bit digits from bit shift_hi down (bits above shift_hi + 8 are 0).
// thr = thr_of(total mass), formed after the first histogram; returns false (nothing selected) when thr >= total.  Then
// exactly one bin qualifies in every pass.  key_of(k, j, key) says whether element j of float4 group k takes part (and its
// key); w_of(k, j) is its weight, evaluated only for elements inside the current prefix.  Workgroup-uniform results.
template <typename KeyF, typename WF, typename ThrF>
__device__ __forceinline__ bool radix_select(KeyF key_of, WF w_of, ThrF thr_of, int shift_hi, SelScratch& sh, uint32_t& out_key,
                                             unsigned long long& out_above, unsigned long long& out_mass,
                                             unsigned long long& out_thr) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t prefix = 0, pmask = shift_hi + 8 >= 32 ? 0u : ~0u << (shift_hi + 8);
    unsigned long long above = 0, mass = 0, thr = 0;
    for (int shift = shift_hi; shift >= 0; shift -= 8) {
        for (int i = tid; i < ROW_WAVES * 256; i += ROW_THREADS) (&sh.hist[0][0])[i] = 0ull;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t key;
                if (key_of(k, j, key) && (key & pmask) == prefix) {
                    const unsigned long long w = w_of(k, j);
                    if (w) atomicAdd(&sh.hist[wave][(key >> shift) & 255u], w);
                }
            }
        __syncthreads();
        if (tid < 256) {
            unsigned long long s = 0;
            for (int w = 0; w < ROW_WAVES; ++w) s += sh.hist[w][tid];
            sh.bin[tid] = s;
        }
        __syncthreads();
        if (shift == shift_hi) {
            unsigned long long total = 0;
            for (int i = 0; i < 256; ++i) total += sh.bin[i];        // (LDS broadcast reads)
            thr = thr_of(total);
            if (thr >= total) { __syncthreads(); return false; }
        }
        if (wave == 0) {
            // lane l owns digits 255 - 4l .. 252 - 4l (descending key order)
            unsigned long long v[4], tot = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) { v[s] = sh.bin[255 - 4 * lane - s]; tot += v[s]; }
            unsigned long long inc = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long o = __shfl_up(inc, off, 64);
                if (lane >= off) inc += o;
            }
            unsigned long long run = above + (inc - tot);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (run <= thr && thr < run + v[s]) { sh.digit = 255u - 4u * lane - s; sh.above = run; sh.mass = v[s]; }
                run += v[s];
            }
        }
        __syncthreads();
        prefix |= sh.digit << shift;
        pmask |= 255u << shift;
        above = sh.above;
        mass = sh.mass;
        __syncthreads();            // (sh is rewritten by the next pass)
    }
    out_key = prefix; out_above = above; out_mass = mass; out_thr = thr;
    return true;
}

// the draw of one row: returns the token (workgroup-uniform)
template <bool FILT>
__device__ __forceinline__ int sample_row(const float* __restrict__ lrow, const uint32_t* __restrict__ prm, uint32_t grow,
                                          uint32_t step) {
    __shared__ SelScratch sh;
    __shared__ float red_f[ROW_WAVES];
    __shared__ int red_i[ROW_WAVES];
    __shared__ uint32_t qtie_s;
    const int tid = threadIdx.x;
    const uint32_t seed_lo = prm[SMP_SEED_LO], seed_hi = prm[SMP_SEED_HI];
    const float top_p = __uint_as_float(prm[SMP_TOP_P]), temp = __uint_as_float(prm[SMP_TEMP]);

    float z[ROW_NV4][4];
    int nan_idx = 0x7fffffff;
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + tid;
        const float4 v = reinterpret_cast<const float4*>(lrow)[i4];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float zz = __fdiv_rn(vv[j], temp) + 0.0f;          // (+ 0: -0 becomes +0, so equal values have equal keys)
            z[k][j] = zz;
            if (vv[j] != vv[j]) nan_idx = min(nan_idx, 4 * i4 + j);
            else m = fmaxf(m, zz);
        }
    }
    nan_idx = block_reduce(nan_idx, [](int a, int b) { return min(a, b); }, red_i);
    if (nan_idx != 0x7fffffff) return nan_idx;          // greedy rule: the first NaN (torch.argmax, dec_argmax_kernel)
    m = block_reduce(m, [](float a, float b) { return fmaxf(a, b); }, red_f);

    // fixed-point mass q = rn(exp(z - m) * 2^31) <= 2^31, so S < 2^47 is exact in fp64 for the threshold; formed where a
    // histogram pass needs it (the first pass for every token, the later ones for the few inside the prefix)
    auto q_of = [&](int k, int j) -> unsigned long long {
        const float zz = opaque(z[k][j]);
        const float e = zz == m ? 1.0f : expf(zz - m);                   // (z == m also covers m = +inf)
        return __float2uint_rn(e * 2147483648.0f);
    };
    bool keep_all = !(top_p < 1.0f);
    uint32_t kstar = 0;                  // boundary key: keys above it are kept
    int idx_cut = 0x7fffffff;            // tokens ON the boundary key are kept up to this index
    if constexpr (FILT) {
        const uint32_t top_k = prm[SMP_TOP_K], qmin = prm[SMP_QMIN];      // tokens with q < qmin are dropped (min_p)
        keep_all = true;                 // until a filter sets a boundary (every key is > 0: the neutral pair keeps all, too)
        if (top_k > 0 && top_k < (uint32_t)SAMPLE_MAX_V) {
            // T = the first top_k tokens of the order: the pair (kstar, idx_cut)
            unsigned long long above, mass, thr;
            radix_select([&](int k, int j, uint32_t& key) { key = order_key(opaque(z[k][j])); return true; }, [](int, int) { return 1ull; },
                         [top_k](unsigned long long) { return (unsigned long long)top_k - 1; }, 24, sh, kstar, above, mass, thr);
            const unsigned long long c = top_k - above;       // 1 <= c <= mass: the tie group's share
            if (c < mass) {
                uint32_t kidx;
                unsigned long long a2, m2, t2;
                radix_select([&](int k, int j, uint32_t& key) {
                                 key = 0xFFFFu - (uint32_t)(4 * (k * ROW_THREADS + opaque(tid)) + j);
                                 return order_key(opaque(z[k][j])) == kstar; },
                             [](int, int) { return 1ull; }, [c](unsigned long long) { return c - 1; }, 8, sh, kidx, a2, m2, t2);
                idx_cut = (int)(0xFFFFu - kidx);
            }
            keep_all = false;
            // every token outside T leaves the row (z = -inf: mass 0 in the nucleus below, and never on its boundary key, whose bin
            // has mass > 0), so the nucleus select and its tie counts see the participants only.  m is in T.
#pragma unroll
            for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t key = order_key(z[k][j]);
                    if (!(key > kstar || (key == kstar && 4 * (k * ROW_THREADS + tid) + j <= idx_cut))) z[k][j] = -INFINITY;
                }
        }
        if (top_p < 1.0f) {
            // the nucleus inside T: the plain select on the masked row.  A boundary it finds lies on or above T's (the tokens below
            // weigh nothing), and its tie group holds tokens of T only.
            uint32_t kp;
            unsigned long long above, mass, thr;
            if (radix_select([&](int k, int j, uint32_t& key) { key = order_key(opaque(z[k][j])); return true; }, q_of,
                             [&](unsigned long long S) { return top_p > 0.0f ? (unsigned long long)((double)top_p * (double)S) : 0ull; },
                             24, sh, kp, above, mass, thr)) {
                kstar = kp; idx_cut = 0x7fffffff; keep_all = false;
#pragma unroll
                for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (order_key(opaque(z[k][j])) == kstar) qtie_s = (uint32_t)q_of(k, j);   // (every writer stores the same value)
                __syncthreads();
                const unsigned long long qt = qtie_s;            // > 0: the boundary bin's mass exceeds thr - above >= 0
                const unsigned long long n_tie = mass / qt, c = (thr - above) / qt + 1;
                if (c < n_tie) {
                    uint32_t kidx;
                    unsigned long long a2, m2, t2;
                    radix_select([&](int k, int j, uint32_t& key) {
                                     key = 0xFFFFu - (uint32_t)(4 * (k * ROW_THREADS + opaque(tid)) + j);
                                     return order_key(opaque(z[k][j])) == kstar; },
                                 [](int, int) { return 1ull; }, [c](unsigned long long) { return c - 1; }, 8, sh, kidx, a2, m2, t2);
                    idx_cut = (int)(0xFFFFu - kidx);
                }
            }
        }
        if (qmin > 0) {
            // min_p is monotone in z: the largest key that fails q >= qmin, if it lies inside the set kept so far, ends the set above
            // it (its whole tie group carries the same q)
            uint32_t kfail = 0;
#pragma unroll
            for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t key = order_key(opaque(z[k][j]));
                    if (key >= kstar && key > kfail && q_of(k, j) < qmin) kfail = key;
                }
            kfail = block_reduce(kfail, [](uint32_t a, uint32_t b) { return a > b ? a : b; }, reinterpret_cast<uint32_t*>(red_i));
            if (kfail >= kstar && kfail > 0) { kstar = kfail; idx_cut = -1; keep_all = false; }
        }
    } else if (!keep_all) {
        unsigned long long above, mass, thr;
        keep_all = !radix_select([&](int k, int j, uint32_t& key) { key = order_key(opaque(z[k][j])); return true; }, q_of,
                                 [&](unsigned long long S) { return top_p > 0.0f ? (unsigned long long)((double)top_p * (double)S) : 0ull; },
                                 24, sh, kstar, above, mass, thr);
        if (!keep_all) {
            // the tokens on kstar all carry the same q (same z): the first c of them by index are kept
#pragma unroll
            for (int k = 0; k < ROW_NV4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (order_key(opaque(z[k][j])) == kstar) qtie_s = (uint32_t)q_of(k, j);   // (every writer stores the same value)
            __syncthreads();
            const unsigned long long qt = qtie_s;            // > 0: the boundary bin's mass exceeds thr - above >= 0
            const unsigned long long n_tie = mass / qt, c = (thr - above) / qt + 1;
            if (c < n_tie) {
                uint32_t kidx;
                unsigned long long a2, m2, t2;
                radix_select([&](int k, int j, uint32_t& key) {
                                 key = 0xFFFFu - (uint32_t)(4 * (k * ROW_THREADS + tid) + j);
                                 return order_key(opaque(z[k][j])) == kstar; },
                             [](int, int) { return 1ull; }, [c](unsigned long long) { return c - 1; }, 8, sh, kidx, a2, m2, t2);
                idx_cut = (int)(0xFFFFu - kidx);
            }
        }
    }

    // Gumbel-max over the kept tokens
    float best = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < ROW_NV4; ++k) {
        const int i4 = k * ROW_THREADS + (FILT ? opaque(tid) : tid);
        bool kept[4], any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t key = order_key(opaque(z[k][j]));
            kept[j] = (keep_all || key > kstar || (key == kstar && 4 * i4 + j <= idx_cut));
            any |= kept[j];
        }
        if (any) {
            uint32_t x[4];
            philox4x32_10((uint32_t)i4, step, grow, 0u, seed_lo, seed_hi, x);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (kept[j]) {
                    const float u = (float)(2u * (x[j] >> 9) + 1u) * 0x1p-24f;
                    const float s = z[k][j] - logf(-logf(u));
                    const int id = 4 * i4 + j;
                    if (s > best || (s == best && id < bidx)) { best = s; bidx = id; }
                }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if ((tid & 63) == 0) { red_f[tid >> 6] = best; red_i[tid >> 6] = bidx; }
    __syncthreads();
    best = red_f[0]; bidx = red_i[0];
    for (int w = 1; w < ROW_WAVES; ++w)
        if (red_f[w] > best || (red_f[w] == best && red_i[w] < bidx)) { best = red_f[w]; bidx = red_i[w]; }
    __syncthreads();
    return min(max(bidx, 0), SAMPLE_MAX_V - 1);
}

}  // namespace

// the decode step's sampler: replaces dec_argmax_kernel when sampling is on; after the draw it runs the step epilogue (step_tail.h)
// LSE (LoopArgs::out_logprob): after the draw, the row's log-sum-exp is merged from the head's (cand_val, cand_sum) partials by the
// function the arg-max kernel uses (common.h: dec_lse_max / dec_lse_sum -- the raw logits, temperature 1, no nucleus), the drawn
// token's logit is read from the logits row the head stored, and logit - lse is recorded where the token is.
template <bool LSE, bool FILT>
__global__ __launch_bounds__(ROW_THREADS) void dec_sample_kernel(const SampleArgs sa, const DecArgs a, int32_t* __restrict__ tokens,
                                                                 const float* __restrict__ embed, int write_x, const LoopArgs lp) {
    __shared__ int tok_s;
    __shared__ float lse_sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [row, dead] = step_slot(lp.row_of_slot, lp.blk_snap, b);
    int idx = 0;
    if (!dead) {
        const int step = lp.out_tokens ? *a.d_pos - lp.T0 + 1 : (int)sa.prm[SMP_STEP];
        idx = sample_row<FILT>(sa.logits + (int64_t)b * sa.ld, sa.prm, sa.prm[SMP_ROW_OFF] + ((uint32_t)row >> sa.row_shift), (uint32_t)step);
    }
    float lse = 0.f;
    if constexpr (LSE) {
        if (!dead) {            // (workgroup-uniform)
            const int n = (int)(sa.ld >> 5);
            const float M = dec_lse_max(a.cand_val + (int64_t)b * n, n, lse_sh);
            lse = dec_lse_value(M, dec_lse_sum(a.cand_val + (int64_t)b * n, a.cand_sum + (int64_t)b * n, n, M, lse_sh));
        }
    }
    if (tid == 0) {
        if (!dead) {
            tokens[b] = idx;
            tok_s = idx;
        }
        if (lp.out_tokens) {
            if (!dead) {
                if constexpr (LSE)
                    step_record(lp, a, b, row, idx, [=, logits = sa.logits, ld = sa.ld] { return logits[(int64_t)b * ld + idx] - lse; });
                else
                    step_record(lp, a, b, row, idx);
            }
            step_publish(lp, [n_seen = lp.n_seen] { return atomicAdd(n_seen, 0); });
        }
    }
    if (dead) return;
    if (write_x) {
        __syncthreads();
        if (tid < 144) step_embed_gather(embed, tok_s, a, b, tid);
    }
}

template <bool FILT>
__global__ __launch_bounds__(ROW_THREADS) void sample_logits_kernel(const SampleArgs sa, int32_t* __restrict__ tokens) {
    const int b = blockIdx.x;
    const uint32_t grow = sa.prm[SMP_ROW_OFF] + (uint32_t)(sa.row_ids ? sa.row_ids[b] : b);
    const int idx = sample_row<FILT>(sa.logits + (int64_t)b * sa.ld, sa.prm, grow, sa.prm[SMP_STEP]);
    if (threadIdx.x == 0) tokens[b] = idx;
}

void launch_dec_sample(const SampleArgs& sa, const DecArgs& a, int B, int32_t* tokens, const float* embed, int write_x,
                       const LoopArgs& loop, hipStream_t s) {
    const bool lse = loop.out_logprob != nullptr && a.cand_sum != nullptr;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B), dim3(ROW_THREADS), 0, s, sa, a, tokens, embed, write_x, loop); };
    if (sa.filtered) { if (lse) go(dec_sample_kernel<true, true>); else go(dec_sample_kernel<false, true>); }
    else { if (lse) go(dec_sample_kernel<true, false>); else go(dec_sample_kernel<false, false>); }
}

void launch_sample_logits(const SampleArgs& sa, int B, int32_t* tokens, hipStream_t s) {
    if (sa.filtered) hipLaunchKernelGGL(sample_logits_kernel<true>, dim3(B), dim3(ROW_THREADS), 0, s, sa, tokens);
    else hipLaunchKernelGGL(sample_logits_kernel<false>, dim3(B), dim3(ROW_THREADS), 0, s, sa, tokens);
}

}  // namespace mellow
