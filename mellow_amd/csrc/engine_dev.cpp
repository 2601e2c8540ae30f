// Developer entry points (not used by the product path): GEMM timing and debug taps, profiler dump, kernel stamps.
#include "engine_internal.h"

#include <memory>

extern "C" {

// developer instrumentation (not part of the public header): time `iters` launches of one plain GEMM shape on
// synthetic device buffers (garbage-in; EPI_LINEAR, no bias) -> average milliseconds per launch
__attribute__((visibility("default"))) int mellow_dev_gemm_time(mellow_engine_t* e, int M, int N, int K, int iters, float* ms_out) {
    if (!e || M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 4 || iters <= 0 || !ms_out) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    mellow_engine::Buf A, W, Cc;
    const size_t NP = (size_t)rup(N, 128);
    CHK(ensure(e, A, (size_t)M * K));
    CHK(ensure(e, W, NP * K));
    CHK(ensure(e, Cc, (size_t)M * N));
    HIPCHK(hipMemsetAsync(A.p, 0x3c, (size_t)M * K * 4, e->stream));      // 0x3c3c3c3c = 0.0115 (finite, non-zero)
    HIPCHK(hipMemsetAsync(W.p, 0x3c, NP * K * 4, e->stream));
    GemmArgs g;
    g.A = A.p; g.lda = K; g.M = M; g.K = K; g.Wp = W.p; g.Nw = N; g.N = N; g.C = Cc.p; g.ldc = N;
    launch_gemm(g, e->stream);
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, e->stream));
    for (int i = 0; i < iters; ++i) launch_gemm(g, e->stream);
    HIPCHK(hipEventRecord(b, e->stream));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *ms_out = ms / iters;
    hipEventDestroy(a); hipEventDestroy(b);
    return 0;
}

// one fp32 GEMM C[M][N] = A[M][K] . W[N][K]^T on host data through the exact fp32 MFMA kernel (mode 0) or the engine's f32x3
// kernels (mode 16: A split in registers; mode 17: A pre-split in APB order, both operands by LDS-DMA): the accuracy tap of
// include/mellow_hip.h
int mellow_debug_gemm_f32(mellow_engine_t* e, int mode, const float* A, int M, int K, const float* W, int N, float* C_out,
                          int iters, float* ms2) {
    if (!e || !A || !W || M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 4) return fail("bad argument");
    if (mode != 0 && mode != 16 && mode != 17) return fail("mode must be 0 (fp32 MFMA), 16 (f32x3, A split in registers) or 17 (f32x3, pre-split A, LDS-DMA)");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const int NP = rup(N, 128);
    mellow_engine::Buf bA, bW, bWp, bC, bA3, bPB;
    CHK(ensure(e, bA, (size_t)M * K));
    CHK(ensure(e, bW, (size_t)N * K));
    CHK(ensure(e, bWp, (size_t)NP * K));
    CHK(ensure(e, bC, (size_t)M * N));
    CHK(ensure(e, bA3, (size_t)rup(M, 128) * K * 6 / 4));      // 6 bytes per element (the three bf16 pieces)
    CHK(ensure(e, bPB, (size_t)NP * K * 6 / 4));
    float *dA = bA.p, *dW = bW.p, *dWp = bWp.p, *dC = bC.p;
    void *dA3 = bA3.p, *dPB = bPB.p;
    HIPCHK(hipMemcpy(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dW, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
    launch_pack_weight(dW, N, K, K, dWp, NP, K, s);
    launch_pack_bf16x3(dWp, NP, K, dPB, s);
    GemmArgs g;
    g.A = dA; g.lda = K; g.M = M; g.K = K; g.Wp = dWp; g.Nw = N; g.N = N; g.C = dC; g.ldc = N;
    g.A8 = reinterpret_cast<const uint8_t*>(dA3); g.lda8 = (int64_t)3 * (K >> 3); g.W8 = reinterpret_cast<const uint8_t*>(dPB);
    auto run = [&](bool pre, bool main) {
        if (mode == 0) { if (main) launch_gemm(g, s); }
        else if (mode == 16) { if (main) launch_gemm_bf16x3_fused(g, s); }
        else { if (pre) launch_split_rows_apb(dA, K, M, K, dA3, s); if (main) launch_gemm_bf16x3_apb(g, s); }
    };
    run(true, true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (C_out) HIPCHK(hipMemcpy(C_out, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    if (ms2 && iters > 0) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        float m0 = 0.f, m1 = 0.f;
        HIPCHK(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) run(true, false);
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&m0, a, b));
        HIPCHK(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) run(false, true);
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&m1, a, b));
        ms2[0] = m0 / iters;
        ms2[1] = m1 / iters;
        hipEventDestroy(a); hipEventDestroy(b);
    }
    return 0;
}

// one fp8 GEMM C[M][N] = A[M][K] . W[N][K]^T on host data (quantise rows, pack + quantise weight, fp8 MFMA GEMM,
// plain epilogue) and, optionally, its average time: the quantisation parity tap of include/mellow_hip.h
int mellow_debug_gemm_fp8(mellow_engine_t* e, const float* A, int M, int K, const float* W, int N, float* C_out, int iters,
                        float* ms_out) {
    if (!e || !A || !W || M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 4) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const int NP = rup(N, 128), K64 = rup(K, 64), Mp = rup(M, 128);
    mellow_engine::Buf bA, bW, bWp, bC, bsa, bsw, bA8, bW8;
    CHK(ensure(e, bA, (size_t)M * K));
    CHK(ensure(e, bW, (size_t)N * K));
    CHK(ensure(e, bWp, (size_t)NP * K));
    CHK(ensure(e, bC, (size_t)M * N));
    CHK(ensure(e, bsa, (size_t)Mp * ((K64 / 64 + 3) / 4) * 2));       // 2 scale words per row and four k64 steps
    CHK(ensure(e, bsw, (size_t)NP));
    CHK(ensure(e, bA8, (size_t)Mp * K64 / 4));                        // one byte per element (Mp, NP and K64 are multiples of 64)
    CHK(ensure(e, bW8, (size_t)NP * K64 / 4));
    float *dA = bA.p, *dW = bW.p, *dWp = bWp.p, *dC = bC.p, *dsa = bsa.p, *dsw = bsw.p;
    uint8_t *dA8 = reinterpret_cast<uint8_t*>(bA8.p), *dW8 = reinterpret_cast<uint8_t*>(bW8.p);
    HIPCHK(hipMemcpy(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dW, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
    launch_pack_weight(dW, N, K, K, dWp, NP, K, s);
    launch_pack_fp8(dWp, NP, K, dW8, dsw, s);
    GemmArgs g;
    g.A = dA; g.lda = K; g.M = M; g.K = K; g.Wp = dWp; g.Nw = N; g.N = N; g.C = dC; g.ldc = N;
    g.A8 = dA8; g.lda8 = K64; g.a_sc = reinterpret_cast<const uint32_t*>(dsa); g.W8 = dW8; g.w_scale = dsw;
    launch_quant_mx8(dA, K, M, K, dA8, dsa, s);
    launch_gemm_fp8(g, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (C_out) HIPCHK(hipMemcpy(C_out, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    if (ms_out && iters > 0) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        float ms_q = 0.f, ms_g = 0.f;
        HIPCHK(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) launch_quant_mx8(dA, K, M, K, dA8, dsa, s);
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&ms_q, a, b));
        HIPCHK(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) launch_gemm_fp8(g, s);
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&ms_g, a, b));
        ms_out[0] = ms_q / iters;
        ms_out[1] = ms_g / iters;
        hipEventDestroy(a); hipEventDestroy(b);
    }
    return 0;
}

// ---- attention taps on host data (include/mellow_hip.h): one launch of an existing launcher on buffers of the call's own ------------
// what the two taps share: the output buffer, filled with 0xFF bytes before the launch and returned whole
struct AttnTapOut {
    mellow_engine::Buf buf;
    size_t bytes = 0;
};
// plain form: M + 32 rows of `width` floats; APB form: the image of rup(M, 128) rows, 6 bytes per element
static int attn_tap_out(mellow_engine* e, AttnTapOut& o, int64_t M, int width, int out_form, int64_t out_capacity) {
    o.bytes = out_form ? (size_t)rup((int)M, 128) * width * 6 : (size_t)(M + 32) * width * 4;
    if (out_capacity < (int64_t)o.bytes) return fail("out_capacity %lld is below the %lld bytes this call returns", (long long)out_capacity, (long long)o.bytes);
    CHK(ensure(e, o.buf, (o.bytes + 3) / 4));
    HIPCHK(hipMemsetAsync(o.buf.p, 0xFF, o.bytes, e->stream));
    return 0;
}
static int attn_tap_finish(mellow_engine* e, const AttnTapOut& o, void* out) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, o.buf.p, o.bytes, hipMemcpyDeviceToHost));
    return 0;
}
// n host floats -> a device buffer; to16: then rounded to bf16 by launch_kv_to_bf16 into a second buffer, which *dev then addresses
static int attn_tap_in(mellow_engine* e, mellow_engine::Buf& b32, mellow_engine::Buf& b16, const float* src, size_t n, bool to16, const float** dev) {
    CHK(ensure(e, b32, n));
    HIPCHK(hipMemcpy(b32.p, src, n * 4, hipMemcpyHostToDevice));
    *dev = b32.p;
    if (to16) {
        CHK(ensure(e, b16, (n + 1) / 2));
        launch_kv_to_bf16(b32.p, b16.p, (int64_t)n, e->stream);
        *dev = b16.p;
    }
    return 0;
}

int mellow_debug_prefill_attn(mellow_engine_t* e, int variant, const float* q, const float* k, const float* v, int B, int T, int Tmax,
                              int qpos0, int out_form, void* out, int64_t out_capacity) {
    if (!e || !q || !k || !v || !out) return fail("null argument");
    if (variant < 0 || variant > 3) return fail("variant must be 0 (fp32 MFMA), 1 (f32x3), 2 (bf16 once, fp32 pages) or 3 (bf16 once, bf16 pages): got %d", variant);
    if (out_form != 0 && out_form != 1) return fail("out_form must be 0 (fp32 rows) or 1 (APB image): got %d", out_form);
    if (B < 1 || T < 1 || B > 1024 || Tmax > 65536) return fail("B = %d, T = %d, Tmax = %d: 1 <= B <= 1024, 1 <= T, Tmax <= 65536", B, T, Tmax);
    if (Tmax < T) return fail("Tmax = %d is below T = %d", Tmax, T);
    if (qpos0 < 0 || qpos0 % 32 != 0 || qpos0 >= T) return fail("qpos0 = %d must be a multiple of 32 in [0, T = %d)", qpos0, T);
    if (qpos0 > 0 && variant >= 2) return fail("the launch with a past exists for variants 0 and 1 only (got variant %d, qpos0 = %d)", variant, qpos0);
    if (out_form == 1 && variant >= 2) return fail("the APB output form is launched for variants 0 and 1 only (got variant %d)", variant);
    const int64_t M = (int64_t)B * (T - qpos0);
    if (M > (1 << 22)) return fail("B * (T - qpos0) = %lld rows exceed the tap's %d", (long long)M, 1 << 22);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const bool p16 = variant == 3;
    const size_t page_floats = (size_t)B * 3 * Tmax * 64;
    mellow_engine::Buf bq, bk, bv, bq16, bk16, bv16;
    const float *dq, *dk, *dv;
    CHK(attn_tap_in(e, bq, bq16, q, (size_t)M * 576, p16, &dq));
    CHK(attn_tap_in(e, bk, bk16, k, page_floats, p16, &dk));
    CHK(attn_tap_in(e, bv, bv16, v, page_floats, p16, &dv));
    AttnTapOut o;
    CHK(attn_tap_out(e, o, M, 576, out_form, out_capacity));
    float* o_rows = out_form ? nullptr : o.buf.p;
    void* o_apb = out_form ? o.buf.p : nullptr;
    if (qpos0 > 0) launch_prefill_attention_past(dq, dk, dv, o_rows, o_apb, B, T, Tmax, qpos0, variant == 1, s);
    else launch_prefill_attention(dq, dk, dv, o_rows, o_apb, B, T, Tmax, variant >= 1, s, nullptr, variant >= 2, p16);
    return attn_tap_finish(e, o, out);
}

int mellow_debug_window_attn(mellow_engine_t* e, const float* qkv, int M, int C, int nH, const float* bias, const float* mask, int nW,
                             int in16, int out_form, void* out, int64_t out_capacity) {
    if (!e || !qkv || !bias || !out) return fail("null argument");
    if (out_form != 0 && out_form != 1) return fail("out_form must be 0 (fp32 rows) or 1 (APB image): got %d", out_form);
    if (M < 64 || M % 64 != 0 || M > (1 << 22)) return fail("M = %d must be a positive multiple of 64 (whole windows), at most %d", M, 1 << 22);
    if (nH != 4 && nH != 8 && nH != 16 && nH != 32) return fail("nH = %d is not a head count of the encoder (4, 8, 16, 32)", nH);
    if (C != 24 * nH) return fail("C = %d is not 24 * nH = %d", C, 24 * nH);
    if (mask && nW <= 0) return fail("a mask needs nW >= 1 (got %d)", nW);
    if (in16 && out_form == 1) return fail("the engine never launches the bf16-input kernel with the APB output form");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    mellow_engine::Buf bx, bx16, bb, bm;
    const float* dx;
    CHK(attn_tap_in(e, bx, bx16, qkv, (size_t)M * 3 * C, in16 != 0, &dx));
    CHK(ensure(e, bb, (size_t)nH * 64 * 64));
    HIPCHK(hipMemcpy(bb.p, bias, (size_t)nH * 64 * 64 * 4, hipMemcpyHostToDevice));
    if (mask) {
        CHK(ensure(e, bm, (size_t)nW * 64 * 64));
        HIPCHK(hipMemcpy(bm.p, mask, (size_t)nW * 64 * 64 * 4, hipMemcpyHostToDevice));
    }
    AttnTapOut o;
    CHK(attn_tap_out(e, o, M, C, out_form, out_capacity));
    launch_window_attention(dx, out_form ? nullptr : o.buf.p, M, C, nH, bb.p, mask ? bm.p : nullptr, mask ? nW : 1, s, out_form ? o.buf.p : nullptr,
                            in16 != 0);
    return attn_tap_finish(e, o, out);
}

// ---- GEMM epilogue tap on host data (include/mellow_hip.h): one launch of a GEMM launcher with the epilogue the caller describes ------
// a device buffer of `bytes` bytes, filled with 0xFF or loaded from `src`
static int gemm_tap_buf(mellow_engine* e, mellow_engine::Buf& b, size_t bytes, const void* src) {
    CHK(ensure(e, b, (bytes + 3) / 4 + 4));
    if (src) HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    else HIPCHK(hipMemsetAsync(b.p, 0xFF, bytes, e->stream));
    return 0;
}
static int gemm_tap_fetch(void* out, int64_t capacity, const mellow_engine::Buf& b, size_t bytes, const char* name) {
    if (!out) return fail("%s is null: this launch writes %lld bytes there", name, (long long)bytes);
    if (capacity < (int64_t)bytes) return fail("%s_capacity %lld is below the %lld bytes this call returns", name, (long long)capacity, (long long)bytes);
    HIPCHK(hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int mellow_debug_gemm_epi(mellow_engine_t* e, const mellow_gemm_epi_t* d, const float* A, const float* W, const float* bias,
                          const float* resid, const int32_t* crow_map, const float* rs_ssq, const float* rope_cos, const float* rope_sin,
                          void* out_c, int64_t c_capacity, void* out_c3, int64_t c3_capacity, float* out_ssq, int64_t ssq_capacity,
                          float* out_q, int64_t q_capacity, float* out_k, float* out_v, int64_t kv_capacity) {
    if (!e || !d || !A || !W) return fail("null argument");
    if (d->size != (int32_t)sizeof(mellow_gemm_epi_t)) return fail("size = %d is not sizeof(mellow_gemm_epi_t) = %d", d->size, (int)sizeof(mellow_gemm_epi_t));
    const int kernel = d->kernel, M = d->M, K = d->K, Nw = d->Nw, N = d->N;
    const bool lin_ = d->epi == 0, swi = d->epi == 1, qkv = d->epi == 2;
    if (kernel != 0 && kernel != 16 && kernel != 17) return fail("kernel must be 0 (fp32 MFMA), 16 (f32x3, A split in registers) or 17 (f32x3, pre-split A, LDS-DMA): got %d", kernel);
    if (!lin_ && !swi && !qkv) return fail("epi must be 0 (linear), 1 (swiglu) or 2 (qkv-rope): got %d", d->epi);
    if (M < 1 || M > (1 << 22)) return fail("M = %d: 1 <= M <= %d", M, 1 << 22);
    if (K < 1 || K > 65536) return fail("K = %d: 1 <= K <= 65536", K);
    if (kernel != 17 && K % 32 != 0) return fail("K = %d must be a multiple of 32 for kernel %d", K, kernel);
    if (kernel == 17 && K % 16 != 0) return fail("K = %d must be a multiple of 16 for kernel 17", K);
    if (kernel == 17 && K < 48) return fail("K = %d is below the 48 (three k16 stages) kernel 17 needs", K);
    if (Nw < 1 || Nw > 65536) return fail("Nw = %d: 1 <= Nw <= 65536", Nw);
    if (swi) {
        if (Nw % 2 != 0 || N != Nw / 2 || N % 4 != 0) return fail("swiglu: Nw = %d counts gate + up rows and N = %d must be Nw / 2, a multiple of 4", Nw, N);
    } else if (N % 4 != 0 || N < rup(Nw, 4) || N > rup(Nw, 128)) {
        return fail("N = %d must be a multiple of 4 with rup(Nw, 4) = %d <= N <= rup(Nw, 128) = %d", N, rup(Nw, 4), rup(Nw, 128));
    }
    if ((int64_t)M * K > (1 << 28) || (int64_t)rup(Nw, 128) * K > (1 << 27)) return fail("M * K = %lld or rup(Nw, 128) * K = %lld exceeds the tap's 2^28 / 2^27 elements", (long long)M * K, (long long)rup(Nw, 128) * K);
    if (d->want_c3 && kernel == 0) return fail("want_c3: kernel 0 hands nothing over in APB order");
    if (d->splitk_max && kernel == 0) return fail("splitk_max: kernel 0 has no split-K");
    if (d->splitk_max < 0 || d->splitk_max == 1 || d->splitk_max > 64) return fail("splitk_max = %d: 0 (no workspace) or 2 .. 64", d->splitk_max);
    if (d->want_ssq && !(lin_ && d->want_c3)) return fail("want_ssq needs want_c3 with the linear epilogue");
    if (d->want_c3 && lin_ && N % 64 != 0) return fail("want_c3 with the linear epilogue needs N %% 64 == 0 (N = %d)", N);
    if (d->want_c3 && swi && N % 16 != 0) return fail("want_c3 with swiglu needs N %% 16 == 0 (N = %d)", N);
    if (d->want_c3 && qkv) return fail("want_c3: the qkv-rope epilogue hands nothing over in APB order");
    const bool has_rs = rs_ssq != nullptr;
    if (has_rs && (d->rs_parts < 1 || d->rs_parts > 64 || !(d->rs_dim > 0.f) || !(d->rs_eps >= 0.f)))
        return fail("rs_ssq needs 1 <= rs_parts <= 64, rs_dim > 0, rs_eps >= 0 (got %d, %g, %g)", d->rs_parts, d->rs_dim, d->rs_eps);
    int64_t c_rows = M;
    int64_t ldc = N;
    if (lin_) {
        if (d->act < 0 || d->act > 2) return fail("act must be 0 (none), 1 (GELU) or 2 (sigmoid): got %d", d->act);
        if (d->resid < 0 || d->resid > 2) return fail("resid must be 0 (none), 1 (a separate buffer) or 2 (in place): got %d", d->resid);
        if (d->resid && !resid) return fail("resid = %d without a residual array", d->resid);
        if (d->bias && !bias) return fail("bias is set without a bias array");
        if (!d->want_c && !d->want_c3) return fail("want_c and want_c3 are both 0: the launch would store nothing");
        if (d->resid == 2 && !d->want_c) return fail("resid = 2 (in place) needs want_c");
        ldc = d->ldc;
        if (ldc < N || ldc % 4 != 0 || ldc > 4 * 65536) return fail("ldc = %lld must be a multiple of 4, >= N = %d", (long long)ldc, N);
        if (crow_map) {
            if (d->rows_in < 1 || d->rows_out < d->rows_in || M % d->rows_in != 0)
                return fail("crow_map needs 1 <= rows_in <= rows_out and M %% rows_in == 0 (rows_in = %d, rows_out = %d, M = %d)", d->rows_in, d->rows_out, M);
            std::vector<char> seen(d->rows_out, 0);
            for (int i = 0; i < d->rows_in; ++i) {
                if (crow_map[i] < 0 || crow_map[i] >= d->rows_out || seen[crow_map[i]]) return fail("crow_map[%d] = %d is outside [0, rows_out = %d) or taken twice", i, crow_map[i], d->rows_out);
                seen[crow_map[i]] = 1;
            }
            c_rows = (int64_t)(M / d->rows_in) * d->rows_out;
        }
    } else if (swi) {
        if (!d->want_c && !d->want_c3) return fail("want_c and want_c3 are both 0: the launch would store nothing");
        if (d->want_c && d->want_c3) return fail("swiglu writes C or the APB image, never both: want_c and want_c3 are both set");
    }
    int B = 0, Tq = 0;
    if (qkv) {
        if (Nw != 960 || N != 960) return fail("qkv-rope has 9 query and 3 kv heads of 64: Nw = N = 960 (got Nw = %d, N = %d)", Nw, N);
        if (d->T < 1 || d->Tmax > 65536) return fail("T = %d, Tmax = %d: 1 <= T, Tmax <= 65536", d->T, d->Tmax);
        if (d->Tmax < d->T) return fail("Tmax = %d is below T = %d", d->Tmax, d->T);
        if (d->pos0 < 0 || d->pos0 >= d->T) return fail("pos0 = %d must lie in [0, T = %d)", d->pos0, d->T);
        Tq = d->T - d->pos0;
        if (M % Tq != 0) return fail("M = %d is not B * (T - pos0) = B * %d", M, Tq);
        B = M / Tq;
        if (B > 1024) return fail("M / (T - pos0) = %d examples exceed the tap's 1024", B);
        if ((rope_cos == nullptr) != (rope_sin == nullptr)) return fail("rope_cos and rope_sin come together or not at all");
    }
    // capacities, before anything is launched
    const size_t c_bytes = (size_t)(c_rows + 32) * ldc * 4;
    const int parts = N / 64;
    const size_t c3_bytes = (size_t)rup(M, 128) * N * 6, ssq_bytes = (size_t)(M + 32) * (parts > 0 ? parts : 1) * 4;
    const size_t q_bytes = (size_t)(M + 32) * 576 * 4, kv_bytes = (size_t)(B + 1) * 3 * d->Tmax * 64 * 4;      // one page set of no example behind the last
    const bool wc = !qkv && d->want_c, wc3 = !qkv && d->want_c3, wssq = lin_ && d->want_ssq;
    if (wc && (!out_c || c_capacity < (int64_t)c_bytes)) return fail("c_capacity %lld is below the %lld bytes this call returns (or out_c is null)", (long long)c_capacity, (long long)c_bytes);
    if (wc3 && (!out_c3 || c3_capacity < (int64_t)c3_bytes)) return fail("c3_capacity %lld is below the %lld bytes this call returns (or out_c3 is null)", (long long)c3_capacity, (long long)c3_bytes);
    if (wssq && (!out_ssq || ssq_capacity < (int64_t)ssq_bytes)) return fail("ssq_capacity %lld is below the %lld bytes this call returns (or out_ssq is null)", (long long)ssq_capacity, (long long)ssq_bytes);
    if (qkv && (!out_q || q_capacity < (int64_t)q_bytes)) return fail("q_capacity %lld is below the %lld bytes this call returns (or out_q is null)", (long long)q_capacity, (long long)q_bytes);
    if (qkv && (!out_k || !out_v || kv_capacity < (int64_t)kv_bytes)) return fail("kv_capacity %lld is below the %lld bytes each page array takes (or out_k / out_v is null)", (long long)kv_capacity, (long long)kv_bytes);

    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const int Nrows = swi ? Nw / 2 : Nw;                 // rows of one logical weight matrix
    const int Nwp = swi ? 64 * ((Nrows + 31) / 32) : Nw;      // packed rows: pairs come in 64-row groups of 32 gate + 32 up
    const int NP = rup(Nwp, 128);
    mellow_engine::Buf bA, bW, bWp, bPB, bA3, bBias, bRes, bMap, bRs, bC, bC3, bSsq, bQ, bKc, bVc, bCos, bSin;
    CHK(gemm_tap_buf(e, bA, (size_t)M * K * 4, A));
    CHK(gemm_tap_buf(e, bW, (size_t)Nw * K * 4, W));
    CHK(ensure(e, bWp, (size_t)NP * K));
    if (swi) launch_pack_weight_pairs(bW.p, bW.p + (size_t)Nrows * K, Nrows, K, K, bWp.p, NP, K, s);
    else launch_pack_weight(bW.p, Nw, K, K, bWp.p, NP, K, s);
    GemmArgs g;
    g.A = bA.p; g.lda = K; g.M = M; g.K = K; g.Wp = bWp.p; g.Nw = Nwp; g.N = N; g.ldc = ldc;
    g.epi = lin_ ? EPI_LINEAR : swi ? EPI_SWIGLU : d->pos0 > 0 ? EPI_QKV_ROPE_AT : EPI_QKV_ROPE;
    if (kernel != 0) {
        CHK(ensure(e, bPB, (size_t)NP * K * 6 / 4));
        launch_pack_bf16x3(bWp.p, NP, K, bPB.p, s);
        g.W8 = reinterpret_cast<const uint8_t*>(bPB.p);
    }
    if (kernel == 17) {
        CHK(ensure(e, bA3, (size_t)rup(M, 128) * K * 6 / 4));
        g.A8 = reinterpret_cast<const uint8_t*>(bA3.p); g.lda8 = (int64_t)3 * (K >> 3);
    }
    if (has_rs) {
        CHK(gemm_tap_buf(e, bRs, (size_t)M * d->rs_parts * 4, rs_ssq));
        g.rs_ssq = bRs.p; g.rs_parts = d->rs_parts; g.rs_dim = d->rs_dim; g.rs_eps = d->rs_eps;
    }
    if (wc) { CHK(gemm_tap_buf(e, bC, c_bytes, nullptr)); g.C = bC.p; }
    if (wc3) { CHK(gemm_tap_buf(e, bC3, c3_bytes, nullptr)); g.C3 = bC3.p; }
    if (wssq) { CHK(gemm_tap_buf(e, bSsq, ssq_bytes, nullptr)); g.ssq_out = bSsq.p; g.ssq_parts = parts; }
    if (lin_) {
        g.act = d->act;
        if (d->bias) {           // the launchers read whole float4 of columns < N: the columns past Nw hold zeros, as the engine's padded biases do
            std::vector<float> hb(rup(N, 128), 0.f);
            memcpy(hb.data(), bias, (size_t)Nw * 4);
            CHK(gemm_tap_buf(e, bBias, hb.size() * 4, hb.data()));
            g.bias = bBias.p;
        }
        if (crow_map) {
            CHK(gemm_tap_buf(e, bMap, (size_t)d->rows_in * 4, crow_map));
            g.crow_map = reinterpret_cast<const int32_t*>(bMap.p); g.rows_in = d->rows_in; g.rows_out = d->rows_out;
        }
        if (d->resid == 1) {                                // resid host [c_rows][N]
            CHK(gemm_tap_buf(e, bRes, (size_t)c_rows * N * 4, resid));
            g.resid = bRes.p; g.ldr = N;
        } else if (d->resid == 2) {                         // in place: the residual is loaded into C after the fill
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy2D(bC.p, (size_t)ldc * 4, resid, (size_t)N * 4, (size_t)N * 4, (size_t)c_rows, hipMemcpyHostToDevice));
            g.resid = bC.p; g.ldr = ldc;
        }
    }
    if (qkv) {
        CHK(gemm_tap_buf(e, bQ, q_bytes, nullptr));
        CHK(gemm_tap_buf(e, bKc, kv_bytes, nullptr));
        CHK(gemm_tap_buf(e, bVc, kv_bytes, nullptr));
        std::vector<float> hc, hs;
        if (!rope_cos) {
            hc.resize((size_t)d->Tmax * 32); hs.resize((size_t)d->Tmax * 32);
            CHK(mellow_host_rope_tables(e->cfg.rope_theta, 64, d->Tmax, hc.data(), hs.data()));
        }
        CHK(gemm_tap_buf(e, bCos, (size_t)d->Tmax * 32 * 4, rope_cos ? rope_cos : hc.data()));
        CHK(gemm_tap_buf(e, bSin, (size_t)d->Tmax * 32 * 4, rope_sin ? rope_sin : hs.data()));
        g.q_out = bQ.p; g.k_cache = bKc.p; g.v_cache = bVc.p; g.rope_cos = bCos.p; g.rope_sin = bSin.p;
        g.T = Tq; g.Tmax = d->Tmax; g.pos0 = d->pos0; g.q_heads = 9; g.kv_heads = 3;
    }
    if (d->splitk_max) {         // the engine's own workspace, as with_splitk hands it to the encoder chain
        CHK(ensure(e, e->sk_ws, (size_t)512 * 16384));
        g.sk_ws = e->sk_ws.p; g.sk_tiles = 256; g.sk_max = d->splitk_max;
    }
    g.no_x3w = d->no_x3w != 0;
    if (kernel == 0) launch_gemm(g, s);
    else if (kernel == 16) launch_gemm_bf16x3_fused(g, s);
    else { launch_split_rows_apb(bA.p, K, M, K, bA3.p, s); launch_gemm_bf16x3_apb(g, s); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (wc) CHK(gemm_tap_fetch(out_c, c_capacity, bC, c_bytes, "c"));
    if (wc3) CHK(gemm_tap_fetch(out_c3, c3_capacity, bC3, c3_bytes, "c3"));
    if (wssq) CHK(gemm_tap_fetch(out_ssq, ssq_capacity, bSsq, ssq_bytes, "ssq"));
    if (qkv) {
        CHK(gemm_tap_fetch(out_q, q_capacity, bQ, q_bytes, "q"));
        CHK(gemm_tap_fetch(out_k, kv_capacity, bKc, kv_bytes, "kv"));
        CHK(gemm_tap_fetch(out_v, kv_capacity, bVc, kv_bytes, "kv"));
    }
    return 0;
}

// ---- norm / hand-over tap on host data (include/mellow_hip.h): one launch of a norm launcher, of launch_split_rows_apb or of
// launch_quant_mx8 on the caller's rows ------------------------------------------------------------------------------------------------
int mellow_debug_norm(mellow_engine_t* e, int op, int form, const float* x, int M, int C, const float* w, const float* b, float eps,
                      const int32_t* row_map, int ntok, int n, int R, void* out, int64_t out_capacity, void* out_scales,
                      int64_t scales_capacity) {
    if (!e) return fail("null argument");
    if (op < 0 || op > 3) return fail("op must be 0 (LayerNorm), 1 (merge-LayerNorm), 2 (RMSNorm) or 3 (no norm): got %d", op);
    if (form < 0 || form > 2) return fail("form must be 0 (fp32 rows), 1 (APB image) or 2 (AMX image + scale bytes): got %d", form);
    if (op == 1 && form != 0) return fail("merge-LayerNorm has the fp32 form only (got form %d)", form);
    if (op == 3 && form == 0) return fail("op 3 (no norm) has the APB and AMX forms only: form 0 would launch nothing");
    if (C < 4 || C % 4 != 0) return fail("C = %d must be a positive multiple of 4", C);
    int64_t rows = M;              // output rows
    int width = C;                 // output columns
    if (op == 1) {
        if (n < 1 || R < 2 || R % 2 != 0 || R > 4096) return fail("merge-LayerNorm needs n >= 1 and an even R in [2, 4096] (n = %d, R = %d)", n, R);
        rows = (int64_t)n * (R / 2) * (R / 2);
        width = 4 * C;
        if (rows != M) return fail("M = %d is not n * (R / 2)^2 = %lld", M, (long long)rows);
    }
    if (M < 1 || rows > (1 << 22)) return fail("M = %lld: 1 <= M <= %d", (long long)rows, 1 << 22);
    if (rows * width > (1 << 28)) return fail("M * C = %lld exceeds the tap's 2^28 elements", (long long)(rows * width));
    if (form == 0 && width > 1536) return fail("%d columns exceed the 1536 (LN_MAXV) a row-per-wave norm kernel holds", width);
    if ((op == 0 || op == 2) && form != 0 && (C % 16 != 0 || C > 768)) return fail("C = %d: the APB / AMX norm kernels need C %% 16 == 0 and C <= 768", C);
    if (op == 2 && form != 0 && (size_t)32 * (C + 4) * 4 > (size_t)96 * 1024)
        return fail("C = %d: launch_rmsnorm_apb stages 32 rows of C + 4 floats in the 96 KiB of LDS it asks for (C <= 752)", C);
    if (op == 3 && form == 1 && C % 16 != 0) return fail("C = %d must be a multiple of 16 for launch_split_rows_apb", C);
    if (!x || !out) return fail("null argument");
    if (op != 3 && !w) return fail("w is null");
    if (op <= 1 && !b) return fail("b is null: LayerNorm has a bias");
    if (op == 2 && !(eps >= 0.f && eps < INFINITY)) return fail("eps = %g must be finite and >= 0", eps);
    if (row_map) {
        if (op != 0) return fail("row_map goes with op 0 (LayerNorm) only");
        if (ntok < 1 || M % ntok != 0) return fail("row_map needs ntok >= 1 and M %% ntok == 0 (ntok = %d, M = %d)", ntok, M);
        std::vector<char> seen(ntok, 0);
        for (int i = 0; i < ntok; ++i) {
            if (row_map[i] < 0 || row_map[i] >= ntok || seen[row_map[i]]) return fail("row_map[%d] = %d is outside [0, ntok = %d) or taken twice: not a permutation", i, row_map[i], ntok);
            seen[row_map[i]] = 1;
        }
    }
    // capacities, before anything is launched
    const int KT64 = (C + 63) / 64, KQ = (KT64 + 3) / 4;
    const size_t Mp = (size_t)rup((int)rows, 128);
    const size_t out_bytes = form == 0 ? (size_t)(rows + 32) * width * 4 : form == 1 ? Mp * C * 6 : Mp * rup(C, 64);
    const size_t sc_bytes = form == 2 ? Mp * 8 * KQ : 0;
    if (out_capacity < (int64_t)out_bytes) return fail("out_capacity %lld is below the %lld bytes this call returns", (long long)out_capacity, (long long)out_bytes);
    if (form == 2 && (!out_scales || scales_capacity < (int64_t)sc_bytes))
        return fail("scales_capacity %lld is below the %lld bytes this call returns (or out_scales is null)", (long long)scales_capacity, (long long)sc_bytes);

    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    mellow_engine::Buf bx, bw, bb, bmap, bo, bsc;
    const size_t in_floats = op == 1 ? (size_t)n * R * R * C : (size_t)M * C;
    CHK(gemm_tap_buf(e, bx, in_floats * 4, x));
    if (w) CHK(gemm_tap_buf(e, bw, (size_t)width * 4, w));
    if (b && op <= 1) CHK(gemm_tap_buf(e, bb, (size_t)width * 4, b));
    if (row_map) CHK(gemm_tap_buf(e, bmap, (size_t)ntok * 4, row_map));
    CHK(gemm_tap_buf(e, bo, out_bytes, nullptr));
    if (form == 2) CHK(gemm_tap_buf(e, bsc, sc_bytes, nullptr));
    const int32_t* dmap = row_map ? reinterpret_cast<const int32_t*>(bmap.p) : nullptr;
    const int nt = row_map ? ntok : M;
    void* dsc = form == 2 ? bsc.p : nullptr;
    if (op == 0) {
        if (form == 0) launch_layernorm(bx.p, bo.p, M, C, bw.p, bb.p, dmap, nt, s);
        else launch_layernorm_apb(bx.p, bo.p, M, C, bw.p, bb.p, dmap, nt, s, dsc);
    } else if (op == 1) {
        launch_merge_layernorm(bx.p, bo.p, n, R, C, bw.p, bb.p, s);
    } else if (op == 2) {
        if (form == 0) launch_rmsnorm(bx.p, bo.p, M, C, bw.p, eps, s);
        else launch_rmsnorm_apb(bx.p, bo.p, M, C, bw.p, eps, s, dsc);
    } else {
        if (form == 1) launch_split_rows_apb(bx.p, C, M, C, bo.p, s);
        else launch_quant_mx8(bx.p, C, M, C, bo.p, dsc, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    CHK(gemm_tap_fetch(out, out_capacity, bo, out_bytes, "out"));
    if (form == 2) CHK(gemm_tap_fetch(out_scales, scales_capacity, bsc, sc_bytes, "scales"));
    return 0;
}

// ---- decode attention tap on host data (include/mellow_hip.h): one launch_dec_attn and, with Wo, one launch_dec_oproj on DecArgs
// filled from buffers of the call's own ------------------------------------------------------------------------------------------------
// host rows [n][B][width] -> device rows [n][rows][width], the slots B .. rows - 1 zero
static int dec_tap_rows(mellow_engine* e, mellow_engine::Buf& b, const float* src, int n, int B, int rows, int width, size_t extra_rows = 0) {
    std::vector<float> h(((size_t)n * rows + extra_rows) * width, 0.f);
    for (int s = 0; s < n; ++s) memcpy(h.data() + (size_t)s * rows * width, src + (size_t)s * B * width, (size_t)B * width * 4);
    if (extra_rows) memset(h.data() + (size_t)n * rows * width, 0xFF, extra_rows * width * 4);
    return gemm_tap_buf(e, b, h.size() * 4, h.data());
}
// host rows [n][B][K] -> n F32-layout images of `rows` rows (common.h f32_idx with K / 8 k-tiles), the slots B .. rows - 1 zero
static int dec_tap_f32_layout(mellow_engine* e, mellow_engine::Buf& b, const float* src, int n, int B, int rows, int K = 576) {
    std::vector<float> h((size_t)n * rows * K, 0.f);
    for (int s = 0; s < n; ++s)
        for (int r = 0; r < B; ++r)
            for (int k = 0; k < K; k += 4) {
                const size_t f4 = ((size_t)(r >> 5) * (K / 8) + (k >> 3)) * 64 + (r & 31) + 32 * ((k >> 2) & 1);
                memcpy(h.data() + (size_t)s * rows * K + f4 * 4, src + ((size_t)s * B + r) * K + k, 16);
            }
    return gemm_tap_buf(e, b, h.size() * 4, h.data());
}

int mellow_debug_dec_attn(mellow_engine_t* e, const mellow_dec_attn_t* d, const float* slabs, const float* ssq1, const float* x_res,
                          const float* down, const float* rope_cur, const float* k_pages, const float* v_pages, const int32_t* blk_live,
                          const int32_t* row_of_slot, const float* Wo, int32_t* out_gs, void* out_att, int64_t att_capacity, float* out_ml,
                          int64_t ml_capacity, void* out_k, void* out_v, int64_t kv_capacity, float* out_xnew, int64_t xnew_capacity,
                          void* out_xmid, int64_t xmid_capacity, void* out_x16, int64_t x16_capacity, float* out_ssq, int64_t ssq_capacity) {
    if (!e || !d) return fail("null argument");
    if (d->size != (int32_t)sizeof(mellow_dec_attn_t)) return fail("size = %d is not sizeof(mellow_dec_attn_t) = %d", d->size, (int)sizeof(mellow_dec_attn_t));
    const int B = d->B, P = d->P, pos = d->pos, Tmax = d->Tmax, ctx_end = d->ctx_end, ts = d->ts;
    if (B < 1 || B > 1024) return fail("B = %d: 1 <= B <= 1024", B);
    if (d->fused != 0 && d->fused != 1) return fail("fused must be 0 (slabs of the q/k/v launch) or 1 (slabs of the fused down + q/k/v launch): got %d", d->fused);
    const bool fused = d->fused != 0, kv16 = d->kv16 != 0;
    const int rows = rup(B, 32), RB = rows / 32;
    if (Tmax < 2 || Tmax > e->cfg.max_positions) return fail("Tmax = %d is not a page length of the engine: 2 <= Tmax <= max_positions = %d", Tmax, e->cfg.max_positions);
    if (pos < 1 || pos >= Tmax) return fail("pos = %d must lie in [1, Tmax = %d)", pos, Tmax);
    if (ctx_end <= pos || ctx_end > Tmax) return fail("ctx_end = %d must lie in (pos = %d, Tmax = %d]", ctx_end, pos, Tmax);
    if (P < rows || P > 4096) return fail("P = %d page sets: rows = %d <= P <= 4096", P, rows);
    if ((int64_t)(P + 1) * 3 * Tmax * 64 > ((int64_t)1 << 28)) return fail("(P + 1) * 3 * Tmax * 64 = %lld page elements exceed the tap's 2^28", (long long)(P + 1) * 3 * Tmax * 64);
    if (ts != dec_key_splits(RB, true) && (kv16 || ts != dec_key_splits(RB, false)))
        return fail("ts = %d is not a key split count of RB = %d row blocks with %s pages (dec_key_splits: %d%s)", ts, RB, kv16 ? "bf16" : "fp32",
                    dec_key_splits(RB, true), kv16 || dec_key_splits(RB, false) == dec_key_splits(RB, true) ? "" : ", or 1 in the f32x3 mode");
    if ((blk_live || row_of_slot) && RB < 2) return fail("blk_live / row_of_slot exist from two row blocks on (RB = %d)", RB);
    if (row_of_slot) {
        std::vector<char> seen(P, 0);
        for (int b = 0; b < rows; ++b) {
            const int r = row_of_slot[b];
            if (r == -1) continue;
            if (r < 0 || r >= P || seen[r]) return fail("row_of_slot[%d] = %d is outside [0, P = %d) or taken twice", b, r, P);
            seen[r] = 1;
        }
    }
    if (d->want_x3 && !Wo) return fail("want_x3 without Wo: the pre-split images are written by the o_proj launch");
    if (!slabs || !x_res || !k_pages || !v_pages || !out_gs) return fail("null argument: slabs, x_res, k_pages, v_pages and out_gs are required");
    if (!fused && !ssq1) return fail("null argument: fused 0 needs ssq1");
    if (fused && !down) return fail("null argument: fused 1 needs the down slabs");
    if (!(d->eps >= 0.f && d->eps < INFINITY)) return fail("eps = %g must be finite and >= 0", d->eps);
    // capacities, before anything is launched
    const size_t n_x = (size_t)rows * 576, page_elems = (size_t)3 * Tmax * 64;
    const size_t att_bytes = ((size_t)ts * n_x + 32 * 576) * 4, ml_bytes = (size_t)9 * rows * ts * 2 * 4;
    const size_t kv_bytes = (size_t)(P + 1) * page_elems * (kv16 ? 2 : 4), xnew_bytes = (size_t)(rows + 32) * 576 * 4;
    const size_t xmid_bytes = n_x * 4, x16_bytes = d->want_x3 ? 2 * n_x * 6 : n_x * 4, ssq_bytes = (size_t)(rows + 32) * 40 * 4;
    if (!out_att || att_capacity < (int64_t)att_bytes) return fail("att_capacity %lld is below the %lld bytes this call returns (or out_att is null)", (long long)att_capacity, (long long)att_bytes);
    if (!out_ml || ml_capacity < (int64_t)ml_bytes) return fail("ml_capacity %lld is below the %lld bytes this call returns (or out_ml is null)", (long long)ml_capacity, (long long)ml_bytes);
    if (!out_k || !out_v || kv_capacity < (int64_t)kv_bytes) return fail("kv_capacity %lld is below the %lld bytes each page array takes (or out_k / out_v is null)", (long long)kv_capacity, (long long)kv_bytes);
    if (!out_xnew || xnew_capacity < (int64_t)xnew_bytes) return fail("xnew_capacity %lld is below the %lld bytes this call returns (or out_xnew is null)", (long long)xnew_capacity, (long long)xnew_bytes);
    if (Wo) {
        if (!out_xmid || xmid_capacity < (int64_t)xmid_bytes) return fail("xmid_capacity %lld is below the %lld bytes this call returns (or out_xmid is null)", (long long)xmid_capacity, (long long)xmid_bytes);
        if (!out_x16 || x16_capacity < (int64_t)x16_bytes) return fail("x16_capacity %lld is below the %lld bytes this call returns (or out_x16 is null)", (long long)x16_capacity, (long long)x16_bytes);
        if (!out_ssq || ssq_capacity < (int64_t)ssq_bytes) return fail("ssq_capacity %lld is below the %lld bytes this call returns (or out_ssq is null)", (long long)ssq_capacity, (long long)ssq_bytes);
    }
    const int gs = dec_attn_split_groups(ctx_end, ts, kv16);
    *out_gs = gs;

    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    mellow_engine::Buf bPq, bSsq1, bXin, bDown, bRope, bK, bV, bK16, bV16, bWords, bW, bWp, bAtt, bMl, bXnew, bXmid, bX16, bSsq;
    CHK(dec_tap_rows(e, bPq, slabs, fused ? Q2_NPQ : DEC_KC_QKV, B, rows, 960));
    std::vector<float> hr(64);
    if (rope_cur) memcpy(hr.data(), rope_cur, 256);
    else {
        std::vector<float> hc((size_t)Tmax * 32), hs((size_t)Tmax * 32);
        CHK(mellow_host_rope_tables(e->cfg.rope_theta, 64, Tmax, hc.data(), hs.data()));
        memcpy(hr.data(), hc.data() + (size_t)pos * 32, 128);
        memcpy(hr.data() + 32, hs.data() + (size_t)pos * 32, 128);
    }
    CHK(gemm_tap_buf(e, bRope, 256, hr.data()));
    if (fused) {
        CHK(dec_tap_f32_layout(e, bXin, x_res, 1, B, rows));
        CHK(dec_tap_f32_layout(e, bDown, down, Q2_HC, B, rows));
        CHK(gemm_tap_buf(e, bXnew, xnew_bytes, nullptr));
    } else {
        CHK(dec_tap_rows(e, bSsq1, ssq1, 1, B, rows, DEC_KC_QKV));
        CHK(dec_tap_rows(e, bXnew, x_res, 1, B, rows, 576, 32));
    }
    // the pages: P sets from the caller and one of no example (0xFF bytes) behind them
    auto pages = [&](mellow_engine::Buf& b32, mellow_engine::Buf& b16, const float* src) -> int {
        CHK(gemm_tap_buf(e, b32, (size_t)(P + 1) * page_elems * 4, nullptr));
        HIPCHK(hipMemcpyAsync(b32.p, src, (size_t)P * page_elems * 4, hipMemcpyHostToDevice, s));
        if (kv16) {
            CHK(gemm_tap_buf(e, b16, kv_bytes, nullptr));
            launch_kv_to_bf16(b32.p, b16.p, (int64_t)((size_t)P * page_elems), s);
        }
        return 0;
    };
    CHK(pages(bK, bK16, k_pages));
    CHK(pages(bV, bV16, v_pages));
    // the device words: position | blk_live [RB] | row_of_slot [rows]
    std::vector<int32_t> hw(1 + RB + rows, 1);
    hw[0] = pos;
    const bool blk = blk_live || row_of_slot;         // (the kernels read row_of_slot in their early-exit instantiation only)
    if (blk_live) memcpy(hw.data() + 1, blk_live, (size_t)RB * 4);
    if (row_of_slot) memcpy(hw.data() + 1 + RB, row_of_slot, (size_t)rows * 4);
    CHK(gemm_tap_buf(e, bWords, hw.size() * 4, hw.data()));
    int32_t* dw = reinterpret_cast<int32_t*>(bWords.p);
    CHK(gemm_tap_buf(e, bAtt, att_bytes, nullptr));
    CHK(gemm_tap_buf(e, bMl, ml_bytes, nullptr));
    DecArgs a;
    a.rows = rows; a.RB = RB; a.Tmax = Tmax; a.eps = d->eps; a.d_pos = dw; a.gs = gs; a.ts = ts; a.kv16 = kv16 ? 1 : 0;
    a.rope_cur = bRope.p; a.ssq1 = bSsq1.p; a.pq = bPq.p;
    a.xmidF = bXin.p; a.dslabF = bDown.p; a.slabF_stride4 = (int64_t)(n_x / 4); a.xnewR = bXnew.p;
    a.attF16 = bAtt.p; a.att_ml = bMl.p;
    a.blk_live = blk ? dw + 1 : nullptr; a.row_of_slot = row_of_slot ? dw + 1 + RB : nullptr;
    if (Wo) {
        CHK(gemm_tap_buf(e, bW, (size_t)576 * 576 * 4, Wo));
        CHK(ensure(e, bWp, (size_t)576 * 576));
        launch_pack_weight16(bW.p, 576, 576, bWp.p, s);
        CHK(gemm_tap_buf(e, bXmid, xmid_bytes, nullptr));
        CHK(gemm_tap_buf(e, bX16, x16_bytes, nullptr));
        CHK(gemm_tap_buf(e, bSsq, ssq_bytes, nullptr));
    }
    launch_dec_attn(a, kv16 ? bK16.p : bK.p, kv16 ? bV16.p : bV.p, fused, s);
    if (Wo) {
        DecArgs o = a;
        o.xmidF = bXmid.p; o.ssq = bSsq.p;
        if (d->want_x3) { o.xmid3_32 = bX16.p; o.xmid3_16 = reinterpret_cast<char*>(bX16.p) + n_x * 6; }
        else o.xmidF16 = bX16.p;
        launch_dec_oproj(o, bWp.p, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    CHK(gemm_tap_fetch(out_att, att_capacity, bAtt, att_bytes, "att"));
    CHK(gemm_tap_fetch(out_ml, ml_capacity, bMl, ml_bytes, "ml"));
    CHK(gemm_tap_fetch(out_k, kv_capacity, kv16 ? bK16 : bK, kv_bytes, "kv"));
    CHK(gemm_tap_fetch(out_v, kv_capacity, kv16 ? bV16 : bV, kv_bytes, "kv"));
    CHK(gemm_tap_fetch(out_xnew, xnew_capacity, bXnew, xnew_bytes, "xnew"));
    if (Wo) {
        CHK(gemm_tap_fetch(out_xmid, xmid_capacity, bXmid, xmid_bytes, "xmid"));
        CHK(gemm_tap_fetch(out_x16, x16_capacity, bX16, x16_bytes, "x16"));
        CHK(gemm_tap_fetch(out_ssq, ssq_capacity, bSsq, ssq_bytes, "ssq"));
    }
    return 0;
}

// ---- decode GEMV tap on host data (include/mellow_hip.h): one call of launch_dec_qkv, launch_dec_gateup / launch_dec_gateup3,
// launch_dec_down, launch_dec_qkv2 / launch_dec_qkv2x3 or launch_dec_final_norm on DecArgs filled from buffers of the call's own;
// the weights packed by the loader's routines (engine_weights.cpp) ------------------------------------------------------------------
int mellow_debug_dec_gemv(mellow_engine_t* e, const mellow_dec_gemv_t* d, const float* W, const float* W2, const float* x,
                          const float* down, const float* h, const void* x_img, int64_t x_img_bytes, const void* h_img,
                          int64_t h_img_bytes, const float* ssq, const float* rope_cos, const float* rope_sin, const int32_t* blk_live,
                          float* out_pq, int64_t pq_capacity, float* out_down, int64_t down_capacity, float* out_ssq1,
                          int64_t ssq1_capacity, float* out_xnew, int64_t xnew_capacity, float* out_rope, int32_t* out_pos,
                          float* out_gu, int64_t gu_capacity, void* out_h3, int64_t h3_capacity, void* out_xn, int64_t xn_capacity,
                          int32_t* out_snap, float* out_q, int64_t q_capacity) {
    if (!e || !d) return fail("null argument");
    if (d->size != (int32_t)sizeof(mellow_dec_gemv_t)) return fail("size = %d is not sizeof(mellow_dec_gemv_t) = %d", d->size, (int)sizeof(mellow_dec_gemv_t));
    const int op = d->op, form = d->form, B = d->B, kcd = d->kcd;
    if (op < 0 || op > 4) return fail("op must be 0 (q/k/v), 1 (gate/up), 2 (down), 3 (fused down + q/k/v) or 4 (final norm): got %d", op);
    if (form != 0 && form != 1) return fail("form must be 0 (the fp32 kernel) or 1 (the f32x3 kernel): got %d", form);
    if (form == 1 && op != 1 && op != 3) return fail("op %d has the fp32 form only: the f32x3 forms are launch_dec_gateup3 (op 1) and launch_dec_qkv2x3 (op 3)", op);
    if (B < 1 || B > 1024) return fail("B = %d: 1 <= B <= 1024", B);
    const int rows = rup(B, 32), RB = rows / 32;
    const bool k_op = op == 0 || op == 4;
    if (k_op && kcd != 0 && kcd != DEC_KC_DOWN) return fail("kcd = %d: the down slabs a launch sums are 0 or DEC_KC_DOWN = %d", kcd, DEC_KC_DOWN);
    if (!k_op && kcd != 0) return fail("kcd goes with ops 0 and 4 only");
    const bool first = d->first != 0, inc_pos = d->inc_pos != 0;
    if ((first || inc_pos) && op != 0) return fail("first / inc_pos go with op 0 only");
    // the step's first q/k/v launch starts from a materialised x, every later one sums the down slabs (enqueue_decode_layer_range)
    if (op == 0 && first != (kcd == 0)) return fail("op 0: first = %d with kcd = %d is no launch of a decode step (first goes with kcd 0, kcd %d with first 0)", (int)first, kcd, DEC_KC_DOWN);
    if (inc_pos && !first) return fail("inc_pos without first: the position word advances in the step's first launch only");
    if (d->want_x3 && op != 4) return fail("want_x3 goes with op 4 only");
    if (d->want_x3 && !dec_head3r_fits(e->cfg.vocab_size)) return fail("want_x3: the streaming f32x3 lm_head does not tile vocab_size = %d, the engine never hands xn3 over", e->cfg.vocab_size);
    if (blk_live && RB < 2) return fail("blk_live exists from two row blocks on (RB = %d)", RB);
    if (!(d->eps >= 0.f && d->eps < INFINITY)) return fail("eps = %g must be finite and >= 0", d->eps);
    const int Tmax = first ? d->Tmax : 2, pos = d->pos;
    if (first) {
        if (Tmax < 2 || Tmax > e->cfg.max_positions) return fail("Tmax = %d is not a page length of the engine: 2 <= Tmax <= max_positions = %d", Tmax, e->cfg.max_positions);
        if (pos < 0 || pos + (int)inc_pos >= Tmax) return fail("pos = %d (+ inc_pos) must lie in [0, Tmax = %d)", pos, Tmax);
        if ((rope_cos == nullptr) != (rope_sin == nullptr)) return fail("rope_cos and rope_sin go together");
    } else if (rope_cos || rope_sin) return fail("RoPE tables without first: only the step's first q/k/v launch reads them");
    const size_t n_x = (size_t)rows * 576, n_h = (size_t)rows * 1536;
    // operands
    if (!W) return fail("null argument: W");
    if ((op == 1 || op == 3) && !W2) return fail("null argument: W2 (op 1 the up weight, op 3 the down weight)");
    if (op != 1 && op != 3 && W2) return fail("W2 goes with ops 1 and 3 only");
    const bool need_x = op == 0 || op == 4 || (op == 3 && form == 0), need_h = op == 2 || (op == 3 && form == 0);
    if (need_x != (x != nullptr)) return fail(need_x ? "null argument: x" : "x is not an operand of this launch");
    if (need_h != (h != nullptr)) return fail(need_h ? "null argument: h" : "h is not an operand of this launch");
    if ((kcd != 0) != (down != nullptr)) return fail(kcd ? "null argument: down" : "down without kcd");
    const size_t x_img_need = op == 1 ? (form ? n_x * 6 : n_x * 4) : (op == 3 && form == 1 ? n_x * 6 : 0);
    const size_t h_img_need = op == 3 && form == 1 ? n_h * 6 : 0;
    if ((x_img_need != 0) != (x_img != nullptr) || (x_img && x_img_bytes != (int64_t)x_img_need))
        return fail("x_img: this launch takes %lld bytes there (got %lld)", (long long)x_img_need, x_img ? (long long)x_img_bytes : 0ll);
    if ((h_img_need != 0) != (h_img != nullptr) || (h_img && h_img_bytes != (int64_t)h_img_need))
        return fail("h_img: this launch takes %lld bytes there (got %lld)", (long long)h_img_need, h_img ? (long long)h_img_bytes : 0ll);
    if ((op == 1) != (ssq != nullptr)) return fail(op == 1 ? "null argument: ssq" : "ssq goes with op 1 only");
    // capacities, before anything is launched
    const bool w_pq = op == 0 || op == 3, w_down = op == 2 || op == 3, w_x3 = op == 4 && d->want_x3;
    const size_t pq_bytes = ((size_t)DEC_KC_QKV * rows + 32) * 960 * 4, down_bytes = ((size_t)DEC_KC_DOWN * n_x + 32 * 576) * 4;
    const size_t ssq1_bytes = (size_t)(rows + 32) * DEC_KC_QKV * 4, xnew_bytes = (size_t)(rows + 32) * 576 * 4;
    const size_t gu_bytes = (n_h + 32 * 1536) * 4, h3_bytes = (n_h + 32 * 1536) * 6, xn_bytes = (n_x + 32 * 576) * (w_x3 ? 6 : 4);
    const size_t q_bytes = (size_t)960 * 1536 * 4;
    auto cap = [&](bool wanted, const void* p, int64_t c, size_t bytes, const char* name) -> int {
        if (wanted && (!p || c < (int64_t)bytes)) return fail("%s_capacity %lld is below the %lld bytes this call returns (or out_%s is null)", name, (long long)c, (long long)bytes, name);
        return 0;
    };
    CHK(cap(w_pq, out_pq, pq_capacity, pq_bytes, "pq"));
    CHK(cap(w_down, out_down, down_capacity, down_bytes, "down"));
    CHK(cap(op == 0, out_ssq1, ssq1_capacity, ssq1_bytes, "ssq1"));
    CHK(cap(op == 0, out_xnew, xnew_capacity, xnew_bytes, "xnew"));
    if (op == 0 && (!out_rope || !out_pos)) return fail("null argument: out_rope (128 floats) and out_pos are required with op 0");
    CHK(cap(op == 1, out_gu, gu_capacity, gu_bytes, "gu"));
    CHK(cap(op == 1 && form == 1, out_h3, h3_capacity, h3_bytes, "h3"));
    CHK(cap(op == 4, out_xn, xn_capacity, xn_bytes, "xn"));
    if (op == 4 && blk_live && !out_snap) return fail("null argument: out_snap (64 words) is required with op 4 and blk_live");
    CHK(cap(op == 3, out_q, q_capacity, q_bytes, "q"));

    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    mellow_engine::Buf bW, bW2, bWp, bWp2, bQ, bCat, bX, bH, bDown, bSsq, bWords, bCos, bSin, bRope, bPq, bSsq1, bXnew, bGu, bH3, bXn;
    // the device words: position | blk_live [32] (zeros behind RB) | blk_snap [32] + 32 words nobody owns (0xFF bytes)
    std::vector<int32_t> hw(1 + 32 + 64, -1);
    hw[0] = pos;
    for (int i = 0; i < 32; ++i) hw[1 + i] = blk_live && i < RB ? blk_live[i] : 0;
    CHK(gemm_tap_buf(e, bWords, hw.size() * 4, hw.data()));
    int32_t* dw = reinterpret_cast<int32_t*>(bWords.p);
    DecArgs a;
    a.rows = rows; a.RB = RB; a.Tmax = Tmax; a.eps = d->eps; a.d_pos = dw; a.first = first ? 1 : 0; a.inc_pos = inc_pos ? 1 : 0;
    a.slabF_stride4 = (int64_t)(n_x / 4);
    a.blk_live = blk_live ? dw + 1 : nullptr; a.blk_snap = dw + 33;
    if (need_x) { CHK(dec_tap_f32_layout(e, bX, x, 1, B, rows)); a.xmidF = bX.p; }
    if (need_h) { CHK(dec_tap_f32_layout(e, bH, h, 1, B, rows, 1536)); a.guF = bH.p; }
    if (kcd) { CHK(dec_tap_f32_layout(e, bDown, down, DEC_KC_DOWN, B, rows)); a.dslabF = bDown.p; }
    if (w_pq) { CHK(gemm_tap_buf(e, bPq, pq_bytes, nullptr)); a.pq = bPq.p; }
    if (w_down) { CHK(gemm_tap_buf(e, bDown, down_bytes, nullptr)); a.dslabF = bDown.p; }
    if (op == 0) {
        CHK(gemm_tap_buf(e, bW, (size_t)960 * 576 * 4, W));
        CHK(ensure(e, bWp, (size_t)1024 * 576));
        launch_pack_weight(bW.p, 960, 576, 576, bWp.p, 1024, 576, s);
        CHK(gemm_tap_buf(e, bSsq1, ssq1_bytes, nullptr));
        CHK(gemm_tap_buf(e, bXnew, xnew_bytes, nullptr));
        CHK(gemm_tap_buf(e, bRope, 128 * 4, nullptr));
        a.ssq1 = bSsq1.p; a.xnewR = bXnew.p; a.rope_cur = bRope.p;
        if (first) {
            std::vector<float> hc, hs;
            if (!rope_cos) {
                hc.resize((size_t)Tmax * 32); hs.resize((size_t)Tmax * 32);
                CHK(mellow_host_rope_tables(e->cfg.rope_theta, 64, Tmax, hc.data(), hs.data()));
            }
            CHK(gemm_tap_buf(e, bCos, (size_t)Tmax * 32 * 4, rope_cos ? rope_cos : hc.data()));
            CHK(gemm_tap_buf(e, bSin, (size_t)Tmax * 32 * 4, rope_sin ? rope_sin : hs.data()));
            a.rope_cos = bCos.p; a.rope_sin = bSin.p;
        }
        launch_dec_qkv(a, bWp.p, 72, kcd, s);
    } else if (op == 1) {
        std::vector<float> il;
        interleave_gate_up8(W, W2, 1536, 576, il);
        CHK(gemm_tap_buf(e, bW, il.size() * 4, il.data()));
        CHK(ensure(e, bWp, il.size()));
        if (form) launch_pack_weight16n(bW.p, 3072, 576, bWp.p, s);
        else launch_pack_weight16(bW.p, 3072, 576, bWp.p, s);
        CHK(gemm_tap_buf(e, bX, x_img_need, x_img));
        CHK(gemm_tap_buf(e, bSsq, (size_t)rows * 40 * 4, ssq));
        CHK(gemm_tap_buf(e, bGu, gu_bytes, nullptr));
        a.ssq = bSsq.p; a.guF = bGu.p;
        if (form) {
            CHK(gemm_tap_buf(e, bH3, h3_bytes, nullptr));
            a.xmid3_16 = bX.p; a.h3 = bH3.p;
            launch_dec_gateup3(a, bWp.p, s);
        } else {
            a.xmidF16 = bX.p;
            launch_dec_gateup(a, bWp.p, s);
        }
    } else if (op == 2) {
        CHK(gemm_tap_buf(e, bW, (size_t)576 * 1536 * 4, W));
        CHK(ensure(e, bWp, (size_t)640 * 1536));
        launch_pack_weight(bW.p, 576, 1536, 1536, bWp.p, 640, 1536, s);
        launch_dec_down(a, bWp.p, 192, s);
    } else if (op == 3) {
        CHK(gemm_tap_buf(e, bW, (size_t)960 * 576 * 4, W));
        CHK(gemm_tap_buf(e, bW2, (size_t)576 * 1536 * 4, W2));
        CHK(ensure(e, bQ, (size_t)960 * 1536));
        CHK(ensure(e, bCat, (size_t)1024 * 2112));
        CHK(ensure(e, bWp, (size_t)1024 * 2112));
        CHK(ensure(e, bWp2, (size_t)640 * 1536));
        launch_compose_f64(bW.p, bW2.p, bQ.p, 960, 1536, 576, s);
        CHK(pack_qkv2_cat(e, bW.p, bQ.p, bCat.p, bWp.p));
        launch_pack_weight(bW2.p, 576, 1536, 1536, bWp2.p, 640, 1536, s);
        if (form) {
            CHK(gemm_tap_buf(e, bX, x_img_need, x_img));
            CHK(gemm_tap_buf(e, bH, h_img_need, h_img));
            a.xmid3_32 = bX.p; a.h3 = bH.p;
            launch_dec_qkv2x3(a, bWp.p, bWp2.p, s);
        } else {
            launch_dec_qkv2(a, bWp.p, bWp2.p, s);
        }
    } else {
        CHK(gemm_tap_buf(e, bW, (size_t)576 * 4, W));
        CHK(gemm_tap_buf(e, bXn, xn_bytes, nullptr));
        if (w_x3) a.xn3 = bXn.p; else a.xnF = bXn.p;
        launch_dec_final_norm(a, bW.p, kcd, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (w_pq) CHK(gemm_tap_fetch(out_pq, pq_capacity, bPq, pq_bytes, "pq"));
    if (w_down) CHK(gemm_tap_fetch(out_down, down_capacity, bDown, down_bytes, "down"));
    if (op == 0) {
        CHK(gemm_tap_fetch(out_ssq1, ssq1_capacity, bSsq1, ssq1_bytes, "ssq1"));
        CHK(gemm_tap_fetch(out_xnew, xnew_capacity, bXnew, xnew_bytes, "xnew"));
        HIPCHK(hipMemcpy(out_rope, bRope.p, 128 * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_pos, dw, 4, hipMemcpyDeviceToHost));
    }
    if (op == 1) {
        CHK(gemm_tap_fetch(out_gu, gu_capacity, bGu, gu_bytes, "gu"));
        if (form) CHK(gemm_tap_fetch(out_h3, h3_capacity, bH3, h3_bytes, "h3"));
    }
    if (op == 3) CHK(gemm_tap_fetch(out_q, q_capacity, bQ, q_bytes, "q"));
    if (op == 4) {
        CHK(gemm_tap_fetch(out_xn, xn_capacity, bXn, xn_bytes, "xn"));
        if (out_snap) HIPCHK(hipMemcpy(out_snap, dw + 33, 64 * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- decode step-tail tap on host data (include/mellow_hip.h): one call of launch_dec_lm_head, launch_dec_argmax, launch_dec_compact
// or launch_dec_load_rows on DecArgs / LoopArgs filled from buffers of the call's own; the head weight packed as the loader packs
// lm_head (engine_weights.cpp: launch_pack_weight into roundup(V, 128) rows) ------------------------------------------------------------
namespace {
// the int32 words a launch can rewrite, as the tap returns them (out_state): seen_stop [rows + 32] | n_seen, arrive, ticket,
// n_compactions + 28 words nobody owns | blk_left [64] | blk_live [64] | row_of_slot [rows + 32]; behind them, on the device only,
// what the launch reads: params {max_len, stop_id}, the position word + 29 words | blk_snap [32]
struct TailWords {
    int rows;
    int seen() const { return 0; }
    int scalars() const { return rows + 32; }
    int left() const { return scalars() + 32; }
    int live() const { return left() + 64; }
    int slot() const { return live() + 64; }
    int state_words() const { return slot() + rows + 32; }
    int params() const { return state_words(); }
    int pos() const { return params() + 2; }
    int snap() const { return params() + 32; }
    int total() const { return snap() + 32; }
};
}  // namespace

int mellow_debug_dec_tail(mellow_engine_t* e, const mellow_dec_tail_t* d, const float* W, const float* x, const void* x_img,
                          int64_t x_img_bytes, const int32_t* blk_live, const float* cand_val, const int32_t* cand_idx,
                          const float* cand_sum, const int32_t* seen_stop, const int32_t* blk_left, const int32_t* blk_snap,
                          const int32_t* row_of_slot, const int32_t* row_ids, float* out_logits, int64_t logits_capacity,
                          float* out_cand_val, int32_t* out_cand_idx, float* out_cand_sum, int64_t cand_capacity, int32_t* out_tokens,
                          int64_t tokens_capacity, int32_t* out_record, float* out_logprob, int64_t record_capacity, int32_t* out_state,
                          int64_t state_capacity, uint64_t* out_progress, float* out_x, int64_t x_capacity) {
    if (!e || !d) return fail("null argument");
    if (d->size != (int32_t)sizeof(mellow_dec_tail_t)) return fail("size = %d is not sizeof(mellow_dec_tail_t) = %d", d->size, (int)sizeof(mellow_dec_tail_t));
    const int op = d->op, form = d->form, B = d->B, V = d->V;
    if (op < 0 || op > 3) return fail("op must be 0 (lm_head), 1 (arg-max), 2 (row repack) or 3 (row load): got %d", op);
    if (form != 0 && form != 1) return fail("form must be 0 (the fp32 kernel) or 1 (the streaming f32x3 kernel): got %d", form);
    if (form == 1 && op != 0) return fail("op %d has one form only: form 1 is the streaming f32x3 lm_head (op 0)", op);
    if (B < 1 || B > 1024) return fail("B = %d: 1 <= B <= 1024", B);
    const int rows = rup(B, 32), RB = rows / 32;
    const bool head = op == 0, amax = op == 1, pack = op == 2, load = op == 3;
    const bool state = amax && d->with_state != 0, lp_on = amax && d->with_logprob != 0, write_x = amax && d->write_x != 0;
    // switches of another op
    if (!head && (d->want_logits || d->want_sum)) return fail("want_logits / want_sum go with op 0 only");
    if (!amax && (d->write_x || d->with_state || d->with_logprob)) return fail("write_x / with_state / with_logprob go with op 1 only");
    if (!state && (d->max_len || d->stop_id || d->T0 || d->pos || d->n_seen || d->arrive || d->ticket))
        return fail("max_len, stop_id, T0, pos, n_seen, arrive and ticket go with op 1 and with_state only");
    if (!pack && d->n_compactions) return fail("n_compactions goes with op 2 only");
    if (!load && (d->ld || d->n_src || d->T_last)) return fail("ld, n_src and T_last go with op 3 only");
    if (!(head || amax) && V) return fail("V goes with ops 0 and 1 only");
    if (head || amax) {
        if (V < 32 || V % 32 != 0 || V > (1 << 20)) return fail("V = %d: the head and the arg-max tile the vocabulary in 32 columns (32 <= V <= 2^20, V %% 32 == 0)", V);
        if ((int64_t)(rows + 32) * V > ((int64_t)1 << 28)) return fail("(rows + 32) * V = %lld elements exceed the tap's 2^28", (long long)(rows + 32) * V);
    }
    if (head && form == 1 && !dec_head3r_fits(V)) return fail("V = %d: the streaming f32x3 lm_head does not tile it (dec_head3r_fits)", V);
    const int n = V / 32;
    // operands
    auto want = [&](bool needed, const void* p, const char* name) -> int {
        if (needed && !p) return fail("null argument: %s", name);
        if (!needed && p) return fail("%s is not an operand of this launch", name);
        return 0;
    };
    CHK(want(head || write_x, W, "W"));
    CHK(want((head && form == 0) || pack || load, x, "x"));
    const size_t x_img_need = head && form == 1 ? (size_t)rows * 576 * 6 : 0;
    if ((x_img_need != 0) != (x_img != nullptr) || (x_img && x_img_bytes != (int64_t)x_img_need))
        return fail("x_img: this launch takes %lld bytes there (got %lld)", (long long)x_img_need, x_img ? (long long)x_img_bytes : 0ll);
    CHK(want(amax, cand_val, "cand_val"));
    CHK(want(amax, cand_idx, "cand_idx"));
    if (cand_sum && !amax) return fail("cand_sum is not an operand of this launch");
    if (lp_on && !cand_sum) return fail("with_logprob without cand_sum: the log-prob is merged from the head's partial sums");
    if (lp_on && !state) return fail("with_logprob without with_state: the log-prob is written where the token record is");
    CHK(want(state || pack, seen_stop, "seen_stop"));
    if (pack && !row_of_slot) return fail("null argument: row_of_slot");
    if (!(state || pack) && row_of_slot) return fail("row_of_slot is not an operand of this launch");
    if (!(state || pack) && blk_left) return fail("blk_left is not an operand of this launch");
    if (load || (amax && !state)) { if (blk_live) return fail("blk_live is not an operand of this launch"); }
    if (pack && (!blk_live || !blk_left)) return fail("null argument: op 2 needs blk_live and blk_left");
    if (state && (blk_live == nullptr) != (blk_left == nullptr)) return fail("blk_live and blk_left go together (LoopArgs: the count and the word it clears)");
    if (blk_snap && !state) return fail("blk_snap is not an operand of this launch");
    if ((blk_live || blk_left || blk_snap || row_of_slot) && RB < 2)
        return fail("blk_live / blk_left / blk_snap / row_of_slot exist from two row blocks on (RB = %d)", RB);
    if (row_ids && !load) return fail("row_ids is not an operand of this launch");
    if (row_of_slot) {
        std::vector<char> taken(rows, 0);
        for (int b = 0; b < rows; ++b) {
            const int r = row_of_slot[b];
            if (r == -1) continue;
            if (r < 0 || r >= rows || taken[r]) return fail("row_of_slot[%d] = %d is outside [0, rows = %d) or taken twice", b, r, rows);
            taken[r] = 1;
        }
    }
    const int max_len = state ? d->max_len : 0;
    if (state) {
        if (max_len < 1 || max_len > 4096) return fail("max_len = %d: 1 <= max_len <= 4096", max_len);
        if (d->T0 < 0 || d->T0 > (1 << 20) || d->pos < -(1 << 20) || d->pos > (1 << 20)) return fail("T0 = %d / pos = %d: 0 <= T0 <= 2^20, |pos| <= 2^20", d->T0, d->pos);
    }
    int64_t ld = 0;
    if (load) {
        ld = d->ld;
        if (ld < 576 || ld % 4 != 0) return fail("ld = %d: the rows are read as float4 (ld >= 576, ld %% 4 == 0)", d->ld);
        if (d->n_src < 1 || (int64_t)d->n_src * ld > ((int64_t)1 << 26)) return fail("n_src = %d: 1 <= n_src and n_src * ld <= 2^26", d->n_src);
        if (row_ids && d->T_last != 0) return fail("T_last = %d with row_ids: the ids address the rows (T_last 0)", d->T_last);
        if (!row_ids && (d->T_last < 1 || (int64_t)B * d->T_last > d->n_src))
            return fail("T_last = %d without row_ids: row b * T_last + T_last - 1 must exist (1 <= T_last, B * T_last <= n_src = %d)", d->T_last, d->n_src);
    }
    // capacities, before anything is launched
    const TailWords tw{rows};
    const size_t logits_bytes = (size_t)(rows + 32) * V * 4, cand_bytes = (size_t)(rows + 32) * n * 4, tokens_bytes = (size_t)(rows + 32) * 4;
    const size_t record_bytes = (size_t)rows * max_len * 4, state_bytes = (size_t)tw.state_words() * 4, x_bytes = (size_t)(rows + 32) * 576 * 4;
    auto cap = [&](bool wanted, const void* p, int64_t c, size_t bytes, const char* name, const char* cname) -> int {
        if (wanted && (!p || c < (int64_t)bytes)) return fail("%s_capacity %lld is below the %lld bytes this call returns (or out_%s is null)", cname, (long long)c, (long long)bytes, name);
        return 0;
    };
    CHK(cap(head, out_logits, logits_capacity, logits_bytes, "logits", "logits"));
    CHK(cap(head, out_cand_val, cand_capacity, cand_bytes, "cand_val", "cand"));
    CHK(cap(head, out_cand_idx, cand_capacity, cand_bytes, "cand_idx", "cand"));
    CHK(cap(head, out_cand_sum, cand_capacity, cand_bytes, "cand_sum", "cand"));
    CHK(cap(amax, out_tokens, tokens_capacity, tokens_bytes, "tokens", "tokens"));
    CHK(cap(state, out_record, record_capacity, record_bytes, "record", "record"));
    CHK(cap(lp_on, out_logprob, record_capacity, record_bytes, "logprob", "record"));
    CHK(cap(state || pack, out_state, state_capacity, state_bytes, "state", "state"));
    if (state && !out_progress) return fail("null argument: out_progress is required with with_state");
    CHK(cap(!head, out_x, x_capacity, x_bytes, "x", "x"));

    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    mellow_engine::Buf bW, bWp, bX, bIn, bIds, bWords, bLogits, bCv, bCi, bCs, bTok, bRec, bLp;
    DecArgs a;
    a.rows = rows; a.RB = RB; a.slabF_stride4 = (int64_t)rows * 576 / 4;
    // the device words (TailWords): 0xFF bytes wherever the caller planted nothing
    std::vector<int32_t> hw(tw.total(), -1);
    if (seen_stop) memcpy(hw.data() + tw.seen(), seen_stop, (size_t)rows * 4);
    if (state) { hw[tw.scalars()] = d->n_seen; hw[tw.scalars() + 1] = d->arrive; hw[tw.scalars() + 2] = d->ticket; }
    if (pack) hw[tw.scalars() + 3] = d->n_compactions;
    auto blocks = [&](int at, const int32_t* src) { for (int i = 0; i < 32; ++i) hw[at + i] = i < RB ? src[i] : 0; };      // zeros behind RB, as the engine's
    if (blk_left) blocks(tw.left(), blk_left);
    if (blk_live) blocks(tw.live(), blk_live);
    if (blk_snap) blocks(tw.snap(), blk_snap);
    if (row_of_slot) memcpy(hw.data() + tw.slot(), row_of_slot, (size_t)rows * 4);
    hw[tw.params()] = max_len; hw[tw.params() + 1] = d->stop_id; hw[tw.pos()] = d->pos;
    CHK(gemm_tap_buf(e, bWords, hw.size() * 4, hw.data()));
    int32_t* dw = reinterpret_cast<int32_t*>(bWords.p);
    a.d_pos = dw + tw.pos();
    struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
    std::unique_ptr<unsigned long long, HostFree> h_prog;       // the mapped host word the last arrival publishes to
    if (head) {
        CHK(gemm_tap_buf(e, bW, (size_t)V * 576 * 4, W));
        const int NP = rup(V, 128);
        CHK(ensure(e, bWp, (size_t)NP * 576));
        launch_pack_weight(bW.p, V, 576, 576, bWp.p, NP, 576, s);
        if (form) { CHK(gemm_tap_buf(e, bX, x_img_need, x_img)); a.xn3 = bX.p; a.x3 = DEC_X3_HEAD; }
        else { CHK(dec_tap_f32_layout(e, bX, x, 1, B, rows)); a.xnF = bX.p; }
        CHK(gemm_tap_buf(e, bLogits, logits_bytes, nullptr));
        CHK(gemm_tap_buf(e, bCv, cand_bytes, nullptr));
        CHK(gemm_tap_buf(e, bCi, cand_bytes, nullptr));
        CHK(gemm_tap_buf(e, bCs, cand_bytes, nullptr));
        a.logits = d->want_logits ? bLogits.p : nullptr;
        a.cand_val = bCv.p; a.cand_idx = reinterpret_cast<int32_t*>(bCi.p); a.cand_sum = d->want_sum ? bCs.p : nullptr;
        a.blk_live = blk_live ? dw + tw.live() : nullptr;
        launch_dec_lm_head(a, bWp.p, 72, V, s);
    } else if (amax) {
        CHK(gemm_tap_buf(e, bCv, (size_t)B * n * 4, cand_val));
        CHK(gemm_tap_buf(e, bCi, (size_t)B * n * 4, cand_idx));
        if (cand_sum) CHK(gemm_tap_buf(e, bCs, (size_t)B * n * 4, cand_sum));
        if (write_x) CHK(gemm_tap_buf(e, bW, (size_t)V * 576 * 4, W));
        CHK(gemm_tap_buf(e, bTok, tokens_bytes, nullptr));
        CHK(gemm_tap_buf(e, bX, x_bytes, nullptr));
        a.cand_val = bCv.p; a.cand_idx = reinterpret_cast<int32_t*>(bCi.p); a.cand_sum = cand_sum ? bCs.p : nullptr;
        a.xmidF = bX.p;
        LoopArgs lp;
        if (state) {
            CHK(gemm_tap_buf(e, bRec, record_bytes, nullptr));
            if (lp_on) CHK(gemm_tap_buf(e, bLp, record_bytes, nullptr));
            unsigned long long *hp = nullptr, *d_prog = nullptr;
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hp), 64, hipHostMallocMapped | hipHostMallocCoherent));
            h_prog.reset(hp);
            memset(hp, 0xFF, 64);
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_prog), hp, 0));
            lp.out_tokens = reinterpret_cast<int32_t*>(bRec.p); lp.params = dw + tw.params(); lp.seen_stop = dw + tw.seen();
            lp.n_seen = dw + tw.scalars(); lp.arrive = dw + tw.scalars() + 1; lp.ticket = dw + tw.scalars() + 2;
            if (blk_left) { lp.blk_left = dw + tw.left(); lp.blk_live = dw + tw.live(); }
            if (blk_snap) lp.blk_snap = dw + tw.snap();
            if (row_of_slot) lp.row_of_slot = dw + tw.slot();
            lp.host_progress = d_prog; lp.T0 = d->T0;
            if (lp_on) lp.out_logprob = bLp.p;
        }
        launch_dec_argmax(a, B, n, reinterpret_cast<int32_t*>(bTok.p), write_x ? bW.p : nullptr, write_x ? 1 : 0, lp, s);
    } else if (pack) {
        // x in F32-layout, in front of 32 rows of margin that hold 0xFF bytes
        CHK(gemm_tap_buf(e, bX, x_bytes, nullptr));
        CHK(dec_tap_f32_layout(e, bIn, x, 1, B, rows));
        HIPCHK(hipMemcpyAsync(bX.p, bIn.p, (size_t)rows * 576 * 4, hipMemcpyDeviceToDevice, s));
        a.xmidF = bX.p;
        LoopArgs lp;
        lp.seen_stop = dw + tw.seen(); lp.blk_left = dw + tw.left(); lp.blk_live = dw + tw.live(); lp.row_of_slot = dw + tw.slot();
        lp.n_compactions = dw + tw.scalars() + 3;
        launch_dec_compact(a, B, lp, s);
    } else {
        CHK(gemm_tap_buf(e, bIn, (size_t)d->n_src * ld * 4, x));
        if (row_ids) CHK(gemm_tap_buf(e, bIds, (size_t)B * 4, row_ids));
        CHK(gemm_tap_buf(e, bX, x_bytes, nullptr));
        a.xmidF = bX.p;
        launch_dec_load_rows(a, B, bIn.p, ld, row_ids ? reinterpret_cast<const int32_t*>(bIds.p) : nullptr, d->T_last, row_ids ? d->n_src : 0, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (head) {
        CHK(gemm_tap_fetch(out_logits, logits_capacity, bLogits, logits_bytes, "logits"));
        CHK(gemm_tap_fetch(out_cand_val, cand_capacity, bCv, cand_bytes, "cand"));
        CHK(gemm_tap_fetch(out_cand_idx, cand_capacity, bCi, cand_bytes, "cand"));
        CHK(gemm_tap_fetch(out_cand_sum, cand_capacity, bCs, cand_bytes, "cand"));
        return 0;
    }
    if (amax) CHK(gemm_tap_fetch(out_tokens, tokens_capacity, bTok, tokens_bytes, "tokens"));
    if (state) {
        CHK(gemm_tap_fetch(out_record, record_capacity, bRec, record_bytes, "record"));
        if (lp_on) CHK(gemm_tap_fetch(out_logprob, record_capacity, bLp, record_bytes, "record"));
        *out_progress = *h_prog.get();
    }
    if (state || pack) CHK(gemm_tap_fetch(out_state, state_capacity, bWords, state_bytes, "state"));
    CHK(gemm_tap_fetch(out_x, x_capacity, bX, x_bytes, "x"));
    return 0;
}

// developer instrumentation (not part of the public header): one CSV line per profiled launch
__attribute__((visibility("default"))) int mellow_dev_prof_dump(mellow_engine_t* e, const char* path) {
    if (!e || !path) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    FILE* f = fopen(path, "w");
    if (!f) return fail("cannot open %s", path);
    fprintf(f, "fam,M,N,K,epi,ms,flops\n");
    for (const auto& r : e->prof) {
        float m = 0.f;
        hipEventElapsedTime(&m, r.a, r.b);
        fprintf(f, "%d,%d,%d,%d,%d,%.6f,%.0f\n", r.fam, r.M, r.N, r.K, r.epi, m, r.flops);
    }
    fclose(f);
    return 0;
}

// developer instrumentation (not part of the public header): s_memtime stamps of workgroup 0 of the decode kernels
__attribute__((visibility("default"))) int mellow_dev_kdebug(mellow_engine_t* e, int on, uint64_t* host_out64) {
    if (!e) return fail("null engine");
    static uint64_t* buf = nullptr;
    HIPCHK(hipSetDevice(e->device));
    if (on) {
        // [0, 64): phase stamps of workgroup 0; [64, 1024): (earliest start, latest end) of every launch of a decode step
        // (DecArgs::dbg_seq, 100 MHz clock), the starts initialised to the maximum
        if (!buf) HIPCHK(hipMalloc(&buf, 1024 * sizeof(uint64_t)));
        std::vector<uint64_t> init(1024, 0);
        for (int i = 64; i < 1024; i += 2) init[i] = ~0ull;
        HIPCHK(hipMemcpy(buf, init.data(), 1024 * sizeof(uint64_t), hipMemcpyHostToDevice));
        set_kernel_debug_buffer(buf);
        set_gemm_debug_buffer(buf);
        e->dbg_seq0 = 0;
    } else {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->dbg_seq0 = -1;
        // (host_out64 receives the 64 phase stamps; mellow_dev_kdebug_spans the launch spans)
        if (buf && host_out64) HIPCHK(hipMemcpy(host_out64, buf, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (buf) HIPCHK(hipMemcpy(e->dbg_spans, buf + 64, 960 * sizeof(uint64_t), hipMemcpyDeviceToHost));
        set_kernel_debug_buffer(nullptr);
        set_gemm_debug_buffer(nullptr);
    }
    return 0;
}

// the launch spans collected by the last mellow_dev_kdebug(on) .. (off) bracket: out[2 i] / out[2 i + 1] = earliest start / latest
// end (10 ns ticks) of launch i of the LAST decode step that ran inside the bracket; 480 pairs
__attribute__((visibility("default"))) int mellow_dev_kdebug_spans(mellow_engine_t* e, uint64_t* out960) {
    if (!e || !out960) return fail("null argument");
    memcpy(out960, e->dbg_spans, 960 * sizeof(uint64_t));
    return 0;
}

}  // extern "C"
