// Developer entry points (not used by the product path): GEMM timing and debug taps, profiler dump, kernel stamps.
#include "engine_internal.h"

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
