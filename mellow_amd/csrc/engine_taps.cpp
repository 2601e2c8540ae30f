// Launch taps (include/mellow_hip.h, not used by the product path): each runs one existing launcher on the caller's host data, on
// device buffers of the call's own, and returns the whole device output.  What the taps share is the record of one call (TapCall)
// and the checks below it; what each validates is knowledge of its launcher and stands in its function.
#include "engine_internal.h"

#include <deque>
#include <memory>

namespace {

// One output of a tap call: `bytes` bytes at the device address p, copied to `host` by TapCall::finish()
struct TapOut {
    float* p = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    bool fill = true;       // a buffer of its own that holds 0xFF bytes before the launch (else: TapCall::from names the buffer)
};

// One tap call.  It owns every device buffer of the call (freed when it goes), knows one way to upload host bytes and one to make a
// 0xFF-filled buffer, and keeps the list of outputs: each is declared once (out) while the arguments are still being checked,
// gets its buffer in begin() and is fetched in finish().  Nothing touches the device before begin().
struct TapCall {
    mellow_engine* e;
    hipStream_t s;
    std::deque<mellow_engine::Buf> bufs;
    std::deque<TapOut> outs;
    TapOut none;            // what the handle of an output the launch does not write addresses: p stays null

    explicit TapCall(mellow_engine* e_) : e(e_), s(e_->stream) {}

    // declares an output (before begin): refuses a null pointer or a capacity below `bytes`.  Outputs that share one capacity
    // argument (k / v pages, the cand_* arrays, record / logprob) are declared one by one with that capacity and its name.
    int out(TapOut*& o, bool wanted, void* host, const char* name, int64_t capacity, size_t bytes, const char* capacity_name, bool fill = true) {
        o = &none;
        if (!wanted) return 0;
        if (!host || capacity < (int64_t)bytes)
            return fail("%s %lld is short of the %lld bytes this call returns there (or %s is null)", capacity_name, (long long)capacity, (long long)bytes, name);
        outs.push_back(TapOut{nullptr, host, bytes, fill});
        o = &outs.back();
        return 0;
    }
    // an output that is no fresh fill buffer (declared with fill = false): the device buffer it is read from
    void from(TapOut* o, void* dev) { if (o != &none) o->p = reinterpret_cast<float*>(dev); }

    // the first device call of a tap, behind every check of its arguments
    int begin() {
        HIPCHK(hipSetDevice(e->device));
        for (TapOut& o : outs)
            if (o.fill) CHK(filled(o.p, o.bytes));
        return 0;
    }
    // `floats` floats of device memory, uninitialised
    template <class T> int scratch(T*& dev, size_t floats) {
        bufs.emplace_back();
        CHK(ensure(e, bufs.back(), floats));
        dev = (T*)bufs.back().p;
        return 0;
    }
    // `bytes` bytes that hold 0xFF (and 16 bytes nobody owns behind them)
    template <class T> int filled(T*& dev, size_t bytes) {
        float* p;
        CHK(scratch(p, (bytes + 3) / 4 + 4));
        HIPCHK(hipMemsetAsync(p, 0xFF, bytes, s));
        dev = (T*)p;
        return 0;
    }
    // `bytes` host bytes, uploaded
    template <class T> int in(T*& dev, const void* src, size_t bytes) {
        float* p;
        CHK(scratch(p, (bytes + 3) / 4 + 4));
        HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        dev = (T*)p;
        return 0;
    }
    // n device floats rounded to bf16 by launch_kv_to_bf16, at the head of a 0xFF-filled buffer of `bytes` bytes
    template <class T> int rounded(T*& dev16, const float* dev32, size_t n, size_t bytes) {
        CHK(filled(dev16, bytes));
        launch_kv_to_bf16(dev32, (void*)dev16, (int64_t)n, s);
        return 0;
    }
    // n host floats, uploaded; to16: then rounded to bf16, and dev addresses the rounded copy
    int in_bf16(const float*& dev, const float* src, size_t n, bool to16) {
        CHK(in(dev, src, n * 4));
        if (to16) CHK(rounded(dev, dev, n, n * 2));
        return 0;
    }
    // behind the launch: its error, the end of the stream's work, every declared output
    int finish() {
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        for (const TapOut& o : outs) HIPCHK(hipMemcpy(o.host, o.p, o.bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};

// ---- checks more than one tap makes ---------------------------------------------------------------------------------------------------
// map [n] is injective into [0, range); holes: entries of -1 (nobody) are passed over
int check_injective(const char* name, const int32_t* map, int n, const char* range_name, int range, bool holes, const char* tail = "") {
    std::vector<char> seen(range, 0);
    for (int i = 0; i < n; ++i) {
        const int r = map[i];
        if (holes && r == -1) continue;
        if (r < 0 || r >= range || seen[r]) return fail("%s[%d] = %d is outside [0, %s = %d) or taken twice%s", name, i, r, range_name, range, tail);
        seen[r] = 1;
    }
    return 0;
}
// an array the launch reads (needed) or has no use for
int no_operand(const void* p, const char* name) { return p ? fail("%s is not an operand of this launch", name) : 0; }
int operand(bool needed, const void* p, const char* name) {
    if (needed && !p) return fail("null argument: %s", name);
    return needed ? 0 : no_operand(p, name);
}
// a raw image the launch reads whole: exactly `need` bytes, or no image at all
int image_bytes(const char* name, const void* img, int64_t got, size_t need) {
    if ((need != 0) != (img != nullptr) || (img && got != (int64_t)need))
        return fail("%s: this launch takes %lld bytes there (got %lld)", name, (long long)need, img ? (long long)got : 0ll);
    return 0;
}
// the RoPE tables [Tmax][32] of a launch: the caller's, or the engine's own (mellow_host_rope_tables)
struct RopeTables {
    std::vector<float> own;
    const float *cos = nullptr, *sin = nullptr;
};
int rope_tables(mellow_engine* e, int Tmax, const float* cos, const float* sin, RopeTables& r) {
    r.cos = cos; r.sin = sin;
    if (cos) return 0;
    r.own.resize((size_t)Tmax * 64);
    r.cos = r.own.data(); r.sin = r.own.data() + (size_t)Tmax * 32;
    return mellow_host_rope_tables(e->cfg.rope_theta, 64, Tmax, r.own.data(), r.own.data() + (size_t)Tmax * 32);
}
// bytes of an attention tap's output.  Plain form: M + 32 rows of `width` floats; APB form: the image of rup(M, 128) rows, 6 bytes per element
size_t attn_out_bytes(int64_t M, int width, int out_form) {
    return out_form ? (size_t)rup((int)M, 128) * width * 6 : (size_t)(M + 32) * width * 4;
}

// host rows [n][B][width] -> device rows [n][rows][width], the slots B .. rows - 1 zero; behind them extra_rows rows of 0xFF bytes
int dec_tap_rows(TapCall& t, float*& dev, const float* src, int n, int B, int rows, int width, size_t extra_rows = 0) {
    std::vector<float> h(((size_t)n * rows + extra_rows) * width, 0.f);
    for (int s = 0; s < n; ++s) memcpy(h.data() + (size_t)s * rows * width, src + (size_t)s * B * width, (size_t)B * width * 4);
    if (extra_rows) memset(h.data() + (size_t)n * rows * width, 0xFF, extra_rows * width * 4);
    return t.in(dev, h.data(), h.size() * 4);
}
// host rows [n][B][K] -> n F32-layout images of `rows` rows (common.h f32_idx with K / 8 k-tiles), the slots B .. rows - 1 zero
int dec_tap_f32_layout(TapCall& t, float*& dev, const float* src, int n, int B, int rows, int K = 576) {
    std::vector<float> h((size_t)n * rows * K, 0.f);
    for (int s = 0; s < n; ++s)
        for (int r = 0; r < B; ++r)
            for (int k = 0; k < K; k += 4) {
                const size_t f4 = ((size_t)(r >> 5) * (K / 8) + (k >> 3)) * 64 + (r & 31) + 32 * ((k >> 2) & 1);
                memcpy(h.data() + (size_t)s * rows * K + f4 * 4, src + ((size_t)s * B + r) * K + k, 16);
            }
    return t.in(dev, h.data(), h.size() * 4);
}

// the int32 words a step-tail launch can rewrite, as the tap returns them (out_state): seen_stop [rows + 32] | n_seen, arrive, ticket,
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

extern "C" {

// ---- attention taps: one launch of a prefill or of the window attention launcher ------------------------------------------------------
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
    TapCall t(e);
    TapOut* o;
    CHK(t.out(o, true, out, "out", out_capacity, attn_out_bytes(M, 576, out_form), "out_capacity"));
    CHK(t.begin());
    const bool p16 = variant == 3;
    const size_t page_floats = (size_t)B * 3 * Tmax * 64;
    const float *dq, *dk, *dv;
    CHK(t.in_bf16(dq, q, (size_t)M * 576, p16));
    CHK(t.in_bf16(dk, k, page_floats, p16));
    CHK(t.in_bf16(dv, v, page_floats, p16));
    float* o_rows = out_form ? nullptr : o->p;
    void* o_apb = out_form ? o->p : nullptr;
    if (qpos0 > 0) launch_prefill_attention_past(dq, dk, dv, o_rows, o_apb, B, T, Tmax, qpos0, variant == 1, t.s);
    else launch_prefill_attention(dq, dk, dv, o_rows, o_apb, B, T, Tmax, variant >= 1, t.s, nullptr, variant >= 2, p16);
    return t.finish();
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
    TapCall t(e);
    TapOut* o;
    CHK(t.out(o, true, out, "out", out_capacity, attn_out_bytes(M, C, out_form), "out_capacity"));
    CHK(t.begin());
    const float *dx, *db, *dm = nullptr;
    CHK(t.in_bf16(dx, qkv, (size_t)M * 3 * C, in16 != 0));
    CHK(t.in(db, bias, (size_t)nH * 64 * 64 * 4));
    if (mask) CHK(t.in(dm, mask, (size_t)nW * 64 * 64 * 4));
    launch_window_attention(dx, out_form ? nullptr : o->p, M, C, nH, db, dm, mask ? nW : 1, t.s, out_form ? o->p : nullptr, in16 != 0);
    return t.finish();
}

// ---- GEMM epilogue tap: one launch of a GEMM launcher with the epilogue the caller describes -------------------------------------------
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
            CHK(check_injective("crow_map", crow_map, d->rows_in, "rows_out", d->rows_out, false));
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
    // the outputs
    const int parts = N / 64;
    const size_t kv_bytes = (size_t)(B + 1) * 3 * d->Tmax * 64 * 4;      // one page set of no example behind the last
    const bool wc = !qkv && d->want_c, wc3 = !qkv && d->want_c3, wssq = lin_ && d->want_ssq;
    TapCall t(e);
    TapOut *oC, *oC3, *oSsq, *oQ, *oK, *oV;
    CHK(t.out(oC, wc, out_c, "out_c", c_capacity, (size_t)(c_rows + 32) * ldc * 4, "c_capacity"));
    CHK(t.out(oC3, wc3, out_c3, "out_c3", c3_capacity, (size_t)rup(M, 128) * N * 6, "c3_capacity"));
    CHK(t.out(oSsq, wssq, out_ssq, "out_ssq", ssq_capacity, (size_t)(M + 32) * (parts > 0 ? parts : 1) * 4, "ssq_capacity"));
    CHK(t.out(oQ, qkv, out_q, "out_q", q_capacity, (size_t)(M + 32) * 576 * 4, "q_capacity"));
    CHK(t.out(oK, qkv, out_k, "out_k", kv_capacity, kv_bytes, "kv_capacity"));
    CHK(t.out(oV, qkv, out_v, "out_v", kv_capacity, kv_bytes, "kv_capacity"));

    CHK(t.begin());
    hipStream_t s = t.s;
    const int Nrows = swi ? Nw / 2 : Nw;                 // rows of one logical weight matrix
    const int Nwp = swi ? 64 * ((Nrows + 31) / 32) : Nw;      // packed rows: pairs come in 64-row groups of 32 gate + 32 up
    const int NP = rup(Nwp, 128);
    float *dA, *dW, *dWp, *dPB, *dA3 = nullptr;
    CHK(t.in(dA, A, (size_t)M * K * 4));
    CHK(t.in(dW, W, (size_t)Nw * K * 4));
    CHK(t.scratch(dWp, (size_t)NP * K));
    if (swi) launch_pack_weight_pairs(dW, dW + (size_t)Nrows * K, Nrows, K, K, dWp, NP, K, s);
    else launch_pack_weight(dW, Nw, K, K, dWp, NP, K, s);
    GemmArgs g;
    g.A = dA; g.lda = K; g.M = M; g.K = K; g.Wp = dWp; g.Nw = Nwp; g.N = N; g.ldc = ldc;
    g.epi = lin_ ? EPI_LINEAR : swi ? EPI_SWIGLU : d->pos0 > 0 ? EPI_QKV_ROPE_AT : EPI_QKV_ROPE;
    if (kernel != 0) {
        CHK(t.scratch(dPB, (size_t)NP * K * 6 / 4));
        launch_pack_bf16x3(dWp, NP, K, dPB, s);
        g.W8 = reinterpret_cast<const uint8_t*>(dPB);
    }
    if (kernel == 17) {
        CHK(t.scratch(dA3, (size_t)rup(M, 128) * K * 6 / 4));
        g.A8 = reinterpret_cast<const uint8_t*>(dA3); g.lda8 = (int64_t)3 * (K >> 3);
    }
    if (has_rs) {
        CHK(t.in(g.rs_ssq, rs_ssq, (size_t)M * d->rs_parts * 4));
        g.rs_parts = d->rs_parts; g.rs_dim = d->rs_dim; g.rs_eps = d->rs_eps;
    }
    g.C = oC->p; g.C3 = oC3->p; g.ssq_out = oSsq->p;
    if (wssq) g.ssq_parts = parts;
    if (lin_) {
        g.act = d->act;
        if (d->bias) {           // the launchers read whole float4 of columns < N: the columns past Nw hold zeros, as the engine's padded biases do
            std::vector<float> hb(rup(N, 128), 0.f);
            memcpy(hb.data(), bias, (size_t)Nw * 4);
            CHK(t.in(g.bias, hb.data(), hb.size() * 4));
        }
        if (crow_map) {
            CHK(t.in(g.crow_map, crow_map, (size_t)d->rows_in * 4));
            g.rows_in = d->rows_in; g.rows_out = d->rows_out;
        }
        if (d->resid == 1) {                                // resid host [c_rows][N]
            CHK(t.in(g.resid, resid, (size_t)c_rows * N * 4));
            g.ldr = N;
        } else if (d->resid == 2) {                         // in place: the residual is loaded into C after the fill
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy2D(oC->p, (size_t)ldc * 4, resid, (size_t)N * 4, (size_t)N * 4, (size_t)c_rows, hipMemcpyHostToDevice));
            g.resid = oC->p; g.ldr = ldc;
        }
    }
    if (qkv) {
        RopeTables r;
        CHK(rope_tables(e, d->Tmax, rope_cos, rope_sin, r));
        CHK(t.in(g.rope_cos, r.cos, (size_t)d->Tmax * 32 * 4));
        CHK(t.in(g.rope_sin, r.sin, (size_t)d->Tmax * 32 * 4));
        g.q_out = oQ->p; g.k_cache = oK->p; g.v_cache = oV->p;
        g.T = Tq; g.Tmax = d->Tmax; g.pos0 = d->pos0; g.q_heads = 9; g.kv_heads = 3;
    }
    if (d->splitk_max) {         // the engine's own workspace, as with_splitk hands it to the encoder chain
        CHK(ensure(e, e->sk_ws, (size_t)512 * 16384));
        g.sk_ws = e->sk_ws.p; g.sk_tiles = 256; g.sk_max = d->splitk_max;
    }
    g.no_x3w = d->no_x3w != 0;
    if (kernel == 0) launch_gemm(g, s);
    else if (kernel == 16) launch_gemm_bf16x3_fused(g, s);
    else { launch_split_rows_apb(dA, K, M, K, dA3, s); launch_gemm_bf16x3_apb(g, s); }
    return t.finish();
}

// ---- norm / hand-over tap: one launch of a norm launcher, of launch_split_rows_apb or of launch_quant_mx8 on the caller's rows ---------
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
        CHK(check_injective("row_map", row_map, ntok, "ntok", ntok, false, ": not a permutation"));
    }
    // the outputs
    const int KT64 = (C + 63) / 64, KQ = (KT64 + 3) / 4;
    const size_t Mp = (size_t)rup((int)rows, 128);
    TapCall t(e);
    TapOut *o, *oSc;
    CHK(t.out(o, true, out, "out", out_capacity, form == 0 ? (size_t)(rows + 32) * width * 4 : form == 1 ? Mp * C * 6 : Mp * rup(C, 64), "out_capacity"));
    CHK(t.out(oSc, form == 2, out_scales, "out_scales", scales_capacity, Mp * 8 * KQ, "scales_capacity"));

    CHK(t.begin());
    hipStream_t s = t.s;
    float *dx, *dw = nullptr, *db = nullptr;
    const int32_t* dmap = nullptr;
    CHK(t.in(dx, x, (op == 1 ? (size_t)n * R * R * C : (size_t)M * C) * 4));
    if (w) CHK(t.in(dw, w, (size_t)width * 4));
    if (b && op <= 1) CHK(t.in(db, b, (size_t)width * 4));
    if (row_map) CHK(t.in(dmap, row_map, (size_t)ntok * 4));
    const int nt = row_map ? ntok : M;
    if (op == 0) {
        if (form == 0) launch_layernorm(dx, o->p, M, C, dw, db, dmap, nt, s);
        else launch_layernorm_apb(dx, o->p, M, C, dw, db, dmap, nt, s, oSc->p);
    } else if (op == 1) {
        launch_merge_layernorm(dx, o->p, n, R, C, dw, db, s);
    } else if (op == 2) {
        if (form == 0) launch_rmsnorm(dx, o->p, M, C, dw, eps, s);
        else launch_rmsnorm_apb(dx, o->p, M, C, dw, eps, s, oSc->p);
    } else {
        if (form == 1) launch_split_rows_apb(dx, C, M, C, o->p, s);
        else launch_quant_mx8(dx, C, M, C, o->p, oSc->p, s);
    }
    return t.finish();
}

// ---- decode attention tap: one launch_dec_attn and, with Wo, one launch_dec_oproj on DecArgs filled from buffers of the call's own -----
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
    if (row_of_slot) CHK(check_injective("row_of_slot", row_of_slot, rows, "P", P, true));
    if (d->want_x3 && !Wo) return fail("want_x3 without Wo: the pre-split images are written by the o_proj launch");
    if (!slabs || !x_res || !k_pages || !v_pages || !out_gs) return fail("null argument: slabs, x_res, k_pages, v_pages and out_gs are required");
    if (!fused && !ssq1) return fail("null argument: fused 0 needs ssq1");
    if (fused && !down) return fail("null argument: fused 1 needs the down slabs");
    if (!(d->eps >= 0.f && d->eps < INFINITY)) return fail("eps = %g must be finite and >= 0", d->eps);
    // the outputs: the page arrays are the buffers the launch reads; x_new holds the caller's rows unless the fused launch forms it
    const size_t n_x = (size_t)rows * 576, page_elems = (size_t)3 * Tmax * 64;
    const size_t kv_bytes = (size_t)(P + 1) * page_elems * (kv16 ? 2 : 4);
    TapCall t(e);
    TapOut *oAtt, *oMl, *oK, *oV, *oXnew, *oXmid, *oX16, *oSsq;
    CHK(t.out(oAtt, true, out_att, "out_att", att_capacity, ((size_t)ts * n_x + 32 * 576) * 4, "att_capacity"));
    CHK(t.out(oMl, true, out_ml, "out_ml", ml_capacity, (size_t)9 * rows * ts * 2 * 4, "ml_capacity"));
    CHK(t.out(oK, true, out_k, "out_k", kv_capacity, kv_bytes, "kv_capacity", false));
    CHK(t.out(oV, true, out_v, "out_v", kv_capacity, kv_bytes, "kv_capacity", false));
    CHK(t.out(oXnew, true, out_xnew, "out_xnew", xnew_capacity, (size_t)(rows + 32) * 576 * 4, "xnew_capacity", fused));
    CHK(t.out(oXmid, Wo != nullptr, out_xmid, "out_xmid", xmid_capacity, n_x * 4, "xmid_capacity"));
    CHK(t.out(oX16, Wo != nullptr, out_x16, "out_x16", x16_capacity, d->want_x3 ? 2 * n_x * 6 : n_x * 4, "x16_capacity"));
    CHK(t.out(oSsq, Wo != nullptr, out_ssq, "out_ssq", ssq_capacity, (size_t)(rows + 32) * 40 * 4, "ssq_capacity"));
    const int gs = dec_attn_split_groups(ctx_end, ts, kv16);
    *out_gs = gs;

    CHK(t.begin());
    hipStream_t s = t.s;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    DecArgs a;
    a.rows = rows; a.RB = RB; a.Tmax = Tmax; a.eps = d->eps; a.gs = gs; a.ts = ts; a.kv16 = kv16 ? 1 : 0;
    a.slabF_stride4 = (int64_t)(n_x / 4); a.attF16 = oAtt->p; a.att_ml = oMl->p;
    CHK(dec_tap_rows(t, a.pq, slabs, fused ? Q2_NPQ : DEC_KC_QKV, B, rows, 960));
    std::vector<float> hr(64);
    if (rope_cur) memcpy(hr.data(), rope_cur, 256);
    else {
        RopeTables r;
        CHK(rope_tables(e, Tmax, nullptr, nullptr, r));
        memcpy(hr.data(), r.cos + (size_t)pos * 32, 128);
        memcpy(hr.data() + 32, r.sin + (size_t)pos * 32, 128);
    }
    CHK(t.in(a.rope_cur, hr.data(), 256));
    if (fused) {
        CHK(dec_tap_f32_layout(t, a.xmidF, x_res, 1, B, rows));
        CHK(dec_tap_f32_layout(t, a.dslabF, down, Q2_HC, B, rows));
    } else {
        CHK(dec_tap_rows(t, a.ssq1, ssq1, 1, B, rows, DEC_KC_QKV));
        float* dx;
        CHK(dec_tap_rows(t, dx, x_res, 1, B, rows, 576, 32));
        t.from(oXnew, dx);
    }
    a.xnewR = oXnew->p;
    // the pages: P sets from the caller and one of no example (0xFF bytes) behind them
    auto pages = [&](TapOut* o, const float* src) -> int {
        float *p32, *p16;
        CHK(t.filled(p32, (size_t)(P + 1) * page_elems * 4));
        HIPCHK(hipMemcpyAsync(p32, src, (size_t)P * page_elems * 4, hipMemcpyHostToDevice, s));
        t.from(o, p32);
        if (kv16) {
            CHK(t.rounded(p16, p32, (size_t)P * page_elems, kv_bytes));
            t.from(o, p16);
        }
        return 0;
    };
    CHK(pages(oK, k_pages));
    CHK(pages(oV, v_pages));
    // the device words: position | blk_live [RB] | row_of_slot [rows]
    std::vector<int32_t> hw(1 + RB + rows, 1);
    hw[0] = pos;
    const bool blk = blk_live || row_of_slot;         // (the kernels read row_of_slot in their early-exit instantiation only)
    if (blk_live) memcpy(hw.data() + 1, blk_live, (size_t)RB * 4);
    if (row_of_slot) memcpy(hw.data() + 1 + RB, row_of_slot, (size_t)rows * 4);
    int32_t* dw;
    CHK(t.in(dw, hw.data(), hw.size() * 4));
    a.d_pos = dw; a.blk_live = blk ? dw + 1 : nullptr; a.row_of_slot = row_of_slot ? dw + 1 + RB : nullptr;
    float* dWp = nullptr;
    if (Wo) {
        float* dW;
        CHK(t.in(dW, Wo, (size_t)576 * 576 * 4));
        CHK(t.scratch(dWp, (size_t)576 * 576));
        launch_pack_weight16(dW, 576, 576, dWp, s);
    }
    if (!launch_dec_attn(a, oK->p, oV->p, fused, s)) return fail("decode attention launched with %d key splits at RB = %d", a.ts, a.RB);
    if (Wo) {
        DecArgs o = a;
        o.xmidF = oXmid->p; o.ssq = oSsq->p;
        if (d->want_x3) { o.xmid3_32 = oX16->p; o.xmid3_16 = reinterpret_cast<char*>(oX16->p) + n_x * 6; }
        else o.xmidF16 = oX16->p;
        launch_dec_oproj(o, dWp, s);
    }
    return t.finish();
}

// ---- decode GEMV tap: one call of launch_dec_qkv, launch_dec_gateup / launch_dec_gateup3, launch_dec_down, launch_dec_qkv2 /
// launch_dec_qkv2x3 or launch_dec_final_norm on DecArgs filled from buffers of the call's own; the weights packed by the loader's
// routines (engine_weights.cpp) ------------------------------------------------------------------------------------------------------
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
    CHK(operand(need_x, x, "x"));
    CHK(operand(need_h, h, "h"));
    if ((kcd != 0) != (down != nullptr)) return fail(kcd ? "null argument: down" : "down without kcd");
    const size_t x_img_need = op == 1 ? (form ? n_x * 6 : n_x * 4) : (op == 3 && form == 1 ? n_x * 6 : 0);
    const size_t h_img_need = op == 3 && form == 1 ? n_h * 6 : 0;
    CHK(image_bytes("x_img", x_img, x_img_bytes, x_img_need));
    CHK(image_bytes("h_img", h_img, h_img_bytes, h_img_need));
    if ((op == 1) != (ssq != nullptr)) return fail(op == 1 ? "null argument: ssq" : "ssq goes with op 1 only");
    // the outputs: the position word and the block snapshot are read from the device words
    const bool w_pq = op == 0 || op == 3, w_down = op == 2 || op == 3, w_x3 = op == 4 && d->want_x3;
    TapCall t(e);
    TapOut *oPq, *oDown, *oSsq1, *oXnew, *oRope, *oPos, *oGu, *oH3, *oXn, *oSnap, *oQ;
    CHK(t.out(oPq, w_pq, out_pq, "out_pq", pq_capacity, ((size_t)DEC_KC_QKV * rows + 32) * 960 * 4, "pq_capacity"));
    CHK(t.out(oDown, w_down, out_down, "out_down", down_capacity, ((size_t)DEC_KC_DOWN * n_x + 32 * 576) * 4, "down_capacity"));
    CHK(t.out(oSsq1, op == 0, out_ssq1, "out_ssq1", ssq1_capacity, (size_t)(rows + 32) * DEC_KC_QKV * 4, "ssq1_capacity"));
    CHK(t.out(oXnew, op == 0, out_xnew, "out_xnew", xnew_capacity, (size_t)(rows + 32) * 576 * 4, "xnew_capacity"));
    if (op == 0 && (!out_rope || !out_pos)) return fail("null argument: out_rope (128 floats) and out_pos are required with op 0");
    CHK(t.out(oRope, op == 0, out_rope, "out_rope", 128 * 4, 128 * 4, "out_rope"));
    CHK(t.out(oPos, op == 0, out_pos, "out_pos", 4, 4, "out_pos", false));
    CHK(t.out(oGu, op == 1, out_gu, "out_gu", gu_capacity, (n_h + 32 * 1536) * 4, "gu_capacity"));
    CHK(t.out(oH3, op == 1 && form == 1, out_h3, "out_h3", h3_capacity, (n_h + 32 * 1536) * 6, "h3_capacity"));
    CHK(t.out(oXn, op == 4, out_xn, "out_xn", xn_capacity, (n_x + 32 * 576) * (w_x3 ? 6 : 4), "xn_capacity"));
    if (op == 4 && blk_live && !out_snap) return fail("null argument: out_snap (64 words) is required with op 4 and blk_live");
    CHK(t.out(oSnap, op == 4 && out_snap, out_snap, "out_snap", 64 * 4, 64 * 4, "out_snap", false));
    CHK(t.out(oQ, op == 3, out_q, "out_q", q_capacity, (size_t)960 * 1536 * 4, "q_capacity"));      // the composed W' Wd

    CHK(t.begin());
    hipStream_t s = t.s;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    // the device words: position | blk_live [32] (zeros behind RB) | blk_snap [32] + 32 words nobody owns (0xFF bytes)
    std::vector<int32_t> hw(1 + 32 + 64, -1);
    hw[0] = pos;
    for (int i = 0; i < 32; ++i) hw[1 + i] = blk_live && i < RB ? blk_live[i] : 0;
    int32_t* dw;
    CHK(t.in(dw, hw.data(), hw.size() * 4));
    t.from(oPos, dw);
    t.from(oSnap, dw + 33);
    DecArgs a;
    a.rows = rows; a.RB = RB; a.Tmax = Tmax; a.eps = d->eps; a.d_pos = dw; a.first = first ? 1 : 0; a.inc_pos = inc_pos ? 1 : 0;
    a.slabF_stride4 = (int64_t)(n_x / 4);
    a.blk_live = blk_live ? dw + 1 : nullptr; a.blk_snap = dw + 33;
    if (need_x) CHK(dec_tap_f32_layout(t, a.xmidF, x, 1, B, rows));
    if (need_h) CHK(dec_tap_f32_layout(t, a.guF, h, 1, B, rows, 1536));
    if (kcd) CHK(dec_tap_f32_layout(t, a.dslabF, down, DEC_KC_DOWN, B, rows));
    if (w_pq) a.pq = oPq->p;
    if (w_down) a.dslabF = oDown->p;
    float *dW, *dW2, *dWp, *dWp2, *dX, *dH;
    if (op == 0) {
        CHK(t.in(dW, W, (size_t)960 * 576 * 4));
        CHK(t.scratch(dWp, (size_t)1024 * 576));
        launch_pack_weight(dW, 960, 576, 576, dWp, 1024, 576, s);
        a.ssq1 = oSsq1->p; a.xnewR = oXnew->p; a.rope_cur = oRope->p;
        if (first) {
            RopeTables r;
            CHK(rope_tables(e, Tmax, rope_cos, rope_sin, r));
            CHK(t.in(a.rope_cos, r.cos, (size_t)Tmax * 32 * 4));
            CHK(t.in(a.rope_sin, r.sin, (size_t)Tmax * 32 * 4));
        }
        launch_dec_qkv(a, dWp, 72, kcd, s);
    } else if (op == 1) {
        std::vector<float> il;
        interleave_gate_up8(W, W2, 1536, 576, il);
        CHK(t.in(dW, il.data(), il.size() * 4));
        CHK(t.scratch(dWp, il.size()));
        if (form) launch_pack_weight16n(dW, 3072, 576, dWp, s);
        else launch_pack_weight16(dW, 3072, 576, dWp, s);
        CHK(t.in(dX, x_img, x_img_need));
        CHK(t.in(a.ssq, ssq, (size_t)rows * 40 * 4));
        a.guF = oGu->p;
        if (form) {
            a.xmid3_16 = dX; a.h3 = oH3->p;
            launch_dec_gateup3(a, dWp, s);
        } else {
            a.xmidF16 = dX;
            launch_dec_gateup(a, dWp, s);
        }
    } else if (op == 2) {
        CHK(t.in(dW, W, (size_t)576 * 1536 * 4));
        CHK(t.scratch(dWp, (size_t)640 * 1536));
        launch_pack_weight(dW, 576, 1536, 1536, dWp, 640, 1536, s);
        launch_dec_down(a, dWp, 192, s);
    } else if (op == 3) {
        float* dCat;
        CHK(t.in(dW, W, (size_t)960 * 576 * 4));
        CHK(t.in(dW2, W2, (size_t)576 * 1536 * 4));
        CHK(t.scratch(dCat, (size_t)1024 * 2112));
        CHK(t.scratch(dWp, (size_t)1024 * 2112));
        CHK(t.scratch(dWp2, (size_t)640 * 1536));
        launch_compose_f64(dW, dW2, oQ->p, 960, 1536, 576, s);
        CHK(pack_qkv2_cat(e, dW, oQ->p, dCat, dWp));
        launch_pack_weight(dW2, 576, 1536, 1536, dWp2, 640, 1536, s);
        if (form) {
            CHK(t.in(dX, x_img, x_img_need));
            CHK(t.in(dH, h_img, h_img_need));
            a.xmid3_32 = dX; a.h3 = dH;
            launch_dec_qkv2x3(a, dWp, dWp2, s);
        } else {
            launch_dec_qkv2(a, dWp, dWp2, s);
        }
    } else {
        CHK(t.in(dW, W, (size_t)576 * 4));
        if (w_x3) a.xn3 = oXn->p; else a.xnF = oXn->p;
        launch_dec_final_norm(a, dW, kcd, s);
    }
    return t.finish();
}

// ---- decode step-tail tap: one call of launch_dec_lm_head, launch_dec_argmax, launch_dec_compact or launch_dec_load_rows on DecArgs /
// LoopArgs filled from buffers of the call's own; the head weight packed as the loader packs lm_head (engine_weights.cpp:
// launch_pack_weight into roundup(V, 128) rows) ----------------------------------------------------------------------------------------
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
    CHK(operand(head || write_x, W, "W"));
    CHK(operand((head && form == 0) || pack || load, x, "x"));
    const size_t x_img_need = head && form == 1 ? (size_t)rows * 576 * 6 : 0;
    CHK(image_bytes("x_img", x_img, x_img_bytes, x_img_need));
    CHK(operand(amax, cand_val, "cand_val"));
    CHK(operand(amax, cand_idx, "cand_idx"));
    if (!amax) CHK(no_operand(cand_sum, "cand_sum"));
    if (lp_on && !cand_sum) return fail("with_logprob without cand_sum: the log-prob is merged from the head's partial sums");
    if (lp_on && !state) return fail("with_logprob without with_state: the log-prob is written where the token record is");
    CHK(operand(state || pack, seen_stop, "seen_stop"));
    if (!state) CHK(operand(pack, row_of_slot, "row_of_slot"));
    if (!(state || pack)) CHK(no_operand(blk_left, "blk_left"));
    if (load || (amax && !state)) CHK(no_operand(blk_live, "blk_live"));
    if (pack && (!blk_live || !blk_left)) return fail("null argument: op 2 needs blk_live and blk_left");
    if (state && (blk_live == nullptr) != (blk_left == nullptr)) return fail("blk_live and blk_left go together (LoopArgs: the count and the word it clears)");
    if (!state) CHK(no_operand(blk_snap, "blk_snap"));
    if ((blk_live || blk_left || blk_snap || row_of_slot) && RB < 2)
        return fail("blk_live / blk_left / blk_snap / row_of_slot exist from two row blocks on (RB = %d)", RB);
    if (!load) CHK(no_operand(row_ids, "row_ids"));
    if (row_of_slot) CHK(check_injective("row_of_slot", row_of_slot, rows, "rows", rows, true));
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
    // the outputs: the state is the head of the device words
    const TailWords tw{rows};
    const size_t cand_bytes = (size_t)(rows + 32) * n * 4, record_bytes = (size_t)rows * max_len * 4;
    TapCall t(e);
    TapOut *oLogits, *oCv, *oCi, *oCs, *oTok, *oRec, *oLp, *oState, *oX;
    CHK(t.out(oLogits, head, out_logits, "out_logits", logits_capacity, (size_t)(rows + 32) * V * 4, "logits_capacity"));
    CHK(t.out(oCv, head, out_cand_val, "out_cand_val", cand_capacity, cand_bytes, "cand_capacity"));
    CHK(t.out(oCi, head, out_cand_idx, "out_cand_idx", cand_capacity, cand_bytes, "cand_capacity"));
    CHK(t.out(oCs, head, out_cand_sum, "out_cand_sum", cand_capacity, cand_bytes, "cand_capacity"));
    CHK(t.out(oTok, amax, out_tokens, "out_tokens", tokens_capacity, (size_t)(rows + 32) * 4, "tokens_capacity"));
    CHK(t.out(oRec, state, out_record, "out_record", record_capacity, record_bytes, "record_capacity"));
    CHK(t.out(oLp, lp_on, out_logprob, "out_logprob", record_capacity, record_bytes, "record_capacity"));
    CHK(t.out(oState, state || pack, out_state, "out_state", state_capacity, (size_t)tw.state_words() * 4, "state_capacity", false));
    if (state && !out_progress) return fail("null argument: out_progress is required with with_state");
    CHK(t.out(oX, !head, out_x, "out_x", x_capacity, (size_t)(rows + 32) * 576 * 4, "x_capacity"));

    CHK(t.begin());
    hipStream_t s = t.s;
    dec_prepare_lds_attributes();
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
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
    int32_t* dw;
    CHK(t.in(dw, hw.data(), hw.size() * 4));
    t.from(oState, dw);
    a.d_pos = dw + tw.pos();
    struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
    std::unique_ptr<unsigned long long, HostFree> h_prog;       // the mapped host word the last arrival publishes to
    if (head) {
        float *dW, *dWp;
        CHK(t.in(dW, W, (size_t)V * 576 * 4));
        const int NP = rup(V, 128);
        CHK(t.scratch(dWp, (size_t)NP * 576));
        launch_pack_weight(dW, V, 576, 576, dWp, NP, 576, s);
        if (form) { CHK(t.in(a.xn3, x_img, x_img_need)); a.x3 = DEC_X3_HEAD; }
        else CHK(dec_tap_f32_layout(t, a.xnF, x, 1, B, rows));
        a.logits = d->want_logits ? oLogits->p : nullptr;
        a.cand_val = oCv->p; a.cand_idx = reinterpret_cast<int32_t*>(oCi->p); a.cand_sum = d->want_sum ? oCs->p : nullptr;
        a.blk_live = blk_live ? dw + tw.live() : nullptr;
        launch_dec_lm_head(a, dWp, 72, V, s);
    } else if (amax) {
        const float* dEmbed = nullptr;
        CHK(t.in(a.cand_val, cand_val, (size_t)B * n * 4));
        CHK(t.in(a.cand_idx, cand_idx, (size_t)B * n * 4));
        if (cand_sum) CHK(t.in(a.cand_sum, cand_sum, (size_t)B * n * 4));
        if (write_x) CHK(t.in(dEmbed, W, (size_t)V * 576 * 4));
        a.xmidF = oX->p;
        LoopArgs lp;
        if (state) {
            unsigned long long *hp = nullptr, *d_prog = nullptr;
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hp), 64, hipHostMallocMapped | hipHostMallocCoherent));
            h_prog.reset(hp);
            memset(hp, 0xFF, 64);
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_prog), hp, 0));
            lp.out_tokens = reinterpret_cast<int32_t*>(oRec->p); lp.params = dw + tw.params(); lp.seen_stop = dw + tw.seen();
            lp.n_seen = dw + tw.scalars(); lp.arrive = dw + tw.scalars() + 1; lp.ticket = dw + tw.scalars() + 2;
            if (blk_left) { lp.blk_left = dw + tw.left(); lp.blk_live = dw + tw.live(); }
            if (blk_snap) lp.blk_snap = dw + tw.snap();
            if (row_of_slot) lp.row_of_slot = dw + tw.slot();
            lp.host_progress = d_prog; lp.T0 = d->T0;
            lp.out_logprob = oLp->p;
        }
        launch_dec_argmax(a, B, n, reinterpret_cast<int32_t*>(oTok->p), dEmbed, write_x ? 1 : 0, lp, s);
    } else if (pack) {
        // x in F32-layout, in front of 32 rows of margin that hold 0xFF bytes
        float* dIn;
        CHK(dec_tap_f32_layout(t, dIn, x, 1, B, rows));
        HIPCHK(hipMemcpyAsync(oX->p, dIn, (size_t)rows * 576 * 4, hipMemcpyDeviceToDevice, s));
        a.xmidF = oX->p;
        LoopArgs lp;
        lp.seen_stop = dw + tw.seen(); lp.blk_left = dw + tw.left(); lp.blk_live = dw + tw.live(); lp.row_of_slot = dw + tw.slot();
        lp.n_compactions = dw + tw.scalars() + 3;
        launch_dec_compact(a, B, lp, s);
    } else {
        const float* dIn;
        const int32_t* dIds = nullptr;
        CHK(t.in(dIn, x, (size_t)d->n_src * ld * 4));
        if (row_ids) CHK(t.in(dIds, row_ids, (size_t)B * 4));
        a.xmidF = oX->p;
        launch_dec_load_rows(a, B, dIn, ld, dIds, d->T_last, row_ids ? d->n_src : 0, s);
    }
    CHK(t.finish());
    if (state) *out_progress = *h_prog.get();
    return 0;
}

}  // extern "C"
