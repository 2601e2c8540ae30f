// The dense GEMM dispatch (run_gemm: the input's hand-over picks the kernel, the caller's chain the stream) and the audio path: front-end
// (A1-A3), HTSAT encoder (A4-A10: swin_block is one block's launches; run_encoder the stage loop around it), c2l + projection (A11-A13); taps.
#include "engine_internal.h"

// ---- GEMM wrappers -------------------------------------------------------------------------------------------------------
// split-K workspace of the f32x3 kernels (kernels.h: sk_*), handed to launches of the encoder chain only
static void with_splitk(mellow_engine* e, GemmArgs& g) {
    if (!e->sk_enable || e->opt.sk_max < 2 || !e->sk_ws.p) return;
    g.sk_ws = e->sk_ws.p;
    g.sk_tiles = 256;
    g.sk_max = e->opt.sk_max;
}
struct GemmScope : ProfScope {      // one record of the family: the shape, and the epilogue code + the kernel's hundred
    GemmScope(mellow_engine* e, hipStream_t chain, const GemmArgs& a, int kernel) : ProfScope(e, PF_GEMM, gemm_flops(a), 0.0, chain) {
        r.M = a.M; r.N = a.Nw; r.K = a.K; r.epi = a.epi + kernel;
    }
};
// The one dispatch of every dense GEMM of encoder and prefill (engine_internal.h): `in` picks the kernel family, `chain`
// is the stream of the launch and of its profile record.
int run_gemm(mellow_engine* e, hipStream_t chain, const GemmArgs& a, const HandOver& in) {
    GemmArgs g = a;
    const bool main_chain = chain == e->stream;
    if (e->prof_on && !main_chain) return fail("internal: a profiled GEMM outside the main chain");      // profiling forces ONE chain
    // The activation arrives from its PRODUCER already in the GEMM's operand format and LDS order, and both operands are staged by
    // LDS-DMA; counted in the same profile family as every other dense GEMM.
    //   fp8 mode:   AMX image (MXFP8) + its scale bytes -> gemm_mx8_kernel
    //   f32x3 mode: APB image (three bf16 pieces, common.h) -> gemm_x3q_kernel
    if (in.image && in.scales) {
        auto it = e->w.fp8_w.find(a.Wp);
        if (it == e->w.fp8_w.end()) return fail("internal: no e4m3 copy of this weight");
        g.A8 = reinterpret_cast<const uint8_t*>(in.image); g.a_sc = reinterpret_cast<const uint32_t*>(in.scales); g.lda8 = rup(a.K, 64);
        g.W8 = it->second.w8; g.w_scale = it->second.scale;
        GemmScope ps(e, chain, a, 500);
        launch_gemm_fp8(g, chain);
        return 0;
    }
    if (in.image) {
        auto it = e->w.bf_w.find(a.Wp);
        if (it == e->w.bf_w.end()) return fail("internal: no bf16-split copy of this weight");
        g.A8 = reinterpret_cast<const uint8_t*>(in.image);
        g.W8 = reinterpret_cast<const uint8_t*>(it->second);
        if (main_chain) with_splitk(e, g);        // (one workspace: a side chain's launches never split K)
        g.no_x3w = !e->opt.x3w;
        GemmScope ps(e, chain, a, 300);
        launch_gemm_bf16x3_apb(g, chain);
        return 0;
    }
    // fp32 rows in g.A.  These paths own e->a8 and (above) sk_ws, one buffer each: the main chain only -- a span that is not APB is
    // never split (prefill_parts, engine_lm.cpp), and the encoder is one chain.
    if (!main_chain) return fail("internal: a GEMM on fp32 rows outside the main chain");
    // f32x3: every dense GEMM of encoder + prefill, the STFT (EPI_POWER, K = 1024, framed A operand) and the mel projection
    // included (-0.6 ms per pass).  Through the split kernel the power spectrum differs from the ORACLE's fp32 conv1d by 2.5e-6
    // of its maximum -- two fp32 summation orders of a 1024-term dot product, squared -- while against an fp64 STFT it is
    // closer than the oracle's own fp32 arithmetic (tests/test_gpu_parity.py::test_encoder_taps holds it to both).
    // Option "x3_stft" = 0 keeps the front-end on the exact fp32 kernel.
    if (e->opt.f32x3_terms && a.K % 16 == 0 &&
        ((a.a_mode == A_PLAIN && (a.epi == EPI_LINEAR || a.epi == EPI_SWIGLU || a.epi == EPI_QKV_ROPE || a.epi == EPI_QKV_ROPE_AT)) || (e->opt.x3_stft && a.K >= 192))) {
        auto it = e->w.bf_w.find(a.Wp);
        if (it != e->w.bf_w.end()) {
            // fused kernel: A stays fp32 (global and LDS) and is split into its three bf16 terms in registers
            g.W8 = reinterpret_cast<const uint8_t*>(it->second);
            with_splitk(e, g);
            GemmScope ps(e, chain, a, 200);
            launch_gemm_bf16x3_fused(g, chain);
            return 0;
        }
    }
    if (e->opt.fp8 && e->opt.fp8_prefill && a.a_mode == A_PLAIN && (a.epi == EPI_LINEAR || a.epi == EPI_SWIGLU || a.epi == EPI_QKV_ROPE)) {
        auto it = e->w.fp8_w.find(a.Wp);
        if (it != e->w.fp8_w.end()) {
            // no producer handed this input over quantised: the standalone fp32 -> AMX pass, then the MX GEMM (same epilogue);
            // profiled as one launch of the family
            const int64_t lda8 = (a.K + 63) / 64 * 64, Mp = rup(a.M, 128);
            CHK(ensure(e, e->a8, ((size_t)Mp * lda8 + 3) / 4));
            CHK(ensure(e, e->a8_scale, (size_t)Mp * ((lda8 / 64 + 3) / 4) * 2));      // 2 scale words per row and four k64 steps
            g.A8 = reinterpret_cast<const uint8_t*>(e->a8.p); g.lda8 = lda8; g.a_sc = reinterpret_cast<const uint32_t*>(e->a8_scale.p);
            g.W8 = it->second.w8; g.w_scale = it->second.scale;
            GemmScope ps(e, chain, a, 100);
            launch_quant_mx8(a.A, a.lda, a.M, a.K, e->a8.p, e->a8_scale.p, chain);
            launch_gemm_fp8(g, chain);
            return 0;
        }
    }
    GemmScope ps(e, chain, a, 0);
    launch_gemm(a, chain);
    return 0;
}
GemmArgs lin(const float* A, int64_t lda, int M, const Packed& w, float* C, int64_t ldc, const float* bias) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.M = M; g.K = w.KP; g.Wp = w.p; g.Nw = w.Nw; g.N = rup(w.N, 4); g.C = C; g.ldc = ldc; g.bias = bias;
    return g;
}

// ---- encoder --------------------------------------------------------------------------------------------------------------
// LayerNorm of M rows x C into the hand-over the next GEMM reads (map / ntok: the row map of the block's first norm)
static void layernorm_to(mellow_engine* e, hipStream_t chain, const float* x, const HandOver& out, int M, int C, const float* w, const float* b, const int32_t* map, int ntok) {
    ProfScope ps(e, PF_NORM, 0, (out.image ? 2.5 : 2.0) * M * C * 4, chain);
    if (out.image) launch_layernorm_apb(x, out.image, M, C, w, b, map, ntok, chain, out.scales);
    else launch_layernorm(x, out.rows, M, C, w, b, map, ntok, chain);
}
struct SwinStage { int st, C, R, N, nH, nW, M1; };      // stage index, channels, R x R = N tokens per view, heads, windows, rows of all views
// One Swin block on `chain`, in place on x [M1][C] (t: M1 x C scratch): norm1 -> qkv -> window attention -> proj (+ residual, row
// map) -> norm2 -> fc1 (GELU) -> fc2 (+ residual).  The modes differ only in what the three hand-overs are.
static int swin_block(mellow_engine* e, hipStream_t chain, const SwinStage& sg, const SwinBlockW& w, bool odd, float* x, float* t) {
    const int st = sg.st, C = sg.C, N = sg.N, M1 = sg.M1;
    const bool shifted = odd && sg.R > kWin;
    const int32_t* map = sg.R > kWin ? e->w.win_map[st][shifted ? 1 : 0] : nullptr;
    // f32x3 mode, stages in enc_apb_stages: the LayerNorms and the GELU epilogue of fc1 write their output pre-split in APB
    // order and qkv / fc1 / fc2 run on the LDS-DMA kernel (gemm_x3q_kernel); H never exists as fp32
    // bit 8 + st: only the LayerNorms hand over pre-split (qkv and fc1 on the APB kernels, fc1 still writes fp32): stage 0,
    // whose K = 96 GEMMs then run on the weight-stationary persistent kernel (gemm_x3w_kernel)
    // fp8 mode (`amx`), every stage: the same hand-over with AMX images (MXFP8, common.h) -- the LayerNorms and the GELU
    // epilogue of fc1 emit e4m3 + block scales in the consumer's LDS order, qkv / fc1 / fc2 run on gemm_mx8_kernel straight
    // from them (K = 96 zero-padded to two k64 steps); the window attention still writes fp32 (head_dim 24 does not tile 32-
    // column blocks) and the proj GEMM takes the standalone quantiser
    const bool amx = e->opt.fp8 && e->opt.fp8_prefill && e->opt.x3_apb && e->w.fp8_w.count(w.qkv.p) && e->w.fp8_w.count(w.fc1.p) && e->w.fp8_w.count(w.fc2.p);
    const bool have_pb = e->opt.f32x3_terms && e->w.bf_w.count(w.qkv.p) && e->w.bf_w.count(w.fc1.p) && e->w.bf_w.count(w.fc2.p);
    const bool apb_h = amx || (have_pb && ((e->opt.enc_apb_stages >> st) & 1));
    const bool apb = apb_h || (have_pb && ((e->opt.enc_apb_stages >> (8 + st)) & 1));
    // bits 4..7 of enc_apb_stages: the window attention hands its output over pre-split too (proj on the x3q kernel)
    const bool apb_proj = apb && !amx && ((e->opt.enc_apb_stages >> (4 + st)) & 1) && e->w.bf_w.count(w.proj.p);
    const bool qkv16 = amx && e->opt.fp8_attn_bf16;      // fp8 mode: q / k / v of the block as bf16 rows (the window attention widens them)
    // a: a LayerNorm's output (qkv, fc1);  p: the attention's (proj; its image shares enc_a3, free between qkv and norm2);  h: GELU(fc1) (fc2)
    HandOver a{t}, p{t}, h{e->H.p};
    if (apb) CHK(ensure(e, e->enc_a3, ((size_t)rup(M1, 128) * C * 6 + 3) / 4));          // whole 128-row panels, 6 bytes per element
    if (apb_h) CHK(ensure(e, e->enc_h3, ((size_t)rup(M1, 128) * 4 * C * 6 + 3) / 4));
    if (apb) a = image_region(e->enc_a3.p, M1, C, amx);
    if (apb_h) h = image_region(e->enc_h3.p, M1, 4 * C, amx);
    if (apb_proj) p.image = a.image;
    layernorm_to(e, chain, x, a, M1, C, w.n1w, w.n1b, map, N);
    GemmArgs qkv = lin(a.rows, C, M1, w.qkv, e->QKV.p, 3 * C, w.qkv_b);
    qkv.c16 = qkv16 ? 1 : 0;
    CHK(run_gemm(e, chain, qkv, a));
    {
        ProfScope ps(e, PF_WINDOW_ATTN, 4.0 * 64 * 64 * 24 * (double)(M1 / 64) * sg.nH, 4.0 * M1 * C * 4, chain);
        launch_window_attention(e->QKV.p, p.rows, M1, C, sg.nH, w.bias_exp, shifted ? w.mask : nullptr, sg.nW, chain, p.image, qkv16);
    }
    GemmArgs proj = lin(p.rows, C, M1, w.proj, x, C, w.proj_b);
    proj.resid = x; proj.ldr = C; proj.crow_map = map; proj.rows_in = N; proj.rows_out = N;
    CHK(run_gemm(e, chain, proj, p));
    layernorm_to(e, chain, x, a, M1, C, w.n2w, w.n2b, nullptr, N);
    GemmArgs fc1 = lin(a.rows, C, M1, w.fc1, h.rows, 4 * C, w.fc1_b);
    fc1.act = ACT_GELU;
    hand_over_to(fc1, h);
    CHK(run_gemm(e, chain, fc1, a));
    GemmArgs fc2 = lin(h.rows, 4 * C, M1, w.fc2, x, C, w.fc2_b);
    fc2.resid = x; fc2.ldr = C;
    CHK(run_gemm(e, chain, fc2, h));
    return 0;
}
// wav dev [n][n_samples] -> proj33 [n][33][576] in e->proj33
int run_encoder(mellow_engine* e, const float* wav, int n, int64_t n_samples, int want_logmel_only, int apply_bn,
                       float* logmel_out) {
    if (n <= 0) return fail("n_clips must be positive");
    if (n_samples % 4 || n_samples < kNfft) return fail("n_samples must be a multiple of 4 and >= 1024");
    hipStream_t s = e->stream;
    struct SkScope {            // the encoder chain is one stream: its under-filled GEMM launches may use the split-K workspace
        mellow_engine* e;
        ~SkScope() { e->sk_enable = false; }
    } sk_scope{e};
    if (e->opt.f32x3_terms && e->opt.sk_max >= 2) {
        CHK(ensure(e, e->sk_ws, (size_t)512 * 16384));
        e->sk_enable = e->sk_ws.p != nullptr;
    }
    const int frames = (int)(n_samples / kHop) + 1;
    const int64_t plen = n_samples + kNfft;
    const int M = n * frames;
    CHK(ensure(e, e->wpad, (size_t)n * plen));
    CHK(ensure(e, e->power, (size_t)M * 544));
    CHK(ensure(e, e->logmel, (size_t)M * 64));
    {
        ProfScope ps(e, PF_MISC, 0, 2.0 * n * plen * 4);
        launch_reflect_pad(wav, n, n_samples, e->wpad.p, plen, kNfft / 2, s);
    }
    if (e->w.fft_win) {   // A1 as a real FFT (f32x3 mode, weights verified to be the windowed DFT basis): 5 N log2 N flops per frame
        ProfScope ps(e, PF_GEMM, 5.0 * kNfft * 10.0 * M, (double)M * (kNfft + 544) * 4);
        ps.r.M = M; ps.r.N = 544; ps.r.K = kNfft; ps.r.epi = 400;
        launch_stft_fft_power(e->wpad.p, frames, plen, kHop, M, e->w.fft_win, e->w.fft_tw1, e->w.fft_tw2, e->power.p, s);
    } else {   // A1: STFT power as DFT GEMM on the checkpoint's conv weights (htsat.py:864)
        GemmArgs g;
        g.A = e->wpad.p; g.a_mode = A_FRAMES; g.fpc = frames; g.clip_stride = plen; g.hop = kHop;
        g.M = M; g.K = kNfft; g.Wp = e->w.dft.p; g.Nw = e->w.dft.Nw; g.N = 544; g.C = e->power.p; g.ldc = 544; g.epi = EPI_POWER;
        CHK(run_gemm(e, s, g, {}));
    }
    CHK(tap(e, "power", e->power.p, (int64_t)M * 544));
    GemmArgs mel;      // A2+A3: mel projection, 10*log10, bn0 (htsat.py:865-870)
    mel.A = e->power.p; mel.lda = 544; mel.M = M; mel.K = 544; mel.Wp = e->w.mel.p; mel.Nw = 64; mel.N = 64;
    mel.C = want_logmel_only ? logmel_out : e->logmel.p; mel.ldc = 64; mel.epi = EPI_LOGMEL;
    mel.apply_bn = apply_bn; mel.bn_alpha = e->w.bn_alpha; mel.bn_beta = e->w.bn_beta;
    CHK(run_gemm(e, s, mel, {}));
    if (want_logmel_only) return 0;
    CHK(tap(e, "logmel_bn", e->logmel.p, (int64_t)M * 64));

    // A4/A4': crops
    int n_crops = 1, crop_len = frames, crop_hop = 0;
    if (frames > 1024) {
        n_crops = 0;
        for (int p = 0; p < frames - kLongCrop - 1; p += kLongHop) ++n_crops;
        crop_len = kLongCrop;
        crop_hop = kLongHop;
    }
    const int nv = n * n_crops;
    const int64_t M0 = (int64_t)nv * 4096;
    CHK(ensure(e, e->X0, (size_t)M0 * 96));
    CHK(ensure(e, e->X1, (size_t)M0 * 96));
    CHK(ensure(e, e->T, (size_t)M0 * 96));
    CHK(ensure(e, e->QKV, (size_t)M0 * 288));
    CHK(ensure(e, e->H, (size_t)M0 * 384));
    {
        ProfScope ps(e, PF_MISC, 0, (double)M0 * 96 * 4);
        launch_fold_patch_embed(e->logmel.p, n, frames, n_crops, crop_hop, crop_len, e->w.pe_w, e->w.pe_b, e->w.pe_nw, e->w.pe_nb,
                                e->X0.p, s);
    }
    CHK(tap(e, "patch", e->X0.p, M0 * 96));
    float *x = e->X0.p, *x2 = e->X1.p, *t = e->T.p;
    for (int st = 0; st < 4; ++st) {
        const int C = 96 << st, R = 64 >> st, N = R * R, nH = kHeads[st];
        const int nW = R > kWin ? (R / kWin) * (R / kWin) : 1;
        const int M1 = nv * N;
        const SwinStage sg{st, C, R, N, nH, nW, M1};
        for (int b = 0; b < kDepths[st]; ++b) CHK(swin_block(e, s, sg, e->w.blocks[st][b], b % 2 == 1, x, t));
        if (st < 3) {
            { ProfScope ps(e, PF_NORM, 0, 2.0 * M1 * C * 4); launch_merge_layernorm(x, t, nv, R, C, e->w.merge[st].nw, e->w.merge[st].nb, s); }
            CHK(run_gemm(e, s, lin(t, 4 * C, M1 / 4, e->w.merge[st].red, x2, 2 * C, nullptr), {}));
            float* tmp = x; x = x2; x2 = tmp;
        }
        if (e->taps_on) {
            char nm[16];
            snprintf(nm, sizeof(nm), "stage%d", st);
            const int64_t cnt = st < 3 ? (int64_t)nv * (N / 4) * (2 * C) : (int64_t)nv * N * C;
            CHK(tap(e, nm, x, cnt));
        }
    }
    // ---- tail (htsat.py:742-796, 950-955; mellow.py:48-52) ----
    CHK(ensure(e, e->ats, (size_t)nv * 32 * 4608));
    CHK(ensure(e, e->fpx, (size_t)nv * 32 * 544));
    CHK(ensure(e, e->emb33, (size_t)n * 33 * 768));
    CHK(ensure(e, e->e1, (size_t)n * 33 * 576));
    CHK(ensure(e, e->gbuf, (size_t)n * 33 * 576));
    CHK(ensure(e, e->sbuf, (size_t)n * 33 * 576));
    CHK(ensure(e, e->proj33, (size_t)n * 33 * 576));
    layernorm_to(e, s, x, HandOver{t}, nv * 64, kEncOut, e->w.fn_w, e->w.fn_b, nullptr, 64);
    float* latent_dst = e->emb33.p;
    int64_t latent_stride = 33 * 768;
    if (n_crops > 1) {
        CHK(ensure(e, e->latv, (size_t)nv * 768));
        CHK(ensure(e, e->fpxavg, (size_t)n * 32 * 544));
        latent_dst = e->latv.p;
        latent_stride = 768;
    }
    { ProfScope ps(e, PF_MISC, 0, 7.0 * nv * 64 * 768 * 4); launch_tail_latent_im2col(t, nv, latent_dst, latent_stride, e->ats.p, s); }
    GemmArgs tscam = lin(e->ats.p, 4608, nv * 32, e->w.tscam, e->fpx.p, 544, e->w.tscam_b);
    tscam.N = 544; tscam.act = ACT_SIGMOID;
    CHK(run_gemm(e, s, tscam, {}));
    const float* fpx = e->fpx.p;
    if (n_crops > 1) {
        ProfScope ps(e, PF_MISC, 0, 0);
        launch_crop_average(e->fpx.p, n, n_crops, 32 * 544, 32 * 544, e->fpxavg.p, 32 * 544, s);
        launch_crop_average(e->latv.p, n, n_crops, 768, 768, e->emb33.p, 33 * 768, s);
        fpx = e->fpxavg.p;
    }
    CHK(tap(e, "fpx", fpx, (int64_t)n * 32 * 544));
    GemmArgs c2l = lin(fpx, 544, n * 32, e->w.c2l, e->emb33.p, 768, e->w.c2l_b);      // c2l on the 32 distinct framewise rows -> embedding rows 1..32 (htsat.py:952-954)
    c2l.crow_map = e->w.emb_row_map; c2l.rows_in = 32; c2l.rows_out = 33;
    CHK(run_gemm(e, s, c2l, {}));
    CHK(tap(e, "emb33", e->emb33.p, (int64_t)n * 33 * 768));
    CHK(run_gemm(e, s, lin(e->emb33.p, 768, n * 33, e->w.lin1, e->e1.p, 576, nullptr), {}));
    { ProfScope ps(e, PF_MISC, 0, 0); launch_gelu(e->e1.p, e->gbuf.p, (int64_t)n * 33 * 576, s); }
    GemmArgs lin2 = lin(e->gbuf.p, 576, n * 33, e->w.lin2, e->sbuf.p, 576, nullptr);
    lin2.resid = e->e1.p; lin2.ldr = 576;
    CHK(run_gemm(e, s, lin2, {}));
    { ProfScope ps(e, PF_NORM, 0, 0); launch_layernorm(e->sbuf.p, e->proj33.p, n * 33, 576, e->w.pln_w, e->w.pln_b, nullptr, 33, s); }
    CHK(tap(e, "proj33", e->proj33.p, (int64_t)n * 33 * 576));
    CHK(tap(e, "latent", e->emb33.p, 768));  // first clip's latent row (row 0 of emb33)
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

int mellow_debug_enable_taps(mellow_engine_t* e, int on) {
    if (!e) return fail("null engine");
    e->taps_on = on != 0;
    return 0;
}

int mellow_debug_tap(mellow_engine_t* e, const char* name, float* out, int64_t capacity, int64_t* numel) {
    if (!e || !name) return fail("null argument");
    auto it = e->tap_numel.find(name);
    if (it == e->tap_numel.end()) return fail("no such tap recorded: %s", name);
    if (numel) *numel = it->second;
    if (out) {
        if (capacity < it->second) return fail("tap buffer too small");
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipMemcpyAsync(out, e->taps[name].p, it->second * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return 0;
}

int mellow_logmel(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_samples, int apply_bn, float* out) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!wav || !out) return fail("null argument");
    HIPCHK(hipSetDevice(e->device));
    CHK(run_encoder(e, wav, n_clips, n_samples, 1, apply_bn, out));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_encode(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_samples, float* out) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!wav || !out) return fail("null argument");
    HIPCHK(hipSetDevice(e->device));
    CHK(run_encoder(e, wav, n_clips, n_samples, 0, 1, nullptr));
    launch_downsample33(e->proj33.p, n_clips, out, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// A0 on the device: torchaudio-style sinc_interp_hann resampling (lowpass_filter_width 6, rolloff 0.99), the polyphase bank
// built exactly like mellow_amd/audio.py::_sinc_resample_kernel (float64, then cast to float32)
int mellow_resample(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_in, int orig_freq, int new_freq, float* out,
                    int64_t out_capacity, int64_t* n_out) {
    if (!e || !wav || n_clips <= 0 || n_in <= 0 || orig_freq <= 0 || new_freq <= 0) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    int a = orig_freq, b = new_freq;
    while (b) { const int t = a % b; a = b; b = t; }
    const int orig = orig_freq / a, nw = new_freq / a;
    const int64_t target = (int64_t)((nw * n_in + orig - 1) / orig);       // ceil(new * length / orig)
    if (n_out) *n_out = target;
    if (!out) return 0;
    if (out_capacity < target) return fail("resample output buffer too small");
    const double PI = 3.14159265358979323846, lpw = 6.0, rolloff = 0.99;
    const double base_freq = (orig < nw ? orig : nw) * rolloff;
    const int width = (int)std::ceil(lpw * orig / base_freq);
    const int klen = 2 * width + orig;
    float* dw = nullptr;
    auto it = e->resample_banks.find({orig, nw});
    if (it != e->resample_banks.end()) {
        dw = it->second;
    } else {    // built once per rate pair and kept (no allocation / host filter design on later calls)
        std::vector<float> wT((size_t)klen * nw);
        const double scale = base_freq / orig;
        for (int p = 0; p < nw; ++p)
            for (int k = 0; k < klen; ++k) {
                double t = (double)(-p) / nw + (double)(k - width) / orig;
                t *= base_freq;
                if (t < -lpw) t = -lpw;
                if (t > lpw) t = lpw;
                const double c = std::cos(t * PI / lpw / 2.0);
                const double window = c * c;
                t *= PI;
                const double kern = t == 0.0 ? 1.0 : std::sin(t) / t;
                wT[(size_t)k * nw + p] = (float)(kern * window * scale);
            }
        HIPCHK(hipMalloc(&dw, wT.size() * sizeof(float)));
        e->allocs.push_back(dw);
        HIPCHK(hipMemcpy(dw, wT.data(), wT.size() * sizeof(float), hipMemcpyHostToDevice));
        e->resample_banks[{orig, nw}] = dw;
    }
    // rows of `out` are `target` long: the kernel writes with stride n_out = target
    launch_resample(wav, n_clips, n_in, dw, orig, nw, klen, width, out, target, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_argmax(mellow_engine_t* e, const float* logits, int B, int32_t* tokens) {
    if (!e || !logits || !tokens || B <= 0) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    launch_argmax(logits, B, e->cfg.vocab_size, e->cfg.vocab_size, tokens, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
