// The decoder LM: KV pages and decode workspaces, prefill (A15: a span's plan, its parts, one layer's launches, the fork / join around
// them), the KV-cached decode step and its per-call mode, prefix assembly (A14), the lm taps and scoring.  The loop on top: engine_generate.cpp.
#include "engine_internal.h"

// key split of the decode attention (DecArgs::gs, 4-key groups per split): balanced at the END of the reserved context, rounded
// down to whole passes of a workgroup when that costs at most 4 groups of imbalance.  ensure_lm and the tap mellow_debug_dec_attn.
int dec_attn_split_groups(int ctx_end, int ts, bool kv16) {
    const int ng_end = (ctx_end - 1 + 3) / 4, chunk = dec_attn_chunk_groups(kv16);
    int gs = (ng_end + ts - 1) / ts;
    if (gs > chunk && gs % chunk <= 4) gs -= gs % chunk;
    return gs < 1 ? 1 : gs;
}

int ensure_lm(mellow_engine* e, int B, int T, int Tmax, int ctx_end, int prefill_B, size_t prefill_rows) {
    if (B > 1024) return fail("batch of %d exceeds the 1024 rows one pass takes (mellow_generate chunks larger batches itself; the decode state block is sized for 32 row blocks)", B);
    if (ctx_end <= 0 || ctx_end > Tmax) ctx_end = Tmax;      // last context length the call will reach (<= page capacity)
    if (Tmax > e->cfg.max_positions) return fail("prefix + max_len = %d exceeds max_positions %d", Tmax, e->cfg.max_positions);
    const size_t Mp = prefill_rows > 0 ? prefill_rows : (size_t)(prefill_B > 0 ? prefill_B : B) * T;
    CHK(ensure(e, e->lm_x, Mp * 576));
    CHK(ensure(e, e->lm_xn, Mp * 576));
    CHK(ensure(e, e->lm_q, Mp * 576));
    CHK(ensure(e, e->lm_o, Mp * 576));
    CHK(ensure(e, e->lm_h, Mp * 1536));
    if (e->opt.f32x3_terms || (e->opt.fp8 && e->opt.fp8_prefill)) {      // 6 bytes per element (the fp8 mode's AMX images + scale bytes need 1.05), rows padded to whole 128-row panels
        const size_t Mq = (size_t)rup((int)Mp, 128) + 3 * 128;   // + three panels: every part of the split prefill starts on a panel boundary
        CHK(ensure(e, e->lm_xn3, Mq * 576 * 6 / 4));
        CHK(ensure(e, e->lm_o3, Mq * 576 * 6 / 4));
        CHK(ensure(e, e->lm_h3, Mq * 1536 * 6 / 4));
        CHK(ensure(e, e->lm_ssq, Mq * 2 * 16));        // two statistics per row (after o_proj / after down), 9 partial sums each
    }
    // fp8 mode at its defaults: K and V exist as bf16 pages ONLY -- written by the q/k/v epilogue (rounded once), read by the bf16-once
    // prefill attention and by the decode attention; the fp32 pages and the conversion pass of round 5 are not touched
    e->kv16_direct = e->opt.kv16 && e->opt.fp8 && e->opt.fp8_prefill && e->opt.fp8_attn_bf16 && e->opt.x3_apb && e->opt.x3_attn && !e->w.layers.empty() &&
                     e->w.fp8_w.count(e->w.layers[0].qkv.p) != 0;
    dec_prepare_lds_attributes();            // (remembered per device: a no-op after the first call)
    const int Bp = rb_of(B) * 32;
    if (e->kv_B != Bp || e->kv_Tmax != Tmax) {
        e->kv_B = Bp;
        e->kv_Tmax = Tmax;
        CHK(ensure(e, e->kcache, kv_layer_floats(e) * e->cfg.num_layers));
        CHK(ensure(e, e->vcache, kv_layer_floats(e) * e->cfg.num_layers));
        if (e->opt.kv16) {
            CHK(ensure(e, e->kcache16, kv_layer_floats(e) * e->cfg.num_layers / 2));
            CHK(ensure(e, e->vcache16, kv_layer_floats(e) * e->cfg.num_layers / 2));
        }
        // the decode attention loads whole key groups before it knows the position and masks them afterwards
        // (weight 0 x value): never-written page slots must hold finite numbers
        HIPCHK(hipMemsetAsync(e->kcache.p, 0, kv_layer_floats(e) * e->cfg.num_layers * sizeof(float), e->stream));
        HIPCHK(hipMemsetAsync(e->vcache.p, 0, kv_layer_floats(e) * e->cfg.num_layers * sizeof(float), e->stream));
        if (e->opt.kv16) {
            HIPCHK(hipMemsetAsync(e->kcache16.p, 0, kv_layer_floats(e) * e->cfg.num_layers * sizeof(float) / 2, e->stream));
            HIPCHK(hipMemsetAsync(e->vcache16.p, 0, kv_layer_floats(e) * e->cfg.num_layers * sizeof(float) / 2, e->stream));
        }
        e->graphs.reset();      // the page geometry is baked into captured launches
    }
    {
        // carve the decode-step buffers out of one arena (all sizes are multiples of 64 floats = 256 B)
        const size_t RB = (size_t)Bp / 32, V = (size_t)e->cfg.vocab_size;
        const size_t n_x = (size_t)Bp * 576;
        size_t off = 0;
        auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };
        const size_t o_xmidF = take(n_x), o_xnewR = take(n_x), o_xnF = take(n_x * 3 / 2);      // (xnF: fp32, or its 6-byte pre-split image)
        const size_t o_dslabF = take(DEC_KC_DOWN * n_x), o_ssq1 = take((size_t)Bp * DEC_KC_QKV), o_rope = take(64);
        const size_t o_pq = take((size_t)DEC_KC_QKV * Bp * 960);
        const size_t o_att = take((size_t)DEC_TS * n_x), o_aml = take((size_t)DEC_TS * 9 * Bp * 2);
        const size_t o_ssq = take((size_t)Bp * 40), o_gu = take(RB * 192 * 256), o_xmidF16 = take(n_x);
        // f32x3 layer kernels: 6-byte pre-split images of x_mid (two fragment orders) and of h
        const bool x3l = (e->opt.dec_x3 & DEC_X3_GATEUP) && (e->opt.dec_x3 & DEC_X3_QKV) && (int)RB >= e->opt.dec_x3_min_rb && !e->opt.fp8_decode &&
                         e->w.layers.size() > 1 && e->w.layers[1].qkv2 != nullptr && e->w.layers[1].gu16n != nullptr;
        const size_t o_x3a = take(x3l ? n_x * 3 / 2 : 0), o_x3b = take(x3l ? n_x * 3 / 2 : 0), o_h3 = take(x3l ? RB * 192 * 256 * 3 / 2 : 0);
        const bool fresh = e->dec.cap < off;
        CHK(ensure(e, e->dec, off));
        CHK(ensure(e, e->dlogits, (size_t)Bp * V));
        CHK(ensure(e, e->cand, (size_t)2 * Bp * (V / 32)));
        if (fresh) {
            // padded batch rows are computed but never read back; start from finite values
            HIPCHK(hipMemsetAsync(e->dec.p, 0, off * sizeof(float), e->stream));
            e->graphs.reset();      // ... and so are the addresses of the decode arena
        }
        float* p = e->dec.p;
        DecArgs& a = e->da;
        a.rows = Bp; a.RB = (int)RB; a.Tmax = Tmax; a.eps = e->cfg.rms_norm_eps; a.d_pos = e->d_pos; a.inc_pos = 0; a.first = 0;
        a.a8 = e->opt.fp8_decode_act ? 1 : 0;
        a.kv16 = e->opt.kv16 ? 1 : 0;
        a.x3 = e->opt.dec_x3;
        a.rope_cos = e->w.rope_cos; a.rope_sin = e->w.rope_sin;
        a.xmidF = p + o_xmidF; a.xnewR = p + o_xnewR; a.xnF = p + o_xnF;
        a.xn3 = (a.x3 & DEC_X3_HEAD) && !e->w.head8 && dec_head3r_fits(e->cfg.vocab_size) ? (void*)(p + o_xnF) : nullptr;
        a.xmid3_32 = x3l ? (void*)(p + o_x3a) : nullptr; a.xmid3_16 = x3l ? (void*)(p + o_x3b) : nullptr; a.h3 = x3l ? (void*)(p + o_h3) : nullptr;
        a.dslabF = p + o_dslabF; a.slabF_stride4 = (int64_t)(n_x / 4); a.ssq1 = p + o_ssq1; a.rope_cur = p + o_rope;
        {
            a.ts = dec_key_splits((int)RB, e->opt.kv16 || e->opt.mode != MELLOW_PRECISION_F32X3);
            const int gs = dec_attn_split_groups(ctx_end, a.ts, e->opt.kv16);
            if (gs != a.gs) e->graphs.reset();     // the split is baked into captured launches
            a.gs = gs;
        }
        a.pq = p + o_pq; a.attF16 = p + o_att; a.att_ml = p + o_aml; a.ssq = p + o_ssq; a.guF = p + o_gu; a.xmidF16 = p + o_xmidF16;
        a.cand_val = e->cand.p; a.cand_idx = reinterpret_cast<int32_t*>(e->cand.p + (size_t)Bp * (V / 32));
        apply_step_mode(e, StepMode());                     // the taps' step; a generation pass applies its own afterwards
    }
    return 0;
}

void apply_step_mode(mellow_engine* e, const StepMode& m) {
    e->mode = m;
    DecArgs& a = e->da;
    // the rules, the guidance, the constraint and the stop strings edit the stored rows, the top log-probs read them
    e->mode.logits = m.logits || m.rules || m.guide || m.top > 0 || m.constrain || m.stop;
    a.logits = e->mode.logits ? e->dlogits.p : nullptr;      // (off: generation's arg-max needs the candidates only, no 6 MB store per step)
    a.cand_sum = m.logprob ? e->cand_sum.p : nullptr;
    a.blk_live = m.early_exit ? e->d_blk_live : nullptr;
    a.blk_snap = e->d_blk_live + 32;
    a.row_of_slot = m.migrate ? e->d_row_of_slot : nullptr;
}

// The decode attention loads whole key groups before it knows the position and masks them by WEIGHT (exp(-inf) = 0): a
// slot beyond the context must therefore hold a finite value, or 0 x NaN poisons the row.  A fresh page is zeroed when it
// is allocated; a reused one may hold an earlier call's appended keys -- even NaN from a poisoned request -- so the V slots
// beyond the prefix, [T, Tmax), are cleared once per prefill (one coalesced fill kernel, 80 MB at B = 32 / max_len 64: ~20 us; K needs none: a NaN score of a masked key is replaced by -inf with a select).
int clear_page_tails(mellow_engine* e, int T, int t_end) {
    const int Tmax = e->kv_Tmax;
    if (t_end > Tmax) t_end = Tmax;
    if (T >= t_end) return 0;
    if (e->kv16_direct) launch_clear_page_slots(e->vcache16.p, (int64_t)e->cfg.num_layers * e->kv_B * 3, Tmax, T, t_end, e->stream, true);
    else launch_clear_page_slots(e->vcache.p, (int64_t)e->cfg.num_layers * e->kv_B * 3, Tmax, T, t_end, e->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

LoopArgs loop_args(mellow_engine* e) {
    LoopArgs lp;
    lp.out_tokens = reinterpret_cast<int32_t*>(e->out_tok.p);
    lp.params = e->d_params; lp.seen_stop = e->d_seen; lp.n_seen = e->d_nseen; lp.arrive = e->d_arrive; lp.ticket = e->d_ticket;
    lp.host_progress = e->d_progress; lp.T0 = e->cfg.prefix_len;
    if (e->da.blk_live) { lp.blk_left = e->d_blk_left; lp.blk_live = e->d_blk_live; lp.blk_snap = e->d_blk_live + 32; }
    if (e->da.row_of_slot) { lp.row_of_slot = e->d_row_of_slot; lp.n_compactions = e->d_ncompact; }
    if (e->mode.logprob) lp.out_logprob = e->out_lp.p;
    return lp;
}

BeamArgs beam_args(mellow_engine* e, int N, int k) {
    float* w = e->beam_ws.p;
    int32_t* wi = reinterpret_cast<int32_t*>(w);
    const size_t tab = (size_t)e->beam_max_len * N, t0 = 3 * 1024 + 3 * 1024 * BEAM_MAX_K;
    BeamArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.k = k; g.N = N;
    g.cum_in = g.cum_state = w; g.fin_in = g.fin_state = wi + 1024; g.cand_n = wi + 2048;
    g.cand_c = w + 3 * 1024; g.cand_tok = wi + 3 * 1024 + 1024 * BEAM_MAX_K; g.cand_lp = w + 3 * 1024 + 2 * 1024 * BEAM_MAX_K;
    g.out_parent = wi + t0; g.out_token = wi + t0 + tab; g.out_lp = w + t0 + 2 * tab; g.out_cum = w + t0 + 3 * tab;
    return g;
}

RulesArgs rules_args(mellow_engine* e, int B) {
    const LoopArgs lp = loop_args(e);
    RulesArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.prm = e->d_rparams; g.bias = e->rules_bias.p;
    g.cand_val = e->da.cand_val; g.cand_idx = e->da.cand_idx; g.cand_sum = e->da.cand_sum;
    g.d_pos = e->d_pos; g.params = lp.params; g.T0 = lp.T0;
    g.row_of_slot = lp.row_of_slot; g.blk_snap = lp.blk_snap;
    if (e->mode.beam) {
        const BeamArgs bm = beam_args(e, B, e->mode.beam);
        g.beam_hist = reinterpret_cast<int32_t*>(e->rules_hist.p); g.hist_ld = e->beam_max_len;
        g.parent_tab = bm.out_parent; g.token_tab = bm.out_token; g.N = B; g.k = e->mode.beam;
    } else {
        g.hist = lp.out_tokens;
    }
    return g;
}

ConstrainArgs constrain_args(mellow_engine* e, int B) {
    const LoopArgs lp = loop_args(e);
    int32_t* ws = reinterpret_cast<int32_t*>(e->con_ws.p);
    ConstrainArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.prm = reinterpret_cast<const uint32_t*>(ws);
    g.trie = reinterpret_cast<const int32_t*>(e->con_trie.p); g.row_root = ws + CON_WORDS; g.state = ws + CON_WORDS + CON_STATE_ROWS;
    g.cand_val = e->da.cand_val; g.cand_idx = e->da.cand_idx; g.cand_sum = e->da.cand_sum;
    g.d_pos = e->d_pos; g.params = lp.params; g.T0 = lp.T0;
    g.row_of_slot = lp.row_of_slot; g.blk_snap = lp.blk_snap;
    if (e->mode.beam) {
        const BeamArgs bm = beam_args(e, B, e->mode.beam);
        g.parent_tab = bm.out_parent; g.token_tab = bm.out_token; g.N = B; g.k = e->mode.beam;
    } else {
        g.hist = lp.out_tokens;
    }
    return g;
}

StopStrArgs stop_str_args(mellow_engine* e, int B) {
    const LoopArgs lp = loop_args(e);
    uint32_t* ws = reinterpret_cast<uint32_t*>(e->stop_ws.p);
    StopStrArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.blk = ws; g.state = ws + STS_BLOCK_WORDS;
    g.tok_off = e->w.vocab_bytes->off; g.tok_bytes = e->w.vocab_bytes->bytes;
    g.cand_val = e->da.cand_val; g.cand_idx = e->da.cand_idx; g.cand_sum = e->da.cand_sum;
    g.d_pos = e->d_pos; g.params = lp.params; g.T0 = lp.T0;
    g.row_of_slot = lp.row_of_slot; g.blk_snap = lp.blk_snap;
    if (e->mode.beam) {
        const BeamArgs bm = beam_args(e, B, e->mode.beam);
        g.parent_tab = bm.out_parent; g.token_tab = bm.out_token; g.N = B; g.k = e->mode.beam;
    } else {
        g.hist = lp.out_tokens;
    }
    return g;
}

GuideArgs guide_args(mellow_engine* e) {
    const LoopArgs lp = loop_args(e);
    GuideArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.prm = e->d_gparams;
    g.cand_val = e->da.cand_val; g.cand_idx = e->da.cand_idx; g.cand_sum = e->da.cand_sum;
    g.blk_snap = lp.blk_snap;
    return g;
}

TopArgs top_args(mellow_engine* e) {
    const LoopArgs lp = loop_args(e);
    TopArgs g;
    g.logits = e->da.logits; g.ld = e->cfg.vocab_size; g.cand_val = e->da.cand_val; g.cand_sum = e->da.cand_sum; g.k = e->mode.top;
    g.out_ids = reinterpret_cast<int32_t*>(e->top_ids.p); g.out_lp = e->top_lp.p;
    g.d_pos = e->d_pos; g.params = lp.params; g.T0 = lp.T0;
    g.row_of_slot = lp.row_of_slot; g.blk_snap = lp.blk_snap;
    return g;
}

// final norm (+ pending down slabs) + lm_head with fused per-tile arg-max candidates -> dlogits, d_tokens
int run_lm_head(mellow_engine* e, int B, int pending_kcd, const RecordArgs* rec) {
    const int NT = e->cfg.vocab_size / 32, Bp = e->da.rows;
    auto dh = [&](int k) { DecArgs x = e->da; x.dbg_seq = e->dbg_seq0 >= 0 ? e->dbg_seq0 + 5 * e->cfg.num_layers + k : -1000; return x; };
    { ProfScope ps(e, PF_NORM, 0, (double)(pending_kcd + 2) * Bp * 576 * 4);
      launch_dec_final_norm(dh(0), e->w.final_norm, pending_kcd, e->stream); }
    { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * 576.0 * e->cfg.vocab_size, 576.0 * e->cfg.vocab_size * 4);
      const DecW h = e->w.head_w();
      launch_dec_lm_head(dh(1), h.p, e->w.lm_head.KP / 8, e->cfg.vocab_size, e->stream, h.scale); }
    if (e->mode.guide && rec) {      // contrastive guidance: both rows of a pair get the combined row before the rules and any picker read them
        ProfScope ps(e, PF_MISC, 0, 6.0 * B * e->cfg.vocab_size * 4);
        launch_dec_guidance(guide_args(e), B / 2, e->stream);
    }
    if (e->mode.rules && rec) {      // repetition controls: the row's logits and tile partials are edited before any picker reads them
        ProfScope ps(e, PF_MISC, 0, 2.0 * B * e->cfg.vocab_size * 4);
        launch_dec_logit_rules(rules_args(e, B), B, e->stream);
    }
    if (e->mode.constrain && rec) {  // constrained decoding: tokens outside the row's allowed set are banned after the rules, before the top log-probs and any picker
        ProfScope ps(e, PF_MISC, 0, 2.0 * B * e->cfg.vocab_size * 4);
        launch_dec_constrain(constrain_args(e, B), B, e->stream);
    }
    if (e->mode.stop && rec) {       // stop strings: a row whose text holds one becomes the one-hot row of the stop id, whatever the earlier launches left
        ProfScope ps(e, PF_MISC, 0, 1.0 * B * e->cfg.vocab_size * 4);
        launch_dec_stop_strings(stop_str_args(e, B), B, e->stream);
    }
    if (e->mode.top && rec) {        // top log-probs: exactly the row the picker below reads, after the guidance, the rules, the constraint and the stop strings
        ProfScope ps(e, PF_MISC, 0, 1.0 * B * e->cfg.vocab_size * 4);
        launch_dec_top_logprobs(top_args(e), B, e->stream);
    }
    { ProfScope ps(e, PF_MISC, 0, 0);
      if (e->mode.beam) {          // mellow_generate_beam: the head stored the logits; the k best continuations per example
          const LoopArgs lp = loop_args(e);
          launch_beam_select(beam_args(e, B, e->mode.beam), B / e->mode.beam, dh(2), e->d_tokens, e->w.embed, &lp, e->stream);
      } else if (e->mode.sample) {        // mellow_generate_sampled: the head stored the logits (da.logits); draw instead of the arg-max
          SampleArgs sa;
          sa.logits = e->da.logits; sa.ld = e->cfg.vocab_size; sa.prm = e->d_sparams;
          sa.row_shift = e->mode.guide ? 1 : 0;        // a guided pair draws from the stream of its pair index
          sa.filtered = e->mode.filtered;
          launch_dec_sample(sa, dh(2), B, e->d_tokens, e->w.embed, (rec && rec->embed_next) ? 1 : 0, rec ? loop_args(e) : LoopArgs(),
                            e->stream);
      } else {
          launch_dec_argmax(dh(2), B, NT, e->d_tokens, e->w.embed, (rec && rec->embed_next) ? 1 : 0, rec ? loop_args(e) : LoopArgs(),
                            e->stream);
      }
      if (rec && e->da.row_of_slot) launch_dec_compact(e->da, B, loop_args(e), e->stream); }
    return 0;
}

// ---- the LM prefill: what a span decides (PrefillPlan), where its rows run (PrefillPart), what a layer launches (prefill_layer) ----
struct PrefillPlan {
    int T, pos0, T_end, Tmax;     // rows per sequence of every activation, their first position; keys [0, T_end); the kernels' page stride
    bool all_layers, amx, apb, p16, fuse_norm, attn_x3, attn_bf16;
    float *kpages, *vpages;       // layer 0, example 0 of what they write: the pages, their bf16 form (p16) or the prefix buffer
    size_t lay, page;             // floats of one layer / of one example of it (halved for bf16 pages: two bytes per element)
};
struct PrefillPart {
    hipStream_t chain;
    int b0, B, M;                 // first example, examples, rows (B * T)
    float *x, *q;                 // the part's rows of the span's input, of lm_q
    HandOver xn, o, h;            // ... of lm_xn / lm_o / lm_h, and, APB or AMX, its panel-aligned region of lm_xn3 / lm_o3 / lm_h3
    float *ssq_in, *ssq_mid;      // [row][9] sum-of-squares partials of the residual stream after down / after o_proj (fuse_norm)
};
static int prefill_plan(mellow_engine* e, int B, const PrefillSpan& sp, PrefillPlan& pl) {
    pl.T = sp.rows; pl.pos0 = sp.pos0; pl.T_end = sp.pos0 + sp.rows; pl.all_layers = sp.all_layers;
    // to_prefix: the K/V of the B sequences go to the prefix buffer (page stride Tp), not to the pages -- a page of example b' would
    // lie inside the rows another example's copies are written to, and one parallel copy kernel cannot order those writes
    const bool fan = sp.to_prefix;
    if (pl.pos0 > 0 && (pl.pos0 % 32 != 0 || fan || sp.all_layers || e->opt.fp8 || e->opt.kv16 || B > e->kv_B))
        return fail("internal: a prefill from position %d needs fp32 pages that hold the positions before it", pl.pos0);
    // fp8 mode: the same producer -> consumer hand-over with AMX images (MXFP8, common.h) instead of APB ones: `amx`; the code below
    // says `apb` for "GEMM inputs leave their producers in operand format"
    pl.amx = e->opt.fp8 && e->opt.fp8_prefill && e->opt.x3_apb && e->w.fp8_w.count(e->w.layers[0].qkv.p) != 0;
    pl.apb = (e->opt.f32x3_terms && e->opt.x3_apb) || pl.amx;        // option "x3_apb" = 0: the register-staged x3p kernel / the standalone quantiser (developer A/B)
    pl.p16 = pl.amx && e->kv16_direct;          // bf16 pages: the same element offsets, two bytes each
    pl.fuse_norm = pl.apb && e->opt.prefill_fuse_norm;
    pl.attn_x3 = (e->opt.f32x3_terms != 0 || pl.amx) && e->opt.x3_attn;      // option "x3_attn" = 0: f32x3 mode on the fp32 kernel (A/B)
    pl.attn_bf16 = pl.amx && e->opt.fp8_attn_bf16;
    // bf16 pages are never a fan-out's target: run_prefill / run_prefill_q refuse kv16 for one, and kv16_direct needs kv16
    if (pl.p16 && fan) return fail("internal: a prefill to the prefix buffer needs fp32 K/V");
    pl.Tmax = fan ? prefix_page_len(e->cfg.prefix_len) : e->kv_Tmax;
    pl.kpages = pl.p16 ? e->kcache16.p : fan ? e->kprefix.p : e->kcache.p;
    pl.vpages = pl.p16 ? e->vcache16.p : fan ? e->vprefix.p : e->vcache.p;
    pl.page = (size_t)3 * pl.Tmax * 64 / (pl.p16 ? 2 : 1);
    pl.lay = fan ? (size_t)B * pl.page : kv_layer_floats(e) / (pl.p16 ? 2 : 1);
    return 0;
}
// Split prefill (f32x3 mode): the batch is cut into independent parts (2 by default) that run the same launches on their own
// streams, so the tails and the fill / drain of one part's kernels are covered by another's (every buffer is indexed by row
// or by example, so a part is an offset; its pre-split operands get their own panel-aligned region).  Measured before it was
// built with two forked contexts (tools/half_chain_probe.py).  MELLOW_PREFILL_SPLIT=n: n parts (1 = one chain, at most 4).
static int prefill_parts(mellow_engine* e, const PrefillPlan& pl, int B, float* x, PrefillPart* parts, int& nh) {
    // The two invariants of a chain.  A span that is not APB is never split: its GEMMs share the quantiser's and the
    // split-K buffers (run_gemm refuses them off the main chain).  Profiling forces one chain: records are read in enqueue order.
    const bool may_split = pl.apb && !e->prof_on;
    if (may_split && (e->prefill_parts > 1 || e->streams_probed)) CHK(ensure_prefill_streams(e));      // (may find that they would serialise: fewer parts)
    nh = std::min(B, std::max(1, std::min(4, may_split ? e->prefill_parts : 1)));
    size_t prow = 0;                                             // first row of the part's panel range
    for (int h = 0, b0 = 0; h < nh; ++h) {
        PrefillPart& p = parts[h];
        p.chain = h ? e->stream2[h - 1] : e->stream; p.b0 = b0; p.B = B / nh + (h < B % nh ? 1 : 0); p.M = p.B * pl.T;
        const int64_t r0 = (int64_t)b0 * pl.T;
        // fp32 rows of the part; APB / AMX: also its pre-split operand region (6 bytes per element, whole 128-row panels)
        auto rows_of = [&](float* rows, const mellow_engine::Buf& img, int K) { return pl.apb ? image_region(reinterpret_cast<char*>(img.p) + prow * K * 6, p.M, K, pl.amx, rows + r0 * K) : HandOver{rows + r0 * K}; };
        p.x = x + r0 * 576; p.q = e->lm_q.p + r0 * 576;
        p.xn = rows_of(e->lm_xn.p, e->lm_xn3, 576); p.o = rows_of(e->lm_o.p, e->lm_o3, 576); p.h = rows_of(e->lm_h.p, e->lm_h3, 1536);
        p.ssq_in = pl.fuse_norm ? e->lm_ssq.p + prow * 9 : nullptr;
        p.ssq_mid = pl.fuse_norm ? e->lm_ssq.p + e->lm_ssq.cap / 2 + prow * 9 : nullptr;    // second half of the buffer
        b0 += p.B; prow += rup(p.M, 128);
    }
    return 0;
}
static void rmsnorm_to(mellow_engine* e, hipStream_t chain, const float* x, const HandOver& out, int M, const float* w) {
    ProfScope ps(e, PF_NORM, 0, (out.image ? 2.5 : 2.0) * M * 576 * 4, chain);
    if (out.image) launch_rmsnorm_apb(x, out.image, M, 576, w, e->cfg.rms_norm_eps, chain, out.scales);
    else launch_rmsnorm(x, out.rows, M, 576, w, e->cfg.rms_norm_eps, chain);
}
// One layer of one part, on the part's chain.  f32x3 mode: every GEMM input of the layer is written by its producer already split
// into three bf16 pieces, in the order the GEMM's LDS stage wants it (APB, common.h), and the GEMM stages both operands by LDS-DMA
// (x3q); fp8 mode: the same with AMX images.
static int prefill_layer(mellow_engine* e, const PrefillPlan& pl, const PrefillPart& p, int l) {
    const LMLayerW& w = e->w.layers[l];
    float *kc = pl.kpages + pl.lay * l + p.b0 * pl.page, *vc = pl.vpages + pl.lay * l + p.b0 * pl.page;
    // norm-free chaining (fz): the residual stream leaves the o_proj / down GEMMs already pre-split together with its
    // sum-of-squares partials (ssq_mid after o_proj, ssq_in after down); the GEMM that follows runs on the norm-folded
    // weight and applies the row statistic to its accumulators -- 59 of the 60 normalisation launches of a prefill disappear
    // (the first layer's input is the prefix, which has no producing GEMM: it keeps its launch)
    const bool fz = pl.fuse_norm && w.gateup_f.p != nullptr;
    const bool fz_in = fz && l > 0;       // this layer's input came out of the previous layer's down GEMM pre-split
    auto with_rs = [&](GemmArgs& g, const float* ssq) { g.rs_ssq = ssq; g.rs_parts = 9; g.rs_dim = 576.f; g.rs_eps = e->cfg.rms_norm_eps; };
    // x += ..., and under fz its image and statistic for the next GEMM
    auto residual_out = [&](GemmArgs& g, float* ssq) { g.resid = p.x; g.ldr = 576; if (fz) { hand_over_to(g, p.xn); g.ssq_out = ssq; g.ssq_parts = 9; } };
    if (!fz_in) rmsnorm_to(e, p.chain, p.x, p.xn, p.M, w.in_ln);
    GemmArgs qkv;
    qkv.A = p.xn.rows; qkv.lda = 576; qkv.M = p.M; qkv.K = 576; qkv.Wp = fz_in ? w.qkv_f.p : w.qkv.p; qkv.Nw = 960; qkv.N = 960;
    qkv.epi = pl.pos0 > 0 ? EPI_QKV_ROPE_AT : EPI_QKV_ROPE; qkv.pos0 = pl.pos0;
    if (fz_in) with_rs(qkv, p.ssq_in);
    qkv.q_out = p.q; qkv.k_cache = kc; qkv.v_cache = vc; qkv.rope_cos = e->w.rope_cos; qkv.rope_sin = e->w.rope_sin;
    qkv.T = pl.T; qkv.Tmax = pl.Tmax; qkv.q_heads = 9; qkv.kv_heads = 3; qkv.kv16 = pl.p16 ? 1 : 0;
    CHK(run_gemm(e, p.chain, qkv, p.xn));
    // The LAST layer only has to produce the final prefix row (nothing consumes the other rows' attention / MLP
    // outputs; their K/V pages were just written above): it is finished by the decode kernels on B rows (finish_prefill).
    if (l == e->cfg.num_layers - 1 && !pl.all_layers) return 0;
    {
        // causal QK^T + PV: 4*64 flops per (query,key) pair per head
        ProfScope ps(e, PF_PREFILL_ATTN, 4.0 * 64 * 9 * (double)p.B * ((double)pl.T_end * (pl.T_end + 1) / 2 - (double)pl.pos0 * (pl.pos0 + 1) / 2), 0, p.chain);
        if (pl.pos0 > 0) launch_prefill_attention_past(p.q, kc, vc, p.o.rows, p.o.image, p.B, pl.T_end, pl.Tmax, pl.pos0, pl.attn_x3, p.chain);
        else launch_prefill_attention(p.q, kc, vc, p.o.rows, p.o.image, p.B, pl.T, pl.Tmax, pl.attn_x3, p.chain, p.o.scales, pl.attn_bf16, pl.p16);
    }
    GemmArgs o = lin(p.o.rows, 576, p.M, w.o, p.x, 576, nullptr);
    residual_out(o, p.ssq_mid);
    CHK(run_gemm(e, p.chain, o, p.o));
    if (!fz) rmsnorm_to(e, p.chain, p.x, p.xn, p.M, w.post_ln);
    GemmArgs gu;
    gu.A = p.xn.rows; gu.lda = 576; gu.M = p.M; gu.K = 576; gu.Wp = fz ? w.gateup_f.p : w.gateup.p; gu.Nw = 3072; gu.N = 1536; gu.C = p.h.rows; gu.ldc = 1536;
    gu.epi = EPI_SWIGLU;
    if (fz) with_rs(gu, p.ssq_mid);
    hand_over_to(gu, p.h);
    CHK(run_gemm(e, p.chain, gu, p.xn));
    GemmArgs down = lin(p.h.rows, 1536, p.M, w.down, p.x, 576, nullptr);
    residual_out(down, p.ssq_in);
    CHK(run_gemm(e, p.chain, down, p.h));
    return 0;
}
// The LM layers over positions [pos0, pos0 + rows) of B sequences (engine_internal.h, PrefillSpan): what run_prefill and
// run_prefill_q are made of.  Nothing of the decode state is touched; every side stream is joined back into e->stream on return.
// The loop is layer-major: the interleaving of the parts within a layer is the enqueue order.
static int run_prefill_span(mellow_engine* e, int B, const PrefillSpan& sp) {
    PrefillPlan plan;
    PrefillPart parts[4];      // nh of them
    int nh = 1;
    CHK(prefill_plan(e, B, sp, plan));
    CHK(prefill_parts(e, plan, B, sp.x, parts, nh));
    StreamFork sides(e, nh - 1);
    CHK(sides.status);
    for (int l = 0; l < e->cfg.num_layers; ++l)
        for (int h = 0; h < nh; ++h) CHK(prefill_layer(e, plan, parts[h], l));
    CHK(sides.run());
    HIPCHK(hipGetLastError());
    return 0;
}

// `x` [rows per sequence = T_last ...] holds the input of the last layer.  Position word = index of the LAST prefix token: the decode
// kernels treat it as "the new token" (keys 0..T-2 from the pages, key T-1 recomputed and re-appended), and the first kernel of
// every later decode step advances it; the arg-max records its token at column (*d_pos - prefix_len + 1) = 0.
// row_ids (null: row r starts from row r * T + T - 1 of x): the source row of every decode row among the n_src rows of x.
static int finish_prefill(mellow_engine* e, int N, int T, const float* x, const int32_t* row_ids, int n_src, const RecordArgs* rec) {
    hipStream_t s = e->stream;
    const int NL = e->cfg.num_layers;
    { ProfScope ps(e, PF_MISC, 0, 0);
      launch_dec_load_rows(e->da, N, x, 576, row_ids, T, row_ids ? n_src : 0, s); }
    e->cur_B = N;
    e->cur_pos = T;
    e->h_pos_word = T - 1;
    HIPCHK(hipMemcpyAsync(e->d_pos, &e->h_pos_word, sizeof(int32_t), hipMemcpyHostToDevice, s));
    CHK(enqueue_decode_layer_range(e, N, NL - 1, NL, false));
    CHK(run_lm_head(e, N, DEC_KC_DOWN, rec));
    HIPCHK(hipGetLastError());
    return 0;
}

int run_prefill(mellow_engine* e, int B, int T, const RecordArgs* rec, bool all_positions, int n) {
    hipStream_t s = e->stream;
    const int NL = e->cfg.num_layers;
    const bool fan = n > 1;
    if (fan && (all_positions || T != e->cfg.prefix_len || e->opt.kv16 || !e->kprefix.p || !e->vprefix.p || !e->nseq_rows.p || B * n > e->kv_B))
        return fail("internal: the fan-out prefill needs fp32 pages for %d rows and its prefix buffer", B * n);
    CHK(run_prefill_span(e, B, PrefillSpan{T, 0, e->lm_x.p, fan, all_positions}));
    if (e->opt.kv16 && !e->kv16_direct && !all_positions) {
        // fp8 mode: the decode step streams a bf16 shadow of the pages (whole pages: the cleared tails travel with them)
        ProfScope ps(e, PF_MISC, 0, 3.0 * kv_layer_floats(e) * NL * 4);
        launch_kv_to_bf16(e->kcache.p, e->kcache16.p, (int64_t)(kv_layer_floats(e) * NL), s);
        launch_kv_to_bf16(e->vcache.p, e->vcache16.p, (int64_t)(kv_layer_floats(e) * NL), s);
    }
    if (all_positions) return 0;        // x = the hidden states after all layers, every position (mellow_lm_forward_logits)
    // n answers per example: every row's pages get its example's prefix K/V, and row r starts from its example's last prefix row
    if (fan) {
        ProfScope ps(e, PF_MISC, 0, (1.0 + n) * 2.0 * NL * B * 3 * T * 64 * 4);
        launch_kv_fanout(e->kprefix.p, e->vprefix.p, e->kcache.p, e->vcache.p, NL, B, n, e->kv_B, T, prefix_page_len(T), e->kv_Tmax, s);
    }
    return finish_prefill(e, B * n, T, e->lm_x.p, fan ? reinterpret_cast<const int32_t*>(e->nseq_rows.p) : nullptr, B * T, rec);
}

// Q questions per example (mellow_generate_q): positions [0, P) of a prefix depend on the clips only, so the layers run over them
// once per EXAMPLE (head: lm_x [B][P], K/V to the prefix buffer), the fan-out copies that K/V to the pages of the example's Q rows,
// and the layers run over [P, T) once per ROW (tail: lm_xq [B * Q][T - P], attention over the row's pages).  From the last prefix
// position on the pass is a plain one of B * Q rows.  P is a multiple of the attention's query tile, so every query of the tail sees
// the key tiles -- composition and order -- of the whole-sequence launch.
int run_prefill_q(mellow_engine* e, int B, int Q, int T, int P, const RecordArgs* rec) {
    const int NL = e->cfg.num_layers, N = B * Q, Tt = T - P;
    if (Q < 2 || P <= 0 || P >= T || P % 32 != 0 || T != e->cfg.prefix_len || e->opt.fp8 || e->opt.kv16 || !e->kprefix.p || !e->vprefix.p ||
        !e->nseq_rows.p || !e->lm_xq.p || N > e->kv_B)
        return fail("internal: the question prefill needs fp32 pages for %d rows, its prefix buffer and its tail input", N);
    CHK(run_prefill_span(e, B, PrefillSpan{P, 0, e->lm_x.p, true, false}));
    { ProfScope ps(e, PF_MISC, 0, (1.0 + Q) * 2.0 * NL * B * 3 * P * 64 * 4);
      launch_kv_fanout(e->kprefix.p, e->vprefix.p, e->kcache.p, e->vcache.p, NL, B, Q, e->kv_B, P, prefix_page_len(T), e->kv_Tmax, e->stream); }
    CHK(run_prefill_span(e, N, PrefillSpan{Tt, P, e->lm_xq.p, false, false}));
    return finish_prefill(e, N, T, e->lm_xq.p, reinterpret_cast<const int32_t*>(e->nseq_rows.p), N * Tt, rec);
}

// the 30 decode layers + head at position *d_pos (enqueue only; capture-safe).  5 launches per layer (dec_gemv.hip, dec_attn.hip):
//   qkv split-K | attention (RMS scale, RoPE, KV append, key-split flash decoding) | o_proj (merge + residual) |
//   gate/up | down split-K (RMS scale, SwiGLU); the down slabs are summed by the next layer's qkv/attention.
int enqueue_decode_layer_range(mellow_engine* e, int B, int l_begin, int l_end, bool inc_pos) {
    hipStream_t s = e->stream;
    const int Bp = e->da.rows;
    // developer knobs (wrong tokens, timing only): every layer on layer 0's weights / KV pages -- is a decode kernel's time the
    // cold fetch of its weights (538 MB per step cycle through the 256 MB Infinity Cache) or of its KV pages?
    // Compiled in only with -DMELLOW_DEVPROBE (tools/ab_build.sh): the release library has no switch that changes its answers.
#ifdef MELLOW_DEVPROBE
    static const bool same_w = getenv("MELLOW_DEV_SAME_WEIGHTS") != nullptr, same_kv = getenv("MELLOW_DEV_SAME_KV") != nullptr;
    // MELLOW_DEV_SKIP: bit mask of the per-layer launches left out (1 qkv, 2 attention, 4 o_proj, 8 gate/up, 16 down): what a
    // fusion that removes that launch could gain at most
    static const int skip = getenv("MELLOW_DEV_SKIP") ? atoi(getenv("MELLOW_DEV_SKIP")) : 0;
#else
    constexpr bool same_w = false, same_kv = false;
    constexpr int skip = 0;
#endif
    for (int l = l_begin; l < l_end; ++l) {
        const LMLayerW& w = e->w.layers[same_w ? 0 : l];
        const DecW qkv = w.qkv_w(), o = w.o_w(), gu = w.gateup_w(), dn = w.down_w();      // fp32, or e4m3 + row scales (fp8 mode)
        // (KV16: the bf16 shadow pages; a layer's pages are half as many floats)
        float* kc = e->opt.kv16 ? e->kcache16.p + kv_layer_floats(e) / 2 * (same_kv ? 0 : l) : e->kcache.p + kv_layer_floats(e) * (same_kv ? 0 : l);
        float* vc = e->opt.kv16 ? e->vcache16.p + kv_layer_floats(e) / 2 * (same_kv ? 0 : l) : e->vcache.p + kv_layer_floats(e) * (same_kv ? 0 : l);
        const int kcd = l == l_begin ? 0 : DEC_KC_DOWN;   // the first layer of the range starts from a materialised x
        // fused_in: this layer's q/k/v slabs (and the down slabs of x_new) were written by the previous layer's dec_qkv2 launch
        // The fused launch pays at ONE row block (B <= 32: 46.8 ms per 63 steps against 49.9 with the five-launch layer) and loses
        // beyond (fp32 weights, same box: B = 64: 68.4 ms fused against 68.0, B = 96: 91.2 / 87.9, B = 128: 105.6 / 102.1,
        // B = 256: 190.3 / 175.7, B = 512: 346.6 / 319.2 -- its composed operand is 1.7x the bytes of the two matrices it
        // replaces, and a larger batch is bound by bytes, not by launches); the e4m3 form was measured ahead at four row blocks
        // (round 3) and stays fused.  MELLOW_DECODE_FUSE_MAX_RB: developer override.
        const bool x3l = e->da.xmid3_32 != nullptr;       // f32x3 forms of gate/up and of the fused down + q/k/v launch (ensure_lm decides)
        const bool fuse_rb = x3l || e->da.RB <= e->opt.dec_fuse_max_rb;
        const bool fused_in = l > l_begin && ((w.qkv2 != nullptr && fuse_rb) || w.q2h8 != nullptr) && !same_w;
        DecArgs a = e->da;
        const int sq = e->dbg_seq0 >= 0 ? e->dbg_seq0 + 5 * (l - l_begin) : -1000;       // launch index inside the step (kdebug builds)
        auto da = [&](int k) { DecArgs x = e->da; x.dbg_seq = sq + k; return x; };
        a.dbg_seq = sq;
        a.first = l == l_begin ? 1 : 0;                     // the first kernel of a step stages the RoPE row ...
        a.inc_pos = (inc_pos && l == l_begin) ? 1 : 0;     // ... and advances the position word
        if (!(skip & 1) && !fused_in)
        { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * 576.0 * 960.0, 576.0 * 960.0 * 4);
          launch_dec_qkv(a, qkv.p, w.qkv_f.KP / 8, kcd, s, qkv.scale); }
        if (!(skip & 2))
        { ProfScope ps(e, PF_DECODE_ATTN, 4.0 * 64 * 9 * (double)B * (e->cur_pos + 1), 2.0 * (double)B * 3 * 64 * 4 * (e->cur_pos + 1));
          if (!launch_dec_attn(da(1), kc, vc, fused_in, s))
              return fail("decode attention launched with %d key splits at RB = %d", e->da.ts, e->da.RB); }
        if (!(skip & 4))
        { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * 576.0 * 576.0, 576.0 * 576.0 * 4);
          launch_dec_oproj(da(2), o.p, s, o.scale); }
        if (!(skip & 8))
        { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * 576.0 * 3072.0, 576.0 * 3072.0 * 4);
          if (x3l && !w.gu8) launch_dec_gateup3(da(3), w.gu16n, s);      // (the f32x3 form reads fp32 weights only)
          else launch_dec_gateup(da(3), gu.p, s, gu.scale); }
        const LMLayerW* nx = (l + 1 < l_end && !same_w) ? &e->w.layers[l + 1] : nullptr;
        if (nx && ((nx->qkv2 && fuse_rb) || nx->q2h8)) {
            // the down projection of this layer and the q/k/v projection of the next one as one launch (dec_gemv.hip, dec_qkv2_kernel)
            if (!(skip & 16))
            { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * (2112.0 * 960.0 + 1536.0 * 576.0), (2112.0 * 960.0 + 1536.0 * 576.0) * (nx->q2h8 ? 1 : 4));
              if (nx->q2h8) launch_dec_qkv2_w8(da(4), nx->qkv8, nx->qkv_sc, nx->q2h8, nx->q2h_sc, w.dn8, w.dn_sc, s);
              else if (x3l) launch_dec_qkv2x3(da(4), nx->qkv2, w.down.p, s);
              else launch_dec_qkv2(da(4), nx->qkv2, w.down.p, s); }
        } else if (!(skip & 16))
        { ProfScope ps(e, PF_SKINNY, 2.0 * Bp * 576.0 * 1536.0, 576.0 * 1536.0 * 4);
          launch_dec_down(da(4), dn.p, w.down.KP / 8, s, dn.scale); }
    }
    return 0;
}
int enqueue_decode_layers(mellow_engine* e, int B, const RecordArgs* rec) {
    CHK(enqueue_decode_layer_range(e, B, 0, e->cfg.num_layers, true));
    CHK(run_lm_head(e, B, DEC_KC_DOWN, rec));
    if (e->mode.beam > 1) {      // every surviving row owns its parent's K/V before the next step's attention reads it
        ProfScope ps(e, PF_MISC, 0, 0);
        launch_beam_reorder(e->kcache.p, e->vcache.p, e->kstage.p, e->vstage.p, beam_args(e, B, e->mode.beam).out_parent, e->d_pos, e->d_params,
                            e->cfg.prefix_len, e->cfg.num_layers, B, e->mode.beam, e->kv_B, e->kv_Tmax, e->stream);
    }
    return 0;
}

// audio1|audio2 are separate caller buffers: stage them into one [2B][n] batch so the encoder runs ONE pass
// of 2B clips (the reference runs two passes of B, mellow.py:105-106)
static int encode_pair(mellow_engine* e, const float* a1, const float* a2, int64_t n_samples, int B) {
    mellow_engine::Buf& cat = e->wavcat;
    CHK(ensure(e, cat, (size_t)2 * B * n_samples));
    HIPCHK(hipMemcpyAsync(cat.p, a1, (size_t)B * n_samples * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(cat.p + (size_t)B * n_samples, a2, (size_t)B * n_samples * 4, hipMemcpyDeviceToDevice, e->stream));
    return run_encoder(e, cat.p, 2 * B, n_samples, 0, 1, nullptr);
}
int encode_pair_to_prefix(mellow_engine* e, const float* a1, const float* a2, int64_t n_samples, const int32_t* ids,
                                 int B, float* prefix_out) {
    CHK(encode_pair(e, a1, a2, n_samples, B));
    { ProfScope ps(e, PF_MISC, 0, 0);
      launch_prefix_assemble(e->proj33.p, e->w.embed, ids, B, e->cfg.text_len, e->cfg.sep_token_id, e->cfg.vocab_size, prefix_out,
                             e->d_progress + 1, e->stream); }
    HIPCHK(hipGetLastError());
    return 0;
}
int encode_pair_to_head_tail(mellow_engine* e, const float* a1, const float* a2, int64_t n_samples, const int32_t* ids, int B, int Q,
                             int P, float* head_out, float* tail_out) {
    CHK(encode_pair(e, a1, a2, n_samples, B));
    { ProfScope ps(e, PF_MISC, 0, 0);
      launch_prefix_assemble_q(e->proj33.p, e->w.embed, ids, B, Q, e->cfg.text_len, P, e->cfg.sep_token_id, e->cfg.vocab_size, head_out,
                               tail_out, e->d_progress + 1, e->stream); }
    HIPCHK(hipGetLastError());
    return 0;
}

// The prompt ids are range-checked on the device (prefix_assemble_kernel sets word 1 of the mapped progress block); the host
// reads it once the stream is synchronised and fails like the reference's embedding lookup (IndexError in the Python binding).
void clear_bad_id(mellow_engine* e) { __atomic_store_n(e->h_progress + 1, 0ull, __ATOMIC_RELEASE); }

int check_bad_id(mellow_engine* e) {
    const unsigned long long w = __atomic_load_n(e->h_progress + 1, __ATOMIC_ACQUIRE);
    if (!w) return 0;
    return fail("index out of range in self: prompt id %d of example %u is outside the vocabulary [0, %d)", (int)(unsigned)(w & 0xffffffffu),
                (unsigned)((w >> 32) & 0x7fffffffu), e->cfg.vocab_size);
}

// ---- scoring: teacher-forced log-probs through an LM head that never writes its logits ------------------------------------------
// The hidden states of every position are in lm_x (run_prefill, all_positions).  The head is the exact fp32 MFMA GEMM of
// mellow_lm_forward_logits with the EPI_LSE epilogue (gemm_epilogue.h): per (row, 64-column group) one (max, sum of exponentials,
// arg-max) partial instead of 64 logits -- vocab / 64 x 12 bytes per row -- merged in ascending group order by lse_merge_kernel.
// Profiled as the family "lm_head_all_positions" (PF_LM_HEAD: gather + final norm + head GEMM + merge).
// A target (or candidate) id outside the vocabulary is flagged by the kernels in word 2 of the mapped progress block.
static void clear_bad_target(mellow_engine* e) { __atomic_store_n(e->h_progress + 2, 0ull, __ATOMIC_RELEASE); }
static int check_bad_target(mellow_engine* e, const char* what, int lo) {
    const unsigned long long w = __atomic_load_n(e->h_progress + 2, __ATOMIC_ACQUIRE);
    if (!w) return 0;
    return fail("index out of range in self: %s id %d of row %u is outside [%d, %d)", what, (int)(unsigned)(w & 0xffffffffu),
                (unsigned)((w >> 32) & 0x7fffffffu), lo, e->cfg.vocab_size);
}

int run_score_head(mellow_engine* e, int B, int T, int from_pos, int n, const int32_t* targets, float* out_logprob,
                   int32_t* out_argmax, float* out_lse, float* out_max) {
    hipStream_t s = e->stream;
    const int V = e->cfg.vocab_size, rows = B * n, groups = V / 64;
    if (V % 64 != 0 || e->w.lm_head.Nw != V) return fail("the scoring head tiles the vocabulary in groups of 64 columns (vocab %d)", V);
    const size_t ld = (size_t)rup(rows, 64);
    CHK(ensure(e, e->sc_part, (size_t)groups * ld * 3));         // (max, sum) pairs, then the arg-max words
    float2* part_ms = reinterpret_cast<float2*>(e->sc_part.p);
    int32_t* part_arg = reinterpret_cast<int32_t*>(e->sc_part.p + (size_t)groups * ld * 2);
    float* tgt_logit = e->sc_ws.p;                               // [rows] (the callers size sc_ws: target logits first)
    GemmArgs g = lin(e->lm_xn.p, 576, rows, e->w.lm_head, nullptr, 0, nullptr);
    g.epi = EPI_LSE;
    g.lse_target = targets; g.lse_ms = part_ms; g.lse_arg = part_arg; g.lse_tgt = tgt_logit; g.lse_ld = (int64_t)ld;
    // bytes: the head weight once, the normed rows, and the partials written by the GEMM and read twice by the merge
    ProfScope ps(e, PF_LM_HEAD, gemm_flops(g), 576.0 * V * 4 + (double)rows * 576 * 4 + 3.0 * rows * groups * 12);
    // final norm on the scored rows only, as mellow_lm_forward_logits does
    launch_gather_span(e->lm_x.p, B, T, from_pos, n, e->lm_o.p, s);
    launch_rmsnorm(e->lm_o.p, e->lm_xn.p, rows, 576, e->w.final_norm, e->cfg.rms_norm_eps, s);
    launch_gemm(g, s);
    launch_lse_merge(part_ms, part_arg, (int64_t)ld, groups, rows, targets, tgt_logit, V, out_logprob, out_argmax, out_lse, out_max,
                     e->d_progress + 2, s);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

int mellow_prefix(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                  int B, float* out) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!audio1 || !audio2 || !input_ids || !out) return fail("null argument");
    if (B <= 0) return fail("B must be positive");
    HIPCHK(hipSetDevice(e->device));
    clear_bad_id(e);
    CHK(encode_pair_to_prefix(e, audio1, audio2, n_samples, input_ids, B, out));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_bad_id(e);
}

int mellow_lm_prefill(mellow_engine_t* e, const float* prefix, int B, int T, int reserve, float* logits) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!prefix || B <= 0 || T <= 0 || reserve < 0) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure_lm(e, B, T, T + reserve + 1));
    HIPCHK(hipMemcpyAsync(e->lm_x.p, prefix, (size_t)B * T * 576 * 4, hipMemcpyDeviceToDevice, e->stream));
    CHK(clear_page_tails(e, T, e->kv_Tmax));
    CHK(run_prefill(e, B, T, nullptr));
    if (logits)
        HIPCHK(hipMemcpyAsync(logits, e->dlogits.p, (size_t)B * e->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_lm_decode_step(mellow_engine_t* e, const int32_t* token_ids, float* logits) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!token_ids) return fail("null argument");
    if (e->cur_B <= 0) return fail("decode step without a prefill");
    if (e->cur_pos + 1 > e->kv_Tmax) return fail("KV pages exhausted (reserve too small)");
    HIPCHK(hipSetDevice(e->device));
    const int B = e->cur_B;
    launch_dec_load_rows(e->da, B, e->w.embed, 576, token_ids, 0, e->cfg.vocab_size, e->stream);
    CHK(enqueue_decode_layers(e, B, nullptr));   // its first kernel advances the device position word
    e->cur_pos += 1;
    if (logits)
        HIPCHK(hipMemcpyAsync(logits, e->dlogits.p, (size_t)B * e->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// Numeric tap of the decode step's lm_head kernel (dec_fullk_kernel) on caller-supplied rows: logits[B][vocab] = x[B][hidden] .
// lm_head^T with the engine's own head weights -- the e4m3 copy when the engine holds one (fp8 mode), and then act_fp8 selects
// whether the activations are quantised in the kernel (fp8 matrix pipe) or stay fp32.  x and logits are device buffers.
int mellow_debug_dec_head(mellow_engine_t* e, const float* x, int B, int act_fp8, float* logits) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!x || !logits || B <= 0 || B > 1024) return fail("bad argument");
    if (e->cfg.hidden_size != 576) return fail("the decode kernels are built for hidden size 576");
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure_lm(e, B, 1, 2));
    DecArgs a = e->da;
    a.blk_live = nullptr; a.row_of_slot = nullptr;
    a.a8 = (act_fp8 && e->w.head8) ? 1 : 0;
    a.xnF = a.xmidF;                                  // dec_load_rows writes the F32-layout operand there
    a.xn3 = nullptr;                                  // (the f32x3 kernel splits these rows itself)
    launch_dec_load_rows(a, B, x, 576, nullptr, 1, 0, e->stream);
    const DecW h = e->w.head_w();
    launch_dec_lm_head(a, h.p, e->w.lm_head.KP / 8, e->cfg.vocab_size, e->stream, h.scale);
    HIPCHK(hipMemcpyAsync(logits, e->dlogits.p, (size_t)B * e->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    return 0;
}

// The twin of mellow_debug_dec_head with the head kernel in its LSE variant (DecArgs::cand_sum) and the merge of the partials that the
// arg-max / the sampler of a scored generate call run (common.h: dec_lse_max, dec_lse_sum): per row lse = M + log S, M, and the arg-max.
int mellow_debug_dec_head_lse(mellow_engine_t* e, const float* x, int B, int act_fp8, float* logits, float* out_lse, float* out_max,
                              int32_t* out_argmax) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!x || !out_lse || !out_max || !out_argmax || B <= 0 || B > 1024) return fail("bad argument");
    if (e->cfg.hidden_size != 576) return fail("the decode kernels are built for hidden size 576");
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure_lm(e, B, 1, 2));
    const int NT = e->cfg.vocab_size / 32;
    CHK(ensure(e, e->cand_sum, (size_t)e->da.rows * NT));
    DecArgs a = e->da;
    a.blk_live = nullptr; a.row_of_slot = nullptr;
    a.a8 = (act_fp8 && e->w.head8) ? 1 : 0;
    a.xnF = a.xmidF;                                  // dec_load_rows writes the F32-layout operand there
    a.xn3 = nullptr;                                  // (fp32 rows: the exact fp32 / e4m3 kernel, as in mellow_debug_dec_head)
    a.cand_sum = e->cand_sum.p;
    if (!logits) a.logits = nullptr;
    launch_dec_load_rows(a, B, x, 576, nullptr, 1, 0, e->stream);
    const DecW h = e->w.head_w();
    launch_dec_lm_head(a, h.p, e->w.lm_head.KP / 8, e->cfg.vocab_size, e->stream, h.scale);
    launch_dec_argmax(a, B, NT, e->d_tokens, e->w.embed, 0, LoopArgs(), e->stream);
    launch_dec_lse_tap(a, B, NT, out_lse, out_max, e->stream);
    HIPCHK(hipMemcpyAsync(out_argmax, e->d_tokens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream));
    if (logits) HIPCHK(hipMemcpyAsync(logits, e->dlogits.p, (size_t)B * e->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->cur_B = 0;                                     // the decode state of an earlier prefill is gone
    return 0;
}

// lm.model.embed_tokens(ids) (reference decoder.py:47,64-66; wrapper.py:237): rows of the embedding table
int mellow_embed_tokens(mellow_engine_t* e, const int32_t* token_ids, int n, float* out) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!token_ids || !out || n <= 0) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    launch_gather_rows(e->w.embed, 576, token_ids, n, e->cfg.vocab_size, out, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// The decoder's forward over a whole embedded sequence (reference decoder.py:57-90 `self.lm(inputs_embeds=embedding_cat)`,
// reached from Mellow.forward mellow.py:89-98 -- the training-time forward): logits of EVERY position t >= from_pos, not only
// the last one.  embeds dev [B][T][hidden]; logits dev [B][T - from_pos][vocab].  All 30 layers run on all positions (the
// generation path's last-layer shortcut does not apply), then the final RMSNorm and the tied lm_head as one GEMM on the
// exact fp32 kernel (in every precision mode: the head is not part of the split / fp8 GEMM set).
int mellow_lm_forward_logits(mellow_engine_t* e, const float* embeds, int B, int T, int from_pos, float* logits) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!embeds || !logits || B <= 0 || T <= 0 || from_pos < 0 || from_pos >= T) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    CHK(ensure_lm(e, B, T, T + 1));
    HIPCHK(hipMemcpyAsync(e->lm_x.p, embeds, (size_t)B * T * 576 * 4, hipMemcpyDeviceToDevice, s));
    CHK(run_prefill(e, B, T, nullptr, true));
    e->cur_B = 0;                                   // no decode state: a decode step needs a real prefill first
    const int n = T - from_pos;
    // final norm on the selected rows only: gather [B][n][576] out of [B][T][576] into lm_xn, then normalise in place
    GemmArgs g = lin(e->lm_xn.p, 576, B * n, e->w.lm_head, logits, e->cfg.vocab_size, nullptr);
    { ProfScope ps(e, PF_LM_HEAD, gemm_flops(g), (576.0 + (double)B * n) * e->cfg.vocab_size * 4 + (double)B * n * 576 * 4);
      launch_gather_span(e->lm_x.p, B, T, from_pos, n, e->lm_o.p, s);
      launch_rmsnorm(e->lm_o.p, e->lm_xn.p, B * n, 576, e->w.final_norm, e->cfg.rms_norm_eps, s);
      launch_gemm(g, s); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int mellow_lm_score(mellow_engine_t* e, const float* embeds, int B, int T, int from_pos, const int32_t* targets,
                    float* out_logprob, int32_t* out_argmax, float* out_lse, float* out_max) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!embeds || !targets || !out_logprob || B <= 0 || T <= 0 || from_pos < 0 || from_pos >= T) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    CHK(ensure_lm(e, B, T, T + 1));
    CHK(ensure(e, e->sc_ws, (size_t)B * (T - from_pos)));
    clear_bad_target(e);
    HIPCHK(hipMemcpyAsync(e->lm_x.p, embeds, (size_t)B * T * 576 * 4, hipMemcpyDeviceToDevice, s));
    CHK(run_prefill(e, B, T, nullptr, true));
    e->cur_B = 0;                                   // no decode state, like mellow_lm_forward_logits
    CHK(run_score_head(e, B, T, from_pos, T - from_pos, targets, out_logprob, out_argmax, out_lse, out_max));
    HIPCHK(hipStreamSynchronize(s));
    return check_bad_target(e, "target", -1);
}

int mellow_score(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids, int B,
                 const int32_t* cand_ids, const int32_t* cand_len, int K, int L, float* out_logprob, float* out_sum,
                 int32_t* out_argmax) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!audio1 || !audio2 || !input_ids || !cand_ids || !cand_len || !out_logprob || !out_sum) return fail("null argument");
    if (B <= 0 || K <= 0 || L <= 0) return fail("B, K and L must be positive");
    if (B > 1024) return fail("mellow_score takes at most 1024 examples per call (got %d)", B);
    const int P = e->cfg.prefix_len, T = P + L - 1;
    if ((int64_t)P + L > e->cfg.max_positions)
        return fail("prefix + candidate length = %d + %d exceeds max_positions %d", P, L, e->cfg.max_positions);
    const int64_t rows = (int64_t)B * K;
    for (int64_t r = 0; r < rows; ++r)
        if (cand_len[r] < 1 || cand_len[r] > L)
            return fail("cand_len[%d][%d] = %d is outside [1, %d]", (int)(r / K), (int)(r % K), cand_len[r], L);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    constexpr int kPassRows = 1024;                  // rows of one LM pass, as in mellow_generate
    const int pass = rows < kPassRows ? (int)rows : kPassRows;
    // per-row words: [target logits: pass x L | targets: pass x L | candidate lengths: rows]
    CHK(ensure(e, e->sc_ws, (size_t)2 * pass * L + (size_t)rows));
    int32_t* d_targets = reinterpret_cast<int32_t*>(e->sc_ws.p + (size_t)pass * L);
    int32_t* d_len = reinterpret_cast<int32_t*>(e->sc_ws.p + (size_t)2 * pass * L);
    CHK(ensure(e, e->sc_prefix, (size_t)B * P * 576));
    clear_bad_id(e);
    clear_bad_target(e);
    HIPCHK(hipMemcpyAsync(d_len, cand_len, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // front-end, encoder, projection and prefix: once per example
    CHK(encode_pair_to_prefix(e, audio1, audio2, n_samples, input_ids, B, e->sc_prefix.p));
    for (int64_t r0 = 0; r0 < rows; r0 += kPassRows) {
        const int nr = rows - r0 < kPassRows ? (int)(rows - r0) : kPassRows;
        CHK(ensure_lm(e, nr, T, T + 1));
        { ProfScope ps(e, PF_MISC, 0, 2.0 * nr * T * 576 * 4);
          launch_score_build_input(e->sc_prefix.p, e->w.embed, cand_ids, d_len, K, L, P, e->cfg.vocab_size, (int)r0, nr, e->lm_x.p,
                                   d_targets, e->d_progress + 2, s); }
        CHK(run_prefill(e, nr, T, nullptr, true));
        e->cur_B = 0;
        CHK(run_score_head(e, nr, T, P - 1, L, d_targets, out_logprob + r0 * L, out_argmax ? out_argmax + r0 * L : nullptr, nullptr,
                           nullptr));
    }
    launch_score_sum(out_logprob, d_len, (int)rows, L, out_sum, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    CHK(check_bad_id(e));
    return check_bad_target(e, "candidate", 0);
}

}  // extern "C"
