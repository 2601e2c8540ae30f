// The generation loop on top of the LM (A16: reference wrapper.py:197-256): one request record and its checks, the split into passes
// of <= 1024 rows, the pass body (loop state, step graphs, ticket waiting, length bookkeeping) and the mellow_generate* entry points.
#include "engine_internal.h"

// Every argument of a generation call, named once.  The four entry points fill one and call generate().
struct GenRequest {
    const float *audio1, *audio2;                // inputs: dev f32 [examples][n_samples] each
    int64_t n_samples;
    const int32_t* input_ids;                    // dev [examples][q][text_len]
    // n answer rows per example (n = 1: every row is an example of its own); q questions per example, a row each (mellow_generate_q);
    // never both above 1
    int examples, n, q, max_len, stop_id, ignore_stop;
    bool on;                                     // sampling: false = the greedy arg-max, and the four fields below are not read
    float top_p, temperature;
    uint64_t seed;
    int32_t row_offset;
    int32_t* out_tokens;                         // outputs: [rows][max_len], host or device
    float* out_logprob;                          // dev f32 [rows][max_len], the log-prob of every recorded token; null: not recorded
    int32_t *out_len, *out_steps;
    float* first_token_ms;
    // beam search (mellow_generate_beam): beam = k >= 1 beams per example, carried in n as the rows per example are; out_tokens /
    // out_logprob are then the token / increment tables [max_len][rows], out_parent the parent table and out_cum [rows]
    int beam = 0;
    int32_t* out_parent = nullptr;
    float* out_cum = nullptr;
    LogitRules rules;                            // repetition controls (mellow_generate_rules): taken from the context at entry, the same for every pass
    Guidance guide;                              // contrastive guidance (mellow_generate_guidance): likewise; rows 2p and 2p + 1 are then pair p
    TopLogprobs top;                             // top log-probs (mellow_generate_top_logprobs): likewise; the record [rows][max_len][k] advances with the passes
    SampleFilters filters;                       // top_k / min_p (mellow_generate_filters): likewise, the same for every pass
    Constraint con;                              // constrained decoding (mellow_generate_constraint): likewise; the roots advance with the passes
    int con_row0 = 0;                            // ... the first row of this pass among the roots of the call
    StopStrings stop;                            // stop strings (mellow_generate_stop_strings): likewise, the same for every pass
    int rows() const { return examples * n * q; }
    // rows [r0, r0 + nb) of an n = 1, q = 1 request as a request of their own; a row's random stream follows its index in the whole call
    GenRequest pass(int r0, int nb, int text_len, int32_t* steps, float* ftm) const {
        GenRequest p = *this;
        p.audio1 += (size_t)r0 * n_samples; p.audio2 += (size_t)r0 * n_samples; p.input_ids += (size_t)r0 * text_len;
        p.examples = nb; p.row_offset += guide.on ? r0 >> 1 : r0;      // (guided: r0 is even, and the streams go by pair)
        p.con_row0 += r0;
        p.out_tokens += (size_t)r0 * max_len;
        if (out_logprob) p.out_logprob += (size_t)r0 * max_len;
        if (top.k) { p.top.ids += (size_t)r0 * max_len * top.k; p.top.lp += (size_t)r0 * max_len * top.k; }
        if (out_len) p.out_len += r0;
        p.out_steps = steps; p.first_token_ms = ftm;
        return p;
    }
};
enum { DOOR_SCORED = 1, DOOR_N = 2, DOOR_Q = 4, DOOR_BEAM = 8 };     // what a rule of one entry point needs to know: mellow_generate_scored, mellow_generate_n, mellow_generate_q, mellow_generate_beam
constexpr int64_t kBeamStageRows = 65536;        // B * k * max_len a beam call may stage: 30 layers x 65536 x 3 x 64 fp32 = 1.5 GB per tensor
constexpr int kPassRows = 1024;                  // rows of one pass: 32 row blocks of loop state
constexpr int64_t kTopRecord = 1 << 24;          // rows * max_len * k the top log-probs record of one pass may hold (two buffers of 67 MB)

static int check_sampling(mellow_engine_t* e, float top_p, float temperature) {
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the sampler is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail("temperature must be finite and > 0 (got %g); greedy is mellow_generate", (double)temperature);
    if (top_p != top_p) return fail("top_p is NaN");
    return 0;
}

// The value rules of a mellow_sample_filters_t, each once (mellow_generate_filters and mellow_sample_logits_filtered): host code
// only, no engine and no device needed.
static int check_filters(const mellow_sample_filters_t* f) {
    if (f->size != (int32_t)sizeof(mellow_sample_filters_t))
        return fail("mellow_sample_filters_t.size is %d, this library's struct has %d bytes", (int)f->size, (int)sizeof(mellow_sample_filters_t));
    if (f->top_k < 0) return fail("top_k must be >= 0 (got %d); 0 is off", (int)f->top_k);
    if (!(f->min_p >= 0.f && f->min_p <= 1.f)) return fail("min_p must be in [0, 1] (got %g); 0 is off", (double)f->min_p);
    return 0;
}

static void stage_sampling(mellow_engine_t* e, float top_p, float temperature, uint64_t seed, int32_t row_offset, int step,
                           const SampleFilters& f = SampleFilters()) {
    uint32_t* w = e->h_sparams;
    w[SMP_SEED_LO] = (uint32_t)seed; w[SMP_SEED_HI] = (uint32_t)(seed >> 32); w[SMP_ROW_OFF] = (uint32_t)row_offset;
    memcpy(&w[SMP_TOP_P], &top_p, 4); memcpy(&w[SMP_TEMP], &temperature, 4); w[SMP_STEP] = (uint32_t)step;
    w[SMP_TOP_K] = (uint32_t)f.top_k;
    w[SMP_QMIN] = (uint32_t)std::nearbyint((double)f.min_p * 2147483648.0);      // rn(min_p * 2^31): the product is exact, ties to even as the kernel's q
}

// The value rules of a mellow_logit_rules_t, each once (mellow_generate_rules and mellow_logit_rules_apply): host code only, no
// engine and no device needed.
static int check_rules(const mellow_logit_rules_t* r) {
    if (r->size != (int32_t)sizeof(mellow_logit_rules_t))
        return fail("mellow_logit_rules_t.size is %d, this library's struct has %d bytes", (int)r->size, (int)sizeof(mellow_logit_rules_t));
    if (!std::isfinite(r->repetition_penalty) || !(r->repetition_penalty > 0.f))
        return fail("repetition_penalty must be finite and > 0 (got %g); 1 is off", (double)r->repetition_penalty);
    if (r->no_repeat_ngram_size < 0) return fail("no_repeat_ngram_size must be >= 0 (got %d); 0 is off", (int)r->no_repeat_ngram_size);
    if (r->min_new_tokens < 0) return fail("min_new_tokens must be >= 0 (got %d); 0 is off", (int)r->min_new_tokens);
    return 0;
}

// a checked struct -> the context: the values, and the bias copied (from host or device memory) into the context's own buffer
static int load_rules(mellow_engine_t* e, const mellow_logit_rules_t* r, LogitRules* out) {
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the logit rules are built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure(e, e->rules_bias, SAMPLE_MAX_V));
    if (r->logit_bias) {
        HIPCHK(hipMemcpyAsync(e->rules_bias.p, r->logit_bias, (size_t)SAMPLE_MAX_V * sizeof(float), hipMemcpyDefault, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));         // the caller's vector is free again on return
    }
    out->on = true; out->theta = r->repetition_penalty; out->ngram = r->no_repeat_ngram_size; out->min_new = r->min_new_tokens;
    out->bias = r->logit_bias != nullptr;
    return 0;
}

// the value block a rules launch reads
static int stage_rules(mellow_engine_t* e, const LogitRules& r, int stop_id) {
    uint32_t* w = e->h_rparams;
    memcpy(&w[RUL_THETA], &r.theta, 4);
    w[RUL_NGRAM] = (uint32_t)r.ngram; w[RUL_MIN_NEW] = (uint32_t)r.min_new; w[RUL_BIAS_ON] = r.bias ? 1u : 0u; w[RUL_STOP] = (uint32_t)stop_id;
    HIPCHK(hipMemcpyAsync(e->d_rparams, e->h_rparams, sizeof(e->h_rparams), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// `n` int32 words of host or device memory -> host memory
static int fetch_words(int32_t* dst, const int32_t* src, size_t n) {
    if (n == 0) return 0;
    hipPointerAttribute_t at;
    const bool on_device = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!on_device) {
        (void)hipGetLastError();                  // a plain host pointer is not an error here
        memcpy(dst, src, n * sizeof(int32_t));
        return 0;
    }
    HIPCHK(hipMemcpy(dst, src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// The value rules of a mellow_constraint_t, each once and in the order the header states (mellow_generate_constraint and
// mellow_constraint_apply): host code only, no engine needed.  -> the arena as the kernel reads it (kernels.h ConstrainArgs::trie)
// and the roots, in host memory.
static int check_constraint(const mellow_constraint_t* c, std::vector<int32_t>* arena, std::vector<int32_t>* roots) {
    if (c->size != (int32_t)sizeof(mellow_constraint_t))
        return fail("mellow_constraint_t.size is %d, this library's struct has %d bytes", (int)c->size, (int)sizeof(mellow_constraint_t));
    const int nn = c->n_nodes, ne = c->n_edges, nr = c->n_rows;
    if (nn < 1 || ne < 0 || nr < 1 || nn > CON_MAX_COUNT || ne > CON_MAX_COUNT || nr > CON_MAX_COUNT)
        return fail("constraint counts: n_nodes %d, n_rows %d must be 1 to %d and n_edges %d 0 to %d", nn, nr, CON_MAX_COUNT, ne, CON_MAX_COUNT);
    if (!c->node_first || !c->node_flags || !c->row_root || (ne > 0 && (!c->edge_token || !c->edge_child))) return fail("constraint: null array");
    if (c->then_free != 0 && c->then_free != 1) return fail("constraint: then_free must be 0 or 1 (got %d)", (int)c->then_free);
    arena->assign((size_t)2 * nn + 1 + 2 * (size_t)ne, 0);
    roots->assign((size_t)nr, 0);
    int32_t *first = arena->data(), *flags = first + nn + 1, *tok = flags + nn, *child = tok + ne;
    CHK(fetch_words(first, c->node_first, (size_t)nn + 1));
    CHK(fetch_words(flags, c->node_flags, (size_t)nn));
    CHK(fetch_words(tok, c->edge_token, (size_t)ne));
    CHK(fetch_words(child, c->edge_child, (size_t)ne));
    CHK(fetch_words(roots->data(), c->row_root, (size_t)nr));
    if (first[0] != 0 || first[nn] != ne) return fail("constraint: node_first must run from 0 to n_edges = %d (got %d .. %d)", ne, (int)first[0], (int)first[nn]);
    for (int u = 0; u < nn; ++u)
        if (first[u + 1] < first[u]) return fail("constraint: node_first decreases at node %d", u);
    for (int u = 0; u < nn; ++u)
        for (int e = first[u] + 1; e < first[u + 1]; ++e)
            if (tok[e] <= tok[e - 1]) return fail("constraint: the edges of node %d are not sorted by token, strictly ascending (%d after %d)", u, (int)tok[e], (int)tok[e - 1]);
    for (int u = 0; u < nn; ++u)
        for (int e = first[u]; e < first[u + 1]; ++e)
            if (child[e] <= u || child[e] >= nn) return fail("constraint: node %d has child %d; every child is > its parent and < n_nodes = %d", u, (int)child[e], nn);
    for (int r = 0; r < nr; ++r) {
        const int u = (*roots)[r];
        if (u < 0 || u >= nn) return fail("constraint: row_root[%d] = %d is outside [0, n_nodes = %d)", r, u, nn);
        if (flags[u] & 1) return fail("constraint: row_root[%d] = node %d is terminal, a root never is (no empty phrase)", r, u);
    }
    for (int e = 0; e < ne; ++e)
        if (tok[e] < 0 || tok[e] >= SAMPLE_MAX_V) return fail("constraint: edge token %d is outside the vocabulary [0, %d)", (int)tok[e], SAMPLE_MAX_V);
    return 0;
}

// the value block a constraint launch reads, into `dst` (device)
static int stage_constraint(mellow_engine_t* e, const Constraint& c, int stop_id, float* dst) {
    uint32_t* w = e->h_cparams;
    w[CON_STOP] = (uint32_t)stop_id; w[CON_THEN_FREE] = c.then_free ? 1u : 0u; w[CON_NODES] = (uint32_t)c.n_nodes; w[CON_EDGES] = (uint32_t)c.n_edges;
    HIPCHK(hipMemcpyAsync(dst, e->h_cparams, sizeof(e->h_cparams), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// The value rules of a mellow_stop_strings_t, each once and in the order the header states (mellow_generate_stop_strings and
// mellow_stop_strings_apply): host code only, no engine needed.  -> the strings as a call carries them.
static int check_stop_strings(const mellow_stop_strings_t* s, StopStrings* out) {
    if (s->size != (int32_t)sizeof(mellow_stop_strings_t))
        return fail("mellow_stop_strings_t.size is %d, this library's struct has %d bytes", (int)s->size, (int)sizeof(mellow_stop_strings_t));
    if (s->n_strings < 1 || s->n_strings > STS_MAX_STRINGS) return fail("stop strings: a call takes 1 to %d strings (got %d)", STS_MAX_STRINGS, (int)s->n_strings);
    if (!s->str_off || !s->str_bytes) return fail("stop strings: null array");
    *out = StopStrings();
    for (int j = 0; j < s->n_strings; ++j) {
        const int64_t m = (int64_t)s->str_off[j + 1] - s->str_off[j];
        if (m < 1 || m > STS_MAX_STR_LEN) return fail("stop strings: string %d has %lld bytes, a string has 1 to %d", j, (long long)m, STS_MAX_STR_LEN);
        memcpy(out->bytes + out->off[j], s->str_bytes + s->str_off[j], (size_t)m);
        out->off[j + 1] = out->off[j] + (int32_t)m;
    }
    for (int j = s->n_strings; j < STS_MAX_STRINGS; ++j) out->off[j + 1] = out->off[j];
    out->on = true; out->n = s->n_strings;
    return 0;
}

// what an engine must be for a stop-strings launch, each rule once
static int check_stop_engine(mellow_engine_t* e) {
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the stop-strings kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    if (!e->w.vocab_bytes || !e->w.vocab_bytes->set) return fail("stop strings need the vocabulary's bytes: call mellow_set_vocab_bytes first");
    return 0;
}
static int check_stop_id(int stop_id, bool never_stops) {
    if (stop_id < 0 || stop_id >= SAMPLE_MAX_V || never_stops)
        return fail("stop strings end a row through the stop token: stop_id = %d%s is no token of the vocabulary [0, %d)", stop_id,
                    never_stops ? " under ignore_stop (a beam call then knows no stop token)" : "", SAMPLE_MAX_V);
    return 0;
}

// the block a stop-strings launch reads, into `dst` (device)
static int stage_stop_strings(mellow_engine_t* e, const StopStrings& st, int stop_id, float* dst) {
    uint32_t* w = e->h_stopblk;       // (a member: alive until the copy has run)
    memset(w, 0, sizeof(e->h_stopblk));
    w[STS_STOP] = (uint32_t)stop_id; w[STS_COUNT] = (uint32_t)st.n;
    for (int j = 0; j <= STS_MAX_STRINGS; ++j) w[STS_OFF + j] = (uint32_t)st.off[j];
    memcpy(w + STS_WORDS, st.bytes, sizeof(st.bytes));
    HIPCHK(hipMemcpyAsync(dst, e->h_stopblk, sizeof(e->h_stopblk), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// the value block a guidance launch reads
static int stage_guidance(mellow_engine_t* e, float scale) {
    memcpy(&e->h_gparams[GDN_SCALE], &scale, 4);
    HIPCHK(hipMemcpyAsync(e->d_gparams, e->h_gparams, sizeof(e->h_gparams), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// Every argument rule of the six entry points, each once.
static int check_request(mellow_engine_t* e, const GenRequest& r, int door) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (r.guide.on) {      // (first: whatever else is wrong with such a call, this is what its caller has to hear)
        if (r.beam) return fail("guidance is armed (mellow_generate_guidance): mellow_generate_beam does not take it (beam search over pairs is not built)");
        if (r.n > 1) return fail("guidance is armed (mellow_generate_guidance): mellow_generate_n with n > 1 does not take it (pass every pair n times to mellow_generate_sampled)");
        if (r.q > 1) return fail("guidance is armed (mellow_generate_guidance): mellow_generate_q with Q > 1 does not take it (pass a pair per question to mellow_generate)");
    }
    if (r.top.k) {         // (likewise)
        if (r.beam) return fail("top log-probs are armed (mellow_generate_top_logprobs): mellow_generate_beam does not take them (top log-probs of a beam hypothesis are not built)");
        if (!r.out_logprob) return fail("top log-probs are armed (mellow_generate_top_logprobs): this call records no log-probs (use mellow_generate_scored, or mellow_generate_n / mellow_generate_q with an out_logprob)");
    }
    if (r.filters.on) {    // (likewise)
        if (r.beam) return fail("sample filters are armed (mellow_generate_filters): mellow_generate_beam does not take them (top_k / min_p filter a sampled draw)");
        if (!r.on) return fail("sample filters are armed (mellow_generate_filters): this call does not sample (use mellow_generate_sampled, or do_sample != 0)");
    }
    if (r.n < 1) return fail("n must be >= 1 (got %d)", r.n);
    if (r.q < 1) return fail("Q must be >= 1 (got %d)", r.q);
    if (r.n > 1 && r.q > 1) return fail("internal: n and Q are never both above 1");
    if (door & DOOR_BEAM) {
        if (r.beam < 1 || r.beam > BEAM_MAX_K) return fail("mellow_generate_beam takes 1 to %d beams per example (got k = %d)", BEAM_MAX_K, r.beam);
        if (r.beam != r.n || r.q != 1 || r.on) return fail("internal: a beam request carries k in n and neither samples nor asks several questions");
        if (!r.out_parent || !r.out_cum) return fail("null argument");
    }
    if ((door & DOOR_N) && !r.on) return fail("mellow_generate_n needs do_sample != 0: %d greedy answers of one example are %d copies of one answer", r.n, r.n);
    if (!r.audio1 || !r.audio2 || !r.input_ids || !r.out_tokens || ((door & DOOR_SCORED) && !r.out_logprob)) return fail("null argument");
    if (r.examples <= 0 || r.max_len <= 0) return fail("B and max_len must be positive");
    if ((door & DOOR_N) && (int64_t)r.examples * r.n > kPassRows)
        return fail("mellow_generate_n takes at most 1024 answer rows per call: B * n = %d * %d = %lld (split the examples over several calls, "
                    "advancing row_offset by n per example)", r.examples, r.n, (long long)r.examples * r.n);
    if ((door & DOOR_Q) && (int64_t)r.examples * r.q > kPassRows)
        return fail("mellow_generate_q takes at most 1024 answer rows per call: B * Q = %d * %d = %lld (split the examples over several calls, "
                    "advancing row_offset by Q per example)", r.examples, r.q, (long long)r.examples * r.q);
    if (door & DOOR_BEAM) {
        if ((int64_t)r.examples * r.beam > kPassRows)
            return fail("mellow_generate_beam takes at most 1024 beam rows per call: B * k = %d * %d = %lld (split the examples over several calls)",
                        r.examples, r.beam, (long long)r.examples * r.beam);
        if (r.beam > 1 && (int64_t)r.examples * r.beam * r.max_len > kBeamStageRows)
            return fail("mellow_generate_beam stages at most %lld rows x positions of K/V per call (1.5 GB per tensor): B * k * max_len = %d * %d * %d "
                        "= %lld (split the examples over several calls, or lower max_len)", (long long)kBeamStageRows, r.examples, r.beam, r.max_len,
                        (long long)r.examples * r.beam * r.max_len);
        if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the beam select is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
        if (r.beam > 1 && (e->opt.fp8 || e->opt.kv16))
            return fail("mellow_generate_beam with k > 1 is not available in MELLOW_PRECISION_FP8: the bf16 K/V pages of that mode have no fan-out "
                        "(k = 1 works; or sample and re-rank with mellow_generate_scored)");
    }
    if (r.out_logprob && !(door & DOOR_BEAM) && e->cfg.vocab_size % 32 != 0) return fail("the log-prob partials tile the vocabulary in groups of 32 columns (vocab %d)", e->cfg.vocab_size);
    if (r.n > 1 && (e->opt.fp8 || e->opt.kv16))
        return fail("mellow_generate_n with n > 1 is not available in MELLOW_PRECISION_FP8: the bf16 K/V pages of that mode have no fan-out "
                    "(n = 1 works; or pass every example n times to mellow_generate_sampled)");
    if (r.q > 1 && (e->opt.fp8 || e->opt.kv16))
        return fail("mellow_generate_q with Q > 1 is not available in MELLOW_PRECISION_FP8: the bf16 K/V pages of that mode have no fan-out "
                    "(Q = 1 works; or pass every example once per question to mellow_generate)");
    if (r.on) {
        CHK(check_sampling(e, r.top_p, r.temperature));
        if (r.row_offset < 0) return fail("row_offset must be >= 0");
    }
    if (r.guide.on) {
        if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the guidance kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
        if (r.examples % 2 != 0) return fail("guidance is armed (mellow_generate_guidance): B counts rows, conditional and negative interleaved, and must be even (got %d)", r.examples);
    }
    if (r.top.k) {
        if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the top log-probs kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
        const int64_t pass_rows = r.rows() < kPassRows ? r.rows() : kPassRows;
        if (pass_rows * r.max_len * r.top.k > kTopRecord)
            return fail("the top log-probs record of one pass holds at most %lld entries: rows * max_len * k = %lld * %d * %d (lower k or max_len, or split the examples over several calls)",
                        (long long)kTopRecord, (long long)pass_rows, r.max_len, r.top.k);
    }
    if (r.rules.on) {
        if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the logit rules are built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
        if (r.max_len > RULES_MAX_HIST) return fail("a call with logit rules takes max_len <= %d, the history one row stages (got %d)", RULES_MAX_HIST, r.max_len);
    }
    if (r.con.on) {
        if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the constraint kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
        if (r.con.n_rows != r.rows())
            return fail("a constraint is armed (mellow_generate_constraint) with n_rows = %d: this call has %d rows (B, B * n, B * Q, B * k, or both rows of every guided pair)",
                        r.con.n_rows, r.rows());
    }
    if (r.stop.on) {
        CHK(check_stop_engine(e));
        CHK(check_stop_id(r.stop_id, r.beam && r.ignore_stop));
    }
    return 0;
}

// `n` consecutive decode steps captured from the stream into one exec.  Once the capture has begun it is ALWAYS ended and the
// hipGraph_t ALWAYS destroyed, whatever failed in between; the first error is the one reported.
static int capture_steps(mellow_engine* e, int B, const RecordArgs* rec, int n, hipGraphExec_t* exec) {
    hipGraph_t gr = nullptr;
    HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int k = 0; k < n && !rc; ++k) rc = enqueue_decode_layers(e, B, rec);
    hipError_t err = hipStreamEndCapture(e->stream, &gr);
    if (!rc && err != hipSuccess) rc = fail("hipStreamEndCapture failed: %s", hipGetErrorString(err));
    if (!rc && (err = hipGraphInstantiate(exec, gr, nullptr, nullptr, 0)) != hipSuccess) { *exec = nullptr; rc = fail("instantiating the captured decode step failed: %s", hipGetErrorString(err)); }
    if (gr) (void)hipGraphDestroy(gr);
    return rc;
}

// Wait (without touching the stream) until the arg-max kernel has published ticket >= want; *nseen = rows stopped so far.
static int wait_ticket(mellow_engine* e, unsigned want, unsigned* nseen) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        const unsigned long long v = __atomic_load_n(e->h_progress, __ATOMIC_ACQUIRE);
        if ((unsigned)(v >> 32) >= want) {
            if (nseen) *nseen = (unsigned)(v & 0xffffffffu);
            return 0;
        }
        if ((spins & 0x3ff) == 0) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) {      // nothing left in flight: the ticket must be there now
                const unsigned long long v2 = __atomic_load_n(e->h_progress, __ATOMIC_ACQUIRE);
                if ((unsigned)(v2 >> 32) >= want) continue;
                return fail("decode progress word stalled at ticket %u (wanted %u) with an idle stream", (unsigned)(v2 >> 32), want);
            }
            if (q != hipErrorNotReady) return fail("stream error while waiting for a decode step: %s", hipGetErrorString(q));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
                return fail("timed out waiting for decode ticket %u", want);
        }
        // spin politely: a pause per poll, and after ~50 us of spinning yield the core between polls (EnginePool runs one
        // such loop per context thread)
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        __asm__ __volatile__("yield");
#endif
        if (spins > 4096) std::this_thread::yield();
    }
}

// The steps a beam call counts: the loop ends after the first step at which every row is finished.  A row is finished after step
// st exactly when its token there is the stop id (a finished row keeps offering it, an unfinished one that takes it finishes).
static int beam_steps(const std::vector<int32_t>& tok, int N, int steps_done, int stop_id, bool ignore_stop) {
    if (ignore_stop) return steps_done;
    for (int st = 0; st < steps_done; ++st) {
        int nfin = 0;
        for (int row = 0; row < N; ++row) nfin += tok[(size_t)st * N + row] == stop_id;
        if (nfin == N) return st + 1;
    }
    return steps_done;
}

// the end of a beam pass: the three tables and cum (after the last counted step) go to the caller; the host backtracks them
static int finish_beam_pass(mellow_engine_t* e, const GenRequest& r, int N, int steps_done, double first_ms) {
    hipStream_t s = e->stream;
    const BeamArgs g = beam_args(e, N, r.beam);
    const size_t tab = (size_t)r.max_len * N;
    std::vector<int32_t> tok(tab);
    HIPCHK(hipMemcpyAsync(tok.data(), g.out_token, tab * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    CHK(check_bad_id(e));
    for (int i = 0; i < 3; ++i) HIPCHK(hipEventElapsedTime(&e->phase_ms[i], e->ev_phase[i], e->ev_phase[i + 1]));
    const int steps = beam_steps(tok, N, steps_done, r.stop_id, r.ignore_stop != 0);
    const size_t used = (size_t)steps * N;
    HIPCHK(hipMemcpyAsync(r.out_parent, g.out_parent, used * sizeof(int32_t), hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(r.out_tokens, g.out_token, used * sizeof(int32_t), hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(r.out_logprob, g.out_lp, used * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(r.out_cum, g.out_cum + (size_t)(steps - 1) * N, (size_t)N * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(hipStreamSynchronize(s));
    if (r.first_token_ms) *r.first_token_ms = (float)first_ms;
    e->last_steps_enqueued = steps_done;
    e->cur_B = 0;
    e->last_compactions = 0;
    if (r.out_steps) *r.out_steps = steps;
    return 0;
}

// one pass: r.examples examples, r.n answer rows or r.q questions each (both 1: every row is encoded and prefilled itself)
static int generate_pass(mellow_engine_t* e, const GenRequest& r) {
    const auto t_entry = std::chrono::steady_clock::now();
    const int examples = r.examples, n = r.n, Q = r.q, max_len = r.max_len, stop_id = r.stop_id;
    const int B = r.rows();           // rows of the pass: pages, decode arena, loop state, records and the step graph are sized by it
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const int T = e->cfg.prefix_len;
    // KV page geometry in buckets of 64 positions, so that nearby max_len values share pages, key split and graphs
    int Tmax = rup(T + max_len, 64);
    if (Tmax > e->cfg.max_positions) Tmax = T + max_len;
    // Q > 1: positions [0, P) of a prefix -- the clips and separators up to the largest multiple of the attention's 32-query tile --
    // are prefilled once per example, positions [P, T) once per row (run_prefill_q)
    const int P = (T - e->cfg.text_len) / 32 * 32, Tt = T - P;
    const size_t tail_rows = (size_t)B * Tt, head_rows = (size_t)examples * P;
    CHK(ensure_lm(e, B, T, Tmax, T + max_len, examples, Q > 1 ? (head_rows > tail_rows ? head_rows : tail_rows) : 0));
    if (Q > 1) CHK(ensure(e, e->lm_xq, tail_rows * 576));
    const int Bp = e->da.rows;
    if (n > 1 || Q > 1) {
        // the prefix K/V of the examples (run_prefill writes, kv_fanout_kernel reads).  Zeroed when (re)allocated: positions
        // [T, Tp) of a page are never written and never read (the prefill attention clamps its key loads to T - 1); a page starts
        // at a multiple of Tp * 64 floats whatever the number of examples, so a larger call finds its tails where they were
        const size_t fl = (size_t)e->cfg.num_layers * examples * 3 * prefix_page_len(T) * 64;
        for (mellow_engine::Buf* b : {&e->kprefix, &e->vprefix})
            if (b->cap < fl) {
                CHK(ensure(e, *b, fl));
                HIPCHK(hipMemsetAsync(b->p, 0, fl * sizeof(float), s));
            }
        // source row of every answer row for launch_dec_load_rows: the last prefix position of its example, or (Q > 1) the last
        // row of its own tail
        CHK(ensure(e, e->nseq_rows, 1024));
        e->h_nseq_rows.assign(1024, 0);      // (a member: alive until the copy has run)
        for (int row = 0; row < B; ++row) e->h_nseq_rows[row] = Q > 1 ? row * Tt + Tt - 1 : (row / n) * T + T - 1;
        HIPCHK(hipMemcpyAsync(e->nseq_rows.p, e->h_nseq_rows.data(), 1024 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    CHK(ensure(e, e->out_tok, (size_t)Bp * max_len));
    if (r.beam) {
        // loop words and tables of the search, and (k > 1) the staging of the reorder; cum = 0 for beam 0 of an example, -inf for
        // the others, nothing finished
        e->beam_max_len = max_len;
        CHK(ensure(e, e->beam_ws, 3 * 1024 + 3 * 1024 * BEAM_MAX_K + (size_t)4 * max_len * B));
        if (r.beam > 1) {
            const size_t fl = (size_t)e->cfg.num_layers * B * 3 * max_len * 64;
            CHK(ensure(e, e->kstage, fl));
            CHK(ensure(e, e->vstage, fl));
        }
        e->h_beam.assign(2048, 0.f);         // (a member: alive until the copy has run; words 1024 .. 2047 are fin = 0)
        for (int row = 0; row < B; ++row) e->h_beam[row] = row % r.beam == 0 ? 0.f : -INFINITY;
        HIPCHK(hipMemcpyAsync(e->beam_ws.p, e->h_beam.data(), 2048 * sizeof(float), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipEventRecord(e->ev_phase[0], s));
    // loop state (the prefill's arg-max already records token 0 and publishes ticket 1)
    __atomic_store_n(e->h_progress, 0ull, __ATOMIC_RELEASE);
    clear_bad_id(e);
    HIPCHK(hipMemsetAsync(e->d_nseen, 0, 3 * sizeof(int32_t), s));       // n_seen, arrive, ticket
    HIPCHK(hipMemsetAsync(e->d_seen, 0, 1024 * sizeof(int32_t), s));
    e->h_params[0] = max_len;
    e->h_params[1] = r.beam && r.ignore_stop ? -1 : stop_id;        // (beam search: no token is the stop id, so nothing ever finishes)
    HIPCHK(hipMemcpyAsync(e->d_params, e->h_params, 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
#ifdef MELLOW_DEVPROBE
    static const bool dev_dead = getenv("MELLOW_DEV_DEAD_BLOCKS") != nullptr;    // developer probe: launch-chain floor of a step
#else
    constexpr bool dev_dead = false;
#endif
    // Per-row-block early exit (reference stop rule, more than one 32-row block): once every row of a block has produced the
    // stop id, the block's workgroups return at once in every later kernel (its rows' texts are already cut there).  Columns a
    // row never reached are -1 in the token record.
    StepMode m;
    m.logits = m.sample = r.on;         // the sampler reads the full logits rows
    m.logprob = r.out_logprob != nullptr && !r.beam;
    m.beam = r.beam;
    if (r.beam) m.logits = true;        // the select reads the full logits rows; every row runs every step: no early exit, no migration
    m.rules = r.rules.on;               // dec_logit_rules_kernel edits the stored rows: the head stores them (apply_step_mode)
    m.guide = r.guide.on;               // dec_guidance_kernel combines the stored rows of a pair: the head stores them (apply_step_mode)
    m.top = r.top.k;                    // dec_top_logprobs_kernel reads the stored rows: the head stores them (apply_step_mode)
    m.filtered = r.filters.on;          // dec_sample_kernel in its filtered instantiation; the values travel in d_sparams
    m.constrain = r.con.on;             // dec_constrain_kernel edits the stored rows: the head stores them (apply_step_mode)
    m.stop = r.stop.on;                 // dec_stop_strings_kernel overwrites the stored rows it hits: the head stores them (apply_step_mode)
    m.early_exit = !r.beam && (dev_dead || (!r.ignore_stop && e->da.RB > 1));
    // a guided call runs without migration (a pair's rows stay neighbours in slots 2p, 2p + 1); block exit stays: both rows of a
    // pair get the same token, so they finish at the same step, and a pair never straddles a 32-row block
    m.migrate = m.early_exit && !dev_dead && e->opt.row_migration && !m.guide;   // option "row_migration" = 0: block exit without repacking (developer A/B)
    if (m.logprob) {
        // the head's partial sums and the record; columns that are never computed stay exactly 0.0
        CHK(ensure(e, e->cand_sum, (size_t)Bp * (e->cfg.vocab_size / 32)));
        CHK(ensure(e, e->out_lp, (size_t)Bp * max_len));
        HIPCHK(hipMemsetAsync(e->out_lp.p, 0, (size_t)Bp * max_len * sizeof(float), s));
    }
    if (m.top) {
        // the record: -1 / exactly 0.0 wherever no token is recorded
        const size_t nrec = (size_t)Bp * max_len * m.top;
        CHK(ensure(e, e->top_ids, nrec));
        CHK(ensure(e, e->top_lp, nrec));
        HIPCHK(hipMemsetAsync(e->top_ids.p, 0xff, nrec * sizeof(int32_t), s));
        HIPCHK(hipMemsetAsync(e->top_lp.p, 0, nrec * sizeof(float), s));
    }
    if (m.rules) {
        // the bias buffer exists whether or not this call has a bias: a captured launch holds its address (StepGraphs::Key)
        CHK(ensure(e, e->rules_bias, SAMPLE_MAX_V));
        if (r.beam) CHK(ensure(e, e->rules_hist, (size_t)2 * B * max_len));
    }
    // value block, roots and state of the pass: one buffer of fixed size, so a captured launch finds it where it was (StepGraphs::Key)
    if (m.constrain) CHK(ensure(e, e->con_ws, CON_WORDS + (size_t)3 * CON_STATE_ROWS));
    // block and state of the pass, likewise of fixed size
    if (m.stop) CHK(ensure(e, e->stop_ws, STS_BLOCK_WORDS + (size_t)2 * STS_STATE_ROWS * STS_ROW_WORDS));
    // the pass runs in its mode; the taps' defaults are back on every way out (the taps never sample, record nor exit early)
    struct ModeScope { mellow_engine* e; ~ModeScope() { apply_step_mode(e, StepMode()); } } mode_scope{e};
    apply_step_mode(e, m);
    if (r.on) {
        stage_sampling(e, r.top_p, r.temperature, r.seed, r.row_offset, 0, r.filters);
        HIPCHK(hipMemcpyAsync(e->d_sparams, e->h_sparams, sizeof(e->h_sparams), hipMemcpyHostToDevice, s));
    }
    if (r.rules.on) CHK(stage_rules(e, r.rules, stop_id));
    if (r.guide.on) CHK(stage_guidance(e, r.guide.scale));
    if (r.con.on) {
        // the roots of this pass's rows go to the front of the pass's words; the state needs no clearing (step 0 writes the roots)
        CHK(stage_constraint(e, r.con, stop_id, e->con_ws.p));
        HIPCHK(hipMemcpyAsync(e->con_ws.p + CON_WORDS, e->con_roots.p + r.con_row0, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    if (r.stop.on) {
        // every row starts from the empty text, not hit (step 0 writes that state too: the clearing covers rows that never run it)
        CHK(stage_stop_strings(e, r.stop, stop_id, e->stop_ws.p));
        HIPCHK(hipMemsetAsync(e->stop_ws.p + STS_BLOCK_WORDS, 0, (size_t)2 * STS_STATE_ROWS * STS_ROW_WORDS * sizeof(uint32_t), s));
    }
    if (dev_dead) {
        HIPCHK(hipMemsetAsync(e->d_blk_left, 0, 96 * sizeof(int32_t), s));
    } else if (m.early_exit) {
        if (m.migrate) {
            std::vector<int32_t> ident(1024);
            for (int i = 0; i < 1024; ++i) ident[i] = i < B ? i : -1;
            e->h_ident = ident;       // kept alive until the copy has run
            HIPCHK(hipMemcpyAsync(e->d_row_of_slot, e->h_ident.data(), 1024 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(e->d_ncompact, 0, sizeof(int32_t), s));
        }
        for (int rb = 0; rb < 32; ++rb) {
            const int left = B - 32 * rb;
            e->h_blk[rb] = left <= 0 ? 0 : (left > 32 ? 32 : left);
            e->h_blk[32 + rb] = left > 0 ? 1 : 0;
        }
        HIPCHK(hipMemcpyAsync(e->d_blk_left, e->h_blk, 64 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(e->out_tok.p, 0xff, (size_t)Bp * max_len * sizeof(int32_t), s));
    }
    CHK(clear_page_tails(e, T, e->kv_Tmax));     // everything a key-group load can touch (whole chunks are loaded, then masked)
    if (Q > 1) CHK(encode_pair_to_head_tail(e, r.audio1, r.audio2, r.n_samples, r.input_ids, examples, Q, P, e->lm_x.p, e->lm_xq.p));
    else CHK(encode_pair_to_prefix(e, r.audio1, r.audio2, r.n_samples, r.input_ids, examples, e->lm_x.p));
    HIPCHK(hipEventRecord(e->ev_phase[1], s));
    RecordArgs rec;
    rec.embed_next = true;
    if (Q > 1) CHK(run_prefill_q(e, examples, Q, T, P, &rec));
    else CHK(run_prefill(e, examples, T, &rec, false, n));
    HIPCHK(hipEventRecord(e->ev_phase[2], s));

    // one decode step = 30 x (qkv | attention | o_proj | gate/up | down) + final norm + lm_head + arg-max/record/embed,
    // captured once per (B, page geometry, buffers) and replayed; max_len and the stop id are read from d_params
    const bool graph = e->use_graph && !e->prof_on && max_len > 1;
    const mellow_engine::StepGraphs::Key want = mellow_engine::StepGraphs::Key::of(e, B);
    if (graph && (!e->graphs.one || !(e->graphs.key == want))) {
        e->graphs.reset();
        // eight consecutive steps as ONE graph: the step reads its position from the device word, so a replay of the
        // same kernel sequence IS the next step; one launch per 8 steps removes the host/CP hand-over between graphs
        int rc = capture_steps(e, B, &rec, 1, &e->graphs.one);
        if (!rc) rc = capture_steps(e, B, &rec, 8, &e->graphs.eight);
        if (rc) { e->graphs.reset(); return rc; }      // never a cache that holds one exec of the two
        e->graphs.key = want;
    }
    int steps_done = 1;   // token 0 came from the prefill
    double first_ms = -1.0;
    auto note_first = [&]() {
        if (first_ms < 0) first_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    };
    if (r.ignore_stop) {
        // fixed-length mode: nothing to decide on the host, everything is enqueued at once
        for (int i = 1; i < max_len;) {
            const bool eight = graph && i + 8 <= max_len;
            if (eight) HIPCHK(hipGraphLaunch(e->graphs.eight, s));
            else if (graph) HIPCHK(hipGraphLaunch(e->graphs.one, s));
            else CHK(enqueue_decode_layers(e, B, &rec));
            i += eight ? 8 : 1;
            e->cur_pos += eight ? 8 : 1;
            steps_done = i;
        }
        CHK(wait_ticket(e, 1, nullptr));
        note_first();
    } else {
        // reference stop rule (wrapper.py:247-249): the loop ends after the first step at which every row has produced the
        // stop id at least once.  The arg-max kernel publishes (step ticket, rows stopped) to a host-visible word, so the
        // host follows the rule one step behind the device without synchronising: step i+1 is enqueued while step i runs,
        // and at most ONE step is ever enqueued past the deciding one.
        for (int i = 1; i < max_len; ++i) {
            if (graph) HIPCHK(hipGraphLaunch(e->graphs.one, s));
            else CHK(enqueue_decode_layers(e, B, &rec));
            e->cur_pos += 1;
            steps_done = i + 1;
            unsigned nseen = 0;
            CHK(wait_ticket(e, (unsigned)i, &nseen));      // ticket i = the arg-max of step index i-1 is complete
            note_first();
            if ((int)nseen >= B) break;
        }
        if (first_ms < 0) { CHK(wait_ticket(e, 1, nullptr)); note_first(); }
    }
    HIPCHK(hipEventRecord(e->ev_phase[3], s));
    HIPCHK(hipGetLastError());
    if (r.beam) return finish_beam_pass(e, r, B, steps_done, first_ms);
    // host-side length bookkeeping (reference wrapper.py:247-254) on the engine-owned record
    std::vector<int32_t> toks((size_t)B * max_len);
    HIPCHK(hipMemcpyAsync(r.out_tokens, e->out_tok.p, toks.size() * sizeof(int32_t), hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(toks.data(), e->out_tok.p, toks.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.out_logprob) HIPCHK(hipMemcpyAsync(r.out_logprob, e->out_lp.p, toks.size() * sizeof(float), hipMemcpyDefault, s));
    if (r.top.k) {
        HIPCHK(hipMemcpyAsync(r.top.ids, e->top_ids.p, toks.size() * r.top.k * sizeof(int32_t), hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(r.top.lp, e->top_lp.p, toks.size() * r.top.k * sizeof(float), hipMemcpyDefault, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    CHK(check_bad_id(e));        // a prompt id outside the vocabulary (flagged by prefix_assemble_kernel): the reference raises IndexError
    for (int i = 0; i < 3; ++i) HIPCHK(hipEventElapsedTime(&e->phase_ms[i], e->ev_phase[i], e->ev_phase[i + 1]));
    if (r.first_token_ms) *r.first_token_ms = (float)first_ms;
    int ref_steps = steps_done;
    if (!r.ignore_stop) {
        // the reference stops after the first step at which every row has produced stop_id at least once
        std::vector<char> seen(B, 0);
        int nseen = 0;
        for (int st = 0; st < steps_done; ++st) {
            for (int b = 0; b < B; ++b)
                if (!seen[b] && toks[(size_t)b * max_len + st] == stop_id) { seen[b] = 1; ++nseen; }
            if (nseen == B) { ref_steps = st + 1; break; }
        }
    }
    e->last_steps_enqueued = steps_done;
    e->cur_B = 0;      // the decode state of a generate call (no logits store, early-exit words) is not a base for the step taps:
                       // mellow_lm_decode_step needs a mellow_lm_prefill of its own
    e->last_compactions = 0;
    if (m.migrate) HIPCHK(hipMemcpy(&e->last_compactions, e->d_ncompact, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (r.out_steps) *r.out_steps = ref_steps;
    if (r.out_len)
        for (int b = 0; b < B; ++b) {
            int len = ref_steps;
            for (int st = 0; st < ref_steps; ++st)
                if (toks[(size_t)b * max_len + st] == stop_id) { len = st; break; }
            r.out_len[b] = len;
        }
    return 0;
}

// What mellow_generate_rules / _guidance / _top_logprobs / _filters / _constraint / _stop_strings armed on the context serves ONE mellow_generate* call, whatever its outcome:
// taken into that call's request, cleared on the context
static void take_armed(mellow_engine_t* e, GenRequest& r) {
    if (!e) return;
    r.rules = e->rules_armed; e->rules_armed = LogitRules();
    r.guide = e->guide_armed; e->guide_armed = Guidance();
    r.top = e->top_armed; e->top_armed = TopLogprobs();
    r.filters = e->filters_armed; e->filters_armed = SampleFilters();
    r.con = e->con_armed; e->con_armed = Constraint();
    r.stop = e->stop_armed; e->stop_armed = StopStrings();
}

// The reference's loop (wrapper.py:216-249) takes any number of examples.  One pass of the engine takes up to 1024 rows (32 row
// blocks of loop state), so a larger batch runs as consecutive passes of <= 1024 rows on the same pages: examples are
// independent, the token record of every pass lands at its rows of `out_tokens`, a pass that stopped before the longest one is
// padded with -1 (never computed), and the reference's stop rule -- the loop ends at the first step at which EVERY row has
// produced the stop id -- is the maximum over the passes (a row's own length never depends on other rows).
static int generate(mellow_engine_t* e, const GenRequest& req, int door = 0) {
    GenRequest r = req;
    take_armed(e, r);
    CHK(check_request(e, r, door));
    if (r.rows() <= kPassRows) return generate_pass(e, r);      // (always so for n > 1 and, through mellow_generate_q, for Q > 1: check_request)
    const int B = r.examples, max_len = r.max_len;
    int steps_all = 0, enq_all = 0, rep_all = 0;
    float ph[3] = {0.f, 0.f, 0.f};
    std::vector<int> pass_steps;
    for (int r0 = 0; r0 < B; r0 += kPassRows) {
        int st = 0;
        float ftm = 0.f;
        CHK(generate_pass(e, r.pass(r0, B - r0 < kPassRows ? B - r0 : kPassRows, e->cfg.text_len, &st, &ftm)));
        if (r0 == 0 && r.first_token_ms) *r.first_token_ms = ftm;      // the first answers of the call: entry -> first token of the first pass
        pass_steps.push_back(st);
        steps_all = st > steps_all ? st : steps_all;
        enq_all = e->last_steps_enqueued > enq_all ? e->last_steps_enqueued : enq_all;
        rep_all += e->last_compactions;
        for (int i = 0; i < 3; ++i) ph[i] += e->phase_ms[i];
    }
    // `bytes` of every row of a [rows][pitch] record set to `byte`, host or device memory
    auto fill_rows = [](void* dst, size_t pitch, int byte, size_t bytes, int rows) -> int {
        hipPointerAttribute_t at;
        const bool on_device = hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeDevice;
        if (!on_device) (void)hipGetLastError();            // a plain host pointer is not an error here
        if (on_device) HIPCHK(hipMemset2D(dst, pitch, byte, bytes, rows));
        else for (int row = 0; row < rows; ++row) memset(static_cast<char*>(dst) + (size_t)row * pitch, byte, bytes);
        return 0;
    };
    // columns a pass never reached (it stopped before the longest pass): -1 in the token record, like the rows of a block that stopped
    // early, and exactly 0.0 in the log-prob record where the token record now says "never computed"; the top record follows them
    for (size_t p = 0; p < pass_steps.size(); ++p) {
        const int r0 = (int)p * kPassRows, nb = B - r0 < kPassRows ? B - r0 : kPassRows;
        if (pass_steps[p] >= steps_all) continue;
        const size_t o = (size_t)r0 * max_len + pass_steps[p], pitch = (size_t)max_len * 4, w = (size_t)(steps_all - pass_steps[p]) * 4;
        CHK(fill_rows(r.out_tokens + o, pitch, 0xff, w, nb));
        if (r.out_logprob) CHK(fill_rows(r.out_logprob + o, pitch, 0, w, nb));
        if (r.top.k) {
            CHK(fill_rows(r.top.ids + o * r.top.k, pitch * r.top.k, 0xff, w * r.top.k, nb));
            CHK(fill_rows(r.top.lp + o * r.top.k, pitch * r.top.k, 0, w * r.top.k, nb));
        }
    }
    e->last_steps_enqueued = enq_all;
    e->last_compactions = rep_all;
    for (int i = 0; i < 3; ++i) e->phase_ms[i] = ph[i];
    if (r.out_steps) *r.out_steps = steps_all;
    return 0;
}

extern "C" {

int mellow_generate(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                    const int32_t* input_ids, int B, int max_len, float top_p, float temperature, int stop_id,
                    int ignore_stop, int32_t* out_tokens, int32_t* out_len, int32_t* out_steps, float* first_token_ms) {
    // greedy: the reference's top-p/temperature path never changes the arg-max (wrapper.py:219-232)
    return generate(e, {audio1, audio2, n_samples, input_ids, B, 1, 1, max_len, stop_id, ignore_stop, false, top_p, temperature, 0, 0,
                        out_tokens, nullptr, out_len, out_steps, first_token_ms});
}

int mellow_generate_sampled(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                            const int32_t* input_ids, int B, int max_len, float top_p, float temperature, uint64_t seed,
                            int32_t row_offset, int stop_id, int ignore_stop, int32_t* out_tokens, int32_t* out_len,
                            int32_t* out_steps, float* first_token_ms) {
    return generate(e, {audio1, audio2, n_samples, input_ids, B, 1, 1, max_len, stop_id, ignore_stop, true, top_p, temperature, seed, row_offset,
                        out_tokens, nullptr, out_len, out_steps, first_token_ms});
}

// mellow_generate (do_sample = 0) or mellow_generate_sampled (do_sample != 0) plus the log-prob record: the same launches with the
// head, the arg-max and the sampler in their LSE instantiations (dec_tail.hip, sample.hip); tokens, lengths and steps are bit-identical
int mellow_generate_scored(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                           int B, int max_len, int do_sample, float top_p, float temperature, uint64_t seed, int32_t row_offset,
                           int stop_id, int ignore_stop, int32_t* out_tokens, float* out_logprob, int32_t* out_len, int32_t* out_steps,
                           float* first_token_ms) {
    return generate(e, {audio1, audio2, n_samples, input_ids, B, 1, 1, max_len, stop_id, ignore_stop, do_sample != 0, top_p, temperature, seed, row_offset,
                        out_tokens, out_logprob, out_len, out_steps, first_token_ms}, DOOR_SCORED);
}

// n sampled answers per example from ONE encode and ONE prefill per example (include/mellow_hip.h states the semantics).  The step
// graph is shared with a plain call of the same B * n rows on purpose: the key holds the row count, the page geometry and every
// address a captured launch reads, and from the first decode step on the two calls run the same launches on the same buffers --
// everything that differs (prefix buffer, fan-out, row table) happens before the loop and is never captured.
int mellow_generate_n(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                      int B, int n, int max_len, int do_sample, float top_p, float temperature, uint64_t seed, int32_t row_offset,
                      int stop_id, int ignore_stop, int32_t* out_tokens, float* out_logprob, int32_t* out_len, int32_t* out_steps,
                      float* first_token_ms) {
    return generate(e, {audio1, audio2, n_samples, input_ids, B, n, 1, max_len, stop_id, ignore_stop, do_sample != 0, top_p, temperature, seed, row_offset,
                        out_tokens, out_logprob, out_len, out_steps, first_token_ms}, DOOR_N);
}

// Q questions per example from ONE encode and ONE prefill of the clips' positions per example (include/mellow_hip.h states the
// semantics; run_prefill_q the pass).  Like mellow_generate_n it shares the step graph of a plain call of the same B * Q rows.
// Q = 1 is that plain call: the request below is then the one mellow_generate / _sampled / _scored build.
int mellow_generate_q(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                      int B, int Q, int max_len, int do_sample, float top_p, float temperature, uint64_t seed, int32_t row_offset,
                      int stop_id, int ignore_stop, int32_t* out_tokens, float* out_logprob, int32_t* out_len, int32_t* out_steps,
                      float* first_token_ms) {
    return generate(e, {audio1, audio2, n_samples, input_ids, B, 1, Q, max_len, stop_id, ignore_stop, do_sample != 0, top_p, temperature, seed, row_offset,
                        out_tokens, out_logprob, out_len, out_steps, first_token_ms}, DOOR_Q);
}

// k beams per example from ONE encode and ONE prefill per example (include/mellow_hip.h states the semantics; beam.hip the kernels).
// The step graph is one of its own: the mode is part of the key (the select replaces the arg-max, the reorder follows the head).
int mellow_generate_beam(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                         int B, int k, int max_len, int stop_id, int ignore_stop, int32_t* out_parent, int32_t* out_token,
                         float* out_lp, float* out_cum, int32_t* out_steps, float* first_token_ms) {
    GenRequest r{audio1, audio2, n_samples, input_ids, B, k, 1, max_len, stop_id, ignore_stop, false, 1.f, 1.f, 0, 0,
                 out_token, out_lp, nullptr, out_steps, first_token_ms};
    r.beam = k; r.out_parent = out_parent; r.out_cum = out_cum;
    if (k < 1) {      // (before the n >= 1 rule words it as n; what was armed is taken and dropped with the call)
        take_armed(e, r);
        return fail("mellow_generate_beam takes 1 to %d beams per example (got k = %d)", BEAM_MAX_K, k);
    }
    return generate(e, r, DOOR_BEAM | DOOR_SCORED);
}

int mellow_generate_rules(mellow_engine_t* e, const mellow_logit_rules_t* rules) {
    if (rules) CHK(check_rules(rules));
    if (!e || !e->finalized) return fail("engine not finalized");
    e->rules_armed = LogitRules();
    if (!rules) return 0;
    LogitRules a;
    CHK(load_rules(e, rules, &a));
    e->rules_armed = a;
    return 0;
}

int mellow_generate_constraint(mellow_engine_t* e, const mellow_constraint_t* c) {
    std::vector<int32_t> arena, roots;
    if (c) CHK(check_constraint(c, &arena, &roots));
    if (!e || !e->finalized) return fail("engine not finalized");
    e->con_armed = Constraint();
    if (!c) return 0;
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the constraint kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure(e, e->con_trie, arena.size()));
    CHK(ensure(e, e->con_roots, roots.size()));
    HIPCHK(hipMemcpyAsync(e->con_trie.p, arena.data(), arena.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->con_roots.p, roots.data(), roots.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));         // the host copies are free again on return
    e->con_armed.on = true; e->con_armed.then_free = c->then_free != 0;
    e->con_armed.n_nodes = c->n_nodes; e->con_armed.n_edges = c->n_edges; e->con_armed.n_rows = c->n_rows;
    return 0;
}

// the constraint launch on caller data, on copies of its own: what is armed on the context stays
int mellow_constraint_apply(mellow_engine_t* e, const mellow_constraint_t* c, float* logits, int B, const int32_t* history, int ld,
                            const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum, int32_t* out_state) {
    std::vector<int32_t> arena, roots;
    if (c) CHK(check_constraint(c, &arena, &roots));
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!c || !logits || !hist_len || !cand_val || !cand_idx || B <= 0 || ld < 0 || (ld > 0 && !history)) return fail("bad argument");
    if (c->n_rows != B) return fail("mellow_constraint_apply: the constraint has n_rows = %d for B = %d rows", (int)c->n_rows, B);
    if (ld > RULES_MAX_HIST) return fail("mellow_constraint_apply takes histories of at most %d tokens (ld = %d)", RULES_MAX_HIST, ld);
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the constraint kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure(e, e->con_tap, CON_WORDS + (size_t)B + arena.size()));
    Constraint a;
    a.on = true; a.then_free = c->then_free != 0; a.n_nodes = c->n_nodes; a.n_edges = c->n_edges; a.n_rows = B;
    CHK(stage_constraint(e, a, stop_id, e->con_tap.p));
    int32_t* ws = reinterpret_cast<int32_t*>(e->con_tap.p);
    HIPCHK(hipMemcpyAsync(ws + CON_WORDS, roots.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(ws + CON_WORDS + B, arena.data(), arena.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    ConstrainArgs g;
    g.logits = logits; g.ld = e->cfg.vocab_size; g.prm = reinterpret_cast<const uint32_t*>(ws); g.row_root = ws + CON_WORDS; g.trie = ws + CON_WORDS + B;
    g.cand_val = cand_val; g.cand_idx = cand_idx; g.cand_sum = cand_sum;
    g.hist = history; g.hist_ld = ld; g.hist_len = hist_len; g.out_state = out_state;
    launch_dec_constrain(g, B, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// The vocabulary's byte table, checked whole in host code and copied into the engine's shared holder (engine_internal.h VocabBytes).
int mellow_set_vocab_bytes(mellow_engine_t* e, const int32_t* tok_off, const uint8_t* tok_bytes, int32_t n_tokens) {
    if (!tok_off || !tok_bytes) return fail("mellow_set_vocab_bytes: null array");
    if (n_tokens != SAMPLE_MAX_V) return fail("mellow_set_vocab_bytes: n_tokens = %d, the table holds the %d tokens of the vocabulary", (int)n_tokens, SAMPLE_MAX_V);
    if (tok_off[0] != 0) return fail("mellow_set_vocab_bytes: tok_off must start at 0 (got %d)", (int)tok_off[0]);
    for (int t = 0; t < n_tokens; ++t) {
        const int64_t m = (int64_t)tok_off[t + 1] - tok_off[t];
        if (m < 0) return fail("mellow_set_vocab_bytes: tok_off decreases at token %d", t);
        if (m > STS_MAX_TOKEN_BYTES) return fail("mellow_set_vocab_bytes: token %d has %lld bytes, a token has at most %d", t, (long long)m, STS_MAX_TOKEN_BYTES);
    }
    if (!e || !e->finalized) return fail("engine not finalized");
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the stop-strings kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    VocabBytes& vb = *e->w.vocab_bytes;
    if (!vb.off) HIPCHK(hipMalloc(&vb.off, ((size_t)SAMPLE_MAX_V + 1) * sizeof(int32_t)));
    if (!vb.bytes) HIPCHK(hipMalloc(&vb.bytes, (size_t)SAMPLE_MAX_V * STS_MAX_TOKEN_BYTES));
    HIPCHK(hipMemcpyAsync(vb.off, tok_off, ((size_t)n_tokens + 1) * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    if (tok_off[n_tokens] > 0) HIPCHK(hipMemcpyAsync(vb.bytes, tok_bytes, (size_t)tok_off[n_tokens], hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));         // the caller's arrays are free again on return, and every context's stream finds the table
    vb.set = true;
    return 0;
}

int mellow_generate_stop_strings(mellow_engine_t* e, const mellow_stop_strings_t* strings) {
    StopStrings st;
    if (strings) CHK(check_stop_strings(strings, &st));
    if (!e || !e->finalized) return fail("engine not finalized");
    e->stop_armed = StopStrings();
    if (!strings) return 0;
    CHK(check_stop_engine(e));
    e->stop_armed = st;
    return 0;
}

// the stop-strings launch on caller data, on a block of its own: what is armed on the context stays
int mellow_stop_strings_apply(mellow_engine_t* e, const mellow_stop_strings_t* strings, float* logits, int B, const int32_t* history, int ld,
                              const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum, int32_t* out_hit) {
    StopStrings st;
    if (strings) CHK(check_stop_strings(strings, &st));
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!strings || !logits || !hist_len || !cand_val || !cand_idx || B <= 0 || ld < 0 || (ld > 0 && !history)) return fail("bad argument");
    if (ld > RULES_MAX_HIST) return fail("mellow_stop_strings_apply takes histories of at most %d tokens (ld = %d)", RULES_MAX_HIST, ld);
    CHK(check_stop_engine(e));
    CHK(check_stop_id(stop_id, false));
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure(e, e->stop_tap, STS_BLOCK_WORDS));
    CHK(stage_stop_strings(e, st, stop_id, e->stop_tap.p));
    StopStrArgs g;
    g.logits = logits; g.ld = e->cfg.vocab_size; g.blk = reinterpret_cast<const uint32_t*>(e->stop_tap.p);
    g.tok_off = e->w.vocab_bytes->off; g.tok_bytes = e->w.vocab_bytes->bytes;
    g.cand_val = cand_val; g.cand_idx = cand_idx; g.cand_sum = cand_sum;
    g.hist = history; g.hist_ld = ld; g.hist_len = hist_len; g.out_hit = out_hit;
    launch_dec_stop_strings(g, B, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_generate_guidance(mellow_engine_t* e, float scale) {
    if (!std::isfinite(scale)) return fail("guidance scale must be finite (got %g); 1 is off", (double)scale);
    if (!e || !e->finalized) return fail("engine not finalized");
    e->guide_armed = Guidance();
    if (scale == 1.f) return 0;          // the conditional distribution itself: nothing to arm
    e->guide_armed.on = true; e->guide_armed.scale = scale;
    return 0;
}

int mellow_guidance_apply(mellow_engine_t* e, float scale, float* logits, int P, float* cand_val, int32_t* cand_idx, float* cand_sum) {
    if (!std::isfinite(scale)) return fail("guidance scale must be finite (got %g)", (double)scale);
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!logits || !cand_val || !cand_idx || P <= 0) return fail("bad argument");
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the guidance kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    CHK(stage_guidance(e, scale));
    GuideArgs g;
    g.logits = logits; g.ld = e->cfg.vocab_size; g.prm = e->d_gparams;
    g.cand_val = cand_val; g.cand_idx = cand_idx; g.cand_sum = cand_sum;
    launch_dec_guidance(g, P, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_generate_top_logprobs(mellow_engine_t* e, int k, int32_t* out_ids, float* out_lp) {
    if (k < 0 || k > TOP_LOGPROBS_MAX_K) return fail("top log-probs: k must be 0 (off) to %d (got %d)", TOP_LOGPROBS_MAX_K, k);
    if (k > 0 && (!out_ids || !out_lp)) return fail("top log-probs: null record buffer");
    if (!e || !e->finalized) return fail("engine not finalized");
    e->top_armed = TopLogprobs();
    if (k == 0) return 0;
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the top log-probs kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    e->top_armed.k = k; e->top_armed.ids = out_ids; e->top_armed.lp = out_lp;
    return 0;
}

int mellow_generate_filters(mellow_engine_t* e, const mellow_sample_filters_t* f) {
    if (f) CHK(check_filters(f));
    if (!e || !e->finalized) return fail("engine not finalized");
    e->filters_armed = SampleFilters();
    if (!f || (f->top_k == 0 && f->min_p == 0.f)) return 0;        // neutral values: nothing to arm
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the sampler is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    e->filters_armed.on = true; e->filters_armed.top_k = f->top_k; e->filters_armed.min_p = f->min_p;
    return 0;
}

int mellow_top_logprobs_apply(mellow_engine_t* e, const float* logits, const float* cand_val, const float* cand_sum, int B, int k,
                              int32_t* out_ids, float* out_lp) {
    if (k < 0 || k > TOP_LOGPROBS_MAX_K) return fail("top log-probs: k must be 1 to %d (got %d)", TOP_LOGPROBS_MAX_K, k);
    if (k > 0 && (!out_ids || !out_lp)) return fail("top log-probs: null record buffer");
    if (!e || !e->finalized) return fail("engine not finalized");
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the top log-probs kernel is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    if (!logits || !cand_val || !cand_sum || B <= 0 || k < 1) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    TopArgs g;
    g.logits = logits; g.ld = e->cfg.vocab_size; g.cand_val = cand_val; g.cand_sum = cand_sum; g.k = k;
    g.out_ids = out_ids; g.out_lp = out_lp;
    launch_dec_top_logprobs(g, B, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_logit_rules_apply(mellow_engine_t* e, const mellow_logit_rules_t* rules, float* logits, int B, const int32_t* history, int ld,
                             const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum) {
    if (rules) CHK(check_rules(rules));
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!rules || !logits || !hist_len || !cand_val || !cand_idx || B <= 0 || ld < 0 || (ld > 0 && !history)) return fail("bad argument");
    if (ld > RULES_MAX_HIST) return fail("mellow_logit_rules_apply takes histories of at most %d tokens (ld = %d)", RULES_MAX_HIST, ld);
    e->rules_armed = LogitRules();          // the tap uses the context's bias buffer: rules armed before it are gone
    LogitRules a;
    CHK(load_rules(e, rules, &a));
    CHK(stage_rules(e, a, stop_id));
    RulesArgs g;
    g.logits = logits; g.ld = e->cfg.vocab_size; g.prm = e->d_rparams; g.bias = e->rules_bias.p;
    g.cand_val = cand_val; g.cand_idx = cand_idx; g.cand_sum = cand_sum;
    g.hist = history; g.hist_ld = ld; g.hist_len = hist_len;
    launch_dec_logit_rules(g, B, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_beam_select(mellow_engine_t* e, const float* logits, const float* cum, const int32_t* fin, int B, int k, int stop_id,
                       int32_t* out_parent, int32_t* out_token, float* out_cum, float* out_lp) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!logits || !cum || !fin || !out_parent || !out_token || !out_cum || !out_lp || B <= 0) return fail("bad argument");
    if (k < 1 || k > BEAM_MAX_K) return fail("mellow_beam_select takes 1 to %d beams per example (got k = %d)", BEAM_MAX_K, k);
    if ((int64_t)B * k > kPassRows) return fail("mellow_beam_select takes at most 1024 rows per call: B * k = %d * %d", B, k);
    if (e->cfg.vocab_size != SAMPLE_MAX_V) return fail("the beam select is built for a vocabulary of %d (engine: %d)", SAMPLE_MAX_V, e->cfg.vocab_size);
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure(e, e->beam_ws, 3 * 1024 + 3 * 1024 * BEAM_MAX_K));
    BeamArgs g = beam_args(e, B * k, k);       // (the survivor words only: the outputs are the caller's)
    g.logits = logits; g.cum_in = cum; g.fin_in = fin; g.cum_state = nullptr; g.fin_state = nullptr; g.stop_id = stop_id;
    g.out_parent = out_parent; g.out_token = out_token; g.out_cum = out_cum; g.out_lp = out_lp;
    launch_beam_select(g, B, DecArgs(), nullptr, nullptr, nullptr, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int mellow_sample_logits(mellow_engine_t* e, const float* logits, int B, const int32_t* row_ids, int step, float top_p,
                         float temperature, uint64_t seed, int32_t* tokens) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!logits || !tokens || B <= 0) return fail("bad argument");
    CHK(check_sampling(e, top_p, temperature));
    HIPCHK(hipSetDevice(e->device));
    stage_sampling(e, top_p, temperature, seed, 0, step);
    HIPCHK(hipMemcpyAsync(e->d_sparams, e->h_sparams, sizeof(e->h_sparams), hipMemcpyHostToDevice, e->stream));
    SampleArgs sa;
    sa.logits = logits; sa.ld = e->cfg.vocab_size; sa.prm = e->d_sparams; sa.row_ids = row_ids;
    launch_sample_logits(sa, B, tokens, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// the tap of the filtered instantiation: always that instantiation, also for neutral values; what is armed on the context stays
int mellow_sample_logits_filtered(mellow_engine_t* e, const float* logits, int B, const int32_t* row_ids, int step, float top_p,
                                  float temperature, uint64_t seed, const mellow_sample_filters_t* f, int32_t* tokens) {
    if (f) CHK(check_filters(f));
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!f || !logits || !tokens || B <= 0) return fail("bad argument");
    CHK(check_sampling(e, top_p, temperature));
    HIPCHK(hipSetDevice(e->device));
    SampleFilters sf;
    sf.on = true; sf.top_k = f->top_k; sf.min_p = f->min_p;
    stage_sampling(e, top_p, temperature, seed, 0, step, sf);
    HIPCHK(hipMemcpyAsync(e->d_sparams, e->h_sparams, sizeof(e->h_sparams), hipMemcpyHostToDevice, e->stream));
    SampleArgs sa;
    sa.logits = logits; sa.ld = e->cfg.vocab_size; sa.prm = e->d_sparams; sa.row_ids = row_ids; sa.filtered = true;
    launch_sample_logits(sa, B, tokens, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
