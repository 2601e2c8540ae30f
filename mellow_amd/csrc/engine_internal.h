// Internal header of the host side of libmellow_hip.so (engine*.cpp): the engine object, its weights, and the helpers the
// translation units share.  Not part of the C ABI (include/mellow_hip.h is).
//   engine.cpp          errors, allocation helpers, create / destroy / fork / load_tensor, precision, profiler read-out
//   engine_weights.cpp  mellow_engine_finalize: every reference checkpoint key -> device layouts (P / PB / P16 / e4m3, composed decode weights)
//   engine_encoder.cpp  the dense GEMM dispatch (run_gemm), front-end + HTSAT encoder (A1-A13; swin_block), the taps mellow_logmel / mellow_encode / mellow_resample
//   engine_lm.cpp       KV pages, LM prefill (A15; plan, parts, prefill_layer), the decode step and its per-call mode, mellow_prefix / lm taps, scoring
//   engine_generate.cpp the generation loop on top of it (A16): request + checks, passes, step graphs, the mellow_generate* entry points,
//                       beam search (mellow_generate_beam, mellow_beam_select)
//   engine_dev.cpp      developer entry points (GEMM timing, the two GEMM accuracy / timing taps, profiler dump, kernel stamps)
//   engine_taps.cpp     the launch taps on caller data (mellow_debug_*_attn, _gemm_epi, _norm, _dec_attn, _dec_gemv, _dec_tail): one call record
// The engine object (below): `Options` + `Weights` are what a fork shares, each copied by one assignment; everything else is one
// context's own -- stream, events, workspaces (`Buf` frees itself), KV pages, loop words, the decode-graph cache (`StepGraphs`).
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <unordered_map>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mellow_hip.h"
#include "kernels.h"

using namespace mellow;

int fail(const char* fmt, ...);
struct mellow_engine;
int apply_options(mellow_engine* e);            // engine.cpp: option table + precision mode -> the engine's resolved fields
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define CHK(expr)            \
    do {                     \
        int _r = (expr);     \
        if (_r) return _r;   \
    } while (0)

// ---- model constants (reference mellow/model/config.py:1-10, htsat.py:599-606) ---------------------------
static const int kDepths[4] = {2, 2, 6, 2};
static const int kHeads[4] = {4, 8, 16, 32};
static const int kWin = 8;
static const int kHop = 320, kNfft = 1024, kNfreq = 513, kMel = 64;
static const int kClasses = 527, kEncOut = 768, kProj = 576;
static const int kLongCrop = 689, kLongHop = 344;
static const char* ENC = "audio_encoder.base.htsat.";
static const char* C2L = "audio_encoder.base.c2l.";
static const char* PRJ = "audio_encoder.projection.";
static const char* LMK = "caption_decoder.lm.";

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// ---- profiler families --------------------------------------------------------------------------------------
// PF_LM_HEAD: the all-position LM head (row gather + final norm + head GEMM), storing (mellow_lm_forward_logits) or fused with the
// log-softmax statistics and their merge (mellow_score / mellow_lm_score); the generation path never runs it
enum { PF_GEMM = 0, PF_SKINNY, PF_PREFILL_ATTN, PF_DECODE_ATTN, PF_WINDOW_ATTN, PF_NORM, PF_MISC, PF_LM_HEAD, PF_COUNT };
static const char* kFamilyNames[PF_COUNT] = {"gemm_f32_mfma", "skinny_gemm_m32", "prefill_attention",
                                             "decode_attention", "window_attention", "norm", "misc", "lm_head_all_positions"};

struct HostTensor {
    std::vector<char> data;
    std::vector<int64_t> shape;
    int dtype = 0;
    int64_t numel() const {
        int64_t n = 1;
        for (auto d : shape) n *= d;
        return n;
    }
    const float* f() const { return reinterpret_cast<const float*>(data.data()); }
};

struct Packed {  // a P-layout weight
    float* p = nullptr;
    int N = 0, K = 0, NP = 0, KP = 0;
    int Nw = 0;  // logical packed rows (pairs: 64*ceil(N/32))
};

struct SwinBlockW {
    float *n1w, *n1b, *n2w, *n2b;
    Packed qkv, proj, fc1, fc2;
    float *qkv_b, *proj_b, *fc1_b, *fc2_b;
    float* bias_exp;  // [nH][64][64]
    float* mask;      // [nW][64][64] or null
};
struct MergeW {
    float *nw, *nb;
    Packed red;
};
// one decode GEMM operand as the launchers take it: the e4m3 copy with its row scales when the layer holds one, else fp32
struct DecW {
    const float *p, *scale;            // scale == nullptr: fp32 weights
};
struct LMLayerW {
    Packed qkv, o, gateup, down;       // prefill (plain weights, P-layout); `down` is also the decode operand
    Packed qkv_f, gateup_f;            // decode: RMSNorm weight folded into the columns (W'[n][k] = W[n][k]*ln[k])
    float* o16 = nullptr;              // decode: P16 layout (16-row tiles) for the complete-output o_proj
    float* gu16n = nullptr;            // decode, f32x3 layer kernels: the same tiles in P16N order (eight consecutive k per lane)
    float* gu16 = nullptr;             // decode: folded gate/up, P16 layout, tile = 8 gate rows + the 8 matching up rows
    // decode, layers >= 1: [W'_l | W'_l Wd_{l-1}] (960 x (576 + 1536), P-layout, the product formed in fp64 at load time): the
    // operand of dec_qkv2_kernel, which runs the down projection of layer l-1 and the q/k/v projection of layer l as one launch
    float* qkv2 = nullptr;
    float *q2h8 = nullptr, *q2h_sc = nullptr;    // fp8 mode: the composed part W'_l . Wd_{l-1} alone, e4m3 + one scale per packed row
    // fp8 mode: e4m3 copies of the four decode operands in the same slot order (one 4-byte word per float4 slot) and one
    // scale per packed weight row (launch_pack_dec_fp8)
    float *qkv8 = nullptr, *qkv_sc = nullptr, *o8 = nullptr, *o_sc = nullptr, *gu8 = nullptr, *gu_sc = nullptr, *dn8 = nullptr,
          *dn_sc = nullptr;
    float *in_ln, *post_ln;
    DecW qkv_w() const { return qkv8 ? DecW{qkv8, qkv_sc} : DecW{qkv_f.p, nullptr}; }
    DecW o_w() const { return o8 ? DecW{o8, o_sc} : DecW{o16, nullptr}; }
    DecW gateup_w() const { return gu8 ? DecW{gu8, gu_sc} : DecW{gu16, nullptr}; }
    DecW down_w() const { return dn8 ? DecW{dn8, dn_sc} : DecW{down.p, nullptr}; }
};

struct ProfRec {
    int fam;
    hipEvent_t a, b;
    double flops, bytes;
    int M = 0, N = 0, K = 0, epi = 0;     // GEMM launches only (developer shape report)
};

// What one call decides about the decode step.  The default is what the taps run: logits stored, arg-max, no record, every block live.
// apply_step_mode (engine_lm.cpp) is the only writer of the engine's copy and of the DecArgs fields that follow from it.
struct StepMode {
    bool logits = true;          // the head stores its logits rows (the taps read them, and so does the sampler)
    bool sample = false;         // dec_sample_kernel draws the token instead of the arg-max
    bool logprob = false;        // head / arg-max / sampler in their LSE forms, log-probs recorded next to the tokens
    bool early_exit = false;     // per-row-block early exit (DecArgs::blk_live)
    bool migrate = false;        // ... with row migration (DecArgs::row_of_slot)
    int beam = 0;                // k >= 1: beam search -- the select (beam.hip) in place of the arg-max, and for k > 1 the two K/V reorder launches after it
    bool rules = false;          // repetition controls: dec_logit_rules_kernel between the head and the picker (forces `logits` on)
    bool guide = false;          // contrastive guidance: dec_guidance_kernel after the head, before the rules launch (forces `logits` on; rows 2p, 2p + 1 are a pair)
    bool filtered = false;       // top_k / min_p: dec_sample_kernel in its filtered instantiation (needs `sample`)
    int top = 0;                 // k >= 1: dec_top_logprobs_kernel after the rules launch, before the picker (forces `logits` on; needs `logprob`)
    bool constrain = false;      // constrained decoding: dec_constrain_kernel after the rules launch, before the top log-probs and the picker (forces `logits` on)
    bool stop = false;           // stop strings: dec_stop_strings_kernel after the constraint launch, before the top log-probs and the picker (forces `logits` on)
};
// The top log-probs record of one generation call (include/mellow_hip.h, mellow_generate_top_logprobs): armed on the context, taken
// into the call's GenRequest at entry.  ids / lp are the caller's [rows][max_len][k], host or device.
struct TopLogprobs {
    int k = 0;
    int32_t* ids = nullptr;
    float* lp = nullptr;
};
// The candidate filters of one sampled generation call (include/mellow_hip.h, mellow_generate_filters): armed on the context, taken
// into the call's GenRequest at entry.
struct SampleFilters {
    bool on = false;
    int top_k = 0;
    float min_p = 0.f;
};
// The guidance of one generation call (include/mellow_hip.h, mellow_generate_guidance): armed on the context, taken into the call's
// GenRequest at entry.
struct Guidance {
    bool on = false;
    float scale = 1.f;
};
// The repetition controls of one generation call (include/mellow_hip.h, mellow_generate_rules): armed on the context, taken into the
// call's GenRequest at entry.  The bias itself lives in the context's rules_bias buffer.
struct LogitRules {
    bool on = false;
    float theta = 1.f;
    int ngram = 0, min_new = 0;
    bool bias = false;
};

// The constraint of one generation call (include/mellow_hip.h, mellow_generate_constraint): armed on the context, taken into the
// call's GenRequest at entry.  The trie and the roots of all rows live in the context's con_trie / con_roots buffers.
struct Constraint {
    bool on = false;
    bool then_free = false;
    int n_nodes = 0, n_edges = 0, n_rows = 0;
};

// The stop strings of one generation call (include/mellow_hip.h, mellow_generate_stop_strings): armed on the context, taken into the
// call's GenRequest at entry.  Small and of fixed size, so the strings themselves travel with the record.
struct StopStrings {
    bool on = false;
    int n = 0;
    int32_t off[STS_MAX_STRINGS + 1] = {0};
    uint8_t bytes[STS_MAX_STRINGS * STS_MAX_STR_LEN] = {0};
};
// The vocabulary's byte table (mellow_set_vocab_bytes): one holder per engine, shared by its forks as the weights are, so that a
// table set on any context is seen by all.  The buffers have their full size from the first call on -- tok_off [49152 + 1], tok_bytes
// [49152 * 256] -- so a captured launch finds them where they were when the table is replaced.
struct VocabBytes {
    int32_t* off = nullptr;
    uint8_t* bytes = nullptr;
    bool set = false;
    VocabBytes() = default; VocabBytes(const VocabBytes&) = delete; VocabBytes& operator=(const VocabBytes&) = delete;
    ~VocabBytes() { if (off) (void)hipFree(off); if (bytes) (void)hipFree(bytes); }
};

// One execution context.  `opt` and `w` are what a fork shares with its parent (copied whole by mellow_engine_fork); the rest is its own.
#define LOCAL __attribute__((visibility("hidden")))      // (the handle type is declared inside the public header's visibility pragma)
struct mellow_engine {
    // A grow-only device workspace (ensure(), engine.cpp).  It owns its memory and frees itself, so it moves and is never copied.
    struct Buf {
        float* p = nullptr;
        size_t cap = 0;
        Buf() = default; Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
        Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
        Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
        LOCAL ~Buf() { if (p) (void)hipFree(p); }
    };
    // The configuration AS CONFIGURED: the caller's option table, the mode and what apply_options() (the only writer) resolves from
    // them; read-only after finalize.  (use_graph and prefill_parts below are seeded there too but change per context: live state.)
    struct LOCAL Options {
        // explicit configuration (mellow_engine_set_option): key -> value as given by the caller.  The library reads NO environment
        // variable; apply_options() turns this table + the mode into the fields below, mellow_engine_describe() reports them
        std::map<std::string, std::string> given;
        int mode = MELLOW_PRECISION_F32X3;
        bool x3_stft = true, stft_fft = true, x3_apb = true, x3_attn = true, x3w = true, row_migration = true, decode_fuse = true;
        int arena_mb = 3400;
        bool kv16 = false;           // fp8 mode default; option "fp8_kv16" = 0 keeps the decode step on the fp32 pages
        // fp8 GEMM mode (BASELINE config 5): every packed weight with KP % 64 == 0 also gets a P8 copy + per-row scales,
        // looked up by the fp32 packed pointer when a GEMM is issued; activations are quantised per row right before the GEMM
        bool fp8 = false;
        bool fp8_decode = false;                     // fp8 mode: the decode kernels read e4m3 weights too (option "fp8_decode")
        bool fp8_decode_act = false;                 // ... and quantise their activations: fp8 matrix pipe (option "fp8_decode_act")
        bool fp8_attn_bf16 = true;                   // fp8 mode: prefill attention on operands rounded once to bf16 (option "fp8_attn_bf16" = 0: the exact 3-way split)
        bool fp8_prefill = true;                     // fp8 mode: e4m3 GEMMs in encoder + prefill (option "fp8_prefill" = 0: a test isolating the decode weights)
        int dec_x3_min_rb = 2;                       // the fewest 32-row blocks at which the layer GEMM launches take their f32x3 forms (option "decode_x3_min_rb")
        int dec_x3 = 0;                              // f32x3 mode: DEC_X3_* mask of the decode GEMM launches on the bf16 pipe (option "decode_x3", developer A/B)
        int f32x3_terms = 0;                         // 0 = off; 6 = fp32 GEMMs on the bf16 pipe by exact 3-way operand splitting (six partial products)
        // f32x3 LM prefill without RMSNorm launches: the o_proj / down GEMMs write their output pre-split + its sum of squares,
        // the q/k/v and gate/up GEMMs run on norm-folded weights and scale their accumulators by the row statistic (run_prefill).
        // option "prefill_fuse_norm" = 0: the two-launch form (developer A/B).
        bool prefill_fuse_norm = true;
        int enc_apb_stages = 0x1CC;                  // f32x3 mode: Swin stages (bit st) whose LayerNorms / fc1 hand their output over pre-split (APB) to x3q GEMMs
        int sk_max = 8;                              // f32x3 encoder: largest split count of the split-K launches (option "splitk"; < 2 = never split)
        int dec_fuse_max_rb = 1;                     // decode: largest number of 32-row blocks that runs the fused down + q/k/v launch (fp32 weights)
    };
    struct Fp8W { uint8_t* w8; float* scale; };
    // Every weight pointer and packed-weight record: memory of the engine that finalized them (allocs / arena), read-only afterwards; a fork copies the POINTERS
    struct LOCAL Weights {
        // encoder weights
        Packed dft, mel;
        // f32x3 mode: the STFT as a real FFT when the checkpoint's conv weights are window[n] * cos / sin(2 pi k n / 1024) (checked
        // element by element at load time); fft_win == nullptr: the DFT GEMM on the checkpoint's weights
        float *fft_win = nullptr, *fft_tw1 = nullptr, *fft_tw2 = nullptr;
        float *bn_alpha = nullptr, *bn_beta = nullptr;
        float *pe_w = nullptr, *pe_b = nullptr, *pe_nw = nullptr, *pe_nb = nullptr;
        std::vector<SwinBlockW> blocks[4];
        MergeW merge[3];
        int32_t* win_map[4][2] = {{nullptr}};     // [stage][shifted]
        float *fn_w = nullptr, *fn_b = nullptr;
        Packed tscam, c2l, lin1, lin2;
        float *tscam_b = nullptr, *c2l_b = nullptr, *pln_w = nullptr, *pln_b = nullptr;
        int32_t* emb_row_map = nullptr;           // {1..32}
        // LM
        float* embed = nullptr;                   // row-major [V][H]
        Packed lm_head;
        std::vector<LMLayerW> layers;
        float* final_norm = nullptr;
        float *rope_cos = nullptr, *rope_sin = nullptr;
        float *head8 = nullptr, *head_sc = nullptr;  // e4m3 lm_head for the decode step
        DecW head_w() const { return head8 ? DecW{head8, head_sc} : DecW{lm_head.p, nullptr}; }
        std::unordered_map<const float*, void*> bf_w;   // fp32 packed pointer -> PB copy
        std::unordered_map<const float*, Fp8W> fp8_w;
        std::shared_ptr<VocabBytes> vocab_bytes;     // created by finalize; a fork shares the holder, so what any context sets all see
    };
    // The captured decode step and what it was captured with: the graphs bake buffer addresses in (max_len / stop id travel in
    // d_params, the sampling parameters in d_sparams).  generate_pass (engine_generate.cpp) captures, ensure_lm invalidates.
    struct LOCAL StepGraphs {
        struct Key {
            std::array<uintptr_t, 29> v{};       // all zero: no capture (a pass has at least one row)
            static Key of(const mellow_engine* e, int B);      // from the engine as configured for the pass (below the engine)
            bool operator==(const Key& k) const { return v == k.v; }
        };
        hipGraphExec_t one = nullptr, eight = nullptr;      // eight: the same step 8 times in a row (the step is position-independent)
        Key key;
        StepGraphs() = default; StepGraphs(const StepGraphs&) = delete; StepGraphs& operator=(const StepGraphs&) = delete;
        void reset() {                              // the only place an exec is destroyed
            for (hipGraphExec_t* x : {&one, &eight}) if (*x) { (void)hipGraphExecDestroy(*x); *x = nullptr; }
        }
        ~StepGraphs() { reset(); }
    };

    mellow_config_t cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    Options opt;
    Weights w;
    bool use_graph = true;                      // live: option "graph", then mellow_set_graph
    int prefill_parts = 2;                      // live: parts of the split LM prefill (option "prefill_split"; ensure_prefill_streams / forks lower it)
    bool streams_probed = false;                // a probe found fewer overlapping streams than asked for (ensure_prefill_streams): re-probed after 16 calls
    int probe_backoff = 0, prefill_parts_ok = 1, prefill_parts_want = 2;
    hipStream_t stream2[3] = {nullptr, nullptr, nullptr};      // further streams of the split LM prefill (run_prefill)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    bool finalized = false;
    bool owns_weights = true;                 // false for a context made by mellow_engine_fork: weight memory belongs to its parent
    std::map<std::string, HostTensor> host;   // until finalize
    std::vector<void*> allocs;                // everything hipMalloc'd for weights
    char* arena = nullptr;                    // one big allocation the weights are carved from
    size_t arena_size = 0, arena_used = 0;
    bool decode_only_weight = false;          // set while packing weights only the decode kernels read: no bf16x3 / fp8 copy

    // workspaces (grow-only; released with the engine)
    Buf wavcat, wpad, power, logmel, X0, X1, T, QKV, H, ats, fpx, fpxavg, latv, emb33, e1, gbuf, sbuf, proj33;
    Buf lm_x, lm_xn, lm_q, lm_o, lm_h, kcache, vcache;
    Buf kcache16, vcache16;      // fp8 mode: bf16 shadow of the pages for the decode step (half the floats of kcache / vcache)
    bool kv16_direct = false;    // ... and the prefill writes them itself (q/k/v epilogue) and reads them (bf16-once attention): no fp32 pages, no conversion pass
    Buf lm_xn3, lm_o3, lm_h3;                  // f32x3 mode: the GEMM inputs of LM prefill, pre-split by their producers (APB order)
    Buf lm_ssq;                                // ... and the per-row sum-of-squares partials of the residual stream (norm-free chaining)
    Buf dec;                                   // one arena for the decode-step buffers (DecArgs)
    Buf dlogits, cand;
    // scoring (mellow_score / mellow_lm_score): the B prefixes of a call [B][prefix_len][hidden], the fused head's per-(64-column
    // group, row) partials (three words per entry), and the small per-row words (targets, target logits, candidate lengths)
    Buf sc_prefix, sc_part, sc_ws;
    Buf sk_ws;                                 // split-K workspace of the f32x3 GEMMs (512 partial tiles of 128 x 128 fp32);
    bool sk_enable = false;                    // ... only launches of the encoder chain (one stream) may use it: run_encoder switches it on
    Buf enc_a3, enc_h3;                        // f32x3 / fp8 encoder: the two pre-split operands (LayerNorm output; GELU(fc1) output)
    Buf a8, a8_scale;                          // quantised A operand of the GEMM in flight (bytes / floats, carved from float buffers)
    DecArgs da;
    int32_t *d_tokens = nullptr, *d_step = nullptr, *d_pos = nullptr, *d_seen = nullptr, *d_nseen = nullptr;
    int32_t *d_arrive = nullptr, *d_ticket = nullptr, *d_params = nullptr;   // loop bookkeeping words (LoopArgs)
    int32_t *d_blk_left = nullptr, *d_blk_live = nullptr;                    // per-row-block early exit (32 blocks max)
    int32_t *d_row_of_slot = nullptr, *d_ncompact = nullptr;                 // row migration (kernels.h, DecArgs::row_of_slot)
    int last_compactions = 0;
    unsigned long long* h_progress = nullptr;  // mapped host word the arg-max kernel publishes (ticket << 32 | rows stopped) to
    unsigned long long* d_progress = nullptr;  // its device alias
    std::map<std::pair<int, int>, float*> resample_banks;   // (orig, new) gcd-reduced -> device polyphase bank [klen][new]; a fork starts from its parent's
    int32_t h_params[2] = {0, 0};              // staging of d_params {max_len, stop id}
    uint32_t* d_sparams = nullptr;             // sampling parameter block (kernels.h SMP_*): graph replays serve any seed / top_p / T
    uint32_t h_sparams[SMP_WORDS] = {0};       // ... its staging
    uint32_t* d_rparams = nullptr;             // rule parameter block (kernels.h RUL_*): graph replays serve any penalty / n-gram size / minimum / bias on-off
    uint32_t h_rparams[RUL_WORDS] = {0};       // ... its staging
    uint32_t* d_gparams = nullptr;             // guidance parameter block (kernels.h GDN_*): graph replays serve any scale
    uint32_t h_gparams[GDN_WORDS] = {0};       // ... its staging
    SampleFilters filters_armed;               // mellow_generate_filters: what the NEXT mellow_generate* call on this context takes (and clears)
    TopLogprobs top_armed;                     // mellow_generate_top_logprobs: what the NEXT mellow_generate* call on this context takes (and clears)
    Guidance guide_armed;                      // mellow_generate_guidance: what the NEXT mellow_generate* call on this context takes (and clears)
    LogitRules rules_armed;                    // mellow_generate_rules: what the NEXT mellow_generate* call on this context takes (and clears)
    // repetition controls, created on first use: the call's dense logit bias [vocab] (a copy: no caller pointer is ever captured),
    // and the ping-pong history of a beam call [2][rows][max_len] int32 (logit_rules.hip)
    Buf rules_bias, rules_hist;
    Constraint con_armed;                      // mellow_generate_constraint: what the NEXT mellow_generate* call on this context takes (and clears)
    // constrained decoding, created on first use (copies: no caller pointer is ever captured): the armed trie arena (kernels.h
    // ConstrainArgs::trie) and the roots of all rows of the call; the words of a pass, of fixed size so that their address never
    // changes -- value block [CON_WORDS] | roots of the pass's rows [1024] | state ping-pong [2][1024]; the tap's own copies --
    // value block | roots | arena -- so that mellow_constraint_apply leaves what is armed as it is
    Buf con_trie, con_roots, con_ws, con_tap;
    uint32_t h_cparams[CON_WORDS] = {0};       // staging of the value block (kernels.h CON_*)
    StopStrings stop_armed;                    // mellow_generate_stop_strings: what the NEXT mellow_generate* call on this context takes (and clears)
    // stop strings, created on first use and of fixed size so that their address never changes: the words of a pass -- value block
    // and string bytes [STS_BLOCK_WORDS] | state ping-pong [2][1024][STS_ROW_WORDS]; the tap's own block, so that
    // mellow_stop_strings_apply leaves what is armed as it is
    Buf stop_ws, stop_tap;
    uint32_t h_stopblk[STS_BLOCK_WORDS] = {0}; // staging of the block (kernels.h STS_*)
    StepMode mode;                             // what apply_step_mode last set (run_lm_head, loop_args and StepGraphs::Key::of read it)
    int32_t h_blk[64] = {0};                   // staging of d_blk_left[32] | d_blk_live[32]
    std::vector<int32_t> h_ident;              // staging of d_row_of_slot
    int last_steps_enqueued = 0;               // decode steps (incl. the prefill's token) the last generate call enqueued
    Buf out_tok;                               // engine-owned token record [rows][max_len] (stable address: graph-safe)
    // mellow_generate_scored, created on first use: the head's per-tile sums of exponentials [rows][vocab / 32] (DecArgs::cand_sum) and
    // the log-prob record [rows][max_len] (LoopArgs::out_logprob)
    Buf cand_sum, out_lp;
    // mellow_generate_top_logprobs, created on first use: the record of a pass, ids int32 and log-probs f32, [rows][max_len][k] each
    Buf top_ids, top_lp;
    // mellow_generate_n (n answers per example from one prefill), created on first use: the prefix K/V of the call's examples
    // [layer][examples][3][Tp][64] -- the prefill writes them here, kv_fanout_kernel copies them to the pages of every answer row
    // (source and destination never alias) -- and the source-row table of launch_dec_load_rows with its host staging
    Buf kprefix, vprefix, nseq_rows;
    // mellow_generate_beam, created on first use: the loop words of the search (cum [1024] | fin [1024] | survivors per row [1024] |
    // survivor values, tokens, increments [1024][8] each | tables parent, token, lp, cum [max_len][rows] each), its host staging, and
    // the K/V staging of the reorder [layer][rows][3][max_len][64] per tensor (k > 1)
    Buf beam_ws, kstage, vstage;
    int beam_max_len = 0;                     // max_len the tables of beam_ws are laid out for
    std::vector<float> h_beam;
    Buf lm_xq;                                // mellow_generate_q: the LM input of the tail prefill, [rows][prefix_len - P][hidden] (run_prefill_q)
    std::vector<int32_t> h_nseq_rows;
    int kv_B = 0, kv_Tmax = 0;                // current page geometry
    int cur_B = 0, cur_pos = 0;               // host mirror of the decode state
    int32_t h_pos_word = 0;                   // staging for the device position word
    StepGraphs graphs;

    // taps
    bool taps_on = false;
    std::map<std::string, Buf> taps;
    std::map<std::string, int64_t> tap_numel;

    uint64_t dbg_spans[960] = {};
    int dbg_seq0 = -1;                           // developer stamps (mellow_dev_kdebug): first launch index of a decode step, -1 = off
    mellow_engine* parent = nullptr;             // a fork: the context whose weights it shares
    int n_forks = 0, prefill_parts_saved = 2;    // a parent: live forks; its own split setting, restored when the last fork goes

    // profiling
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t ev_phase[4] = {nullptr, nullptr, nullptr, nullptr};
    float phase_ms[3] = {0, 0, 0};
};

#undef LOCAL
// Everything a captured step bakes in that differs between calls, and which launch bakes it in.  A new StepMode field that changes
// a captured launch or one of its arguments belongs here.
inline mellow_engine::StepGraphs::Key mellow_engine::StepGraphs::Key::of(const mellow_engine* e, int B) {
    return Key{{(uintptr_t)B,                      // rows: every launch's grid and its live-row count
                (uintptr_t)e->kv_Tmax,             // page stride: dec_attn, and with it the arena and page addresses (ensure_lm)
                (uintptr_t)e->mode.sample,         // dec_sample_kernel or the arg-max; the head with or without its logits store
                (uintptr_t)e->out_tok.p,           // token record: LoopArgs of the arg-max / sampler (and of dec_compact)
                (uintptr_t)e->da.blk_live,         // early exit: the DecArgs of every launch
                (uintptr_t)e->da.row_of_slot,      // row table: the DecArgs of every launch, and whether dec_compact is in the step
                (uintptr_t)e->mode.logprob,        // LSE forms of the head and of the arg-max / sampler
                (uintptr_t)e->da.cand_sum,         // partial sums: DecArgs of the head and of the arg-max / sampler
                (uintptr_t)(e->mode.logprob ? e->out_lp.p : nullptr),        // log-prob record: LoopArgs of the arg-max / sampler
                (uintptr_t)e->mode.beam,           // beam search: the select in place of the arg-max, the reorder launches (k > 1)
                (uintptr_t)(e->mode.beam ? e->beam_ws.p : nullptr),          // ... its loop words and tables: BeamArgs, the reorder's parent table
                (uintptr_t)(e->mode.beam ? e->beam_max_len : 0),             // ... the table offsets inside beam_ws
                (uintptr_t)(e->mode.beam > 1 ? e->kstage.p : nullptr),       // ... the staging buffers of the reorder
                (uintptr_t)(e->mode.beam > 1 ? e->vstage.p : nullptr),
                (uintptr_t)e->mode.rules,          // repetition controls: dec_logit_rules_kernel in the step; the head with its logits store
                (uintptr_t)(e->mode.rules ? e->rules_bias.p : nullptr),                     // ... the bias buffer: RulesArgs
                (uintptr_t)(e->mode.rules && e->mode.beam ? e->rules_hist.p : nullptr),     // ... the beam rows' history buffer: RulesArgs
                (uintptr_t)e->mode.guide,          // contrastive guidance: dec_guidance_kernel in the step; the head with its logits store; the sampler's stream by pair
                (uintptr_t)e->mode.top,            // top log-probs: dec_top_logprobs_kernel in the step and its k (a launch argument); the head with its logits store
                (uintptr_t)(e->mode.top ? e->top_ids.p : nullptr),           // ... its record: TopArgs
                (uintptr_t)(e->mode.top ? e->top_lp.p : nullptr),
                (uintptr_t)e->mode.filtered,       // top_k / min_p: dec_sample_kernel's filtered instantiation (the values are in the SMP_* block)
                (uintptr_t)e->mode.constrain,      // constrained decoding: dec_constrain_kernel in the step; the head with its logits store
                (uintptr_t)(e->mode.constrain ? e->con_trie.p : nullptr),      // ... the trie arena: ConstrainArgs (its contents and counts are not baked in)
                (uintptr_t)(e->mode.constrain ? e->con_ws.p : nullptr),        // ... value block, roots and state of the pass: ConstrainArgs
                (uintptr_t)e->mode.stop,           // stop strings: dec_stop_strings_kernel in the step; the head with its logits store
                (uintptr_t)(e->mode.stop ? e->stop_ws.p : nullptr),            // ... block and state of the pass: StopStrArgs (the strings are not baked in)
                (uintptr_t)(e->mode.stop && e->w.vocab_bytes ? e->w.vocab_bytes->off : nullptr),      // ... the vocabulary's byte table: StopStrArgs
                (uintptr_t)(e->mode.stop && e->w.vocab_bytes ? e->w.vocab_bytes->bytes : nullptr)}};
}
static_assert(!std::is_copy_constructible<mellow_engine::Buf>::value, "a Buf owns its device memory: it moves, it is never copied");
static_assert(std::is_copy_assignable<mellow_engine::Weights>::value && std::is_copy_assignable<mellow_engine::Options>::value, "a fork copies these by assignment: no owning member (Buf, StepGraphs) belongs in them");

// ---- helpers shared by the translation units (engine.cpp unless noted) ------------------------------------------------------
int ensure(mellow_engine* e, mellow_engine::Buf& b, size_t floats);
int dev_alloc(mellow_engine* e, float** out, size_t floats);
int upload(mellow_engine* e, float** out, const float* src, size_t floats, size_t alloc_floats = 0);
// engine_weights.cpp: two packing steps of the decode weights that the loader and the tap mellow_debug_dec_gemv share.
// il [2 I][H]: 16-row tile t = gate[8t .. 8t + 7] then up[8t .. 8t + 7] (the source of launch_pack_weight16 / 16n)
void interleave_gate_up8(const float* g, const float* u, int I, int H, std::vector<float>& il);
// device: cat [960][2112] = [F (960 x 576) | Q (960 x 1536)] row-major, then its P-layout [1024][2112] into out; enqueues only
int pack_qkv2_cat(mellow_engine* e, const float* dF, const float* dQ, float* dCat, float* out);
hipEvent_t next_event(mellow_engine* e);
int tap(mellow_engine* e, const char* name, const float* src, int64_t n);
std::vector<std::string> build_required(const mellow_config_t* cfg);
const std::vector<std::string>& default_required();
bool is_ignored_key(const std::string& k);
void window_map_host(int R, int shift, int32_t* out);
void pack_weight_host(const float* w, int N, int K, int NP, int KP, float* out);
void rope_tables_host(float theta, int head_dim, int P, float* c, float* s);
int alloc_state_words(mellow_engine* e);
// `chain`: the stream the scope's launches go on (null: e->stream).  Records are read in enqueue order: profiling forces ONE chain.
struct ProfScope {
    mellow_engine* e;
    ProfRec r;
    bool on;
    hipStream_t chain;
    ProfScope(mellow_engine* e_, int fam, double flops, double bytes, hipStream_t chain_ = nullptr) : e(e_), on(e_->prof_on), chain(chain_ ? chain_ : e_->stream) {
        if (on) {
            r.fam = fam;
            r.flops = flops;
            r.bytes = bytes;
            r.a = next_event(e);
            r.b = next_event(e);
            hipEventRecord(r.a, chain);
        }
    }
    ~ProfScope() {
        if (on) {
            hipEventRecord(r.b, chain);
            e->prof.push_back(r);
        }
    }
};
// Forks the side streams stream2[0 .. n) off e->stream when it is made (`status`: what that returned); run() joins them back, and so
// does the destructor if nothing has yet.  Once a side stream waits on ev_fork, EVERY exit of the forking function has to join -- an
// early error return would leave side-stream launches running against buffers the caller's next call reuses or frees from e->stream.
struct StreamFork {
    mellow_engine* e; int n; bool joined; int status;
    StreamFork(mellow_engine* e_, int n_) : e(e_), n(n_), joined(n_ <= 0), status(fork()) {}
    StreamFork(const StreamFork&) = delete;
    int fork() {
        if (n > 0) HIPCHK(hipEventRecord(e->ev_fork, e->stream));
        for (int i = 0; i < n; ++i) HIPCHK(hipStreamWaitEvent(e->stream2[i], e->ev_fork, 0));
        return 0;
    }
    int run() {
        if (joined) return 0;
        joined = true;
        for (int i = 0; i < n; ++i) {
            HIPCHK(hipEventRecord(e->ev_join[i], e->stream2[i]));
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[i], 0));
        }
        return 0;
    }
    ~StreamFork() { (void)run(); }
};
// engine_encoder.cpp
// What a producer leaves for the GEMM that follows it: fp32 rows, or an image of K-long rows in the GEMM's operand format
// and LDS order -- APB (three bf16 pieces, f32x3 mode; common.h) when scales is null, else AMX (MXFP8, fp8 mode) + its scale bytes.
// `rows` beside an image: what the GEMM's A and the producer's fp32 output are given (null where the fp32 form does not exist).
struct HandOver { float* rows = nullptr; char *image = nullptr, *scales = nullptr; int K = 0; };
// the image of M rows x K at `base`: whole 128-row panels, and an AMX image's scale bytes live behind its data
static inline HandOver image_region(void* base, int M, int K, bool amx, float* rows = nullptr) {
    char* p = static_cast<char*>(base);
    return HandOver{rows, p, amx ? p + (size_t)rup(M, 128) * rup(K, 64) : nullptr, K};
}
// g writes its output (also) as the image `out`: the epilogue's C3 fields
static inline void hand_over_to(GemmArgs& g, const HandOver& out) {
    g.C3 = out.image;
    if (out.scales) { g.c3_fmt = 1; g.C3s = reinterpret_cast<uint8_t*>(out.scales); g.c3_kt64 = rup(out.K, 64) / 64; }
}
// One dense GEMM on `chain`, one profile record there.  `in` picks the kernel: an image the LDS-DMA kernel of its format, anything
// else -- `{}` where no producer handed g.A over -- what the mode gives fp32 rows (main chain only).
int run_gemm(mellow_engine* e, hipStream_t chain, const GemmArgs& g, const HandOver& in);
GemmArgs lin(const float* A, int64_t lda, int M, const Packed& w, float* C, int64_t ldc, const float* bias);
int run_encoder(mellow_engine* e, const float* wav, int n, int64_t n_samples, int want_logmel_only, int apply_bn, float* logmel_out);
// engine_lm.cpp
static inline int rb_of(int B) { return (B + 31) / 32; }
static inline size_t kv_layer_floats(const mellow_engine* e) { return (size_t)e->kv_B * 3 * e->kv_Tmax * 64; }
// loop bookkeeping fused into the arg-max kernel (reference wrapper.py:232-249): only mellow_generate records
struct RecordArgs {
    bool embed_next = false;
};
// B rows of pages and decode arena; the prefill workspaces hold prefill_B examples (0 = B: every row is prefilled itself)
// (prefill_rows > 0: their row count itself, for a prefill that is not prefill_B x T rows)
int ensure_lm(mellow_engine* e, int B, int T, int Tmax, int ctx_end = 0, int prefill_B = 0, size_t prefill_rows = 0);
int dec_attn_split_groups(int ctx_end, int ts, bool kv16);      // DecArgs::gs of a context that ends at ctx_end
static inline int prefix_page_len(int T) { return rup(T, 64); }      // positions per page of kprefix / vprefix (rounded as the pages are)
int clear_page_tails(mellow_engine* e, int T, int t_end);
LoopArgs loop_args(mellow_engine* e);
// sets e->mode and the DecArgs fields logits, cand_sum, blk_live, blk_snap, row_of_slot from it (cand_sum must be allocated for logprob)
void apply_step_mode(mellow_engine* e, const StepMode& m);
int run_lm_head(mellow_engine* e, int B, int pending_kcd, const RecordArgs* rec);
// the words of beam_ws (engine_internal.h, the member's comment) as the select takes them, tables laid out for e->beam_max_len
BeamArgs beam_args(mellow_engine* e, int N, int k);
// the rules launch of a generation step on B rows, from the engine as apply_step_mode configured it (engine_lm.cpp)
RulesArgs rules_args(mellow_engine* e, int B);
// the constraint launch of a generation step on B rows, likewise
ConstrainArgs constrain_args(mellow_engine* e, int B);
// the stop-strings launch of a generation step on B rows, likewise
StopStrArgs stop_str_args(mellow_engine* e, int B);
// the guidance launch of a generation step, from the engine as apply_step_mode configured it (engine_lm.cpp)
GuideArgs guide_args(mellow_engine* e);
// the top log-probs launch of a generation step, from the engine as apply_step_mode configured it (engine_lm.cpp)
TopArgs top_args(mellow_engine* e);
// n > 1 (mellow_generate_n; fp32 pages only): the layers run on the B examples and write K/V to kprefix / vprefix; the fan-out and
// everything from the last prefix row on (last layer, head, first token) run on B * n rows
int run_prefill(mellow_engine* e, int B, int T, const RecordArgs* rec, bool all_positions = false, int n = 1);
// One run of the LM layers: positions [pos0, pos0 + rows) of every sequence.  run_prefill is one span over the whole prefix;
// run_prefill_q is two, with the fan-out between them.
struct PrefillSpan {
    int rows;            // positions per sequence the run computes; q, attention output and MLP buffers hold this many rows each
    int pos0;            // their first position: 0, or a multiple of 32 with the K/V of [0, pos0) already in the pages
    float* x;            // [sequences][rows][hidden]: the layer-0 input, updated in place to the input of the last layer that ran whole
    bool to_prefix;      // K/V go to kprefix / vprefix (one page per example, stride prefix_page_len) instead of the decode pages
    bool all_layers;     // the last layer runs whole too (x = the final hidden states); else it stops after its q/k/v GEMM
};
// mellow_generate_q, Q > 1 (fp32 pages only): head [0, P) on the B examples (input lm_x), fan-out, tail [P, T) on the B * Q rows
// (input lm_xq), then everything from the last prefix row on as run_prefill does it for B * Q rows
int run_prefill_q(mellow_engine* e, int B, int Q, int T, int P, const RecordArgs* rec);
int enqueue_decode_layer_range(mellow_engine* e, int B, int l_begin, int l_end, bool inc_pos);
int enqueue_decode_layers(mellow_engine* e, int B, const RecordArgs* rec);
int ensure_prefill_streams(mellow_engine* e);      // creates + probes the split prefill's side streams; may lower e->prefill_parts to 1
int encode_pair_to_prefix(mellow_engine* e, const float* a1, const float* a2, int64_t n_samples, const int32_t* ids, int B, float* prefix_out);
// ids [B][Q][text_len]: head_out [B][P][hidden] and tail_out [B * Q][prefix_len - P][hidden] (kernels.h, launch_prefix_assemble_q)
int encode_pair_to_head_tail(mellow_engine* e, const float* a1, const float* a2, int64_t n_samples, const int32_t* ids, int B, int Q,
                             int P, float* head_out, float* tail_out);
// final norm + fused log-softmax head (EPI_LSE + merge) on rows from_pos .. from_pos + n - 1 of the hidden states in lm_x [B][T]
int run_score_head(mellow_engine* e, int B, int T, int from_pos, int n, const int32_t* targets, float* out_logprob,
                   int32_t* out_argmax, float* out_lse, float* out_max);
void clear_bad_id(mellow_engine* e);
int check_bad_id(mellow_engine* e);
