/*
 * mellow_hip.h — C ABI of libmellow_hip.so, the MI355X (gfx950) engine behind MellowWrapper.generate().
 *
 * This is the drop-in boundary for the reference's inference hot path.  The reference has no native
 * interface (it is pure Python on PyTorch ATen); the seams this library replaces are the Python calls
 * listed per function below (file:line in soham97/mellow).  Nothing in these signatures is a torch
 * type: plain pointers, sizes and scalars, so the same library binds from ctypes (what
 * mellow_amd/engine.py does), cffi, pybind11 or cgo.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; mellow_last_error() then returns a
 *     thread-local message.  The Python wrapper re-raises the reference's exception types
 *     (ValueError / AssertionError / RuntimeError) from it.
 *   - "dev" pointers are HIP device pointers on the engine's device (caller-owned; a torch tensor's
 *     data_ptr() is fine).  "host" pointers are ordinary host memory.
 *   - all tensors are dense, row-major, fp32 unless marked int32.
 *   - calls on one engine are serialised by the caller (the reference is single-threaded, blocking:
 *     wrapper.py:212 `torch.no_grad()`, no re-entrancy).  Work is issued on the engine's private HIP
 *     stream; every data-path call returns after that stream has drained unless stated otherwise.
 *   - the engine owns weights, KV pages and workspaces; the caller owns inputs and outputs.
 */
#ifndef MELLOW_HIP_H
#define MELLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared between these two pragmas are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* 2: out_tokens may hold -1 (never-computed steps), first_token_ms is host wall-clock time, a decode step needs a prefill of
 *    its own after mellow_generate / mellow_lm_forward_logits, the optional "mellow.rope_cos/sin" tensors, new symbols */
#define MELLOW_ABI_VERSION 2
/* Minor revisions (same struct layouts and symbol meanings: a version-2 caller keeps working; mellow_abi_minor() reports it):
 *  1: the DEFAULT numeric mode of mellow_engine_create is MELLOW_PRECISION_F32X3 (round 4).  A caller that never calls
 *     mellow_engine_set_precision gets fp32-accurate GEMMs whose LAST BITS depend on how many examples share the call
 *     (split-K for small launches; from round 5 the decode step of a batch of more than 32 rows runs other kernels than one of
 *     up to 32 rows; from round 6 its attention merges one key split instead of two from two row blocks on): greedy tokens are
 *     asserted equal across those forms on the reference's fixtures, logits agree to 1e-3.  A caller that needs
 *     batch-size-independent GEMMs selects MELLOW_PRECISION_F32: encoder and prefill are then bit-identical whatever the batch;
 *     the decode step still picks wave counts per launch by the number of 32-row blocks (another fp32 summation order: <= 5e-4
 *     on the logits, same arg-max: tests/test_gpu_parity.py test_exact_fp32_mode_across_batch_sizes).
 *  2: mellow_prefill_parts (round 5).
 *  3: mellow_engine_set_option / mellow_engine_describe (round 6): the library no longer reads ANY environment variable; every
 *     switch it has is a named option, and the resolved configuration can be printed.  mellow_debug_gemm_f32 modes 6 / 9 are gone
 *     (the pre-split debug kernel was removed; 16 / 17 are the engine's own f32x3 kernels).
 *  4: opt-in seeded nucleus sampling: mellow_generate_sampled and mellow_sample_logits.  mellow_generate is unchanged (greedy).
 *     The scoring symbols mellow_score and mellow_lm_score were added later under this same minor (no existing symbol or struct
 *     changed): a binding that must also load an older minor-4 library detects them by symbol lookup (dlsym), not by the number.
 *     mellow_generate_scored and mellow_debug_dec_head_lse (log-probs of the generated tokens) were added the same way, and so
 *     was mellow_generate_n (n sampled answers per example from one encode and one prefill), and then mellow_generate_q (several
 *     questions per example from one encode and one prefill of the clips' positions), and then mellow_generate_beam with its tap
 *     mellow_beam_select (beam search inside the decode step), and then mellow_generate_rules with its tap mellow_logit_rules_apply
 *     (repetition controls: logit rules inside the decode step), and then mellow_generate_guidance with its tap mellow_guidance_apply
 *     (contrastive guidance inside the decode step), and then mellow_generate_top_logprobs with its tap mellow_top_logprobs_apply
 *     (the k likeliest tokens of every step), and then mellow_generate_filters with its tap mellow_sample_logits_filtered (top_k and
 *     min_p inside the sampler), and then mellow_generate_constraint with its tap mellow_constraint_apply (answers held to a phrase
 *     set inside the decode step), and then mellow_set_vocab_bytes and mellow_generate_stop_strings with its tap
 *     mellow_stop_strings_apply (answers end at a string, matched on bytes inside the decode step) -- added while the minor was 5,
 *     detected by symbol lookup all the same.
 *  5: the attention taps on host data, mellow_debug_prefill_attn and mellow_debug_window_attn.  No existing symbol or struct
 *     changed; a binding that must also load a minor-4 library detects them by symbol lookup.  The GEMM epilogue tap
 *     mellow_debug_gemm_epi was added later under this same minor, detected by symbol lookup all the same, and so was the norm /
 *     hand-over tap mellow_debug_norm, and then the decode attention tap mellow_debug_dec_attn, and then the decode GEMV tap
 *     mellow_debug_dec_gemv, and then the decode step-tail tap mellow_debug_dec_tail. */
#define MELLOW_ABI_MINOR 5

typedef struct mellow_engine mellow_engine_t;

/* Decoder LM hyper-parameters (reference: HF config.json of SmolLM2-135M fetched at decoder.py:25;
 * kept as data in mellow_amd/config/lm_smollm2_135m.yaml) + encoder/prefix constants of v0.yaml. */
typedef struct mellow_config {
    int32_t abi_version;        /* must be MELLOW_ABI_VERSION */
    int32_t vocab_size;         /* 49152 */
    int32_t hidden_size;        /* 576  (must equal encoder d_proj, wrapper.py:62) */
    int32_t intermediate_size;  /* 1536 */
    int32_t num_layers;         /* 30 */
    int32_t num_heads;          /* 9 */
    int32_t num_kv_heads;       /* 3 */
    int32_t head_dim;           /* 64 */
    float   rms_norm_eps;       /* 1e-5 */
    float   rope_theta;         /* 100000 */
    int32_t max_positions;      /* rows of the RoPE table to build (>= 389 + max_len) */
    int32_t text_len;           /* 129 (v0.yaml text_tokenization_len) */
    int32_t prefix_len;         /* 389 (v0.yaml prefix_length) */
    int32_t sep_token_id;       /* 0 (decoder.py:49) */
} mellow_config_t;

enum { MELLOW_F32 = 0, MELLOW_I32 = 1, MELLOW_I64 = 2 };

/* ---- library ------------------------------------------------------------------------------------ */
int         mellow_abi_version(void);
const char* mellow_last_error(void);
/* number of HIP devices visible (0 when there is no GPU; never fails) */
int         mellow_device_count(void);

/* ---- lifetime: replaces MellowWrapper.get_model_and_tokenizer's model construction + load_state_dict
 *      + model.to(cuda) (reference wrapper.py:59-88) ------------------------------------------------ */
int  mellow_engine_create(const mellow_config_t* cfg, int device, mellow_engine_t** out);
void mellow_engine_destroy(mellow_engine_t* e);
/* A second execution context on the same device that SHARES a finalized engine's weights (no copy): its own HIP stream,
 * workspaces, KV pages and captured graphs.  Calls on `parent` and on the fork may overlap from different host threads (a
 * serving front-end pipelines independent batches this way: mellow_amd/serve.py); each handle is still serialised by its
 * caller.  Destroy every fork before its parent.  mellow_engine_fork / the fork's mellow_engine_destroy touch the PARENT (its
 * fork count; while it has forks the parent runs its LM prefill as one chain instead of two half-batches on two streams, and it
 * goes back to the split form when its last fork is destroyed): do not call them while a call is running on the parent.
 * On failure nothing is leaked.  The reference has no counterpart (one synchronous model object). */
int  mellow_engine_fork(mellow_engine_t* parent, mellow_engine_t** out);

/* Hand one checkpoint tensor to the engine under its reference state_dict key, e.g.
 * "audio_encoder.base.htsat.layers.0.blocks.1.attn.qkv.weight".  `data` may be a host or a device
 * pointer; the engine copies / re-tiles it into its own arena before returning.  Keys the inference
 * path never reads are accepted and ignored (returns 0).  Unknown keys fail.
 *
 * Two OPTIONAL tensors that are not checkpoint keys: "mellow.rope_cos" and "mellow.rope_sin", f32 [max_positions][head_dim/2],
 * the rotary tables cos / sin(position * inv_freq).  The reference never stores them: transformers' LlamaRotaryEmbedding
 * recomputes them with torch on every forward, so their last bit is whatever torch's vectorised cos/sin give on the host it
 * runs on.  A binding that wants the engine to use EXACTLY the numbers its own torch would produce computes them the HF way
 *  and loads them here before finalize.  Without them the engine builds the tables itself
 * (mellow_host_rope_tables: fp32 inv_freq and angle as in HF, cos/sin evaluated in double and rounded to fp32 -- within
 * 1 ulp of torch's, tests/test_abi_cpu.py); both paths are parity-tested for 300 decode steps. */
int  mellow_engine_load_tensor(mellow_engine_t* e, const char* key, const void* data,
                               const int64_t* shape, int ndim, int dtype);
/* Verifies that every tensor the hot path reads has been loaded (strict, like load_state_dict at
 * wrapper.py:76) and builds derived tables (expanded relative-position bias, window maps, RoPE). */
int  mellow_engine_finalize(mellow_engine_t* e);
/* number of state_dict keys the engine requires / name of the i-th one (for loader validation) */
int         mellow_engine_num_required(void);
const char* mellow_engine_required_key(int i);

/* ---- the hot path: replaces Mellow.generate_prefix_inference (mellow.py:100-108, called
 *      wrapper.py:285) + MellowWrapper._generate_batch (wrapper.py:197-249) -------------------------
 * audio1/audio2 : dev f32 [B][n_samples]  (what preprocess_audio returns, wrapper.py:170-179)
 * input_ids     : dev i32 [B][text_len]   (preprocess_text's input_ids, wrapper.py:181-195)
 * max_len       : entry_length of the loop (wrapper.py:200)
 * top_p, temperature : accepted for API parity; the reference's filter never removes the arg-max
 *                 (wrapper.py:220-232) so the result is greedy for every value;
 *                 mellow_generate_sampled is the opt-in sampling form
 * stop_id       : tokenizer.encode(stop_token)[0] (wrapper.py:208)
 * ignore_stop   : 0 = reference semantics (loop ends when every row has produced stop_id,
 *                 wrapper.py:247-249); 1 = always run max_len steps (fixed-work benchmark mode)
 * out_tokens    : dev i32 [B][max_len]; columns >= *out_steps are undefined.  In reference-semantics mode with more than
 *                 one 32-row block, a block whose rows have ALL produced stop_id stops being computed (per-block early
 *                 exit): its rows hold -1 in the columns after that step (every such row's text is already cut)
 * out_len       : host i32 [B], tokens before the row's first stop_id (the text cut of wrapper.py:254)
 * out_steps     : host, number of loop iterations the reference would have run
 * first_token_ms: host wall-clock milliseconds from call entry until the first token id of every row exists
 *                 (observed through the device's progress word, without synchronising the stream)
 * In reference-semantics mode the host follows the stop rule one step behind the device through a mapped progress
 * word the arg-max kernel publishes: no stream synchronisation inside the loop, at most one step is enqueued past
 * the deciding one (mellow_last_steps_enqueued reports how many were).
 */
int  mellow_generate(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                     const int32_t* input_ids, int B, int max_len, float top_p, float temperature,
                     int stop_id, int ignore_stop, int32_t* out_tokens, int32_t* out_len,
                     int32_t* out_steps, float* first_token_ms);
/* Opt-in seeded nucleus (top-p) / temperature sampling: mellow_generate with the arg-max of every step (the prefill's token
 * included) replaced by a draw, inside the same captured decode step.  The default call above stays greedy and
 * reference-identical.  For a row with fp32 logits l[0..vocab), global row index r and step t (the column of out_tokens):
 *   1. z_i = l_i / temperature in fp32; temperature must be finite and > 0 (else an error).
 *   2. Nucleus (the reference's rule, wrapper.py:219-226): order the tokens by (z desc, index asc), p = softmax(z); token i is
 *      kept iff the mass of the tokens strictly before it in that order is <= top_p.  The first token is always kept:
 *      top_p <= 0 keeps exactly the arg-max, top_p >= 1 every token; top_p NaN is an error.  Masses are fixed-point
 *      integers (2^-31 of the row maximum's weight) summed exactly, so the boundary depends on no summation order.
 *   3. Draw (Gumbel-max): the token is argmax over kept i of (z_i + g_i), ties to the lowest index, g_i = -log(-log(u_i)),
 *      u_i = (2 * (x >> 9) + 1) * 2^-24 with x = word (i & 3) of Philox4x32-10 at counter (i >> 2, t, r, 0) and key
 *      (lo32(seed), hi32(seed)).
 *   4. A row holding a NaN logit yields its first NaN index (the greedy rule).
 * r = row_offset + the row's index in this call, so a row's stream depends on (seed, r, t) only: not on its batch slot, the
 * 1024-row passes, row migration or the engine context.  Results are bit-deterministic, graph or eager.  The vocabulary must be
 * 49152 (the sampler's one-workgroup-per-row tiling). */
int  mellow_generate_sampled(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                             const int32_t* input_ids, int B, int max_len, float top_p, float temperature, uint64_t seed,
                             int32_t row_offset, int stop_id, int ignore_stop, int32_t* out_tokens, int32_t* out_len,
                             int32_t* out_steps, float* first_token_ms);
/* mellow_generate (do_sample == 0) or mellow_generate_sampled (do_sample != 0: the same validation and errors) that also records the
 * log-probability of every token it records: out_logprob dev f32 [B][max_len], column t belongs to column t of out_tokens.  Tokens,
 * lengths and steps are bit-identical to those calls.  The number is formed inside the decode step -- no second forward, and no
 * logits store in a greedy call: the lm_head reduces every 32-column tile of a row to a partial of its log-sum-exp next to the
 * arg-max candidate it already forms, and the kernel that picks the token merges the partials.
 *
 * Definition.  For the fp32 logits l[0..vocab) that chose token k at a step (the prefill's token included):
 *     logprob = l_k - lse,   lse = M + log S,   M = max l,   S = sum over 32-column tiles t of s_t * exp(m_t - M),
 *     m_t = max of tile t,   s_t = sum over the columns j of tile t of exp(l_j - m_t).
 * It is the model's own log-softmax -- temperature 1, no nucleus -- also in a sampled call, whatever top_p / temperature drew the
 * token: the number mellow_score returns for the same tokens (another kernel and summation order there: equal to rounding, not
 * bit-equal).  A greedy call picks k = arg-max, so l_k = M and it records -log S; a sampled call reads l_k from the logits row the
 * head stored for the sampler and records l_k - lse.  log S is taken in fp64 and rounded once; exp is fp32 expf.
 * Summation orders (all fixed; no float atomics -- results are bit-identical run to run, graph or eager, and do not depend on the
 * row's batch slot, on row migration or on the 1024-row passes):
 *   - within a tile, streaming f32x3 head (the default mode): the two lanes of a pair hold columns 8 q + 4 h + j (h = lane half,
 *     q = 0..3, j = 0..3); each adds its 16 terms in the order q, then j, ascending; s_t = (sum of h = 0) + (sum of h = 1).
 *   - within a tile, fp32 / e4m3 head (MELLOW_PRECISION_F32, MELLOW_PRECISION_FP8, a vocabulary the streaming head does not tile):
 *     eight threads hold columns 4 q .. 4 q + 3 (q = 0..7); each adds its four terms ascending; s_t = the eight sums, ascending q.
 *   - over the tiles of a row: 256 threads, thread i adds the terms of tiles i, i + 256, ... ascending, starting from 0 (a tile
 *     whose m_t is -inf contributes exactly 0); then a butterfly over each 64-lane wave (partner = lane xor 32, 16, 8, 4, 2, 1, each
 *     lane adding its partner's value to its own); then the four waves: ((w0 + w1) + w2) + w3.
 * A row whose M is not finite (a NaN or infinite logit) reports NaN.  Columns that are never computed hold exactly 0.0 wherever
 * out_tokens holds -1 (per-block early exit; passes of a batch of more than 1024 rows that stopped before the longest pass).
 * The vocabulary must be a multiple of 32 (and 49152 with do_sample). */
int  mellow_generate_scored(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                            const int32_t* input_ids, int B, int max_len, int do_sample, float top_p, float temperature,
                            uint64_t seed, int32_t row_offset, int stop_id, int ignore_stop, int32_t* out_tokens,
                            float* out_logprob, int32_t* out_len, int32_t* out_steps, float* first_token_ms);
/* n sampled answers for each of B examples from ONE encode and ONE prefill per example: n = num_return_sequences >= 1, the call
 * answers with N = B * n rows, row b * n + j is answer j of example b.  audio1 / audio2 / input_ids describe the B examples;
 * out_tokens dev i32 [N][max_len], out_logprob dev f32 [N][max_len] (may be NULL: no log-prob record), out_len host i32 [N].
 *
 * Definition.  The result IS what mellow_generate_sampled (out_logprob NULL) or mellow_generate_scored (do_sample != 0) returns when
 * it is given every example n times in a row -- B * n examples, example b at rows b * n .. b * n + n - 1 -- with the same seed and
 * row_offset: tokens, lengths, steps, the -1 columns and the log-prob record.  So
 *   - the global row index of the Philox stream of answer j of example b is row_offset + b * n + j (a caller that cuts its examples
 *     into several calls advances row_offset by n per example);
 *   - the stop rule, the per-block early exit and row migration act on the N rows exactly as they do there;
 *   - in MELLOW_PRECISION_F32 the two results are bit-identical: that mode's prefill does not depend on the batch (minor 1), and both
 *     forms run the last layer of the prefill, the head and every decode step on the same N rows;
 *   - in the default MELLOW_PRECISION_F32X3 they agree as closely as two batch compositions do (minor 1: the prefill here runs on B
 *     examples, there on B * n; last bits may differ, and a draw that such a bit decides may differ with them);
 *   - n == 1 takes the path of those calls and returns their bytes.
 * What the engine does with n > 1: front-end, encoder, projection and the LM prefill run on the B examples, with the prefill's K/V
 * written to a prefix buffer of its own; one copy kernel hands every example's prefix K/V to the pages of its n rows; the last prefix
 * position, the head, the first draw and the captured decode loop then run on N rows.  The kernels of the decode step and of the
 * prefill are those of the calls above.
 * Errors: do_sample == 0 (n greedy answers of one example are n copies of one answer: not offered); n < 1; B * n > 1024 (one pass
 * of rows: the caller splits its examples); n > 1 on an MELLOW_PRECISION_FP8 engine (its bf16 K/V pages have no fan-out); and every
 * error of mellow_generate_sampled.
 * Added under minor 4 like the scoring symbols: a binding detects it by symbol lookup. */
int  mellow_generate_n(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                       int B, int n, int max_len, int do_sample, float top_p, float temperature, uint64_t seed, int32_t row_offset,
                       int stop_id, int ignore_stop, int32_t* out_tokens, float* out_logprob, int32_t* out_len, int32_t* out_steps,
                       float* first_token_ms);
/* Q questions about every example -- N = B * Q answers, row b * Q + j answers question j of example b -- from ONE pass of front-end,
 * encoder and projection per example and ONE LM prefill of the positions that depend on the clips only.  audio1 / audio2 describe
 * the B examples; input_ids dev i32 [B][Q][text_len]; out_tokens dev i32 [N][max_len], out_logprob dev f32 [N][max_len] (may be
 * NULL: no log-prob record), out_len host i32 [N].
 *
 * Definition.  The result IS what the plain call returns for N examples, example b * Q + j being (audio1[b], audio2[b],
 * input_ids[b][j]), with the same seed and row_offset: tokens, lengths, steps, the -1 columns and the log-prob record.  The plain
 * call is mellow_generate_scored when out_logprob != NULL, else mellow_generate_sampled when do_sample != 0, else mellow_generate.  So
 *   - the global row index of the Philox stream of answer j of example b is row_offset + b * Q + j (a caller that cuts its examples
 *     into several calls advances row_offset by Q per example);
 *   - the stop rule, the per-block early exit and row migration act on the N rows exactly as they do there;
 *   - a prompt id outside the vocabulary, in any question, fails as it does there;
 *   - in MELLOW_PRECISION_F32 the two results are bit-identical: that mode's GEMMs do not depend on the batch (minor 1), the cut
 *     between the two prefills is a multiple of the attention's query tile, so every query meets the key tiles it meets there in the
 *     same order, and both forms run the last layer of the prefill, the head and every decode step on the same N rows;
 *   - in the default MELLOW_PRECISION_F32X3 they agree as closely as two batch compositions do (minor 1);
 *   - Q == 1 takes the path of those calls and returns their bytes.
 * What the engine does with Q > 1: of the prefix_len = 389 positions [audio1 129 | sep | audio2 129 | sep | prompt text_len] the
 * first 260 are the same for every question, and in a causal decoder so are their K/V at every layer.  The LM runs over positions
 * [0, 256) -- the largest multiple of 32 below 260 -- of the B examples into a prefix buffer; one copy kernel hands that K/V to the
 * pages of each example's Q rows; the LM then runs over positions [256, 389) of the N rows, attending to the row's pages; the last
 * prefix position, the head, the first token and the captured decode loop run on N rows as in the plain call.
 * Errors: Q < 1; B * Q > 1024 (one pass of rows: the caller splits its examples); Q > 1 on an MELLOW_PRECISION_FP8 engine (its bf16
 * K/V pages have no fan-out); and every error of the plain call.
 * Added under minor 4 like the scoring symbols: a binding detects it by symbol lookup. */
int  mellow_generate_q(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                       int B, int Q, int max_len, int do_sample, float top_p, float temperature, uint64_t seed, int32_t row_offset,
                       int stop_id, int ignore_stop, int32_t* out_tokens, float* out_logprob, int32_t* out_len, int32_t* out_steps,
                       float* first_token_ms);
/* Beam search: B examples, k beams each, N = B * k rows, row b * k + j = beam j of example b; 1 <= k <= 8 and N <= 1024.  ONE
 * encoder pass and ONE LM prefill per example, as in mellow_generate_n (prefix buffer, fan-out copy with n = k, row table); the
 * selection and the K/V hand-over below run inside the captured decode step.  audio1 / audio2 / input_ids describe the B examples.
 *
 * Definition.
 *   State per row: cum (fp32, the sum of the log-probs of the row's tokens) and fin (0 / 1, set when the row's last token was the
 *   stop id).  Initially cum = 0 for j = 0 and -inf for j > 0, fin = 0: the first selection expands one beam into k distinct tokens.
 *   A step: step s = 0 is the prefill's logits, steps s >= 1 are the decode steps.  An unfinished row r with fp32 logits l offers,
 *   for every token i, the candidate (parent = r, token = i) with value c = cum[r] + (l_i - lse(l)); lse = M + log S, M = max l,
 *   S = sum exp(l_i - M) added in one fixed order (no float atomics), everything in fp32 except the one logarithm (fp64, rounded
 *   once).  A finished row offers exactly one candidate, (r, stop_id) with c = cum[r] and log-prob increment 0: it stays finished.
 *   Selection: the new beams 0 .. k - 1 of an example are its k best candidates in the order c descending, then parent ascending,
 *   then token ascending.  A NaN candidate ranks as the arg-max kernel ranks a NaN: it is the maximum, and several NaNs rank by
 *   (parent, token) ascending.  A NaN logit makes lse, and with it EVERY candidate of its row, NaN; a row whose maximum is +-inf
 *   likewise.  Values that are equal AS fp32 numbers tie (two tokens of a row whose logits differ by less than the rounding of c
 *   tie on c and rank by token).
 *   Record: per (step, row) the step writes parent (0 .. k - 1, the beam index inside the example), token and lp (the increment)
 *   into tables [max_len][N]; a fourth table holds cum after the step.  The caller backtracks the tables; no token record is
 *   permuted on the device.
 *   K/V ownership: after the selection of step s >= 1, row r's pages hold its parent's K/V at positions [T, T + s - 1] (T =
 *   prefix_len) for every layer and kv head; position T + s - 1 was appended by this step's attention launch.  Rows whose parent is
 *   another row gather that span from the parent's pages into a staging buffer [layer][N][3][max_len][64] per tensor and scatter it
 *   into their own (a parent can itself be overwritten in the same step: never in place); rows that keep their page move nothing.
 *   Positions below T are identical across an example's rows after the fan-out and never move.
 *   End: the loop ends after the first step at which every row of every example is finished, or at max_len; ignore_stop != 0 (or a
 *   stop_id no token has, e.g. -1) means nothing ever finishes.  The count of finished rows can fall as well as rise (a finished
 *   beam can be displaced), so the kernel that finishes a step publishes the CURRENT count with the step ticket; the host follows
 *   it one step behind without synchronising, and at most one step is enqueued past the deciding one.
 * Outputs (host or device memory): out_parent / out_token i32 [max_len][N] and out_lp f32 [max_len][N], rows 0 .. *out_steps - 1
 * written; out_cum f32 [N] = cum after step *out_steps - 1 (the hypotheses' log-probs; during the search the beams compete on this
 * raw sum -- length penalties and the final ranking are the caller's, from the tables).  *out_steps = steps counted by the rule
 * above.  k = 1 is the greedy call with frozen finished rows.
 * Errors: k < 1 or k > 8; B * k > 1024 (the caller splits its examples); k > 1 with B * k * max_len > 65536 (the staging bound:
 * 30 layers x 65536 x 3 x 64 fp32 = 1.5 GB per tensor); k > 1 on an MELLOW_PRECISION_FP8 engine (its bf16 K/V pages have no
 * fan-out); a vocabulary other than 49152 (the row tiling of the sampler); and every error of mellow_generate.
 * Added under minor 4 like the scoring symbols: a binding detects it by symbol lookup. */
int  mellow_generate_beam(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                          int B, int k, int max_len, int stop_id, int ignore_stop, int32_t* out_parent, int32_t* out_token,
                          float* out_lp, float* out_cum, int32_t* out_steps, float* first_token_ms);
/* The same selection on caller data, no loop state (numeric tap): logits dev f32 [B * k][vocab], cum dev f32 [B * k], fin dev i32
 * [B * k] -> out_parent / out_token dev i32 [B * k], out_cum / out_lp dev f32 [B * k] (row b * k + j = the new beam j of example b).
 * Added under minor 4 with mellow_generate_beam. */
int  mellow_beam_select(mellow_engine_t* e, const float* logits, const float* cum, const int32_t* fin, int B, int k, int stop_id,
                        int32_t* out_parent, int32_t* out_token, float* out_cum, float* out_lp);
/* Repetition controls: rules that edit a row's fp32 logits on the device, inside the decode step, between the lm_head and the kernel
 * that picks the token -- for the prefill's first token as for every decode step, and for every picker (arg-max, sampler, beam select).
 *
 * Definition.  A row that has generated tokens h[0 .. s) is about to choose token s (s = 0 at the prefill's head).  The history is the
 * GENERATED tokens only (the prompt enters the model as embeddings and is not part of it); a beam row's history is its hypothesis --
 * what backtracking the tables gives for the row -- not the past of the slot it sits in.  l[v] are the raw fp32 logits.  Four rules,
 * applied in this order:
 *   1. repetition_penalty t (finite, > 0; 1 = off): for every DISTINCT token v of h, l[v] = l[v] < 0 ? l[v] * t : l[v] / t -- once per
 *      token however often it occurred; one correctly rounded fp32 multiplication or division.
 *   2. logit_bias: an optional dense vector bias[vocab], the same for all rows of the call: l[v] = l[v] + bias[v] (one fp32 addition).
 *      Values are finite or -inf (a suppressed token); NaN and +inf are the caller's error (the Python bindings reject them).
 *   3. no_repeat_ngram_size n (>= 0; 0 = off): if s >= n - 1, then for every i in [0, s - n] with h[i .. i + n - 2] == h[s - n + 1 .. s - 1]:
 *      l[h[i + n - 1]] = -inf.  n = 1 bans every token of the history.
 *   4. min_new_tokens m (>= 0; 0 = off): if s < m and the call's stop_id is >= 0: l[stop_id] = -inf.
 * Every picker then reads the processed row: the arg-max keeps its order (a NaN is the maximum, lowest index on ties), the sampler
 * applies temperature and nucleus to the processed row, the beam select forms its log-softmax from it.  A recorded log-prob
 * (mellow_generate_scored, _n, _q, the lp table of mellow_generate_beam) is then the log-softmax of the PROCESSED row at temperature 1:
 * the distribution the token was chosen from, in which a banned token has probability 0.  With rules on it is therefore NOT the number
 * mellow_score returns for the same answer.  A row in which every token is banned is the caller's error: it is not detected, the
 * result is token 0 with a NaN log-prob.
 *
 * mellow_generate_rules arms the rules for the NEXT mellow_generate* call on this context (mellow_generate, _sampled, _scored, _n, _q,
 * _beam all honour them); NULL disarms.  That call takes them at entry and clears them whatever its outcome, so a call after it runs
 * without rules unless they are armed again.  A fork has rules of its own, initially none.  logit_bias (host or device memory, or
 * NULL) is copied when the rules are armed.  A struct with t = 1, n = 0, m = 0 and no bias is still "on": the rules launch runs as the
 * identity (tokens are those of the call without rules; log-probs agree to the rounding of another summation order).  A call with
 * rules takes max_len <= 8192 (the history one row stages).  A call without armed rules launches exactly what it launched before
 * these symbols existed.
 * Errors (host code, before any device is touched): a `size` other than sizeof(mellow_logit_rules_t), t not finite or <= 0, negative
 * n or m; then a null or unfinalized engine; then a vocabulary other than 49152 (the row tiling of the sampler).
 * Added while the minor was 5 without raising it: a binding detects the two symbols by lookup. */
typedef struct mellow_logit_rules {
    int32_t size;                 /* sizeof(mellow_logit_rules_t) */
    float   repetition_penalty;   /* finite, > 0; 1 = off */
    int32_t no_repeat_ngram_size; /* >= 0; 0 = off */
    int32_t min_new_tokens;       /* >= 0; 0 = off */
    const float* logit_bias;      /* [vocab] fp32, host or device, or null; copied when armed */
} mellow_logit_rules_t;
int  mellow_generate_rules(mellow_engine_t* e, const mellow_logit_rules_t* rules);
/* The same rules on caller data, no loop state (numeric tap): logits dev f32 [B][vocab], edited in place; history dev i32 [B][ld]
 * (ld <= 8192) with hist_len dev i32 [B] tokens of every row (each row has its own s, clamped to [0, ld]); stop_id as in a
 * generate call.  cand_val / cand_idx dev [B][vocab / 32] receive, per 32-column tile of the processed row, its maximum and the
 * lowest index attaining it (the arg-max order); cand_sum dev f32 [B][vocab / 32] (may be NULL) the tile's sum of exp(l - cand_val),
 * exactly 0 for a tile whose maximum is -inf -- the partials the greedy arg-max and the log-prob merges of a step read.  Disarms rules
 * armed on the context (it uses the context's bias buffer).  Errors as above, and a null buffer, B <= 0 or ld outside [0, 8192]. */
int  mellow_logit_rules_apply(mellow_engine_t* e, const mellow_logit_rules_t* rules, float* logits, int B, const int32_t* history, int ld,
                              const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum);
/* Constrained decoding: every answer of a call is held to a set of phrases (token-id sequences) on the device, inside the decode step --
 * for the prefill's first token as for every decode step, and for every picker (arg-max, sampler, beam select).
 *
 * Constraint data.  Every answer row of the call has a root node in one shared trie arena:
 *   node_first[n_nodes + 1]  offsets into the edge arrays: the edges of node u are [node_first[u], node_first[u + 1]);
 *   node_flags[n_nodes]      bit 0 = terminal: a phrase ends here;
 *   edge_token[n_edges], edge_child[n_edges];
 *   row_root[n_rows]         n_rows = the row count N of the armed call's out_tokens;
 *   then_free                0 or 1.
 * The edges of a node are sorted by token, strictly ascending.  Every child > its parent, so the arena is acyclic.  A root is never
 * terminal: there are no empty phrases.  n_nodes, n_edges and n_rows are at most 1 << 20 (n_nodes and n_rows at least 1).
 *
 * State of a row.  A row that has generated h[0 .. s) is in one of four kinds of state: a node index u >= 0, DEAD (-1), FREE (-2) or
 * DONE (-3).  The state starts at row_root[row].  On token t the transition from u is:
 *   1. if u has an edge for t: the child c -- with then_free and c terminal: FREE instead;
 *   2. otherwise, if t == stop_id, stop_id >= 0 and u is terminal: DONE;
 *   3. otherwise DEAD.
 * DEAD, FREE and DONE absorb.  An edge wins over the stop rule.  The history is the row's GENERATED tokens, as for the rules: a beam
 * row's history is its hypothesis, not its slot's past.
 *
 * Allowed set.  node u: the edge tokens of u, plus stop_id if u is terminal and stop_id >= 0.  DEAD, DONE: {stop_id} if stop_id >= 0,
 * else empty.  FREE: everything.  An empty allowed set constrains nothing, so no row is ever banned whole.
 *
 * Effect on the row.  For a row whose allowed set is everything, or empty, the launch returns without touching it: the logits and the
 * tile partials stay byte-identical to what the head (or the guidance, or the rules) left.  For any other row l[v] = -inf for every v
 * outside the set; allowed values keep their bits; the row's tile partials are formed anew from the processed values (a tile banned
 * whole has maximum -inf and sums to exactly 0).
 *
 * Order in the step: guidance, then rules, then the constraint, then top log-probs, then the picker.  A recorded log-prob
 * (mellow_generate_scored, _n, _q, the lp table of mellow_generate_beam) and the top log-probs are those of the CONSTRAINED row: over
 * the phrase set (with the stop id) they multiply along the trie to probabilities that sum to 1.  Two consequences: they are NOT the
 * numbers mellow_score returns for the same answers; and min_new_tokens together with a set whose phrases are shorter can leave only
 * banned tokens before the constraint runs -- as with the rules, a row in which every token is banned is the caller's error.
 * A phrase that holds the stop id itself is followed like any other (the edge wins), so "phrase p, then stop" and a longer phrase
 * "p, stop id, ..." are then one path: keep the stop id out of the phrases if the probabilities are to sum to 1.
 * With then_free = 1 the set constrains only the start of an answer (a one-phrase set is a forced prefix): once a phrase is complete
 * the row is FREE and continues unconstrained; without it a row that has completed a phrase may only continue along the trie or stop.
 *
 * mellow_generate_constraint arms the constraint for the NEXT mellow_generate* call on this context (mellow_generate, _sampled,
 * _scored, _n, _q, _beam all honour it, in every precision, with and without armed rules, guidance, top log-probs and filters); NULL
 * disarms.  That call takes it at entry and clears it whatever its outcome.  A fork has a constraint of its own, initially none.  The
 * arrays (host or device memory) are copied into engine-owned buffers when the constraint is armed.  n_rows must equal the call's row
 * count -- B, B * n, B * Q, B * k, or 2 P for a guided call, whose two rows of a pair carry the same root -- else the call fails; a
 * call of more than 1024 rows advances through row_root pass by pass.  That a constraint is armed is part of the captured step's key,
 * the trie's contents and counts are not.  A call without an armed constraint launches exactly what it launched before these symbols
 * existed.
 * Errors (host code, before any device is touched, in this order): a `size` other than sizeof(mellow_constraint_t); a negative count
 * or one over its limit (and a null array, a then_free other than 0 or 1, a node_first that does not run from 0 to n_edges without
 * decreasing); unsorted edges; a child <= its parent or out of range; a root out of range or terminal; a token outside [0, 49152).
 * Then a null or unfinalized engine; then a vocabulary other than 49152 (the row tiling of the sampler).
 * Added while the minor was 5 without raising it: a binding detects the two symbols by lookup. */
typedef struct mellow_constraint {
    int32_t size;                 /* sizeof(mellow_constraint_t) */
    int32_t n_nodes;              /* 1 .. 1 << 20 */
    int32_t n_edges;              /* 0 .. 1 << 20 */
    const int32_t* node_first;    /* [n_nodes + 1] */
    const int32_t* node_flags;    /* [n_nodes], bit 0 = terminal */
    const int32_t* edge_token;    /* [n_edges] */
    const int32_t* edge_child;    /* [n_edges] */
    int32_t n_rows;               /* 1 .. 1 << 20: the rows of the armed call */
    const int32_t* row_root;      /* [n_rows] */
    int32_t then_free;            /* 0 or 1 */
} mellow_constraint_t;
int  mellow_generate_constraint(mellow_engine_t* e, const mellow_constraint_t* c);
/* The same launch on caller data, no loop state (numeric tap); the arguments are those of mellow_logit_rules_apply, with
 * c->n_rows == B: logits dev f32 [B][vocab], edited in place; history dev i32 [B][ld] (ld <= 8192) with hist_len dev i32 [B] tokens
 * of every row; the row's state is its root advanced by one transition per history token, and goes to out_state dev i32 [B] (may be
 * NULL).  cand_val / cand_idx / cand_sum (may be NULL) dev [B][vocab / 32] receive the tile partials of a constrained row; those of a
 * row whose allowed set is everything, or empty, are left as they are, like its logits.  It works on copies of its own and leaves
 * whatever is armed on the context as it is.  Errors as above, and a null buffer, B <= 0, c->n_rows != B or ld outside [0, 8192]. */
int  mellow_constraint_apply(mellow_engine_t* e, const mellow_constraint_t* c, float* logits, int B, const int32_t* history, int ld,
                             const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum, int32_t* out_state);
/* Stop strings: an answer ends once its TEXT contains one of a call's strings, decided on the device inside the decode step -- on the
 * bytes of the generated tokens, so a string that lies across a token boundary or inside a token is found -- for every picker
 * (arg-max, sampler, beam select).
 *
 * Vocabulary bytes.  An engine gets one byte string per token id: tok_off[V + 1] int32, starting at 0 and never decreasing, and
 * tok_bytes[tok_off[V]] uint8, V = 49152.  A token has at most 256 bytes and may be empty.  mellow_set_vocab_bytes copies the table
 * (host arrays) to the device.  It belongs to the SHARED engine state, like the weights: set once on any context, seen by the engine
 * and every fork of it.  Setting it again replaces it; never while a call runs on any context.
 * Errors (host code, before any device is touched, in this order): a null array; n_tokens other than 49152; offsets that do not start
 * at 0 or that decrease; a token of more than 256 bytes (the message names the token id and its length).  Then a null or unfinalized
 * engine; then a vocabulary other than 49152.
 *
 * Stop strings of a call: 1 to 16 byte strings of 1 to 64 bytes each, string j = str_bytes[str_off[j] .. str_off[j + 1]) (host
 * arrays, copied when armed).
 *
 * Text and hit.  The text of a row that has generated h[0 .. s) is X(s) = bytes(h[0]) | ... | bytes(h[s - 1]).  The row is HIT at s
 * iff some stop string is a substring of X(s).  The hit is sticky and is maintained step by step from a fixed-size state, the flag
 * and the last 63 bytes of the text:  hit(s) = hit(s - 1), or a stop string occurs in tail63(X(s - 1)) | bytes(h[s - 1]).  The
 * history is the row's GENERATED tokens, as for the rules and the constraint: a beam row's history is its hypothesis, not its slot's
 * past.  An id outside [0, 49152) in a history (the tap) has no bytes.
 *
 * Effect on the row.  A hit row gets l[stop_id] = 0.0f and l[v] = -inf for every other v, and its per-32-column tile partials are
 * formed anew: the stop id's tile gets value 0.0, index stop_id and sum exactly 1.0, every other tile value -inf, its lowest index and
 * sum exactly 0.  Every picker then takes the stop id, and the row ends through the EXISTING stop rule, one step after the token that
 * completed the match; loop control, tickets, block exit and row migration are untouched.  The launch returns without touching the
 * logits or the partials of a row that is not hit: they stay byte-identical.
 *
 * Order in the step: guidance, rules, constraint, stop strings, top log-probs, picker.  The launch overwrites rather than
 * intersects, so it wins over both earlier stages: over min_new_tokens (which only keeps the stop TOKEN out; Hugging Face behaves the
 * same way) and over an armed constraint.  It can never leave a row banned whole.
 * Log-probs: the recorded log-prob of the forced stop token is exactly zero (lp == 0.0f; the greedy form records -log 1.0f, which is the
 * zero with the sign bit set), those of the tokens before it are the ones of the same
 * call without stop strings, so a sum of log-probs runs over the answer up to the end of the token that completed the match.  A top
 * log-probs record at the forced step holds (stop_id, 0.0) first.
 *
 * mellow_generate_stop_strings arms the strings for the NEXT mellow_generate* call on this context (mellow_generate, _sampled,
 * _scored, _n, _q, _beam all honour it, in every precision, with and without armed rules, guidance, constraint, top log-probs and
 * filters); NULL disarms.  That call takes them at entry and clears them whatever its outcome.  A fork has strings of its own,
 * initially none.  That strings are armed is part of the captured step's key; their contents are not: they sit in fixed buffers.  A
 * call without armed strings launches exactly what it launched before these symbols existed.
 * Errors (in this order): a `size` other than sizeof(mellow_stop_strings_t); a count outside 1..16 (and a null array); a string length
 * outside 1..64; a null or unfinalized engine; a vocabulary other than 49152; no vocabulary bytes set; and, at the armed call, a
 * stop_id outside [0, 49152) -- mellow_generate_beam with ignore_stop is one such case, it knows no stop token.
 * Added while the minor was 5 without raising it: a binding detects the three symbols by lookup. */
int  mellow_set_vocab_bytes(mellow_engine_t* e, const int32_t* tok_off, const uint8_t* tok_bytes, int32_t n_tokens);
typedef struct mellow_stop_strings {
    int32_t size;                 /* sizeof(mellow_stop_strings_t) */
    int32_t n_strings;            /* 1 .. 16 */
    const int32_t* str_off;       /* [n_strings + 1], from 0; every string 1 .. 64 bytes */
    const uint8_t* str_bytes;     /* [str_off[n_strings]] */
} mellow_stop_strings_t;
int  mellow_generate_stop_strings(mellow_engine_t* e, const mellow_stop_strings_t* strings);
/* The same launch on caller data, no loop state (numeric tap); the arguments and conventions are those of mellow_constraint_apply:
 * logits dev f32 [B][vocab], edited in place; history dev i32 [B][ld] (ld <= 8192) with hist_len dev i32 [B] tokens of every row; the
 * row's state is the empty text advanced once per history token, and its hit flag, 0 or 1, goes to out_hit dev i32 [B] (may be NULL).
 * cand_val / cand_idx / cand_sum (may be NULL) dev [B][vocab / 32] receive the tile partials of a hit row; those of a row that is not
 * hit are left as they are, like its logits.  It works on copies of its own and leaves what is armed on the context alone.  Errors as
 * above, and a null buffer, B <= 0, ld outside [0, 8192] or a stop_id outside [0, 49152). */
int  mellow_stop_strings_apply(mellow_engine_t* e, const mellow_stop_strings_t* strings, float* logits, int B, const int32_t* history, int ld,
                               const int32_t* hist_len, int stop_id, float* cand_val, int32_t* cand_idx, float* cand_sum, int32_t* out_hit);
/* Contrastive (classifier-free) guidance: the step's distribution is contrasted with that of a NEGATIVE input on the device, inside
 * the decode step, between the lm_head and the rules launch / the kernel that picks the token -- for the prefill's first token as for
 * every decode step.
 *
 * Definition.  A guided call on P examples runs 2 * P rows: row 2i is example i (the conditional row), row 2i + 1 its negative (the same
 * question over silence, over the swapped pair, over another pair: the caller's choice; the two are ordinary rows of the batch for the
 * encoder, the prefill, the K/V pages and the decode layers).  Per step and pair, with l_c, l_u the fp32 logits of the two rows and s
 * the scale:
 *     lse_x = m_x + log(sum_v exp(l_x[v] - m_x)),  m_x = max_v l_x[v]          (x = c, u)
 *     a[v]  = l_c[v] - lse_c;  b[v] = l_u[v] - lse_u
 *     g[v]  = b[v] + s * (a[v] - b[v])
 * (the form of Hugging Face's unbatched classifier-free guidance processor: s = 1 gives the conditional log-softmax, s = 0 the
 * negative's, s > 1 moves away from the negative).  g is written to BOTH rows of the pair and the per-tile partials of both rows are
 * formed anew from it, so everything downstream sees two identical rows: the repetition controls, if armed, run after the guidance
 * (on g, with the pair's common history), then the arg-max or the sampler.  Both rows therefore get the same token and both K/V
 * histories advance with the answer actually produced.  A recorded log-prob is that of the processed distribution the token was
 * chosen from (the log-softmax of g, after the rules if armed), not the number mellow_score returns.  The sampler's random stream of
 * pair i is that of global row `row_offset + i` -- the PAIR index -- so guided answer i draws from the stream un-guided example i
 * would, whatever the batch layout.  All arithmetic is fp32 in one fixed order (the bits depend on the inputs only); logits that come
 * from the head are finite, and the definition says nothing about +-inf or NaN inputs.
 *
 * mellow_generate_guidance arms the scale for the NEXT mellow_generate* call on this context; that call takes it at entry and clears
 * it whatever its outcome.  A fork has its own, initially none.  Scale 1 arms nothing (and disarms).  Honoured by mellow_generate,
 * _sampled and _scored (and by _n with n = 1 and _q with Q = 1, which are those calls), with and without armed rules: their B is then
 * the ROW count 2 * P and must be even; every output holds all rows, rows 2i and 2i + 1 equal.  A call of more than 1024 rows splits
 * at an even row and its row offset advances by pairs.  Refused with a message, and disarmed, by mellow_generate_n with n > 1,
 * mellow_generate_q with Q > 1 and mellow_generate_beam.  Guidance needs no K/V fan-out: it is available in every precision.  A
 * guided call runs without row migration (a pair's rows stay neighbours); per-block early exit stays.  A call without armed guidance
 * launches exactly what it launched before these symbols existed.  Not built yet: beams, n > 1, question lists, sharding pairs over
 * data-parallel ranks.  Measured cost: 32 pairs take about 30 us (3 %) more per decode step than the un-guided call of
 * the same 64 rows, 28 us with rules armed on both.
 * Errors: a scale that is not finite (host code, before any device is touched); then a null or unfinalized engine.
 * Added while the minor was 5 without raising it: a binding detects the two symbols by lookup. */
int  mellow_generate_guidance(mellow_engine_t* e, float scale);
/* The same combination on caller data, no loop state (numeric tap): logits dev f32 [2 * P][vocab], rows 2i / 2i + 1 the conditional and
 * the negative row of pair i, both overwritten in place with g.  cand_val / cand_idx dev [2 * P][vocab / 32] receive, per 32-column tile
 * of g, its maximum and the lowest index attaining it (the arg-max order); cand_sum dev f32 [2 * P][vocab / 32] (may be NULL) the tile's
 * sum of exp(g - cand_val).  Any finite scale, 1 included.  Leaves guidance armed on the context as it is.  Errors as above, and a null
 * buffer, P <= 0 or a vocabulary other than 49152. */
int  mellow_guidance_apply(mellow_engine_t* e, float scale, float* logits, int P, float* cand_val, int32_t* cand_idx, float* cand_sum);
/* Top log-probs: next to the log-prob of the token that was chosen, the k likeliest tokens of every step and their log-probs, found
 * on the device inside the decode step, between the rules launch and the kernel that picks the token -- for the prefill's first token
 * as for every decode step.
 *
 * Definition.
 * - The row is a row of fp32 logits l[0..49152), as the picker of that step reads it: after guidance and after the rules, if armed.
 * - Alternatives 0 .. k-1 are the first k tokens in the order (value descending, index ascending).  A -0 counts as +0, as in the
 *   sampler's okey.  The selection moves fp32 values only, so it is exact.
 * - Each alternative's log-prob is l[v] - lse, one fp32 subtraction.
 * - lse = dec_lse_value(M, S), with M, S merged from the row's (cand_val, cand_sum) partials by dec_lse_max / dec_lse_sum (common.h).
 *   These are the same functions, in the same order, that dec_sample_kernel<true> uses.  So when the drawn token is among the k, its
 *   entry is bit-equal to the call's out_logprob.
 * - The greedy kernel records -log S directly.  There the entry agrees to the rounding of lse, not to the bit.
 * - A banned token (-inf) ranks last and reports -inf.  If fewer than k tokens are finite, the -inf ones follow by index.
 * - A row whose M is not finite (a NaN or +inf logit, or every token banned) reports NaN for all k log-probs.  Its ids are
 *   unspecified, but lie inside [0, vocab).
 * - 1 <= k <= 20 (TOP_LOGPROBS_MAX_K).  The vocabulary must be 49152, the sampler's row tiling.
 *
 * mellow_generate_top_logprobs arms the record for the NEXT mellow_generate* call on this context; that call takes it at entry and
 * clears it whatever its outcome.  A fork has its own, initially none.  k = 0 disarms.  out_ids i32 / out_lp f32 are [N][max_len][k],
 * host or device, for the N rows and the max_len of that call's out_tokens (a guided call's 2P rows included, rows 2i and 2i + 1
 * equal); an entry is -1 / exactly 0.0 wherever out_tokens holds -1.  A call of more than 1024 rows advances through the record pass by
 * pass, as it does through out_tokens.  Honoured by mellow_generate_scored, and by mellow_generate_n / mellow_generate_q when their
 * out_logprob is non-NULL, with and without armed rules and guidance, with do_sample 0 or 1, in every precision.  A call that records
 * no log-probs (mellow_generate, mellow_generate_sampled, _n / _q with a NULL out_logprob) fails with a message and disarms; so does
 * mellow_generate_beam (top log-probs of a beam hypothesis are not built).  k is part of the captured step's key: a captured graph
 * never replays with another k.  A call without the arming launches exactly what it launched before these symbols existed.  Measured
 * cost: at 32 rows about 14 us (k = 5) to 22 us (k = 20) more per decode step, 2 to 3 %.
 * Errors, host code first, before any device is touched: k outside [0, 20], or a null buffer with k > 0; then a null or unfinalized
 * engine; then a vocabulary other than 49152; and, inside the call, rows_of_a_pass * max_len * k > 1 << 24 (the record of one pass:
 * 134 MB).
 * Added while the minor was 5 without raising it: a binding detects the two symbols by lookup. */
int  mellow_generate_top_logprobs(mellow_engine_t* e, int k, int32_t* out_ids, float* out_lp);
/* The same selection on caller data, one launch, no loop state (numeric tap): logits dev f32 [B][vocab]; cand_val / cand_sum dev f32
 * [B][vocab / 32], the partials as mellow_logit_rules_apply or mellow_guidance_apply return them -> out_ids dev i32 [B][k], out_lp dev
 * f32 [B][k].  Leaves whatever is armed as it is.  Errors as above (here k = 0 is a bad argument), plus B <= 0 or a null input. */
int  mellow_top_logprobs_apply(mellow_engine_t* e, const float* logits, const float* cand_val, const float* cand_sum, int B, int k,
                               int32_t* out_ids, float* out_lp);
/* The same draw on caller logits, no loop state (numeric tap): logits dev [B][vocab], row_ids dev i32 [B] (global row index
 * of each row; NULL = 0..B-1), step = t above -> tokens dev i32 [B]. */
int  mellow_sample_logits(mellow_engine_t* e, const float* logits, int B, const int32_t* row_ids, int step, float top_p,
                          float temperature, uint64_t seed, int32_t* tokens);
/* Candidate filters of the sampled draw: top_k and min_p next to the nucleus, inside the sampler's launch of the captured step.
 *
 * Definition.  Steps 1 - 4 of mellow_generate_sampled become the following; the order is Hugging Face's (temperature, top_k, top_p,
 * min_p).
 * 1. z_i = l_i / temperature, exactly as there.  A row with a NaN yields its first NaN index, as there.
 * 2. top_k = K (K >= 0; 0 is off; K >= 49152 keeps every token).  T is the first K tokens in the order (z descending, index
 *    ascending).  The set has exactly K members: a tie group on the K-th value is cut by index (Hugging Face would keep the whole
 *    group; this is the order the nucleus tie-cut and the top log-probs use).  The selection moves fp32 values only, so it is exact.
 * 3. The nucleus inside T.  q_i = rn(exp(z_i - m) * 2^31), m the row maximum, as there; S_T = sum of q_i over T, an integer sum.
 *    Token i of T is kept iff the integer mass of the tokens of T strictly before it in the order is
 *    <= (u64)((double)top_p * (double)S_T).  With K = 0 this is the rule of mellow_generate_sampled, bit for bit.
 * 4. min_p (in [0, 1]; 0 is off).  Token i is kept iff q_i >= qmin, qmin = rn(min_p * 2^31) (an exact power-of-two scaling, rounded
 *    once).  The arg-max has q = 2^31 >= qmin, so it is always kept; min_p = 1 keeps exactly the tokens tied at the maximum.
 *    p_i / p_max does not change under renormalisation, so this is Hugging Face's "p_i >= min_p * p_max after the earlier filters",
 *    whatever those kept.
 * 5. The kept set is the intersection of 2 - 4.  It is always a prefix of the order -- whole tie groups, except where an index cut
 *    ends it -- so one (boundary key, index cut) pair and the q test describe it.  The Gumbel-max draw, the Philox keying (seed,
 *    global row, step) and the loop bookkeeping are exactly those of mellow_generate_sampled.
 * Recorded log-probs (out_logprob, top log-probs) stay the model's log-softmax at temperature 1 without any filter.
 *
 * mellow_generate_filters arms the filters for the NEXT mellow_generate* call on this context; that call takes them at entry and
 * clears them whatever its outcome.  A fork has its own, initially none.  NULL disarms, and so does top_k = 0 with min_p = 0 (nothing
 * is armed).  Honoured by mellow_generate_sampled and by mellow_generate_scored / _n / _q with do_sample != 0, with and without armed
 * rules, guidance and top log-probs, in every precision; a call of more than 1024 rows applies them in every pass.  A greedy call
 * (mellow_generate, do_sample == 0) and mellow_generate_beam fail with a message and disarm.  The armed call runs the sampler's
 * filtered instantiation, which is part of the captured step's key; K and qmin travel in the sampler's parameter block, so one
 * capture serves every value.  A call without the arming launches exactly what it launched before these symbols existed.
 * Errors, host code first, before any device is touched: a `size` other than sizeof(mellow_sample_filters_t), top_k < 0, min_p NaN
 * or outside [0, 1]; then a null or unfinalized engine; then a vocabulary other than 49152.
 * Added while the minor was 5 without raising it: a binding detects the two symbols by lookup. */
typedef struct mellow_sample_filters {
    int32_t size;                 /* sizeof(mellow_sample_filters_t) */
    int32_t top_k;                /* K >= 0; 0 = off */
    float   min_p;                /* in [0, 1]; 0 = off */
} mellow_sample_filters_t;
int  mellow_generate_filters(mellow_engine_t* e, const mellow_sample_filters_t* f);
/* The filtered draw on caller logits, no loop state (numeric tap): the arguments of mellow_sample_logits plus the filters (not NULL).
 * Always the filtered instantiation, also for neutral values (whose tokens are then bit-equal to mellow_sample_logits').  Leaves
 * whatever is armed as it is.  Errors as above, then those of mellow_sample_logits. */
int  mellow_sample_logits_filtered(mellow_engine_t* e, const float* logits, int B, const int32_t* row_ids, int step, float top_p,
                                   float temperature, uint64_t seed, const mellow_sample_filters_t* f, int32_t* tokens);

/* ---- parity taps (same kernels as mellow_generate, stage by stage) ------------------------------- */
/* A1-A3: htsat.py:864-870.  wav dev [n][n_samples] -> out dev [n][frames][64]; apply_bn=0 gives the
 * LogmelFilterBank output, 1 the post-bn0 tensor. */
int  mellow_logmel(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_samples, int apply_bn,
                   float* out);
/* A1-A13: AudioEncoder.forward (mellow.py:64-68) + downsample (decoder.py:14-18):
 * wav dev [n][n_samples] -> out dev [n][129][576]. */
int  mellow_encode(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_samples, float* out);
/* A1-A14: generate_prefix_inference -> out dev [B][prefix_len][hidden]. */
int  mellow_prefix(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples,
                   const int32_t* input_ids, int B, float* out);
/* A15 prefill: lm(inputs_embeds=prefix).logits[:, -1, :] (wrapper.py:217-218) with the KV pages
 * written.  prefix dev [B][T][hidden]; reserve = max extra tokens that will follow; logits dev [B][vocab]
 * (may be NULL). */
int  mellow_lm_prefill(mellow_engine_t* e, const float* prefix, int B, int T, int reserve, float* logits);
/* A15 decode step: append embed_tokens(token_ids) (wrapper.py:237) at the next position and return the
 * new last-position logits.  token_ids dev i32 [B]; logits dev [B][vocab] (may be NULL).  Continues the state of the last
 * mellow_lm_prefill; a mellow_generate or mellow_lm_forward_logits call in between ends that state (error). */
int  mellow_lm_decode_step(mellow_engine_t* e, const int32_t* token_ids, float* logits);
/* lm.model.embed_tokens(ids) (decoder.py:47,64-66; wrapper.py:237): token_ids dev i32 [n] -> out dev [n][hidden]. */
int  mellow_embed_tokens(mellow_engine_t* e, const int32_t* token_ids, int n, float* out);
/* The decoder's forward over a whole embedded sequence, `self.lm(inputs_embeds=embedding_cat).logits` of the training-time
 * forward (Mellow.forward mellow.py:89-98 -> DecoderModel.forward decoder.py:57-90, which concatenates the prefix with the
 * embedded answer tokens): embeds dev [B][T][hidden] -> logits dev [B][T - from_pos][vocab], the rows of positions
 * t >= from_pos.  Inference arithmetic only (no loss, no gradient); leaves no decode state behind. */
int  mellow_lm_forward_logits(mellow_engine_t* e, const float* embeds, int B, int T, int from_pos, float* logits);

/* ---- scoring: teacher-forced log-probabilities of given tokens.  The reference has no counterpart as a function; the numbers are
 *      `log_softmax(model(input_dict).logits, -1)` gathered at the answer ids (Mellow.forward, mellow.py:89-98).  The LM head of these
 *      two calls is the exact fp32 MFMA GEMM of the logits tap above (in every precision mode) with an epilogue that reduces each
 *      row's logits to log-softmax statistics instead of storing them: no [rows][vocab] tensor is written, and a row's target logit
 *      and maximum logit are bit-identical to the entries the logits tap returns.  Results are bit-deterministic run to run.
 *      The ABI is defined on results only (how much work the candidates of one example share is the engine's business).
 *
 * The tap-level twin of the logits tap: embeds dev [B][T][hidden]; element (b, j) of every output describes the logits of position
 * from_pos + j, scored against targets dev i32 [B][T - from_pos]:
 *   out_logprob dev f32 [B][T - from_pos]  logit[target] - lse, or 0 for a target of -1 ("not scored")
 *   out_argmax  dev i32 (may be NULL)      arg-max of the position's logits, first-index ties and NaN rule of the arg-max tap
 *   out_lse     dev f32 (may be NULL)      log(sum(exp(logits))) = M + log(sum_g s_g exp(m_g - M)) over 64-column groups g, ascending
 *   out_max     dev f32 (may be NULL)      maximum logit M
 * A target outside [-1, vocab) is an error (the binding raises IndexError).  Leaves no decode state behind. */
int  mellow_lm_score(mellow_engine_t* e, const float* embeds, int B, int T, int from_pos, const int32_t* targets,
                     float* out_logprob, int32_t* out_argmax, float* out_lse, float* out_max);
/* The end-to-end form: K candidate answers of at most L tokens for each of B examples.  audio1 / audio2 / input_ids as for the
 * generate call; cand_ids dev i32 [B][K][L] (entries at j >= cand_len are padding: read, never scored; any id in the vocabulary),
 * cand_len HOST i32 [B][K], each in [1, L]; prefix_len + L <= max_positions.  Front-end, encoder, projection and prefix run once
 * per example; the LM input [prefix_b | embed(cand_{b,k})] of the B x K rows is built on the device and the all-position forward
 * runs over them (more than 1024 rows: consecutive passes inside the call).  Token j of a candidate is scored by the logits of
 * position prefix_len - 1 + j (the last prefix position predicts token 0):
 *   out_logprob dev f32 [B][K][L]  log_softmax(logits[prefix_len - 1 + j])[cand_ids[b][k][j]] for j < cand_len, exactly 0 beyond
 *   out_sum     dev f32 [B][K]     sum of out_logprob over j < cand_len, accumulated in ascending j in fp32
 *   out_argmax  dev i32 [B][K][L]  (may be NULL) arg-max of the logits of every position, padding positions included
 * A candidate id outside the vocabulary at j < cand_len is an error (IndexError in the binding), as is a cand_len outside [1, L].
 * A candidate's results do not depend on K, on its slot k, on the other rows or on L in MELLOW_PRECISION_F32 (bit-equal); in the
 * default mode they agree to the 1e-3 stated under minor 1 above.  Drains the stream before returning; the next generate call is
 * undisturbed. */
int  mellow_score(mellow_engine_t* e, const float* audio1, const float* audio2, int64_t n_samples, const int32_t* input_ids,
                  int B, const int32_t* cand_ids, const int32_t* cand_len, int K, int L, float* out_logprob, float* out_sum,
                  int32_t* out_argmax);
/* A0 (host harness of the reference, wrapper.py:146 `torchaudio.transforms.Resample(sr, 32000)`) on the device:
 * sinc-interpolation resampling with a Hann window, lowpass_filter_width 6, rolloff 0.99, gcd-reduced polyphase bank.
 * wav dev [n][n_in] -> out dev [n][*n_out], *n_out = ceil(new_freq * n_in / orig_freq); out == NULL only queries *n_out. */
int  mellow_resample(mellow_engine_t* e, const float* wav, int n_clips, int64_t n_in, int orig_freq, int new_freq,
                     float* out, int64_t out_capacity, int64_t* n_out);
/* arg-max with first-index ties (torch.argmax, wrapper.py:232): logits dev [B][vocab] -> tokens dev i32 [B] */
int  mellow_argmax(mellow_engine_t* e, const float* logits, int B, int32_t* tokens);

/* Copy a named internal activation of the LAST mellow_encode / mellow_prefix call to `out` (dev).
 * Taps are recorded only after mellow_debug_enable_taps(e, 1).  Names: "power", "logmel_bn", "patch",
 * "stage0".."stage3", "latent", "fpx", "emb33", "proj33".  *numel receives the element count. */
int  mellow_debug_enable_taps(mellow_engine_t* e, int on);
int  mellow_debug_tap(mellow_engine_t* e, const char* name, float* out, int64_t capacity, int64_t* numel);

/* Numeric taps on HOST data (work on any engine, finalised or not): C[M][N] = A[M][K] . W[N][K]^T through one GEMM kernel.
 * iters > 0 and ms2 != NULL: ms2[0] / ms2[1] receive the average milliseconds of the operand pre-pass / of the GEMM.
 *   mellow_debug_gemm_f32: mode 0 = the exact fp32 MFMA kernel (no pre-pass), 16 / 17 = the six-product f32x3 kernels
 *     MELLOW_PRECISION_F32X3 runs: 16 splits A in registers (no pre-pass), 17 takes A pre-split in APB order by a pre-pass and
 *     stages both operands by LDS-DMA.  Any other mode is an error.  K % 32 == 0, N % 4 == 0.
 *   mellow_debug_gemm_fp8: the MELLOW_PRECISION_FP8 GEMM -- A quantised per row and W per row to OCP e4m3 (scale =
 *     amax / 448, round to nearest even), exact products, fp32 accumulation.  K % 64 == 0, N % 4 == 0. */
int  mellow_debug_gemm_f32(mellow_engine_t* e, int mode, const float* A, int M, int K, const float* W, int N, float* C,
                           int iters, float* ms2);
int  mellow_debug_gemm_fp8(mellow_engine_t* e, const float* A, int M, int K, const float* W, int N, float* C,
                           int iters, float* ms2);
/* GEMM epilogue tap on HOST data (works on any engine, finalised or not): ONE call of a GEMM launcher the engine itself calls --
 * kernel 0 launch_gemm (exact fp32 MFMA), 16 launch_gemm_bf16x3_fused (f32x3, A split in registers), 17 launch_split_rows_apb then
 * launch_gemm_bf16x3_apb (f32x3, both operands by LDS-DMA) -- with the epilogue the descriptor describes, after the weight packing
 * that epilogue needs (launch_pack_weight / launch_pack_weight_pairs, launch_pack_bf16x3).  mellow_debug_gemm_f32 stays the plain
 * timing and accuracy tap.  The fp8 kernel, c16, kv16 and the AMX hand-over are not reachable from here.
 *   A host f32 [M][K]; W host f32 [Nw][K] logical rows (swiglu: rows [0, Nw / 2) gate, [Nw / 2, Nw) up; qkv-rope: 576 q, 192 k,
 *   192 v rows); bias host f32 [Nw] or NULL; resid host f32 [C rows][N] or NULL; crow_map host i32 [rows_in] or NULL (C row of
 *   row m = (m / rows_in) * rows_out + crow_map[m % rows_in], a one-to-one map into [0, rows_out), M % rows_in == 0; C rows =
 *   M / rows_in * rows_out, else M); rs_ssq host f32 [M][rs_parts] or NULL (every accumulator of row m is scaled by
 *   1 / sqrt(sum_p rs_ssq[m][p] / rs_dim + rs_eps)); rope_cos / rope_sin host f32 [Tmax][32], or both NULL for the tables of
 *   mellow_host_rope_tables(cfg.rope_theta, 64, Tmax).
 * Every output the launch can write is filled with 0xFF bytes first and returned whole (capacities in bytes):
 *   out_c    f32 [C rows + 32][ldc]           (linear with want_c, swiglu with want_c; resid = 2 loads the residual into it first)
 *   out_c3   the raw APB image of N columns, roundup(M, 128) rows, 6 bytes per element (want_c3)
 *   out_ssq  f32 [M + 32][N / 64]             (want_ssq: sums of squares of the stored row over each 64-column group)
 *   out_q    f32 [M + 32][576]                (qkv-rope)
 *   out_k / out_v  f32 pages [B + 1][3][Tmax][64], B = M / (T - pos0): every position, and one page set of no example
 * Refused by name, nothing launched: K % 32 != 0 (kernels 0 / 16) or K % 16 != 0 or K < 48 (kernel 17); N not a multiple of 4 in
 * [rup(Nw, 4), rup(Nw, 128)] (swiglu: N != Nw / 2); want_c3 with linear and N % 64 != 0 or with swiglu and N % 16 != 0; want_c3
 * or splitk_max with kernel 0; want_ssq without want_c3; ldc < N; pos0 outside [0, T); Tmax < T; M != B * (T - pos0); qkv-rope
 * with Nw or N != 960; a capacity that is too small. */
typedef struct mellow_gemm_epi {
    int32_t size;            /* sizeof(mellow_gemm_epi_t) */
    int32_t kernel;          /* 0, 16, 17 */
    int32_t epi;             /* 0 linear, 1 swiglu, 2 qkv-rope */
    int32_t M, K, Nw, N;     /* Nw logical weight rows, N stored columns */
    int32_t act;             /* linear: 0 none, 1 GELU, 2 sigmoid */
    int32_t bias;            /* linear: 0 / 1 */
    int32_t resid;           /* linear: 0 none, 1 a separate buffer, 2 in place (resid == C) */
    int32_t rows_in, rows_out;   /* linear, with crow_map */
    int32_t ldc;             /* linear: floats between C rows, >= N (swiglu: N) */
    int32_t want_c, want_c3, want_ssq;
    int32_t rs_parts;        /* with rs_ssq */
    float rs_dim, rs_eps;
    int32_t splitk_max;      /* 0 = no workspace; else the engine's 512-tile workspace with sk_tiles = 256 and this sk_max */
    int32_t no_x3w;          /* keep a K = 96, M >= 8192 launch of kernel 17 on the tile kernel */
    int32_t T, Tmax, pos0;   /* qkv-rope: pos0 > 0 selects EPI_QKV_ROPE_AT; rows m = b * (T - pos0) + i are positions pos0 + i */
} mellow_gemm_epi_t;
int  mellow_debug_gemm_epi(mellow_engine_t* e, const mellow_gemm_epi_t* d, const float* A, const float* W, const float* bias,
                           const float* resid, const int32_t* crow_map, const float* rs_ssq, const float* rope_cos,
                           const float* rope_sin, void* out_c, int64_t c_capacity, void* out_c3, int64_t c3_capacity, float* out_ssq,
                           int64_t ssq_capacity, float* out_q, int64_t q_capacity, float* out_k, float* out_v, int64_t kv_capacity);
/* Attention taps on HOST data (work on any engine, finalised or not): ONE launch of an attention kernel of the engine on the
 * caller's arrays, through the launcher the engine itself calls.  The device output is filled with 0xFF bytes before the launch
 * and returned whole, so that a caller sees every byte the kernel did not write:
 *   out_form 0  fp32 rows: M + 32 rows of `width` floats, the real rows first (out_capacity >= (M + 32) * width * 4 bytes);
 *   out_form 1  the raw APB image the f32x3 GEMMs take as their pre-split A operand (three bf16 pieces per element, 16-byte
 *               slots in the order of mellow_amd/csrc/common.h): roundup(M, 128) rows, 6 bytes per element
 *               (out_capacity >= roundup(M, 128) * width * 6 bytes).
 * out_capacity is in bytes.  Every argument the engine itself never passes is an error, and nothing is launched.
 *
 * Causal GQA prefill attention (9 query heads of 64 on 3 kv heads; width = 576, M = B * (T - qpos0)):
 *   q host f32 [B][T - qpos0][576], k / v host f32 pages [B][3][Tmax][64] (positions >= T are never read).
 *   variant 0 = the exact fp32 MFMA kernel, 1 = the f32x3 kernel (operands split exactly in three bf16), 2 = operands rounded once
 *   to bf16, fp32 pages, 3 = the same on bf16 pages and bf16 q rows (q, k, v are rounded to bf16 on the device first).
 *   qpos0 = 0: the whole-sequence launch.  qpos0 > 0 (a multiple of 32, < T): the launch for the queries at positions [qpos0, T)
 *   only, variants 0 and 1.  out_form 1: variants 0 and 1.
 *   Errors: Tmax < T, qpos0 % 32 != 0, qpos0 >= T, qpos0 > 0 or out_form 1 with variant 2 or 3, too small a capacity. */
int  mellow_debug_prefill_attn(mellow_engine_t* e, int variant, const float* q, const float* k, const float* v, int B, int T,
                               int Tmax, int qpos0, int out_form, void* out, int64_t out_capacity);
/* Swin window attention (windows of 64 tokens, head_dim 24; width = C): qkv host f32 [M][3 C] rows in window order, bias host
 *   f32 [nH][64][64], mask host f32 [nW][64][64] or NULL (window w takes mask w % nW).  in16 != 0: qkv is rounded to bf16 rows on
 *   the device first and the bf16-input kernel runs (out_form 0 only).
 *   Errors: M % 64 != 0, C != 24 * nH, nH not in {4, 8, 16, 32}, a mask with nW <= 0, in16 with out_form 1, too small a capacity. */
int  mellow_debug_window_attn(mellow_engine_t* e, const float* qkv, int M, int C, int nH, const float* bias, const float* mask,
                              int nW, int in16, int out_form, void* out, int64_t out_capacity);
/* Norm / hand-over tap on HOST data (works on any engine, finalised or not): ONE launch of a norm launcher of the engine, or of one
 * of the two stand-alone hand-over producers, on the caller's rows.
 *   op 0  LayerNorm (eps 1e-5, biased variance): launch_layernorm (form 0) / launch_layernorm_apb (forms 1, 2).  x host f32 [M][C];
 *         row_map host i32 [ntok] or NULL: output row m reads input row (m / ntok) * ntok + row_map[m % ntok], a permutation of
 *         [0, ntok), M % ntok == 0.
 *   op 1  patch-merging LayerNorm: launch_merge_layernorm.  x host f32 [n][R * R][C]; the output has M = n * (R / 2)^2 rows of 4 C
 *         columns, row (clip, i, j) = the tokens (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) side by side; w, b host f32 [4 C].
 *   op 2  RMSNorm w * (x * rsqrt(mean x^2 + eps)): launch_rmsnorm (form 0) / launch_rmsnorm_apb (forms 1, 2).
 *   op 3  no norm: launch_split_rows_apb (form 1) / launch_quant_mx8 (form 2) on x itself, lda = C; w and b are not read.
 * The device outputs are filled with 0xFF bytes before the launch and returned whole (capacities in bytes):
 *   form 0  out = f32 [M + 32][columns]                                          (ops 0, 1, 2)
 *   form 1  out = the raw APB image: roundup(M, 128) rows, 6 bytes per element    (ops 0, 2, 3)
 *   form 2  out = the raw AMX image (MXFP8: e4m3 elements in the order of mellow_amd/csrc/common.h): roundup(M, 128) *
 *           roundup(C, 64) bytes; out_scales = its E8M0 scale bytes: roundup(M, 128) * 8 * KQ bytes, KQ = ceil(ceil(C / 64) / 4)
 *           (ops 0, 2, 3)
 * Refused by name, nothing launched: C % 4 != 0; form 0 with more than 1536 columns; ops 0 / 2 in forms 1 / 2 with C % 16 != 0 or
 * C > 768 (op 2: C > 752, the 96 KiB of LDS launch_rmsnorm_apb asks for); op 3 form 1 with C % 16 != 0; op 3 form 0; op 1 in form
 * 1 or 2, with an odd R or with M != n * (R / 2)^2; M < 1 or M > 2^22; a null w (ops 0 - 2) or b (ops 0, 1); a row_map that is no
 * permutation, or with an op other than 0; eps < 0; a capacity that is too small. */
int  mellow_debug_norm(mellow_engine_t* e, int op, int form, const float* x, int M, int C, const float* w, const float* b, float eps,
                       const int32_t* row_map, int ntok, int n, int R, void* out, int64_t out_capacity, void* out_scales,
                       int64_t scales_capacity);
/* Decode attention tap on HOST data (works on any engine, finalised or not): ONE call of launch_dec_attn and, when Wo is given,
 * then ONE call of launch_dec_oproj (whose prologue merges the key splits) -- the launchers the decode step itself calls, on
 * DecArgs the tap fills from buffers of its own.  rows = roundup(B, 32), RB = rows / 32; the slots B .. rows - 1 run on zeros.
 *   slabs   host f32 [8][B][960] (fused 0: the split-K partial sums of the q/k/v projection, p = their sum) or [6][B][960] (fused 1)
 *   ssq1    host f32 [B][8] (fused 0: rscale = 1 / sqrt(sum / 576 + eps)); NULL with fused 1
 *   x_res   host f32 [B][576]: fused 0 x_new, the o_proj's residual; fused 1 x_mid
 *   down    host f32 [4][B][576] (fused 1: x_new = x_mid + their sum, rscale from x_new); NULL with fused 0
 *   rope_cur host f32 [64], cos then sin of the position, or NULL for row `pos` of the tables of mellow_host_rope_tables with
 *           cfg.rope_theta, 64 dims, Tmax positions
 *   k_pages / v_pages  host f32 [P][3][Tmax][64], P >= rows; kv16 != 0: rounded to bf16 on the device (launch_kv_to_bf16) and the
 *           launch gets the bf16 pages
 *   blk_live host i32 [RB] and row_of_slot host i32 [rows], or NULL (RB >= 2 only): a block with blk_live 0 and a slot with
 *           row_of_slot -1 do not run; slot b reads and extends the pages of example row_of_slot[b]
 *   Wo      host f32 [576][576] (x_mid' = x_new + att . Wo^T), or NULL: no o_proj launch
 * d->ts must be what dec_key_splits gives for this RB and kv16 (2; or 1 from two row blocks on with fp32 pages); gs, the 4-key
 * groups per key split, follows from ctx_end, ts and kv16 by the engine's own rule and is returned in *out_gs.
 * Every output is filled with 0xFF bytes before the launches and returned whole and raw (capacities in bytes):
 *   out_att   f32 [ts][RB][36][2][64][4] (F16-layout partials) + one more block [36][2][64][4]
 *   out_ml    f32 [9][rows][ts][2]
 *   out_k / out_v  the pages [P + 1][3][Tmax][64]: f32, or the 2-byte form with kv16 (kv_capacity: bytes of each)
 *   out_xnew  f32 [rows + 32][576] (fused 0: what was sent, in rows < rows)
 *   with Wo: out_xmid f32 [rows][576] (F32-layout, raw); out_x16 f32 [rows][576] (F16-layout, raw) or, with want_x3, the F3-32
 *   image followed by the F3-16 image (rows * 576 * 6 bytes each); out_ssq f32 [rows + 32][40]
 * Refused by name, nothing launched: B < 1; pos < 1 or pos >= Tmax; ctx_end <= pos or ctx_end > Tmax; Tmax < 2 or above
 * cfg.max_positions; P < rows; ts not admissible; fused not 0 / 1; blk_live or row_of_slot at one row block; row_of_slot not
 * one-to-one or outside [0, P); want_x3 without Wo; a null required pointer; eps not finite or negative; a capacity too small.
 * Invalidates the decode state of an earlier prefill. */
typedef struct mellow_dec_attn {
    int32_t size;            /* sizeof(mellow_dec_attn_t) */
    int32_t B, P;            /* batch slots in use, page sets in k_pages / v_pages */
    int32_t pos, Tmax, ctx_end;
    int32_t ts, fused, kv16;
    int32_t want_x3;
    float eps;
} mellow_dec_attn_t;
int  mellow_debug_dec_attn(mellow_engine_t* e, const mellow_dec_attn_t* d, const float* slabs, const float* ssq1, const float* x_res,
                           const float* down, const float* rope_cur, const float* k_pages, const float* v_pages,
                           const int32_t* blk_live, const int32_t* row_of_slot, const float* Wo, int32_t* out_gs, void* out_att,
                           int64_t att_capacity, float* out_ml, int64_t ml_capacity, void* out_k, void* out_v, int64_t kv_capacity,
                           float* out_xnew, int64_t xnew_capacity, void* out_xmid, int64_t xmid_capacity, void* out_x16,
                           int64_t x16_capacity, float* out_ssq, int64_t ssq_capacity);
/* Decode GEMV tap on HOST data (works on any engine, finalised or not): ONE call of ONE of the launchers that make up the rest of a
 * decode layer and the step's final norm -- the launchers the decode step itself calls, on DecArgs the tap fills from buffers of
 * its own.  rows = roundup(B, 32), RB = rows / 32; in the row-major operands the slots B .. rows - 1 run on zeros.
 *   op 0  launch_dec_qkv:        the split-K q/k/v projection.  (kcd 0, first 1): the step's first launch, on x alone; it stages
 *                                rope_cur from row pos + inc_pos of the tables and, with inc_pos, advances the position word.
 *                                (kcd 8 = DEC_KC_DOWN, first 0): x_new = x + the sum of the down slabs.
 *   op 1  launch_dec_gateup (form 0) / launch_dec_gateup3 (form 1): gate/up with the SwiGLU and its RMS factor
 *   op 2  launch_dec_down:       the split-K down projection
 *   op 3  launch_dec_qkv2 (form 0) / launch_dec_qkv2x3 (form 1): the down projection and the next q/k/v projection in one launch
 *   op 4  launch_dec_final_norm: kcd 0 or 8; xnF, or with want_x3 the pre-split xn3
 * Weights, logical row-major host f32, packed on the device by the routines the loader uses (launch_pack_weight; the 8 + 8 row
 * gate/up interleave and launch_pack_weight16 / launch_pack_weight16n; launch_compose_f64, the [W' | Q] concatenation and the pack):
 *   op 0: W = W' [960][576], the q/k/v weight with the norm weight folded in;   op 1: W = gate, W2 = up [1536][576], folded;
 *   op 2: W = Wd [576][1536];   op 3: W = W' [960][576], W2 = Wd [576][1536];   op 4: W = the norm vector [576]
 * Activations:
 *   x       host f32 [B][576]: x_mid (ops 0, 4; op 3 form 0), sent in F32-layout
 *   down    host f32 [8][B][576] with kcd 8 (ops 0, 4), NULL with kcd 0
 *   h       host f32 [B][1536] (op 2; op 3 form 0), sent in F32-layout with 192 k-tiles
 *   x_img   raw image of x_mid as a device kernel leaves it, whole (all `rows` rows): op 1 form 0 the F16-layout (rows * 576 * 4
 *           bytes), op 1 form 1 the F3-16 triples, op 3 form 1 the F3-32 triples (rows * 576 * 6 bytes)
 *   h_img   raw F3-32 image of h, 96 pairs (op 3 form 1: rows * 1536 * 6 bytes)
 *   ssq     raw f32 [rows][40], the o_proj's sums of squares of x_mid (op 1; a row's 36 partials are summed, columns 36 .. 39 are not read)
 *   rope_cos / rope_sin  host f32 [Tmax][32] (op 0 with first), or NULL for the tables of mellow_host_rope_tables
 *   blk_live host i32 [RB] or NULL (RB >= 2 only): a block with blk_live 0 does not run (the f32x3 forms skip its stores)
 * Every output the launch can write is filled with 0xFF bytes first and returned whole and raw (capacities in bytes):
 *   out_pq    f32 [8][rows][960] + 32 rows   (ops 0, 3; op 3 owns the slabs 0 .. Q2_NPQ - 1 = 5 only)
 *   out_down  f32 [8][rows * 576] F32-layout slabs + 32 * 576 floats   (ops 2, 3; op 3 owns the slabs 0 .. Q2_HC - 1 = 3 only)
 *   out_ssq1  f32 [rows + 32][8];  out_xnew f32 [rows + 32][576];  out_rope f32 [128] (cos | sin, then 64 floats nobody owns);
 *   out_pos   the position word after the launch   (op 0)
 *   out_gu    f32 [rows * 1536 + 32 * 1536] (h in F32-layout with 192 k-tiles);  out_h3 the F3-32 image of h, 96 pairs, 6 bytes
 *             per element of the same count (op 1; out_h3 form 1 only)
 *   out_xn    [rows * 576 + 32 * 576] elements: f32 in F32-layout, or with want_x3 the F3-32 image, 6 bytes each   (op 4)
 *   out_snap  i32 [64]: blk_snap [32] and 32 words nobody owns   (op 4 with blk_live)
 *   out_q     f32 [960][1536] row-major: Q = W' . Wd as launch_compose_f64 rounded it   (op 3)
 * Out of scope: the fp8 forms (wscale, a8, launch_dec_qkv2_w8); the lm_head, arg-max, compaction and row load have mellow_debug_dec_tail.
 * Refused by name, nothing launched: op outside 0 .. 4; form outside 0 / 1, or form 1 with op 0, 2 or 4; B < 1 or B > 1024; kcd
 * not 0 / 8, or with an op other than 0 / 4; op 0 with first != (kcd == 0); inc_pos without first; first / inc_pos with another
 * op; with first: Tmax < 2 or above cfg.max_positions, pos < 0 or pos + inc_pos >= Tmax, one table without the other; tables
 * without first; want_x3 with another op or with a vocabulary the streaming lm_head does not tile; blk_live at one row block; eps
 * not finite or negative; a missing operand of the launch or one the launch does not take (W2, x, h, down, x_img, h_img, ssq); an
 * image of another byte count; a null output or a capacity too small.  Invalidates the decode state of an earlier prefill. */
typedef struct mellow_dec_gemv {
    int32_t size;            /* sizeof(mellow_dec_gemv_t) */
    int32_t op, form;
    int32_t B;
    int32_t kcd, first, inc_pos;
    int32_t pos, Tmax;       /* op 0 with first */
    int32_t want_x3;         /* op 4 */
    float eps;
} mellow_dec_gemv_t;
int  mellow_debug_dec_gemv(mellow_engine_t* e, const mellow_dec_gemv_t* d, const float* W, const float* W2, const float* x,
                           const float* down, const float* h, const void* x_img, int64_t x_img_bytes, const void* h_img,
                           int64_t h_img_bytes, const float* ssq, const float* rope_cos, const float* rope_sin,
                           const int32_t* blk_live, float* out_pq, int64_t pq_capacity, float* out_down, int64_t down_capacity,
                           float* out_ssq1, int64_t ssq1_capacity, float* out_xnew, int64_t xnew_capacity, float* out_rope,
                           int32_t* out_pos, float* out_gu, int64_t gu_capacity, void* out_h3, int64_t h3_capacity, void* out_xn,
                           int64_t xn_capacity, int32_t* out_snap, float* out_q, int64_t q_capacity);
/* Decode step-tail tap on HOST data (works on any engine, finalised or not): ONE call of ONE of the launchers that end a decode
 * step -- the launchers the step itself calls, on DecArgs and LoopArgs the tap fills from buffers of its own.  rows = roundup(B, 32),
 * RB = rows / 32.
 *   op 0  launch_dec_lm_head:   form 0 the fp32 kernel (x host f32 [B][576], sent in F32-layout; the slots B .. rows - 1 run on
 *                               zeros), form 1 the streaming f32x3 kernel (x_img = the raw F3-32 image of all `rows` rows, 36 pairs,
 *                               rows * 576 * 6 bytes; DecArgs::x3 = DEC_X3_HEAD).  W = the logical head weight [V][576], packed on the
 *                               device as the loader packs lm_head (launch_pack_weight into roundup(V, 128) rows, K8p = 72).
 *                               want_logits: DecArgs::logits set or null; want_sum: DecArgs::cand_sum set or null; blk_live host i32
 *                               [RB] or NULL (RB >= 2 only): a block with blk_live 0 stores nothing.
 *   op 1  launch_dec_argmax on planted partials: cand_val f32 / cand_idx i32 / cand_sum f32 (or NULL) [B][V / 32]; write_x: gather
 *                               row `token` of W = the embedding table [V][576] (the model ties it to the head) into the F32-layout
 *                               row of the slot.  with_state 0: LoopArgs() -- the token only.  with_state 1: params {max_len,
 *                               stop_id}, T0 and the position word `pos`, seen_stop i32 [rows], n_seen / arrive / ticket, blk_left +
 *                               blk_live i32 [RB] (together, or both NULL), blk_snap i32 [RB] or NULL, row_of_slot i32 [rows] or
 *                               NULL, with_logprob (LoopArgs::out_logprob; needs cand_sum); host_progress is a mapped host word of
 *                               the call's own.
 *   op 2  launch_dec_compact:   row_of_slot [rows], blk_live / blk_left [RB], seen_stop [rows], x host f32 [B][576] (sent in
 *                               F32-layout), n_compactions
 *   op 3  launch_dec_load_rows: x = the source rows host f32 [n_src][ld]; row_ids i32 [B] with T_last 0 (the kernel clamps an id
 *                               to [0, n_src)), or NULL with T_last >= 1 (row b * T_last + T_last - 1)
 * Every output the launch can write is filled with 0xFF bytes first and returned whole and raw (capacities in bytes):
 *   out_logits    f32 [rows + 32][V]; out_cand_val f32 / out_cand_idx i32 / out_cand_sum f32 [rows + 32][V / 32] each   (op 0)
 *   out_tokens    i32 [rows + 32]   (op 1)
 *   out_record    i32 [rows][max_len], out_logprob f32 of the same shape (with_logprob), out_progress the host word   (op 1, with_state)
 *   out_state     i32 words: seen_stop [rows + 32] | n_seen, arrive, ticket, n_compactions and 28 words nobody owns | blk_left [64] |
 *                 blk_live [64] (the words RB .. 31 are sent as zeros, as the engine's are; 32 .. 63 nobody owns) | row_of_slot
 *                 [rows + 32]; what the caller did not plant holds 0xFF bytes   (op 1 with_state, op 2)
 *   out_x         f32 [rows * 576 + 32 * 576]: the residual rows in F32-layout   (ops 1, 2, 3)
 * Out of scope: the fp8 forms (wscale, a8) have no argument here.
 * Refused by name, nothing launched: op outside 0 .. 3; form outside 0 / 1, or form 1 with another op; B < 1 or B > 1024; V not a
 * multiple of 32 in [32, 2^20], (rows + 32) * V above 2^28, or (form 1) a V the streaming kernel does not tile; a switch or scalar
 * of another op that is not 0; blk_live / blk_left / blk_snap / row_of_slot at one row block; blk_live without blk_left or the
 * reverse (op 1); with_logprob without cand_sum or without with_state; row_of_slot entries outside -1 .. rows - 1 or taken twice;
 * max_len outside 1 .. 4096, T0 outside 0 .. 2^20, |pos| above 2^20; ld below 576 or no multiple of 4, n_src < 1 or n_src * ld above
 * 2^26, T_last != 0 with row_ids, T_last < 1 or B * T_last > n_src without; a missing operand of the launch or one the launch does
 * not take; an image of another byte count; a null output or a capacity too small.  Invalidates the decode state of an earlier
 * prefill. */
typedef struct mellow_dec_tail {
    int32_t size;            /* sizeof(mellow_dec_tail_t) */
    int32_t op, form;
    int32_t B;
    int32_t V;               /* ops 0 and 1: the vocabulary (n = V / 32 tiles) */
    int32_t want_logits, want_sum;               /* op 0 */
    int32_t write_x, with_state, with_logprob;   /* op 1 */
    int32_t max_len, stop_id, T0, pos;           /* op 1 with with_state */
    int32_t n_seen, arrive, ticket;              /* op 1 with with_state */
    int32_t n_compactions;   /* op 2 */
    int32_t ld, n_src, T_last;                   /* op 3 */
} mellow_dec_tail_t;
int  mellow_debug_dec_tail(mellow_engine_t* e, const mellow_dec_tail_t* d, const float* W, const float* x, const void* x_img,
                           int64_t x_img_bytes, const int32_t* blk_live, const float* cand_val, const int32_t* cand_idx,
                           const float* cand_sum, const int32_t* seen_stop, const int32_t* blk_left, const int32_t* blk_snap,
                           const int32_t* row_of_slot, const int32_t* row_ids, float* out_logits, int64_t logits_capacity,
                           float* out_cand_val, int32_t* out_cand_idx, float* out_cand_sum, int64_t cand_capacity,
                           int32_t* out_tokens, int64_t tokens_capacity, int32_t* out_record, float* out_logprob,
                           int64_t record_capacity, int32_t* out_state, int64_t state_capacity, uint64_t* out_progress, float* out_x,
                           int64_t x_capacity);
/* The decode step's lm_head kernel on caller-supplied rows (dev): logits[B][vocab] = x[B][hidden] . lm_head^T with the engine's
 * own head weights (the e4m3 copy in MELLOW_PRECISION_FP8; act_fp8 != 0 then also quantises x inside the kernel: one scale per
 * batch row and 72-column slice, fp8 matrix pipe).  Invalidates the decode state of an earlier prefill. */
int  mellow_debug_dec_head(mellow_engine_t* e, const float* x, int B, int act_fp8, float* logits);
/* Its twin for mellow_generate_scored: the same kernel in the variant that also emits the per-tile log-sum-exp partials, and the
 * merge above, on caller rows: logits dev [B][vocab] (may be NULL; bit-equal to mellow_debug_dec_head's), out_lse / out_max dev
 * f32 [B] (lse = M + log S, M), out_argmax dev i32 [B] (the arg-max tap's rule).  Invalidates the decode state the same way. */
int  mellow_debug_dec_head_lse(mellow_engine_t* e, const float* x, int B, int act_fp8, float* logits, float* out_lse,
                               float* out_max, int32_t* out_argmax);

/* (The library also exports three developer instrumentation entry points that are NOT part of this ABI and may change without
 *  a version bump: mellow_dev_gemm_time, mellow_dev_prof_dump, mellow_dev_kdebug -- timers and stamps used by tools/, none of
 *  them changes a result.) */

/* ---- measurement ---------------------------------------------------------------------------------
 * Per-kernel-family accounting with HIP events on the engine's stream.  When enabled, every launch
 * of a profiled family is bracketed by an event pair and its algorithmic work is accumulated;
 * hipGraph replay is switched off while profiling (events cannot be interleaved into a replay).
 * families: see mellow_prof_family_name(). */
int         mellow_prof_enable(mellow_engine_t* e, int on);
int         mellow_prof_reset(mellow_engine_t* e);
int         mellow_prof_num_families(void);
const char* mellow_prof_family_name(int i);
/* launches, total milliseconds, algorithmic flops and algorithmic bytes accumulated for family i */
int         mellow_prof_get(mellow_engine_t* e, int i, int64_t* launches, double* ms, double* flops,
                            double* bytes);
/* phase wall times of the last mellow_generate call (HIP events): front-end+encoder+prefix, prefill,
 * decode loop; milliseconds */
int         mellow_last_phase_ms(mellow_engine_t* e, float* encode_ms, float* prefill_ms, float* decode_ms);
/* decode steps (counting the prefill's token) the last mellow_generate call enqueued: *out_steps, or *out_steps + 1 */
int         mellow_last_steps_enqueued(mellow_engine_t* e);
/* Diagnostic: how many times the last mellow_generate call repacked the still-running rows into fewer 32-row blocks
 * (reference-semantics mode, B > 32: a block's kernels return at once when all of ITS rows have produced the stop id; rows
 * migrate between blocks so that this happens as early as the number of running rows allows). */
int         mellow_last_row_repacks(mellow_engine_t* e);
/* 1 when this engine runs the STFT (A1, htsat.py:864) as a 1024-point FFT per frame instead of the DFT GEMM: f32x3 mode and a
 * checkpoint whose conv_real / conv_imag weights are window[n] * cos / sin(2 pi k n / 1024) to 1e-6 (checked at finalize). */
int         mellow_stft_is_fft(mellow_engine_t* e);
/* Number of independent parts the next f32x3 LM prefill of this engine runs as (2 by default: two half-batches on two HIP
 * streams, so that one part's kernel tails are covered by the other's).  The engine OWNS this configuration: the first call
 * (this function or the first prefill) creates the side stream(s) and MEASURES with a device-clock probe whether they really
 * run beside the main stream -- HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the variable says
 * otherwise when the runtime starts), and two streams that share a queue serialise.  A side stream that does not overlap is
 * replaced (up to 8 attempts); if none does, the engine falls back to ONE chain and this function returns 1.  Results are
 * bit-identical for every value; only the speed differs (the reference has no counterpart: wrapper.py:87-88 is its device model). */
int         mellow_prefill_parts(mellow_engine_t* e);
/* MELLOW_ABI_MINOR of the library */
int         mellow_abi_minor(void);
/* 1 = replay the decode step from a captured hipGraph (default), 0 = eager launches */
int         mellow_set_graph(mellow_engine_t* e, int on);

/* ---- numeric mode of the dense GEMMs of the encoder (Swin linears) and of LM prefill; call before the first
 *      mellow_engine_load_tensor.  The reference has no counterpart (fp32 ATen matmuls throughout).
 *   MELLOW_PRECISION_F32: exact fp32 on v_mfma_f32_32x32x2_f32 everywhere (fmaf-chain accumulation, the closest arithmetic to the
 *     reference's ATen matmuls); the parity suite runs in this mode AND in the default one with the same tolerances.
 *   MELLOW_PRECISION_FP8: BASELINE config 5 -- OCP e4m3 weights (per-output-channel scale) and activations (per-row
 *     scale, quantised on the fly), fp32 accumulate on v_mfma_f32_32x32x16_fp8_fp8; the GEMM kernels of the decode step read
 *     e4m3 weights and quantise their activations in registers (one scale per batch row and wave k-slice).  Front-end (STFT,
 *     mel), K % 64 != 0 layers, the attentions and the norms stay fp32.  Not bit-exact: report token agreement.
 *   MELLOW_PRECISION_F32X3 (DEFAULT of mellow_engine_create, of the Python `Engine` / `MellowWrapper`, and the mode bench.py
 *     reports): fp32 GEMMs on the bf16 matrix pipe -- every fp32 operand is split EXACTLY into three bf16 terms, the six largest
 *     partial products (the rest is < 2^-23 |a*b|) are accumulated in fp32: fp32-accurate (error against fp64 measured <= the
 *     fp32 MFMA kernel's), not bit-identical to MELLOW_PRECISION_F32.  Every engine-level parity test (tolerances against the
 *     reference's fp32 outputs, exact greedy tokens) runs in this mode and in MELLOW_PRECISION_F32.  In this mode the last bits
 *     of an example's activations may depend on how many examples the call holds: encoder launches of few output tiles are split
 *     along K (a fixed summation order per launch shape; option "splitk" = 0 turns it off). */
#define MELLOW_PRECISION_F32 0
#define MELLOW_PRECISION_FP8 1
#define MELLOW_PRECISION_F32X3 2
int         mellow_engine_set_precision(mellow_engine_t* e, int mode);

/* ---- explicit configuration (round 6).  The library reads no environment variable: a consumer's environment cannot change its
 *      arithmetic.  Every switch is a named integer option, set after mellow_engine_create and before mellow_engine_finalize
 *      ("arena_mb": before the first mellow_engine_load_tensor); an unknown key or a malformed value is an error.  The defaults
 *      are the configuration bench.py measures and the parity suite runs; the reference has no counterpart (wrapper.py:35-49 has
 *      no hidden modes, and neither has a default engine).  Keys: prefill_split, prefill_fuse_norm, decode_fuse,
 *      decode_fuse_max_rb, splitk, enc_apb, graph, fp8_decode, fp8_prefill, fp8_decode_act, fp8_kv16, fp8_attn_bf16, decode_x3, decode_x3_min_rb,
 *      x3_stft, stft_fft, x3_apb, x3_attn, x3w, row_migration, arena_mb (mellow_amd/csrc/engine.cpp: kOptions says what each does
 *      and whether it can change the answers). */
int         mellow_engine_set_option(mellow_engine_t* e, const char* key, const char* value);
/* JSON text: {"abi": [major, minor], "precision": "f32x3" | "f32" | "fp8", "reads_environment": false, "finalized": ...,
 *  "stft_is_fft": ..., "non_default": [keys], "options": {key: {"value", "default", "changes_answers"}}}.  Returns the bytes the
 *  text needs including its terminator (-1 for a null engine); writes it only when `capacity` suffices (call with buf = NULL
 *  to size). */
int64_t     mellow_engine_describe(mellow_engine_t* e, char* buf, int64_t capacity);

/* ---- host-only helpers (callable without a GPU; used by CPU tests) -------------------------------- */
/* token permutation of a Swin block: out[m] = source token (h*R+w) feeding window-order row m, for
 * resolution R and cyclic shift `shift` (htsat.py:427-436).  out host i32 [R*R]. */
int  mellow_host_window_map(int R, int shift, int32_t* out);
/* packs a row-major [N][K] fp32 matrix into the engine's MFMA fragment order:
 * out host f32 [NP/32][KP/8][64][4] with NP = roundup(N,npad), KP = roundup(K,32), zero padded. */
int  mellow_host_pack_weight(const float* w, int N, int K, int npad, float* out, int64_t out_capacity);
/* the rotary tables the engine builds when "mellow.rope_cos/sin" are not loaded (transformers LlamaRotaryEmbedding:
 * inv_freq = 1 / theta^(2i/head_dim) and angle = position * inv_freq in fp32; cos / sin correctly rounded to fp32).
 * cos_out / sin_out host f32 [max_pos][head_dim/2]. */
int  mellow_host_rope_tables(float theta, int head_dim, int max_pos, float* cos_out, float* sin_out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MELLOW_HIP_H */
