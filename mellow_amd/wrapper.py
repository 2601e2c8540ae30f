"""`MellowWrapper` — drop-in for the reference's public API (reference mellow/wrapper.py:25-287,
re-exported by mellow/__init__.py:1):

    from mellow_amd import MellowWrapper
    mellow = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True)
    response = mellow.generate(examples=[[path1, path2, prompt]], max_len=300, top_p=0.8, temperature=1.0)

Host code stays Python (yaml config, checkpoint loading, wav ingest, tokenisation); everything from the
(B, 320000) waveforms to the generated token ids runs in libmellow_hip.so on the MI355X through the C ABI of
include/mellow_hip.h.  There is no CPU model path: `use_cuda=False` / `device="cpu"` raise.

What is kept from the reference, quirks included: class attributes `model_repo`/`model_name`;
`ValueError` for an unknown model; `config/<config>.yaml` key layout; strict `state_dict` load with the
'module.' retry; prompt right-padded with '!' to 129 ids; sep = token 0; pads attended; multi-channel wav
flattened not mixed; crop start from the unseeded `random` module; sampling parameters accepted but the result
is greedy for every value (the reference's top-p filter never removes the arg-max, wrapper.py:220-232) -- the default
call stays exactly that; the
loop stops only when every row has produced the stop id; text is cut at the first '<|endoftext|>'.
Extension (opt-in, keyword-only): `generate(..., do_sample=True, seed=s)` draws every token by seeded nucleus sampling
inside the captured decode step -- z = logits / temperature, the nucleus of the reference's rule (a token is kept iff the
softmax mass strictly before it in (z desc, index asc) order is <= top_p), then Gumbel-max with Philox4x32-10 noise keyed by
(seed, row, step); include/mellow_hip.h mellow_generate_sampled gives the exact definition.  seed=None draws a 63-bit seed from
`random` (kept as `last_seed`); under data parallelism the seed must be given and equal on every rank.
Extension (keyword-only): `generate(..., do_sample=True, top_k=K, min_p=p)` adds the two candidate filters users of Hugging Face
`generate` reach for, inside the same sampler launch and in Hugging Face's order (temperature, top_k, top_p, min_p): only the K
likeliest tokens, the nucleus inside them, and of those only tokens at least p times as likely as the likeliest
(include/mellow_hip.h mellow_generate_filters).  Both are off (0) by default: Hugging Face's top_k = 50 is not adopted.
Extension (keyword-only): `generate(..., do_sample=True, num_return_sequences=n)` returns n sampled answers per example -- a list
of n strings (with return_logprobs=True: of n dicts, so `max(out[i], key=lambda a: a["logprob"])` re-ranks) -- for self-consistency
voting or re-ranking.  Log-mel, encoder, projection and the LM prefill run ONCE per example; the prefix K/V is copied to the n answer
rows, which then decode like n rows of a batch (include/mellow_hip.h mellow_generate_n).  Answer j of example i draws from the random
stream of global row i * n + j: the answers are those of the same call on a list that holds every example n times in a row.
Extension: the third element of an example may be a list (or tuple) of prompts, several questions about the one pair of clips:
`generate([[a, b, ["what differs?", "caption both"]]], ...)` returns, per example, the list of answers in question order (greedy,
do_sample and return_logprobs all apply).  Log-mel, encoder and projection run ONCE per example, and so does the LM prefill of the
256 prefix positions that depend on the clips only; their K/V is copied to the example's answer rows, and only the remaining 133
positions are prefilled per question (include/mellow_hip.h mellow_generate_q).  Question counts may differ between examples.  Answer j
of example i draws from the random stream of global row i * Q + j (Q = the largest count): the answers are those of the same call on a
list that holds the pair once per question.  Not combined with num_return_sequences > 1, data parallelism or precision="fp8".
Extension: `score(examples, candidates)` returns the teacher-forced log-probability of given answer strings and
`choose(examples, candidates)` the index of the likeliest one (multiple-choice ranking, re-ranking of sampled answers); the LM
head of that path reduces its logits to log-softmax statistics on the fly (include/mellow_hip.h mellow_score).
Extension (keyword-only): `generate(..., choices=[...])` holds every answer to a set of phrases -- the labels of a classification set,
the options of a multiple-choice question -- by constrained decoding: inside the captured decode step every token that does not
continue one of the phrases is banned before the token is chosen (include/mellow_hip.h mellow_generate_constraint,
mellow_amd/constraint.py), so the answer IS one of the phrases and, with return_logprobs=True, its log-prob is that of the constrained
distribution, a probability over the phrase set.  One decode serves any number of phrases (`choose()` runs one teacher-forced row
per candidate), and it combines with do_sample, num_return_sequences, question lists, num_beams (the k likeliest labels with their
probabilities from one decode), guidance and the repetition keywords.  `choices_then="free"` constrains only the start of the answer
(a one-phrase set is a forced answer prefix).
Extension (keyword-only): `generate(..., stop_strings=[...])` ends an answer once its text contains one of the strings ("the first
sentence", "up to the first newline").  The match runs on the device inside the captured decode step, on the bytes of the generated
tokens (include/mellow_hip.h mellow_generate_stop_strings, mellow_amd/stop_strings.py), so a string that lies across a token
boundary or inside a token is found, the row stops one step after the token that completed it, and no step after the cut is paid
for or counted in `logprob`.  The returned text is cut at the string (`include_stop_str_in_output=True` keeps it).
Deviations: `tqdm` progress output is not produced; the B>1/steps==1 mis-shape and B==1/steps==1 crash of
reference wrapper.py:251-253 are not reproduced (one string per example is always returned).
"""
from __future__ import annotations

import argparse
import math
import os
import random
import warnings
from collections import OrderedDict
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import yaml

from . import spec
from .audio import load_audio_into_tensor
from .engine import DEFAULT_PRECISION, Engine, EngineError
from .spec import LMConfig


def get_model_class(model_type: str):
    """reference mellow/model/model.py:3-7."""
    if model_type == "Mellow":
        return Engine
    raise NotImplementedError


def get_audio_encoder(name: str):
    """reference mellow/model/audio.py:3-7."""
    if name == "HTSAT":
        return "HTSAT"
    raise Exception("The audio encoder name {} is incorrect or not supported".format(name))


class MellowWrapper:
    """A class for interfacing the Mellow model on MI355X."""

    model_repo = "soham97/mellow"
    model_name = {"v0": "v0.ckpt", "v0_s": "v0_s.ckpt"}
    last_seed: Optional[int] = None      # seed of the last generate(do_sample=True) call

    def __init__(self, config, model, device, use_cuda=True, *, checkpoint: Optional[str] = None,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, tokenizer=None, max_positions: Optional[int] = None,
                 data_parallel: Optional[bool] = None, precision: Optional[str] = None,
                 engine_options: Optional[Dict[str, int]] = None):
        """Reference signature `MellowWrapper(config, model, device, use_cuda=True)` (wrapper.py:35) plus keyword-only
        extensions: `checkpoint` (a local .ckpt instead of the hub download), `state_dict` (already loaded), `tokenizer`
        (an object with encode / encode_plus / decode), `max_positions` (prefix 389 + max_len may not exceed it; default: the LM's
        max_position_embeddings, 8192), `data_parallel` (True or MELLOW_DATA_PARALLEL=1: shard `generate` over the ranks of an
        initialised torch.distributed group, one process per GPU, every rank calling with the SAME examples -- checked; default
        off: like the reference, every process answers its own examples), `precision` ("f32x3" (default) | "f32" | "fp8"),
        `engine_options` (named options of the HIP library, mellow_engine_set_option; default none: the library's defaults --
        the library itself reads no environment variable)."""
        self.supported_versions = self.model_name.keys()
        if model not in self.supported_versions:
            raise ValueError(f"The model {model} is not supported. The supported versions are {str(self.supported_versions)}")
        self.parent_path = Path(os.path.realpath(__file__)).parent
        self.config_path = os.path.join(self.parent_path, "config", config + ".yaml")
        self.use_cuda = use_cuda
        self.device = device
        self._state_dict = state_dict
        self.model_path = self._resolve_checkpoint(model, checkpoint) if state_dict is None else "<state_dict>"
        self._tokenizer_override = tokenizer
        self._max_positions = max_positions
        self._data_parallel = data_parallel
        # numeric mode of the dense GEMMs (include/mellow_hip.h): "f32x3" fp32-accurate bf16-split (default = the mode
        # bench.py reports), "f32" exact fp32 MFMA, "fp8" BASELINE config 5; keyword or MELLOW_PRECISION
        self._precision = precision or os.environ.get("MELLOW_PRECISION") or DEFAULT_PRECISION
        self._engine_options = dict(engine_options or {})
        self.model, self.tokenizer, self.args = self.get_model_and_tokenizer(config_path=self.config_path)

    # ---- construction -------------------------------------------------------------------------------------
    def _resolve_checkpoint(self, model: str, checkpoint: Optional[str]) -> str:
        if checkpoint is not None:
            return checkpoint
        name = self.model_name[model]
        local = os.environ.get("MELLOW_CKPT_DIR")
        if local and os.path.exists(os.path.join(local, name)):
            return os.path.join(local, name)
        try:  # reference wrapper.py:41-42
            from huggingface_hub.file_download import hf_hub_download
            path = hf_hub_download(self.model_repo, name)
            try:
                hf_hub_download(self.model_repo, "config.json")   # the reference's download counter
            except Exception:
                pass
            return path
        except Exception as e:
            raise FileNotFoundError(
                f"checkpoint {name} not available offline: pass checkpoint=..., state_dict=..., or set MELLOW_CKPT_DIR ({e})")

    def read_config_as_args(self, config_path):
        """yaml -> argparse.Namespace whose fields are plain dicts (reference wrapper.py:51-57)."""
        with open(config_path, "r") as f:
            yml_config = yaml.load(f, Loader=yaml.FullLoader)
        return argparse.Namespace(**{k: v for k, v in yml_config.items()})

    def get_model_and_tokenizer(self, config_path):
        args = self.read_config_as_args(config_path)
        args.model["decoder"]["prefix_dim"] = args.model["encoder"]["d_proj"]
        get_model_class(model_type=args.model["model_type"])                  # NotImplementedError on unknown type
        get_audio_encoder(args.model["encoder"]["audioenc_name"])             # Exception on unknown encoder
        text_decoder = args.model["decoder"]["text_decoder"]
        if "smollm2" not in text_decoder.lower():                            # reference decoder.py:30-31
            raise ValueError(f"text decoder {text_decoder.lower()} not supported")
        if args.model["decoder"]["prefix_length"] != spec.PREFIX_LEN or args.data["text_tokenization_len"] != spec.TEXT_LEN \
                or args.model["encoder"]["d_proj"] != spec.D_PROJ or args.data["sampling_rate"] != spec.SAMPLE_RATE:
            raise ValueError("config does not describe the v0 geometry this engine is built for")
        if not self.use_cuda or isinstance(self.device, str):
            raise RuntimeError("MellowWrapper (MI355X engine) has no CPU path: pass use_cuda=True and an integer device")
        lm = LMConfig.load()
        engine = Engine(lm=lm, device=int(self.device), max_positions=self._max_positions, precision=self._precision,
                        options=self._engine_options)
        sd = self._state_dict
        if sd is None:
            sd = torch.load(self.model_path, map_location=torch.device("cpu"))
        params = 0
        for k, v in sd.items():
            kk = k[7:] if k.startswith("module.") else k
            if kk.endswith(("running_mean", "running_var", "num_batches_tracked", "attn_mask", "relative_position_index")) \
                    or kk == spec.LM + "lm_head.weight":
                continue
            params += math.prod(v.size())
        engine.load_state_dict(sd, strict=True)       # strict, with the 'module.' retry of wrapper.py:75-82 in the engine
        tokenizer = self._tokenizer_override
        if tokenizer is None:
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(text_decoder)
            tokenizer.add_special_tokens({"pad_token": "!"})
        model_path = self.model_path.split(os.path.sep)[-1]
        cfg_name = config_path.split(os.path.sep)[-1]
        print(f"model {model_path}, {cfg_name}, parameter count: {params}")
        return engine, tokenizer, args

    # ---- preprocessing ----------------------------------------------------------------------------------------
    def load_audio_into_tensor(self, audio_path, audio_duration, resample=True):
        return load_audio_into_tensor(audio_path, audio_duration, self.args.data["sampling_rate"], resample)

    def preprocess_audio(self, audio_files, resample):
        """-> float32 (B, segment_seconds*sampling_rate) on the engine's device (reference wrapper.py:170-179).
        With MELLOW_DEVICE_RESAMPLE=1 the resampling runs on the GPU (mellow_resample, the device twin of audio.resample):
        files are decoded on the host, resampled per file on the device, then tiled / cropped as in the reference."""
        if resample and os.environ.get("MELLOW_DEVICE_RESAMPLE") == "1":
            from .audio import fit_duration, load_wav
            sr_t = self.args.data["sampling_rate"]
            rows = []
            for f in audio_files:
                wav, sr = load_wav(str(f))
                w = self.model.resample(wav, sr, sr_t) if sr != sr_t else wav.to(self.model.tdev)
                rows.append(fit_duration(w.reshape(-1), self.args.data["segment_seconds"] * sr_t).to(torch.float32).reshape(1, -1))
            return torch.cat(rows, 0).to(self.model.tdev)
        # files are independent: decode / resample / tile-or-crop on a thread pool (torch releases the GIL in the conv1d of
        # the resampler); output order = input order.  The reference does this serially; its crop start is an unseeded
        # `random` draw per file (wrapper.py:164), so the draw order carries no meaning.
        def one(f):
            return self.load_audio_into_tensor(f, self.args.data["segment_seconds"], resample).reshape(1, -1)
        if len(audio_files) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(len(audio_files), os.cpu_count() or 1, 32)) as pool:
                tensors = list(pool.map(one, audio_files))
        else:
            tensors = [one(f) for f in audio_files]
        return torch.cat(tensors, 0).to(self.model.tdev)

    def _encode_padded(self, text, L):
        """One prompt -> BatchEncoding padded / truncated to L ids.  The reference calls `tokenizer.encode_plus(...,
        pad_to_max_length=True)` (wrapper.py:186-190, transformers 4.46); newer transformers spell the padding
        `padding="max_length"`, and transformers >= 5 dropped `encode_plus` in favour of `tokenizer(...)` (same arguments)."""
        enc = getattr(self.tokenizer, "encode_plus", None) or self.tokenizer
        last = None
        for pad_kw in ({"padding": "max_length"}, {"pad_to_max_length": True}):
            try:
                return enc(text=text, add_special_tokens=True, truncation=True, max_length=L, return_tensors="pt", **pad_kw)
            except TypeError as e:      # this spelling is not known to the installed tokenizer
                last = e
        raise last

    def preprocess_text(self, prompts):
        """-> {'input_ids', 'attention_mask'} int64 (B, 129) (reference wrapper.py:181-195; the mask is never used)."""
        L = self.args.data["text_tokenization_len"]
        ids, masks = [], []
        for ttext in prompts:
            ttext = ttext + " <|endoftext|>" if "gpt" in self.args.model["decoder"]["text_decoder"] else ttext
            tok = self._encode_padded(ttext, L)
            ids.append(torch.as_tensor(tok["input_ids"]).reshape(-1))
            masks.append(torch.as_tensor(tok["attention_mask"]).reshape(-1))
        return {"input_ids": torch.stack(ids, 0), "attention_mask": torch.stack(masks, 0)}

    # ---- generation ---------------------------------------------------------------------------------------------
    def _dp(self):
        """(rank, world) of the data-parallel group `generate` shards over, (0, 1) when not distributed."""
        import torch.distributed as dist
        # opt-in (the reference has no such behaviour: under torchrun every rank normally holds its OWN examples)
        on = self._data_parallel is True or (self._data_parallel is None and os.environ.get("MELLOW_DATA_PARALLEL") == "1")
        if on and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _check_same_examples(self, examples, extra: bytes = b""):
        """Sharding is only meaningful when every rank was handed the same list: compare (count, content digest) across ranks and
        raise on every rank otherwise (a silent mismatch would return other ranks' texts, or hang in the gather).  The exchange
        runs over the process group's rendezvous store (mellow_amd.dist.agree_on_examples): the token all-gather is the only
        collective of the call."""
        from . import dist as mdist
        mdist.agree_on_examples(mdist.examples_signature(examples) + extra)

    def _clamp_max_len(self, entry_length: int) -> int:
        limit = self.model.max_new_tokens_limit()
        if entry_length > limit:
            # the reference treats max_len as a safety bound (the loop normally ends at the stop token, wrapper.py:247-249)
            warnings.warn(f"max_len {entry_length} exceeds what the engine's KV pages hold (prefix {spec.PREFIX_LEN} + "
                          f"max_len <= {limit + spec.PREFIX_LEN}); clamped to {limit}")
            return limit
        return entry_length

    def _generate_batch(self, audio1, audio2, input_ids, entry_length=300, top_p=0.8, temperature=1.0,
                        stop_token: str = "<|endoftext|>", n_total: Optional[int] = None, do_sample: bool = False,
                        seed: Optional[int] = None, row_offset: int = 0, return_logprobs: bool = False, nseq: int = 1,
                        counts: Optional[Sequence[int]] = None, engine_kw: Optional[dict] = None):
        """Tokens for the rows given (this rank's shard under data parallelism), decoded for ALL `n_total` examples:
        the shards' token ids are all-gathered once (mellow_amd.dist, RCCL over xGMI under backend "nccl").
        nseq > 1: nseq answer rows per example (row_offset counts rows); the result is nested, one list of nseq per example.
        counts (question lists; one rank only): input_ids is [B][Q][text_len], example i asked counts[i] <= Q questions and the
        rest of its Q rows is padding; the result is nested, one list of counts[i] answers per example.
        engine_kw: the Engine.generate keywords of the call's options (repetition controls, guidance; top_logprobs goes only with
        return_logprobs=True); None: none."""
        stop_token_index = self.tokenizer.encode(stop_token)[0]
        entry_length = self._clamp_max_len(int(entry_length))
        rank, world = self._dp()
        n_local = int(audio1.shape[0])
        if n_local:
            samp = dict(do_sample=True, seed=seed, row_offset=row_offset) if do_sample else {}
            samp.update({k: v for k, v in (engine_kw or {}).items() if k != "top_logprobs" or return_logprobs})
            if nseq > 1:
                samp["num_return_sequences"] = nseq
            if return_logprobs:       # (refused under data-parallel sharding by generate(): the gather below carries tokens only)
                toks, lens, steps, ftm, logprobs, *top = self.model.generate(audio1, audio2, input_ids, max_len=entry_length, top_p=top_p,
                                                                             temperature=temperature, stop_id=stop_token_index,
                                                                             return_logprobs=True, **samp)
                self.last_first_token_ms = ftm
                res = self._scored_results(toks, logprobs, stop_token_index, top if samp.get("top_logprobs") else None)
                if counts is not None:
                    return self._per_question(res, counts, int(input_ids.shape[1]))
                return res if nseq == 1 else [res[i:i + nseq] for i in range(0, len(res), nseq)]
            toks, lens, steps, ftm = self.model.generate(audio1, audio2, input_ids, max_len=entry_length, top_p=top_p,
                                                         temperature=temperature, stop_id=stop_token_index, **samp)
            self.last_first_token_ms = ftm
        else:
            toks, lens = np.zeros((0, 0), dtype=np.int32), np.zeros((0,), dtype=np.int32)
        if world > 1:
            import torch.distributed as dist
            from . import dist as mdist
            dev = self.model.tdev if dist.get_backend() == "nccl" else torch.device("cpu")
            if nseq > 1:      # shards are whole examples: every rank's block holds nseq rows per example of a full shard
                toks, lens = mdist.gather_tokens(toks, lens, int(n_total) * nseq, entry_length, device=dev,
                                                 per_rank=nseq * ((int(n_total) + world - 1) // world))
            else:
                toks, lens = mdist.gather_tokens(toks, lens, int(n_total), entry_length, device=dev)
        # -1 = never computed: padding of shards that stopped earlier, or steps after a whole 32-row block had stopped
        rows = [r[r >= 0] for r in toks]
        texts = [self.tokenizer.decode(x).split("<|endoftext|>")[0] for x in rows]
        if counts is not None:
            return self._per_question(texts, counts, int(input_ids.shape[1]))
        return texts if nseq == 1 else [texts[i:i + nseq] for i in range(0, len(texts), nseq)]

    @staticmethod
    def _per_question(rows, counts, Q: int):
        """rows of the padded [B][Q] layout -> per example the answers to its own counts[i] questions (the padding is dropped)"""
        return [rows[i * Q:i * Q + int(c)] for i, c in enumerate(counts)]

    def _scored_results(self, toks, logprobs, stop_id: int, top=None):
        """One dict per row of a generate(return_logprobs=True) call.  The counted tokens are those before the row's first stop id
        plus the stop id itself if the row produced it -- score()'s append_stop=True convention, so `logprob` is the number
        score() gives for `text`; it is their fp32 sum in ascending order.
        top = (top_ids [rows, steps, k], top_logprobs [rows, steps, k]) of a call with top_logprobs=k: every dict gains
        "top_logprobs", one list per counted token of k dicts {"token_id", "token", "logprob"}, best first."""
        out = []
        for i, (r, lp) in enumerate(zip(np.asarray(toks), np.asarray(logprobs, dtype=np.float32))):
            valid = r >= 0                       # -1 = never computed (wrapper docstring): a prefix of the row is valid
            n_valid = int(valid.sum())
            hit = np.nonzero(r[:n_valid] == stop_id)[0]
            n = int(hit[0]) + 1 if hit.size else n_valid
            total = np.float32(0.0)
            for x in lp[:n]:
                total = np.float32(total + x)
            out.append({"text": self.tokenizer.decode(r[valid]).split("<|endoftext|>")[0],
                        "token_ids": [int(t) for t in r[:n]], "token_logprobs": [float(x) for x in lp[:n]],
                        "logprob": float(total), "tokens": n})
            if top is not None:
                ids, tlp = np.asarray(top[0])[i], np.asarray(top[1], dtype=np.float32)[i]
                out[-1]["top_logprobs"] = [[{"token_id": int(t), "token": self.tokenizer.decode([int(t)]), "logprob": float(x)}
                                            for t, x in zip(ids[st], tlp[st])] for st in range(n)]
        return out

    def generate(self, examples, max_len, top_p, temperature, stop_token="<|endoftext|>", audio_resample=True, *,
                 do_sample: bool = False, seed: Optional[int] = None, return_logprobs: bool = False,
                 num_return_sequences: int = 1, num_beams: int = 1, length_penalty: float = 1.0, repetition_penalty: float = 1.0,
                 no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, suppress_tokens: Optional[Sequence[int]] = None,
                 logit_bias: Optional[dict] = None, guidance_scale: float = 1.0, negative_examples=None, top_logprobs: int = 0,
                 top_k: int = 0, min_p: float = 0.0, choices=None, choices_then: str = "stop", stop_strings=None,
                 include_stop_str_in_output: bool = False):
        r"""Produces text response for the given audio files and text prompts
        examples: (list<list>) each example is [audio path 1, audio path 2, text prompt]; the text prompt may be a list or tuple of
                     prompts, several questions about the one pair of clips (module docstring).  If any example has a list, the
                     result holds, per example, a list of answers in question order (one answer for an example with a plain string).
        max_len: (int) maximum length for text generation
        top_p, temperature: accepted for API parity; decoding is greedy (see module docstring) unless do_sample
        do_sample, seed: opt-in seeded nucleus sampling (module docstring); seed=None draws one (kept as `last_seed`)
        stop_token: (str) token used to stop text generation
        audio_resample (bool) True for resampling audio. The model supports only 32 kHz
        return_logprobs: (bool) instead of a string per example return a dict {"text", "token_ids", "token_logprobs", "logprob",
                     "tokens"}: the model's log-probability (its own log-softmax: temperature 1, no nucleus, also when sampling)
                     of every generated token up to and including the stop token, and their sum -- what `score` returns for the
                     same answer, formed inside the decode step.  Not sharded: NotImplementedError with more than one rank.
        num_return_sequences: (int) n > 1 (needs do_sample=True, else ValueError): n sampled answers per example from one encoder
                     pass and one prefill per example; the result holds, per example, a list of n strings (or of n dicts with
                     return_logprobs=True).  1 (default): one answer per example, exactly as without the keyword.
        num_beams: (int) k > 1 (at most 8): beam search with k beams per example from one encoder pass and one prefill per example,
                     deterministic.  The answer is the best hypothesis by score = logprob / tokens ** length_penalty (tokens counts
                     the stop token); with num_return_sequences = m <= k the result holds, per example, a list of the m best, best
                     first.  With return_logprobs=True the dicts also carry "score".  ValueError together with do_sample=True, with
                     a list of prompts, or for m > k; NotImplementedError under data parallelism with more than one rank.
                     1 (default): the call without the keyword.
        length_penalty: (float) exponent of the hypothesis length in the final ranking (0: rank by logprob alone); the beams compete
                     on the raw logprob during the search.
        repetition_penalty: (float) t > 0: the logit of every token the answer already holds is divided by t if positive and
                     multiplied by t if negative, once per distinct token (1, the default: off).
        no_repeat_ngram_size: (int) n > 0: no n-gram of tokens occurs twice in an answer (0: off).
        min_new_tokens: (int) the stop token cannot be chosen before an answer holds this many tokens (0: off).
        suppress_tokens: (list<int>) token ids that are never chosen.
        logit_bias: (dict) {token id: float added to that token's logit}; -inf suppresses the token.
                     These five work with every other keyword (do_sample, return_logprobs, num_return_sequences, question lists,
                     num_beams, data parallelism: the rules are per call and the same on every rank) and run on the device, on the
                     generated tokens of each answer (the prompt is not part of the history).  With any of them set, a returned
                     log-prob is that of the processed distribution the token was chosen from -- no longer what `score` returns.
                     ValueError for t <= 0 or not finite, a negative n or m, an id outside the vocabulary, a NaN or +inf bias, or
                     min_new_tokens > max_len.  All at their defaults: the call without the keywords.
        guidance_scale: (float) s != 1: contrastive (classifier-free) guidance against `negative_examples`.  Every example is run next
                     to its negative; at every step the two log-softmax rows a (example) and b (negative) are combined on the device
                     to b + s * (a - b) and the token is chosen from that, so s > 1 penalises what the model would have said about
                     the negative as well -- its language prior -- and keeps what the clips contributed.  The result has exactly
                     the shape of the un-guided call (strings, or dicts with return_logprobs=True; a log-prob is then that of the
                     combined distribution).  Combines with do_sample / seed, return_logprobs and the five repetition keywords
                     (which run after the guidance).  ValueError together with num_beams > 1, num_return_sequences > 1 or a list of
                     prompts, for a scale that is not finite, for s != 1 without negatives, or for a negatives list of another
                     length; NotImplementedError under data parallelism with more than one rank.  1 (default): the call without
                     the keyword -- nothing is armed and the negatives are ignored.
        negative_examples: a list parallel to `examples` of [audio path 1, audio path 2, prompt], or the string "silence": every
                     example's own prompt over two all-zero clips of the configured length (no file is read).
        top_logprobs: (int) k = 1 .. 20 (needs return_logprobs=True): every result dict gains "top_logprobs", one list per counted
                     token (stop token included) of k dicts {"token_id", "token", "logprob"}, best first: the k likeliest tokens of
                     the distribution that token was chosen from (the model's log-softmax at temperature 1 without the nucleus,
                     after the guidance and the repetition keywords if set), found on the device inside the decode step.  With
                     max_len=1 on a multiple-choice prompt these are the first-token option probabilities.  Works with do_sample,
                     num_return_sequences, question lists, the five repetition keywords and guidance_scale.  ValueError without
                     return_logprobs=True, with num_beams > 1, or for k outside [0, 20].  0 (default): the call without the keyword.
        top_k: (int) K > 0 (needs do_sample=True): only the K likeliest tokens of a step can be drawn (ties on the K-th value are cut
                     by token id, so the set has exactly K members).
        min_p: (float) p in (0, 1] (needs do_sample=True): only tokens whose probability is at least p times the likeliest token's
                     can be drawn, so the set shrinks when the model is confident and widens when it is not.
                     Both run on the device inside the sampler, in Hugging Face's order temperature, top_k, top_p, min_p (the
                     nucleus is taken inside the K tokens), and work with seed, num_return_sequences, question lists, return_logprobs
                     / top_logprobs (which stay the unfiltered log-softmax), the five repetition keywords, guidance_scale and data
                     parallelism (the values are per call and the same on every rank).  ValueError without do_sample=True, with
                     num_beams > 1, for K < 0 or p outside [0, 1].  Both 0 (default -- Hugging Face's top_k = 50 is not adopted):
                     the call without the keywords.
        choices: a list of strings -- the same phrase set for every example -- or a list parallel to `examples` of lists of strings:
                     every answer is exactly one of its example's phrases (with a list of prompts: every answer of the example),
                     followed by the stop token.  The phrases are tokenised with `tokenizer.encode(text)`, as `choose()` tokenises
                     its candidates, and enforced on the device inside the decode step: a token that does not continue a phrase
                     cannot be chosen, whatever chooses it (arg-max, sampler, beam select), after the guidance and the repetition
                     keywords.  With return_logprobs=True the log-probs are those of the constrained distribution: over the phrase
                     set they sum to 1, and they are not what `score` returns.  With num_beams=k and num_return_sequences=m the
                     result is the m likeliest phrases with their probabilities from one decode.  Works with every other keyword
                     and under data parallelism (the sets are sliced with the shard and must be the same on every rank).
                     ValueError for an empty set or an empty string, a per-example list of another length than `examples`, a
                     phrase of more than max_len - 1 tokens (the stop token needs a place; max_len with choices_then="free"), or,
                     with num_beams, num_return_sequences greater than the number of distinct phrases of some example.  min_new_tokens
                     larger than a phrase can leave no allowed token: that stays the caller's error.  None (default): the call
                     without the keyword.
        choices_then: "stop" (default): the answer ends after its phrase.  "free": the set constrains only the start of the answer,
                     which then continues freely up to max_len; a one-phrase set is a forced answer prefix ("The difference is").
        stop_strings: a string or a list of 1 to 16 strings of 1 to 64 bytes each (as UTF-8): an answer ends once its text contains
                     one of them (`stop` of OpenAI and vLLM, `stop_strings` of Hugging Face).  The match runs on the device inside
                     the decode step, on the bytes of the generated tokens: a string across a token boundary or inside a token is
                     found.  The step after the token that completed a match the row's only choice is the stop token (log-prob
                     exactly 0.0), whatever chooses it, so the row ends as at any stop token; this wins over min_new_tokens (as in
                     Hugging Face) and over `choices`.  The table of the vocabulary's bytes is built from the tokenizer on first use
                     (mellow_amd/stop_strings.py vocab_bytes), kept on the wrapper and handed to the engine once.  The text is cut
                     at the start of the first match -- the occurrence that ends first, on equal end the one that starts first --
                     after the cut at `<|endoftext|>`.  With return_logprobs=True every dict gains "stop_reason", the matched
                     string or None, and `logprob` sums over the answer up to the end of the token that completed the match (the
                     forced stop token adds 0.0).  Works with every other keyword and under data parallelism (the strings are per
                     call and must be the same on every rank).  ValueError for an empty list or an empty string, more than 16
                     strings, a string over 64 bytes, or a vocabulary token over 256 bytes.  A tokenizer whose `decode(ids)` is
                     not the concatenation of its per-token texts (one that cleans up spaces, say) can make the device stop where
                     the host text shows no match: that text is returned uncut, with "stop_reason" None.  None (default): the
                     call without the keyword.
        include_stop_str_in_output: keep the matched string at the end of the text (cut at its end, not its start).

        With `data_parallel=True` (or MELLOW_DATA_PARALLEL=1) under an initialised torch.distributed group (one process per
        GPU, every rank calling with the same examples) the examples are sharded contiguously over the ranks, each rank ingests
        and runs only its shard, and every rank returns the full list."""
        audio_paths1, audio_paths2, text_prompts = [], [], []
        for example in examples:
            ap1, ap2, tp = example
            audio_paths1.append(ap1)
            audio_paths2.append(ap2)
            text_prompts.append(tp)
        rules_kw = self._rules_keywords(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, logit_bias, max_len)
        nseq = int(num_return_sequences)
        if nseq < 1:
            raise ValueError(f"num_return_sequences must be >= 1 (got {nseq})")
        k = int(num_beams)
        if k < 1:
            raise ValueError(f"num_beams must be >= 1 (got {k})")
        gscale, negatives = self._guidance_request(guidance_scale, negative_examples, examples, text_prompts, k, nseq)
        engine_kw = dict(rules_kw, **self._top_request(top_logprobs, return_logprobs, k))
        filters_kw = self._filters_request(top_k, min_p, do_sample, k)
        engine_kw.update(filters_kw)
        choices_kw = self._choices_request(choices, choices_then, len(examples), max_len, k, nseq)
        engine_kw.update(choices_kw)
        stop_kw, stop_texts = self._stop_request(stop_strings)
        engine_kw.update(stop_kw)
        # a call with stop strings is the same call, its texts cut at the first stop string on the way out
        finish = (lambda res: self._cut_results(res, stop_texts, bool(include_stop_str_in_output))) if stop_kw else (lambda res: res)
        if k > 1:
            return finish(self._generate_beams(examples, audio_paths1, audio_paths2, text_prompts, max_len, stop_token, audio_resample,
                                               do_sample, return_logprobs, k, nseq, float(length_penalty),
                                               dict(rules_kw, **choices_kw, **stop_kw)))
        if nseq > 1 and not do_sample:
            raise ValueError("num_return_sequences > 1 needs do_sample=True: greedy answers of one example are all the same")
        if nseq > 1024:
            raise ValueError(f"num_return_sequences = {nseq} exceeds the 1024 answer rows one pass of the engine takes")
        rank, world = self._dp()
        if any(isinstance(tp, (list, tuple)) for tp in text_prompts):
            return finish(self._generate_questions(audio_paths1, audio_paths2, text_prompts, max_len, top_p, temperature, stop_token,
                                                   audio_resample, do_sample, seed, return_logprobs, nseq, engine_kw))
        if return_logprobs and world > 1:
            raise NotImplementedError("generate(return_logprobs=True) is not sharded over data-parallel ranks: call it on one rank (or with data_parallel off)")
        n = len(examples)
        if n == 0:          # the reference fails in torch.cat(audio_tensors) (wrapper.py:178) on an empty list
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        extra = b""
        if do_sample:
            if seed is None:
                if world > 1:       # every rank raises here: no rank reaches the agreement or the gather
                    raise ValueError("data_parallel generate(do_sample=True) needs an explicit seed, the same on every rank")
                seed = random.getrandbits(63)
            seed = int(seed)
            self.last_seed = seed
            extra = repr(("sample", seed, float(top_p), float(temperature))).encode()
            if nseq > 1:
                extra += repr(("nseq", nseq)).encode()
        if rules_kw:      # the rules are per call and the same on every rank: a mismatch is refused by the same exchange
            import hashlib
            extra += repr(sorted((k, hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest() if k == "logit_bias" else v)
                                 for k, v in rules_kw.items())).encode()
        if filters_kw:    # likewise
            extra += repr(("filters", filters_kw["top_k"], filters_kw["min_p"])).encode()
        if choices_kw and world > 1:    # likewise: the sets of ALL examples, before the shard is cut
            from .constraint import constraint_digest
            extra += repr(("choices", constraint_digest(choices_kw["constraint"]), choices_kw["constraint_then_free"])).encode()
        if stop_kw:       # likewise
            from .stop_strings import stop_strings_digest
            extra += repr(("stop_strings", stop_strings_digest(stop_kw["stop_strings"]))).encode()
        lo, hi = 0, n
        if world > 1:
            from .dist import shard_range
            self._check_same_examples(examples, extra)      # a sampling mismatch is refused by the same exchange
            lo, hi = shard_range(n, rank, world)
        if hi > lo:
            audio1 = self.preprocess_audio(audio_paths1[lo:hi], resample=audio_resample)
            audio2 = self.preprocess_audio(audio_paths2[lo:hi], resample=audio_resample)
            ids = self.preprocess_text(text_prompts[lo:hi])["input_ids"]
        else:
            audio1 = audio2 = torch.zeros((0, 1))
            ids = torch.zeros((0, spec.TEXT_LEN), dtype=torch.int64)
        if choices_kw:                  # the sets follow their examples into the shard
            engine_kw["constraint"] = choices_kw["constraint"][lo:hi]
        if negatives is not None:       # (one rank: lo, hi = 0, n)
            if negatives == "silence":      # the examples' own prompts over all-zero clips: nothing is read
                neg = (torch.zeros_like(audio1), torch.zeros_like(audio2), ids)
            else:
                neg = (self.preprocess_audio([e[0] for e in negatives], resample=audio_resample),
                       self.preprocess_audio([e[1] for e in negatives], resample=audio_resample),
                       self.preprocess_text([e[2] for e in negatives])["input_ids"])
            engine_kw.update(guidance_scale=gscale, negative=neg)
        return finish(self._generate_batch(audio1, audio2, ids, entry_length=max_len, top_p=top_p,
                                           temperature=temperature, stop_token=stop_token, n_total=n, do_sample=do_sample,
                                           seed=seed, row_offset=lo * nseq, return_logprobs=return_logprobs, nseq=nseq, engine_kw=engine_kw))

    def _stop_request(self, stop_strings):
        """The keyword rules of stop_strings -> ({} for None: the call without it, else the keyword for Engine.generate; the strings
        as text).  The first call with strings builds the vocabulary's byte table and hands it to the engine."""
        if stop_strings is None:
            return {}, []
        texts = [stop_strings] if isinstance(stop_strings, str) else list(stop_strings)
        if len(texts) == 0:
            raise ValueError("stop_strings is an empty list: give at least one string (None is off)")
        for t in texts:
            if not isinstance(t, str):
                raise TypeError(f"a stop string must be a string, got {type(t).__name__}")
            if t == "":
                raise ValueError("stop_strings holds an empty string: every text contains it")
        from .engine import check_stop_strings
        raw = check_stop_strings([t.encode("utf-8") for t in texts])
        if getattr(self, "_vocab_bytes", None) is None:
            from .stop_strings import vocab_bytes
            table = vocab_bytes(self.tokenizer, int(self.model.lm.vocab_size))
            self.model.set_vocab_bytes(*table)
            self._vocab_bytes = table
        return dict(stop_strings=raw), texts

    @staticmethod
    def _cut_results(res, stop_texts, include):
        """every text of a generate() result -- strings or the dicts of return_logprobs=True, flat or nested per example -- cut by
        stop_strings.cut_text; a dict gains "stop_reason", the matched string or None"""
        from .stop_strings import cut_text

        def one(r):
            if isinstance(r, list):
                return [one(x) for x in r]
            if isinstance(r, dict):
                text, why = cut_text(r["text"], stop_texts, include)
                return dict(r, text=text, stop_reason=why)
            return cut_text(r, stop_texts, include)[0]
        return one(res)

    def _choices_request(self, choices, choices_then, n_examples, max_len, k, nseq):
        """The keyword rules of choices / choices_then -> the keywords for Engine.generate ({} for None: the call without them):
        constraint = per example the list of its phrases' token ids, constraint_then_free."""
        if choices_then not in ("stop", "free"):
            raise ValueError(f"choices_then must be 'stop' or 'free', got {choices_then!r}")
        if choices is None:
            return {}
        if isinstance(choices, str):
            raise ValueError("choices is a list of strings, or a list parallel to the examples of lists of strings")
        choices = list(choices)
        if len(choices) == 0:
            raise ValueError("choices is an empty set: a constrained answer needs at least one phrase")
        if all(isinstance(c, str) for c in choices):
            per_example = [choices] * int(n_examples)
        else:
            if any(isinstance(c, str) for c in choices):
                raise ValueError("choices mixes strings and lists: give one flat list of strings, or one list of strings per example")
            per_example = [list(c) for c in choices]
            if len(per_example) != int(n_examples):
                raise ValueError(f"choices holds {len(per_example)} phrase sets for {int(n_examples)} examples: one list per example")
        cache, done, sets = {}, {}, []
        for i, phrases in enumerate(per_example):
            if id(phrases) in done:          # the one flat list of every example: tokenised once, and one object for the trie builder
                sets.append(done[id(phrases)])
                continue
            if len(phrases) == 0:
                raise ValueError(f"choices[{i}] is an empty set: a constrained answer needs at least one phrase")
            row = []
            for text in phrases:
                if not isinstance(text, str):
                    raise TypeError(f"a choice must be a string, got {type(text).__name__}")
                if text not in cache:
                    cache[text] = [int(t) for t in self.tokenizer.encode(text)]       # the convention of _candidate_ids
                if text == "" or not cache[text]:
                    raise ValueError(f"choices[{i}] holds an empty string (or one without tokens): every phrase needs at least one token")
                row.append(cache[text])
            done[id(phrases)] = row
            sets.append(row)
        free = choices_then == "free"
        longest = max(len(p) for row in sets for p in row)
        room = int(max_len) if free else int(max_len) - 1
        if longest > room:
            raise ValueError(f"the longest phrase of choices has {longest} tokens: max_len = {int(max_len)} holds phrases of at most {room}"
                             + ("" if free else " (the stop token needs a place)"))
        if k > 1:
            for i, row in enumerate(sets):
                distinct = len({tuple(p) for p in row})
                if nseq > distinct:
                    raise ValueError(f"num_return_sequences = {nseq} exceeds the {distinct} distinct phrases of choices[{i}]: a constrained "
                                     "beam search has no more finite hypotheses than that")
        from .constraint import check_constraint
        check_constraint(sets)
        return dict(constraint=sets, constraint_then_free=free)

    @staticmethod
    def _filters_request(top_k, min_p, do_sample, k):
        """The keyword rules of top_k / min_p -> the keywords for Engine.generate ({} for both off: the call without them)."""
        from .engine import check_sample_filters
        fk, fp = check_sample_filters(top_k, min_p)
        if not fk and not fp:
            return {}
        if k > 1:
            raise ValueError("top_k / min_p and num_beams > 1 do not combine: they filter a sampled draw, beam search is deterministic")
        if not do_sample:
            raise ValueError("top_k / min_p need do_sample=True: they filter the sampled draw, greedy decoding takes the arg-max whatever they are")
        return dict(top_k=fk, min_p=fp)

    @staticmethod
    def _top_request(top_logprobs, return_logprobs, k):
        """The keyword rules of top_logprobs -> the keyword for Engine.generate ({} for 0: the call without it)."""
        from .engine import check_top_logprobs
        t = check_top_logprobs(top_logprobs)
        if t == 0:
            return {}
        if k > 1:
            raise ValueError("top_logprobs and num_beams > 1 do not combine: top log-probs of a beam hypothesis are not built")
        if not return_logprobs:
            raise ValueError("top_logprobs needs return_logprobs=True: the alternatives are part of the result dicts")
        return dict(top_logprobs=t)

    def _guidance_request(self, guidance_scale, negative_examples, examples, text_prompts, k, nseq):
        """The keyword rules of guidance_scale / negative_examples -> (scale, negatives): negatives is None for an un-guided call
        (scale 1: whatever was given is ignored), else "silence" or the checked list."""
        from .engine import check_guidance_scale
        s = check_guidance_scale(guidance_scale)
        if s == 1.0:
            return s, None
        if k > 1:
            raise ValueError("guidance_scale and num_beams > 1 do not combine: beam search over pairs is not built")
        if nseq > 1:
            raise ValueError("guidance_scale and num_return_sequences > 1 do not combine: repeat the example (and its negative) in the list")
        if any(isinstance(tp, (list, tuple)) for tp in text_prompts):
            raise ValueError("guidance_scale and question lists do not combine: pass an example per question")
        if negative_examples is None:
            raise ValueError(f"guidance_scale = {s} needs negative_examples: a list parallel to the examples, or \"silence\"")
        if isinstance(negative_examples, str):
            if negative_examples != "silence":
                raise ValueError(f"negative_examples = {negative_examples!r}: the only string it takes is \"silence\"")
            negatives = "silence"
        else:
            negatives = [list(e) for e in negative_examples]
            if len(negatives) != len(examples):
                raise ValueError(f"negative_examples holds {len(negatives)} entries for {len(examples)} examples: one negative per example")
            if any(len(e) != 3 or isinstance(e[2], (list, tuple)) for e in negatives):
                raise ValueError("every negative example is [audio path 1, audio path 2, prompt]")
        if self._dp()[1] > 1:
            raise NotImplementedError("guided generation is not sharded over data-parallel ranks: call generate on one rank (or with "
                                      "data_parallel off)")
        return s, negatives

    def _rules_keywords(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, logit_bias, max_len):
        """The repetition controls of a generate() call as keywords of Engine.generate: only those that differ from their neutral
        value, so a call that sets none passes none.  suppress_tokens and logit_bias are merged into one dense vector."""
        from .engine import check_logit_rules
        t, n, m, _ = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        if m > int(max_len):
            raise ValueError(f"min_new_tokens = {m} exceeds max_len = {int(max_len)}")
        kw = {}
        if t != 1.0:
            kw["repetition_penalty"] = t
        if n:
            kw["no_repeat_ngram_size"] = n
        if m:
            kw["min_new_tokens"] = m
        entries = [(tok, val) for tok, val in (logit_bias or {}).items()] + [(tok, -math.inf) for tok in (suppress_tokens or [])]
        if entries:
            lm = getattr(self.model, "lm", None) or LMConfig.load()
            V = int(lm.vocab_size)
            dense = np.zeros((V,), dtype=np.float32)
            for tok, val in entries:
                if isinstance(tok, bool) or int(tok) != tok or not 0 <= int(tok) < V:
                    raise ValueError(f"token id {tok!r} is outside the vocabulary [0, {V})")
                val = float(val)
                if math.isnan(val) or val == math.inf:
                    raise ValueError(f"logit_bias[{int(tok)}] = {val}: values must be finite or -inf")
                dense[int(tok)] += np.float32(val)          # (a suppressed token stays suppressed: -inf + finite = -inf)
            kw["logit_bias"] = dense
        return kw

    def _generate_beams(self, examples, audio_paths1, audio_paths2, text_prompts, max_len, stop_token, audio_resample, do_sample,
                        return_logprobs, k, m, length_penalty, rules_kw):
        """generate(num_beams=k > 1): one engine call on every example; the m best hypotheses per example, best first"""
        from .engine import check_beam_request
        if do_sample:
            raise ValueError("num_beams > 1 and do_sample=True do not combine: beam search is deterministic")
        if any(isinstance(tp, (list, tuple)) for tp in text_prompts):
            raise ValueError("num_beams > 1 and question lists do not combine: ask each question in a call of its own")
        if m > k:
            raise ValueError(f"num_return_sequences = {m} exceeds num_beams = {k}: a beam search ends with k hypotheses")
        if self._dp()[1] > 1:
            raise NotImplementedError("beam search is not sharded over data-parallel ranks: call generate on one rank (or with "
                                      "data_parallel off)")
        n = len(examples)
        if n == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        if getattr(self.model, "precision", None) == "fp8":
            raise ValueError('num_beams > 1 is not available with precision="fp8": the bf16 K/V pages of that mode have no fan-out')
        entry_length = self._clamp_max_len(int(max_len))
        check_beam_request(n, k, entry_length, m)
        stop_id = self.tokenizer.encode(stop_token)[0]
        audio1 = self.preprocess_audio(audio_paths1, resample=audio_resample)
        audio2 = self.preprocess_audio(audio_paths2, resample=audio_resample)
        ids = self.preprocess_text(text_prompts)["input_ids"]
        kw = dict(max_len=entry_length, stop_id=stop_id, num_beams=k, length_penalty=length_penalty, num_return_sequences=m)
        kw.update(rules_kw)
        if return_logprobs:
            toks, lens, steps, ftm, logprobs, scores = self.model.generate(audio1, audio2, ids, return_logprobs=True, **kw)
            res = self._scored_results(toks, logprobs, stop_id)
            for r, sc in zip(res, scores):
                r["score"] = float(sc)
        else:
            toks, lens, steps, ftm = self.model.generate(audio1, audio2, ids, **kw)
            res = [self.tokenizer.decode(x).split("<|endoftext|>")[0] for x in np.asarray(toks)]
        self.last_first_token_ms = ftm
        return res if m == 1 else [res[i:i + m] for i in range(0, len(res), m)]

    def _generate_questions(self, audio_paths1, audio_paths2, text_prompts, max_len, top_p, temperature, stop_token, audio_resample,
                            do_sample, seed, return_logprobs, nseq, engine_kw):
        """generate() with a list of prompts in at least one example.  Every example gets Q = the largest question count of the
        call; one with fewer is padded by repeating its first question (as _candidate_ids pads candidates) and the padded answers
        are dropped.  Answer j of example i is global row i * Q + j of that layout: the row its random stream is keyed by."""
        questions = [list(tp) if isinstance(tp, (list, tuple)) else [tp] for tp in text_prompts]
        if any(len(q) == 0 for q in questions):
            raise ValueError("an example has an empty list of questions")
        if nseq > 1:
            raise ValueError("num_return_sequences > 1 and question lists do not combine: ask the question in a call of its own with "
                             "num_return_sequences, or repeat it in the list")
        rank, world = self._dp()
        if world > 1:
            raise NotImplementedError("question lists are not sharded over data-parallel ranks: call generate on one rank (or with "
                                      "data_parallel off), or pass the pair once per question")
        counts = [len(q) for q in questions]
        B, Q = len(questions), max(counts)
        if Q > 1 and getattr(self.model, "precision", None) == "fp8":
            raise ValueError('question lists are not available with precision="fp8": the bf16 K/V pages of that mode have no fan-out '
                             "(pass the pair once per question instead)")
        if B * Q > 1024:
            raise ValueError(f"{B} examples x {Q} questions = {B * Q} answer rows exceed the 1024 one call takes: split the examples "
                             "over several calls")
        if do_sample:
            seed = random.getrandbits(63) if seed is None else int(seed)
            self.last_seed = seed
        flat = [q[j] if j < len(q) else q[0] for q in questions for j in range(Q)]
        audio1 = self.preprocess_audio(audio_paths1, resample=audio_resample)
        audio2 = self.preprocess_audio(audio_paths2, resample=audio_resample)
        ids = self.preprocess_text(flat)["input_ids"].reshape(B, Q, spec.TEXT_LEN)
        return self._generate_batch(audio1, audio2, ids, entry_length=max_len, top_p=top_p, temperature=temperature,
                                    stop_token=stop_token, n_total=B, do_sample=do_sample, seed=seed, row_offset=0,
                                    return_logprobs=return_logprobs, counts=counts, engine_kw=engine_kw)

    # ---- scoring ------------------------------------------------------------------------------------------------
    def _candidate_ids(self, candidates, append_stop: bool, stop_token: str):
        """candidate strings -> (ids int64 [B][K][L], lengths int32 [B][K], K of every example).  An example with fewer than the
        largest K is padded by repeating its first candidate; ids beyond a candidate's length are 0 (never scored)."""
        stop = int(self.tokenizer.encode(stop_token)[0]) if append_stop else None
        rows, counts = [], []
        for cands in candidates:
            if isinstance(cands, str) or len(cands) == 0:
                raise ValueError("candidates[i] must be a non-empty list of answer strings")
            toks = []
            for text in cands:
                if not isinstance(text, str):
                    raise TypeError(f"a candidate must be a string, got {type(text).__name__}")
                ids = [int(t) for t in self.tokenizer.encode(text)]
                if stop is not None:
                    ids.append(stop)
                if not ids:
                    raise ValueError(f"candidate {text!r} has no tokens (append_stop=False and an empty encoding)")
                toks.append(ids)
            rows.append(toks)
            counts.append(len(toks))
        K = max(counts)
        L = max(len(t) for toks in rows for t in toks)
        limit = self.model.max_candidate_tokens()
        if L > limit:
            # not clamped: a truncated answer has another score
            raise ValueError(f"a candidate has {L} tokens; the engine's KV pages hold prefix {spec.PREFIX_LEN} + at most {limit} "
                             f"candidate tokens (max_positions {limit + spec.PREFIX_LEN})")
        ids = np.zeros((len(rows), K, L), dtype=np.int64)
        lens = np.zeros((len(rows), K), dtype=np.int32)
        for b, toks in enumerate(rows):
            for k in range(K):
                t = toks[k] if k < len(toks) else toks[0]
                ids[b, k, : len(t)] = t
                lens[b, k] = len(t)
        return ids, lens, counts

    def score(self, examples, candidates, append_stop=True, stop_token="<|endoftext|>", audio_resample=True):
        r"""Teacher-forced log-probabilities of given answers
        examples: (list<list>) as in `generate`: [audio path 1, audio path 2, text prompt]
        candidates: (list<list<str>>) candidates[i] = the answer strings to score for example i (any number per example)
        append_stop: (bool) append the stop token's id to every candidate, so that its score includes ending there (what makes
                     answers of different length comparable)
        Returns per example a list, one entry per candidate: {"logprob": sum of the token log-probs, "tokens": how many tokens
        were scored, "token_logprobs": [float per token]}.  The encoder and prefix run once per example, whatever the number of
        candidates.  Not sharded: under data parallelism with more than one rank it raises NotImplementedError."""
        if self._dp()[1] > 1:
            raise NotImplementedError("score() is not sharded over data-parallel ranks: call it on one rank (or with data_parallel off)")
        if len(examples) == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        if len(candidates) != len(examples):
            raise ValueError(f"{len(examples)} examples but {len(candidates)} candidate lists")
        ids, lens, counts = self._candidate_ids(candidates, append_stop, stop_token)
        audio1 = self.preprocess_audio([ex[0] for ex in examples], resample=audio_resample)
        audio2 = self.preprocess_audio([ex[1] for ex in examples], resample=audio_resample)
        prompt_ids = self.preprocess_text([ex[2] for ex in examples])["input_ids"]
        logprob, sums, _ = self.model.score(audio1, audio2, prompt_ids, ids, lens)
        return [[{"logprob": float(sums[b, k]), "tokens": int(lens[b, k]),
                  "token_logprobs": [float(x) for x in logprob[b, k, : lens[b, k]]]} for k in range(counts[b])]
                for b in range(len(examples))]

    def choose(self, examples, candidates, normalize="sum", **score_kwargs):
        """Index of the likeliest candidate of every example (lowest index on ties).  normalize="sum": by the answer's total
        log-probability; "mean": by its log-probability per token."""
        if normalize not in ("sum", "mean"):
            raise ValueError(f"normalize must be 'sum' or 'mean', got {normalize!r}")
        out = []
        for cands in self.score(examples, candidates, **score_kwargs):
            vals = [c["logprob"] / c["tokens"] if normalize == "mean" else c["logprob"] for c in cands]
            out.append(max(range(len(vals)), key=lambda k: (vals[k], -k)))
        return out
