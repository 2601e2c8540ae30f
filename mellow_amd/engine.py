"""ctypes binding of libmellow_hip.so (C ABI in include/mellow_hip.h).

This is the only way Python reaches the hot path.  There is NO CPU fallback: if the shared library is
missing, or no HIP device is visible, constructing an `Engine` raises — the product path never routes
through oracle/ or eager PyTorch.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import spec
from .spec import LMConfig

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libmellow_hip.so")
ABI_VERSION = 2
DEFAULT_PRECISION = "f32x3"      # = MELLOW_PRECISION_F32X3, what mellow_engine_create selects (include/mellow_hip.h)

_F32, _I32, _I64 = 0, 1, 2


class MellowConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("vocab_size", C.c_int32), ("hidden_size", C.c_int32),
        ("intermediate_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
        ("num_kv_heads", C.c_int32), ("head_dim", C.c_int32), ("rms_norm_eps", C.c_float),
        ("rope_theta", C.c_float), ("max_positions", C.c_int32), ("text_len", C.c_int32),
        ("prefix_len", C.c_int32), ("sep_token_id", C.c_int32),
    ]


class LogitRules(C.Structure):
    """mellow_logit_rules_t (include/mellow_hip.h)"""
    _fields_ = [("size", C.c_int32), ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32),
                ("min_new_tokens", C.c_int32), ("logit_bias", C.c_void_p)]


class Constraint(C.Structure):
    """mellow_constraint_t (include/mellow_hip.h)"""
    _fields_ = [("size", C.c_int32), ("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("node_first", C.c_void_p),
                ("node_flags", C.c_void_p), ("edge_token", C.c_void_p), ("edge_child", C.c_void_p), ("n_rows", C.c_int32),
                ("row_root", C.c_void_p), ("then_free", C.c_int32)]


class StopStrings(C.Structure):
    """mellow_stop_strings_t (include/mellow_hip.h)"""
    _fields_ = [("size", C.c_int32), ("n_strings", C.c_int32), ("str_off", C.c_void_p), ("str_bytes", C.c_void_p)]


class SampleFilters(C.Structure):
    """mellow_sample_filters_t (include/mellow_hip.h)"""
    _fields_ = [("size", C.c_int32), ("top_k", C.c_int32), ("min_p", C.c_float)]


class GemmEpi(C.Structure):
    """mellow_gemm_epi_t (include/mellow_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("size", "kernel", "epi", "M", "K", "Nw", "N", "act", "bias", "resid", "rows_in", "rows_out", "ldc",
                                         "want_c", "want_c3", "want_ssq", "rs_parts")] + \
               [("rs_dim", C.c_float), ("rs_eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("splitk_max", "no_x3w", "T", "Tmax", "pos0")]


class DecAttn(C.Structure):
    """mellow_dec_attn_t (include/mellow_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("size", "B", "P", "pos", "Tmax", "ctx_end", "ts", "fused", "kv16", "want_x3")] + [("eps", C.c_float)]


class DecGemv(C.Structure):
    """mellow_dec_gemv_t (include/mellow_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("size", "op", "form", "B", "kcd", "first", "inc_pos", "pos", "Tmax", "want_x3")] + [("eps", C.c_float)]


class DecTail(C.Structure):
    """mellow_dec_tail_t (include/mellow_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("size", "op", "form", "B", "V", "want_logits", "want_sum", "write_x", "with_state", "with_logprob",
                                         "max_len", "stop_id", "T0", "pos", "n_seen", "arrive", "ticket", "n_compactions", "ld", "n_src",
                                         "T_last")]


class EngineError(RuntimeError):
    pass


_lib = None
# symbols added without a new ABI minor (include/mellow_hip.h): detected by lookup, so that a library built before them still loads
_ADDED_UNDER_MINOR_4 = ("mellow_lm_score", "mellow_score", "mellow_generate_scored", "mellow_debug_dec_head_lse", "mellow_generate_n",
                        "mellow_generate_q", "mellow_generate_beam", "mellow_beam_select")
# symbols of minor 5 (the attention taps on host data): looked up the same way, so that a minor-4 library still loads
_ADDED_UNDER_MINOR_5 = ("mellow_debug_prefill_attn", "mellow_debug_window_attn", "mellow_generate_rules", "mellow_logit_rules_apply",
                        "mellow_generate_guidance", "mellow_guidance_apply", "mellow_generate_top_logprobs", "mellow_top_logprobs_apply",
                        "mellow_debug_gemm_epi", "mellow_generate_filters", "mellow_sample_logits_filtered", "mellow_debug_norm",
                        "mellow_debug_dec_attn", "mellow_debug_dec_gemv", "mellow_debug_dec_tail", "mellow_generate_constraint",
                        "mellow_constraint_apply", "mellow_set_vocab_bytes", "mellow_generate_stop_strings", "mellow_stop_strings_apply")


def load_library(path: Optional[str] = None):
    """dlopen libmellow_hip.so and declare every symbol of include/mellow_hip.h.  Raises if missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MELLOW_HIP_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise EngineError(
            f"{p} not found: build it with `python mellow_amd/csrc/build.py` (hipcc, gfx950). "
            "The Mellow engine has no CPU fallback.")
    lib = C.CDLL(p)
    vp, ci, cf, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
    P = C.POINTER
    sig = {
        "mellow_abi_version": (ci, []),
        "mellow_last_error": (C.c_char_p, []),
        "mellow_device_count": (ci, []),
        "mellow_engine_create": (ci, [P(MellowConfig), ci, P(vp)]),
        "mellow_engine_destroy": (None, [vp]),
        "mellow_engine_fork": (ci, [vp, P(vp)]),
        "mellow_engine_load_tensor": (ci, [vp, C.c_char_p, vp, P(i64), ci, ci]),
        "mellow_engine_finalize": (ci, [vp]),
        "mellow_engine_num_required": (ci, []),
        "mellow_engine_required_key": (C.c_char_p, [ci]),
        "mellow_generate": (ci, [vp, vp, vp, i64, vp, ci, ci, cf, cf, ci, ci, vp, P(C.c_int32), P(C.c_int32), P(cf)]),
        "mellow_generate_sampled": (ci, [vp, vp, vp, i64, vp, ci, ci, cf, cf, C.c_uint64, C.c_int32, ci, ci, vp, P(C.c_int32),
                                         P(C.c_int32), P(cf)]),
        "mellow_generate_scored": (ci, [vp, vp, vp, i64, vp, ci, ci, ci, cf, cf, C.c_uint64, C.c_int32, ci, ci, vp, vp, P(C.c_int32),
                                        P(C.c_int32), P(cf)]),
        "mellow_generate_n": (ci, [vp, vp, vp, i64, vp, ci, ci, ci, ci, cf, cf, C.c_uint64, C.c_int32, ci, ci, vp, vp, P(C.c_int32),
                                   P(C.c_int32), P(cf)]),
        "mellow_generate_q": (ci, [vp, vp, vp, i64, vp, ci, ci, ci, ci, cf, cf, C.c_uint64, C.c_int32, ci, ci, vp, vp, P(C.c_int32),
                                   P(C.c_int32), P(cf)]),
        "mellow_generate_beam": (ci, [vp, vp, vp, i64, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, P(C.c_int32), P(cf)]),
        "mellow_beam_select": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]),
        "mellow_sample_logits": (ci, [vp, vp, ci, vp, ci, cf, cf, C.c_uint64, vp]),
        "mellow_generate_filters": (ci, [vp, P(SampleFilters)]),
        "mellow_sample_logits_filtered": (ci, [vp, vp, ci, vp, ci, cf, cf, C.c_uint64, P(SampleFilters), vp]),
        "mellow_generate_rules": (ci, [vp, P(LogitRules)]),
        "mellow_logit_rules_apply": (ci, [vp, P(LogitRules), vp, ci, vp, ci, vp, ci, vp, vp, vp]),
        "mellow_generate_constraint": (ci, [vp, P(Constraint)]),
        "mellow_constraint_apply": (ci, [vp, P(Constraint), vp, ci, vp, ci, vp, ci, vp, vp, vp, vp]),
        "mellow_set_vocab_bytes": (ci, [vp, vp, vp, C.c_int32]),
        "mellow_generate_stop_strings": (ci, [vp, P(StopStrings)]),
        "mellow_stop_strings_apply": (ci, [vp, P(StopStrings), vp, ci, vp, ci, vp, ci, vp, vp, vp, vp]),
        "mellow_generate_guidance": (ci, [vp, cf]),
        "mellow_guidance_apply": (ci, [vp, cf, vp, ci, vp, vp, vp]),
        "mellow_generate_top_logprobs": (ci, [vp, ci, vp, vp]),
        "mellow_top_logprobs_apply": (ci, [vp, vp, vp, vp, ci, ci, vp, vp]),
        "mellow_logmel": (ci, [vp, vp, ci, i64, ci, vp]),
        "mellow_encode": (ci, [vp, vp, ci, i64, vp]),
        "mellow_prefix": (ci, [vp, vp, vp, i64, vp, ci, vp]),
        "mellow_lm_prefill": (ci, [vp, vp, ci, ci, ci, vp]),
        "mellow_lm_decode_step": (ci, [vp, vp, vp]),
        "mellow_argmax": (ci, [vp, vp, ci, vp]),
        "mellow_embed_tokens": (ci, [vp, vp, ci, vp]),
        "mellow_lm_forward_logits": (ci, [vp, vp, ci, ci, ci, vp]),
        "mellow_lm_score": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
        "mellow_score": (ci, [vp, vp, vp, i64, vp, ci, vp, P(C.c_int32), ci, ci, vp, vp, vp]),
        "mellow_resample": (ci, [vp, vp, ci, i64, ci, ci, vp, i64, P(i64)]),
        "mellow_debug_enable_taps": (ci, [vp, ci]),
        "mellow_debug_tap": (ci, [vp, C.c_char_p, vp, i64, P(i64)]),
        "mellow_debug_gemm_fp8": (ci, [vp, vp, ci, ci, vp, ci, vp, ci, vp]),
        "mellow_debug_gemm_f32": (ci, [vp, ci, vp, ci, ci, vp, ci, vp, ci, vp]),
        "mellow_debug_gemm_epi": (ci, [vp, P(GemmEpi), vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64]),
        "mellow_debug_norm": (ci, [vp, ci, ci, vp, ci, ci, vp, vp, cf, vp, ci, ci, ci, vp, i64, vp, i64]),
        "mellow_debug_dec_attn": (ci, [vp, P(DecAttn), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i64,
                                       vp, i64, vp, i64]),
        "mellow_debug_dec_gemv": (ci, [vp, P(DecGemv), vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp,
                                       vp, vp, i64, vp, i64, vp, i64, vp, vp, i64]),
        "mellow_debug_dec_tail": (ci, [vp, P(DecTail), vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, i64, vp, vp,
                                       i64, vp, i64, vp, vp, i64]),
        "mellow_debug_prefill_attn": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, i64]),
        "mellow_debug_window_attn": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, vp, i64]),
        "mellow_debug_dec_head": (ci, [vp, vp, ci, ci, vp]),
        "mellow_debug_dec_head_lse": (ci, [vp, vp, ci, ci, vp, vp, vp, vp]),
        "mellow_prof_enable": (ci, [vp, ci]),
        "mellow_prof_reset": (ci, [vp]),
        "mellow_prof_num_families": (ci, []),
        "mellow_prof_family_name": (C.c_char_p, [ci]),
        "mellow_prof_get": (ci, [vp, ci, P(i64), P(C.c_double), P(C.c_double), P(C.c_double)]),
        "mellow_last_phase_ms": (ci, [vp, P(cf), P(cf), P(cf)]),
        "mellow_last_steps_enqueued": (ci, [vp]),
        "mellow_last_row_repacks": (ci, [vp]),
        "mellow_stft_is_fft": (ci, [vp]),
        "mellow_prefill_parts": (ci, [vp]),
        "mellow_abi_minor": (ci, []),
        "mellow_engine_set_precision": (ci, [vp, ci]),
        "mellow_engine_set_option": (ci, [vp, C.c_char_p, C.c_char_p]),
        "mellow_engine_describe": (i64, [vp, C.c_char_p, i64]),
        "mellow_set_graph": (ci, [vp, ci]),
        "mellow_host_window_map": (ci, [ci, ci, P(C.c_int32)]),
        "mellow_host_pack_weight": (ci, [P(cf), ci, ci, ci, P(cf), i64]),
        "mellow_host_rope_tables": (ci, [cf, ci, ci, P(cf), P(cf)]),
    }
    for name, (res, args) in sig.items():
        if name in _ADDED_UNDER_MINOR_4 + _ADDED_UNDER_MINOR_5 and not hasattr(lib, name):
            continue                     # an older library: the Engine methods that need the symbol raise when called
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.mellow_abi_version() != ABI_VERSION:
        raise EngineError(f"ABI mismatch: library {lib.mellow_abi_version()}, binding {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "mellow_abi_version", "mellow_last_error", "mellow_device_count", "mellow_engine_create",
    "mellow_engine_destroy", "mellow_engine_fork", "mellow_engine_load_tensor", "mellow_engine_finalize",
    "mellow_engine_num_required", "mellow_engine_required_key", "mellow_generate", "mellow_generate_sampled", "mellow_sample_logits", "mellow_logmel",
    "mellow_encode", "mellow_prefix", "mellow_lm_prefill", "mellow_lm_decode_step", "mellow_argmax", "mellow_embed_tokens", "mellow_lm_forward_logits",
    "mellow_lm_score", "mellow_score", "mellow_generate_scored", "mellow_debug_dec_head_lse", "mellow_generate_n", "mellow_generate_q",
    "mellow_generate_beam", "mellow_beam_select", "mellow_generate_rules", "mellow_logit_rules_apply", "mellow_generate_constraint", "mellow_constraint_apply", "mellow_set_vocab_bytes", "mellow_generate_stop_strings", "mellow_stop_strings_apply", "mellow_generate_guidance", "mellow_guidance_apply", "mellow_generate_top_logprobs", "mellow_top_logprobs_apply", "mellow_generate_filters", "mellow_sample_logits_filtered", "mellow_debug_enable_taps", "mellow_debug_tap", "mellow_prof_enable", "mellow_prof_reset",
    "mellow_prof_num_families", "mellow_prof_family_name", "mellow_prof_get", "mellow_last_phase_ms", "mellow_last_steps_enqueued", "mellow_last_row_repacks", "mellow_stft_is_fft", "mellow_prefill_parts", "mellow_abi_minor",
    "mellow_resample", "mellow_engine_set_precision", "mellow_engine_set_option", "mellow_engine_describe", "mellow_debug_gemm_fp8", "mellow_debug_gemm_f32", "mellow_debug_gemm_epi", "mellow_debug_norm", "mellow_debug_dec_attn", "mellow_debug_dec_gemv", "mellow_debug_dec_tail", "mellow_debug_prefill_attn", "mellow_debug_window_attn", "mellow_debug_dec_head", "mellow_set_graph", "mellow_host_window_map", "mellow_host_pack_weight", "mellow_host_rope_tables",
)


def hf_rope_tables(max_pos: int, head_dim: int, theta: float):
    """cos/sin [max_pos][head_dim/2] computed exactly the way transformers' LlamaRotaryEmbedding does
    (fp32 inv_freq, fp32 outer product, fp32 cos/sin) so the engine uses bit-identical tables."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    pos = torch.arange(max_pos, dtype=torch.float32)
    freqs = (inv_freq[None, :, None].float() @ pos[None, None, :].float()).transpose(1, 2)[0]
    return freqs.cos().contiguous().numpy(), freqs.sin().contiguous().numpy()


def _seed64(seed) -> int:
    """a sampling seed as the u64 the C ABI takes (any Python int, taken modulo 2^64); None is an error"""
    if seed is None:
        raise ValueError("do_sample needs an integer seed")
    return int(seed) & 0xFFFFFFFFFFFFFFFF


NSEQ_PASS_ROWS = 1024      # answer rows one mellow_generate_n call takes (B * n)


def plan_nseq_passes(B: int, n: int, row_offset: int = 0):
    """The consecutive mellow_generate_n calls that answer B examples with n rows each: [(lo, hi, row_offset)] -- examples
    [lo, hi) of at most 1024 // n per call, with the random-stream offset of the call's first row (the caller's row_offset plus
    n per example before it), so that the rows are those of one call on every example given n times in a row."""
    B, n, row_offset = int(B), int(n), int(row_offset)
    if n < 1:
        raise ValueError(f"num_return_sequences must be >= 1 (got {n})")
    if n > NSEQ_PASS_ROWS:
        raise ValueError(f"num_return_sequences = {n} exceeds the {NSEQ_PASS_ROWS} answer rows one pass of the engine takes")
    per = NSEQ_PASS_ROWS // n
    return [(lo, min(B, lo + per), row_offset + lo * n) for lo in range(0, B, per)]


RULES_MAX_LEN = 8192           # max_len of a call with logit rules (the history one row stages)


def check_logit_rules(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, logit_bias=None, vocab: Optional[int] = None):
    """The value rules of the repetition controls that need no engine (the C entry repeats the first three).  -> (penalty, n, m,
    bias as a dense float32 [vocab] array or None)."""
    import math
    t = float(repetition_penalty)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError(f"repetition_penalty must be finite and > 0 (got {repetition_penalty}); 1 is off")
    n, m = int(no_repeat_ngram_size), int(min_new_tokens)
    if n < 0:
        raise ValueError(f"no_repeat_ngram_size must be >= 0 (got {n}); 0 is off")
    if m < 0:
        raise ValueError(f"min_new_tokens must be >= 0 (got {m}); 0 is off")
    bias = None
    if logit_bias is not None:
        bias = np.ascontiguousarray(torch.as_tensor(logit_bias).detach().cpu().numpy() if isinstance(logit_bias, torch.Tensor)
                                    else logit_bias, dtype=np.float32).reshape(-1)
        if vocab is not None and bias.shape[0] != int(vocab):
            raise ValueError(f"logit_bias must hold one value per token of the vocabulary ({int(vocab)}), got {bias.shape[0]}")
        if np.isnan(bias).any() or np.isposinf(bias).any():
            raise ValueError("logit_bias values must be finite or -inf (NaN and +inf are refused)")
    return t, n, m, bias


def check_guidance_scale(guidance_scale=1.0) -> float:
    """The one value rule of contrastive guidance (the C entry repeats it): a finite scale.  1 is off."""
    import math
    s = float(guidance_scale)
    if not math.isfinite(s):
        raise ValueError(f"guidance_scale must be finite (got {guidance_scale}); 1 is off")
    return s


TOP_LOGPROBS_MAX_K = 20        # alternatives per step mellow_generate_top_logprobs records


def check_top_logprobs(top_logprobs=0) -> int:
    """The one value rule of top_logprobs (the C entry repeats it): 0 (off) to 20 alternatives per step."""
    k = int(top_logprobs)
    if k < 0 or k > TOP_LOGPROBS_MAX_K:
        raise ValueError(f"top_logprobs must be 0 (off) to {TOP_LOGPROBS_MAX_K} (got {top_logprobs})")
    return k


def check_sample_filters(top_k=0, min_p=0.0):
    """The value rules of the sampler's candidate filters (the C entry repeats them): top_k >= 0 (0 is off), min_p in [0, 1] (0 is
    off).  -> (top_k, min_p)"""
    k, p = int(top_k), float(min_p)
    if k != top_k:
        raise ValueError(f"top_k must be an integer >= 0 (got {top_k}); 0 is off")
    if k < 0:
        raise ValueError(f"top_k must be >= 0 (got {top_k}); 0 is off")
    if k > 0x7fffffff:
        k = 0x7fffffff                 # (any K >= the vocabulary keeps every token)
    if not (0.0 <= p <= 1.0):
        raise ValueError(f"min_p must be in [0, 1] (got {min_p}); 0 is off")
    return k, p


STOP_MAX_STRINGS, STOP_MAX_STR_LEN, STOP_MAX_TOKEN_BYTES = 16, 64, 256      # what mellow_generate_stop_strings / mellow_set_vocab_bytes take


def check_stop_strings(stop_strings) -> List[bytes]:
    """The value rules of stop_strings (the C entry repeats them): a list of 1 to 16 byte strings of 1 to 64 bytes each.  -> the
    strings as bytes objects."""
    if isinstance(stop_strings, (str, bytes, bytearray)) or stop_strings is None:
        raise ValueError("stop_strings is a list of byte strings")
    out = []
    for b in stop_strings:
        if isinstance(b, str) or not isinstance(b, (bytes, bytearray, memoryview, np.ndarray)):
            raise ValueError(f"a stop string is a bytes object (encode text as UTF-8), got {type(b).__name__}")
        out.append(bytes(b))
    if not 1 <= len(out) <= STOP_MAX_STRINGS:
        raise ValueError(f"stop_strings holds {len(out)} strings: a call takes 1 to {STOP_MAX_STRINGS}")
    for j, b in enumerate(out):
        if not 1 <= len(b) <= STOP_MAX_STR_LEN:
            raise ValueError(f"stop string {j} has {len(b)} bytes: a string has 1 to {STOP_MAX_STR_LEN}")
    return out


def check_vocab_bytes(offsets, data, vocab: int):
    """The value rules of a vocabulary byte table (the C entry repeats them) -> (offsets int32 [vocab + 1], data uint8)."""
    off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int64).reshape(-1)
    dat = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)).reshape(-1)
    if off.shape[0] != int(vocab) + 1:
        raise ValueError(f"vocabulary bytes: {off.shape[0]} offsets, the table has vocab + 1 = {int(vocab) + 1}")
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != dat.shape[0]:
        raise ValueError("vocabulary bytes: the offsets start at 0, never decrease and end at the number of bytes")
    ln = np.diff(off)
    if ln.size and int(ln.max()) > STOP_MAX_TOKEN_BYTES:
        t = int(ln.argmax())
        raise ValueError(f"vocabulary bytes: token {t} has {int(ln[t])} bytes, a token has at most {STOP_MAX_TOKEN_BYTES}")
    return off.astype(np.int32), dat


class _CallStopStrings:
    """The stop strings of one generate() call as the arrays of mellow_stop_strings_t (it keeps them alive while the struct points
    at them)."""
    __slots__ = ("strings", "off", "data", "struct")

    def __init__(self, stop_strings):
        self.strings = check_stop_strings(stop_strings)
        self.off = np.zeros(len(self.strings) + 1, dtype=np.int32)
        self.off[1:] = np.cumsum([len(b) for b in self.strings])
        self.data = np.frombuffer(b"".join(self.strings), dtype=np.uint8).copy()
        self.struct = StopStrings(size=C.sizeof(StopStrings), n_strings=len(self.strings), str_off=self.off.ctypes.data,
                                  str_bytes=self.data.ctypes.data)


BEAM_MAX_K = 8                 # beams per example mellow_generate_beam takes
BEAM_STAGE_ROWS = 65536        # B * k * max_len its K/V staging takes (1.5 GB per tensor)


def check_beam_request(B: int, k: int, max_len: int, m: int = 1):
    """the argument rules of a beam call that need no engine (the C entry repeats the first three)"""
    B, k, max_len, m = int(B), int(k), int(max_len), int(m)
    if k < 1 or k > BEAM_MAX_K:
        raise ValueError(f"num_beams must be 1 .. {BEAM_MAX_K} (got {k})")
    if m < 1 or m > k:
        raise ValueError(f"num_return_sequences must be 1 .. num_beams = {k} with beam search (got {m})")
    if B * k > NSEQ_PASS_ROWS:
        raise ValueError(f"{B} examples x {k} beams = {B * k} rows exceed the {NSEQ_PASS_ROWS} one call takes: split the examples "
                         "over several calls")
    if k > 1 and B * k * max_len > BEAM_STAGE_ROWS:
        raise ValueError(f"{B} examples x {k} beams x max_len {max_len} = {B * k * max_len} exceeds the {BEAM_STAGE_ROWS} rows x "
                         "positions of K/V one beam call stages (1.5 GB per tensor): split the examples or lower max_len")


def backtrack_beams(parent, token, lp, k: int):
    """The sequences a beam search ended with, from its tables.  parent / token int [steps][N] and lp float [steps][N] as
    mellow_generate_beam records them (N = B * k, row b * k + j = beam j of example b; parent[s][r] = the beam INDEX 0 .. k - 1
    inside r's example that row r continued at step s).  -> (tokens int32 [N][steps], token_logprobs float64 [N][steps]): row r is
    the history of the beam that sits in row r after the last step."""
    parent, token, lp = np.asarray(parent), np.asarray(token), np.asarray(lp, dtype=np.float64)
    steps, N = token.shape
    k = int(k)
    if k < 1 or N % k != 0 or parent.shape != token.shape or lp.shape != token.shape:
        raise ValueError(f"tables of shape {parent.shape} / {token.shape} / {lp.shape} are not [steps][B * {k}]")
    if steps and (int(parent.min()) < 0 or int(parent.max()) >= k):
        raise ValueError(f"a parent index outside 0 .. {k - 1}")
    toks = np.zeros((N, steps), dtype=np.int32)
    lps = np.zeros((N, steps), dtype=np.float64)
    base = np.arange(N) // k * k
    cur = np.arange(N)
    for s in range(steps - 1, -1, -1):
        toks[:, s] = token[s, cur]
        lps[:, s] = lp[s, cur]
        cur = base + parent[s, cur]
    return toks, lps


def rank_beams(tokens, token_logprobs, cum, k: int, stop_id: int, length_penalty: float = 1.0, ignore_stop: bool = False):
    """The final ranking of a beam search, on the host in fp64: tokens [N][steps] / token_logprobs [N][steps] from backtrack_beams,
    cum [N] the hypotheses' summed log-probs.  A hypothesis holds its tokens up to and INCLUDING its first stop id (or all `steps`);
    score = logprob / tokens ** length_penalty; an example's hypotheses are sorted by score descending, then beam index.
    -> (order int [B][k] of beam indices, lengths int32 [N] = tokens before the stop id, counts int32 [N] = tokens of the hypothesis,
    scores float64 [N]), the last three by row."""
    tokens = np.asarray(tokens)
    N, steps = tokens.shape
    k = int(k)
    lengths = np.full((N,), steps, dtype=np.int32)
    if not ignore_stop:
        hit = tokens == int(stop_id)
        lengths = np.where(hit.any(axis=1), hit.argmax(axis=1), steps).astype(np.int32)
    counts = np.minimum(lengths + 1, steps).astype(np.int32)
    scores = np.asarray(cum, dtype=np.float64) / np.maximum(counts, 1).astype(np.float64) ** float(length_penalty)
    order = np.zeros((N // k, k), dtype=np.int64)
    for b in range(N // k):
        sc = scores[b * k:(b + 1) * k]
        order[b] = sorted(range(k), key=lambda j: (-sc[j] if sc[j] == sc[j] else np.inf, j))      # (a NaN score ranks last)
    return order, lengths, counts, scores


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def has_question_axis(input_ids) -> bool:
    """input_ids is [B][Q][text_len]: several questions per example"""
    return (input_ids.ndim if hasattr(input_ids, "ndim") else np.ndim(input_ids)) == 3


class _CallOptions:
    """What one generate() call arms before EVERY C call it makes (an armed record serves the next mellow_generate* call only): the
    rules struct or None (it keeps its bias vector alive), the guidance scale or None, the k of top_logprobs, the sampler's filters
    struct (top_k / min_p of the draw) or None, the constraint (_CallConstraint) or None, the stop strings (_CallStopStrings) or None.
    Built once per call and handed to the route that runs it; nothing of a call is kept on the engine."""
    __slots__ = ("rules", "guide", "top_k", "filters", "constraint", "stop")

    def __init__(self, rules, guide, top_k, filters=None, constraint=None, stop=None):
        self.rules, self.guide, self.top_k, self.filters, self.constraint, self.stop = rules, guide, top_k, filters, constraint, stop

    def expand_constraint(self, examples: int, per_example: int):
        """the route knows its rows: `per_example` consecutive answer rows of every example carry the example's root"""
        if self.constraint is not None:
            self.constraint.expand(examples, per_example)

    def arm(self, engine, top, row0: int = 0, rows: Optional[int] = None):
        """arm the engine's context for its next C call; top = the rows of the top record that call fills (ids, log-probs), or None;
        rows [row0, row0 + rows) of the generate() call are the rows of that C call (the constraint arms their roots)"""
        if self.constraint is not None:
            engine._chk(engine.lib.mellow_generate_constraint(engine.h, C.byref(self.constraint.struct(row0, rows))))
        if self.stop is not None:
            engine._chk(engine.lib.mellow_generate_stop_strings(engine.h, C.byref(self.stop.struct)))
        if self.rules is not None:
            engine._chk(engine.lib.mellow_generate_rules(engine.h, C.byref(self.rules)))
        if self.guide is not None:
            engine._chk(engine.lib.mellow_generate_guidance(engine.h, float(self.guide)))
        if self.top_k and top is not None:
            engine._chk(engine.lib.mellow_generate_top_logprobs(engine.h, int(self.top_k), _ptr(top[0]), _ptr(top[1])))
        if self.filters is not None:
            engine._chk(engine.lib.mellow_generate_filters(engine.h, C.byref(self.filters)))


class _CallConstraint:
    """The constraint of one generate() call: the trie arrays of constraint.build_trie over the EXAMPLES' phrase sets (it keeps them
    alive while a struct points at them) and, once the route has expanded them, the root of every answer row."""
    __slots__ = ("trie", "then_free", "roots", "_struct")

    def __init__(self, phrases_per_example, then_free: bool, vocab: int):
        from .constraint import build_trie
        self.trie = build_trie(phrases_per_example, vocab)
        self.then_free, self.roots, self._struct = bool(then_free), None, None

    def expand(self, examples: int, per_example: int):
        ex = self.trie["row_root"]
        if ex.shape[0] != int(examples):
            raise ValueError(f"constraint holds {ex.shape[0]} phrase sets for {int(examples)} examples: one set per example")
        self.roots = np.ascontiguousarray(np.repeat(ex, int(per_example)), dtype=np.int32)

    def struct(self, row0: int = 0, rows: Optional[int] = None) -> "Constraint":
        assert self.roots is not None, "the route has not expanded the constraint to its rows"
        t = self.trie
        rows = self.roots.shape[0] - row0 if rows is None else int(rows)
        assert 0 <= row0 and row0 + rows <= self.roots.shape[0], (row0, rows, self.roots.shape)
        self._struct = Constraint(size=C.sizeof(Constraint), n_nodes=t["node_flags"].shape[0], n_edges=t["edge_token"].shape[0],
                                  node_first=t["node_first"].ctypes.data, node_flags=t["node_flags"].ctypes.data,
                                  edge_token=t["edge_token"].ctypes.data, edge_child=t["edge_child"].ctypes.data, n_rows=rows,
                                  row_root=self.roots.ctypes.data + 4 * int(row0), then_free=1 if self.then_free else 0)
        return self._struct


from .taps import DebugTaps      # noqa: E402  (behind the structures above, which its methods fill in)


class Engine(DebugTaps):
    """One engine per device.  Inputs/outputs are torch tensors on that device (plumbing only).  The debug_* methods (the launch
    taps of include/mellow_hip.h) are the DebugTaps mixin, taps.py."""

    def __init__(self, lm: Optional[LMConfig] = None, device: int = 0, max_positions: Optional[int] = None,
                 precision: Optional[str] = None, options: Optional[Dict[str, int]] = None):
        self.lib = load_library()
        if self.lib.mellow_device_count() <= 0:
            raise EngineError("no HIP device visible: the Mellow engine needs an MI355X (no CPU fallback)")
        self.lm = lm or LMConfig.load()
        self.device = int(device)
        self.tdev = torch.device(f"cuda:{self.device}")
        # positions the KV pages / RoPE tables may reach: the LM's own limit (8192 for SmolLM2-135M) unless the caller asks for
        # less -- the reference's loop is bounded by nothing else (wrapper.py:216, decoder.py:25)
        max_positions = int(max_positions) if max_positions else int(self.lm.max_position_embeddings)
        cfg = MellowConfig(
            abi_version=ABI_VERSION, vocab_size=self.lm.vocab_size, hidden_size=self.lm.hidden_size,
            intermediate_size=self.lm.intermediate_size, num_layers=self.lm.num_hidden_layers,
            num_heads=self.lm.num_attention_heads, num_kv_heads=self.lm.num_key_value_heads,
            head_dim=self.lm.head_dim, rms_norm_eps=self.lm.rms_norm_eps, rope_theta=self.lm.rope_theta,
            max_positions=int(max_positions), text_len=spec.TEXT_LEN, prefix_len=spec.PREFIX_LEN,
            sep_token_id=0)
        self.cfg = cfg
        h = C.c_void_p()
        self._chk(self.lib.mellow_engine_create(C.byref(cfg), self.device, C.byref(h)))
        self.h = h
        self.finalized = False
        # "f32x3" (default, = the library's default and the mode bench.py reports): fp32-accurate GEMMs as exact 3-way bf16 splits
        # on the bf16 MFMA pipe.  "f32": exact fp32 MFMA GEMMs.  "fp8": BASELINE config 5 (e4m3 GEMMs, not bit-exact).
        # The parity suite runs "f32x3" and "f32" with the same tolerances and exact tokens.  MELLOW_PRECISION overrides the default.
        precision = precision or os.environ.get("MELLOW_PRECISION") or DEFAULT_PRECISION
        if precision not in ("f32", "fp8", "f32x3"):
            raise ValueError(f"unknown precision {precision!r}")
        self.precision = precision
        self._chk(self.lib.mellow_engine_set_precision(self.h, {"f32": 0, "fp8": 1, "f32x3": 2}[precision]))
        # explicit configuration (include/mellow_hip.h: mellow_engine_set_option): the library reads no environment variable; the
        # A/B forms the tests and tools compare are selected here, by name, and show up in describe()["non_default"]
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, key: str, value) -> None:
        self._chk(self.lib.mellow_engine_set_option(self.h, key.encode(), str(int(value)).encode()))

    def describe(self) -> dict:
        """the engine's resolved configuration (mellow_engine_describe): precision, every option with value / default, ABI"""
        import json
        n = int(self.lib.mellow_engine_describe(self.h, None, 0))
        buf = C.create_string_buffer(n)
        self.lib.mellow_engine_describe(self.h, buf, n)
        return json.loads(buf.value.decode())

    # ---- errors ------------------------------------------------------------------------------------
    def _chk(self, rc: int):
        if rc != 0:
            msg = self.lib.mellow_last_error().decode("utf-8", "replace")
            if msg.startswith("index out of range in self"):      # the reference's embedding lookup raises IndexError with this text
                raise IndexError(msg)
            raise EngineError(msg)

    def _need(self, symbol: str):
        if not hasattr(self.lib, symbol):
            raise EngineError(f"this libmellow_hip.so predates {symbol}: rebuild it with `python mellow_amd/csrc/build.py`")

    def close(self):
        if getattr(self, "h", None):
            for f in getattr(self, "_forks", []):
                f.close()
            self.lib.mellow_engine_destroy(self.h)
            self.h = None

    def fork(self) -> "Engine":
        """Another execution context on the same device sharing this engine's weights (mellow_engine_fork): own stream, KV pages,
        workspaces and graphs; calls on the two objects may overlap from different threads.  Closed with (or before) its parent."""
        if not self.finalized:
            raise EngineError("fork needs a loaded engine")
        c = object.__new__(Engine)
        c.lib, c.lm, c.device, c.tdev, c.cfg, c.precision, c.finalized = self.lib, self.lm, self.device, self.tdev, self.cfg, self.precision, True
        h = C.c_void_p()
        self._chk(self.lib.mellow_engine_fork(self.h, C.byref(h)))
        c.h = h
        c._parent = self              # keeps the weights alive
        self._forks = getattr(self, "_forks", []) + [c]
        return c

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -----------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Mirror of `model.load_state_dict` (reference wrapper.py:74-82): every tensor goes to the engine
        under its reference key; a leading 'module.' is stripped by the engine."""
        for k, v in sd.items():
            t = v.detach().cpu().contiguous()
            if t.dtype == torch.float32:
                dt = _F32
            elif t.dtype == torch.int64:
                dt = _I64
            elif t.dtype == torch.int32:
                dt = _I32
            else:
                t, dt = t.float(), _F32
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            rc = self.lib.mellow_engine_load_tensor(self.h, k.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), dt)
            if rc != 0 and strict:
                self._chk(rc)
        cos, sin = hf_rope_tables(self.cfg.max_positions, self.lm.head_dim, self.lm.rope_theta)
        for name, arr in (("mellow.rope_cos", cos), ("mellow.rope_sin", sin)):
            shape = (C.c_int64 * 2)(*arr.shape)
            self._chk(self.lib.mellow_engine_load_tensor(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), shape, 2, _F32))
        self._chk(self.lib.mellow_engine_finalize(self.h))
        self.finalized = True

    def required_keys(self):
        n = self.lib.mellow_engine_num_required()
        return [self.lib.mellow_engine_required_key(i).decode() for i in range(n)]

    # ---- helpers -----------------------------------------------------------------------------------
    def _f32(self, x) -> torch.Tensor:
        t = torch.as_tensor(x)
        return t.to(device=self.tdev, dtype=torch.float32).contiguous()

    def _i32(self, x) -> torch.Tensor:
        t = torch.as_tensor(x)
        return t.to(device=self.tdev, dtype=torch.int32).contiguous()

    def _ids(self, x) -> torch.Tensor:
        """token ids -> int32 on the device; ids outside the vocabulary raise like the reference's embedding lookup
        (`lm.model.embed_tokens`, decoder.py:47 / wrapper.py:237) instead of reaching a kernel."""
        t = torch.as_tensor(x)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.lm.vocab_size):
            raise IndexError("index out of range in self")
        return t.to(device=self.tdev, dtype=torch.int32).contiguous()

    def _prompt_ids(self, x) -> torch.Tensor:
        """prompt ids -> int32 on the device with NO torch kernel and NO synchronisation when they already are device int32 (the
        timed path of bench.py): their range is checked on the device by prefix_assemble_kernel, which flags the call's error word;
        the C call then fails with the reference's IndexError text.  Host arrays (what a tokenizer returns) are checked right here
        in numpy; a device tensor of another dtype is clamped to [-1, vocab] before it is narrowed, so an out-of-range 64-bit id
        cannot alias a valid 32-bit one."""
        t = torch.as_tensor(x)
        if t.device.type == "cpu":
            a = t.numpy()
            if a.size and (int(a.min()) < 0 or int(a.max()) >= self.lm.vocab_size):
                raise IndexError("index out of range in self")
        elif t.dtype != torch.int32:
            t = t.clamp(-1, self.lm.vocab_size)
        return t.to(device=self.tdev, dtype=torch.int32).contiguous()

    def _sync_inputs(self):
        """The engine runs on its own non-blocking HIP stream: device tensors produced by still-running torch kernels
        (resample / tile / cat on torch's current stream) must be complete before their raw pointers cross the C ABI."""
        torch.cuda.current_stream(self.tdev).synchronize()

    def max_new_tokens_limit(self) -> int:
        """largest max_len the KV pages / RoPE tables of this engine can hold"""
        return int(self.cfg.max_positions) - spec.PREFIX_LEN

    # ---- hot path ----------------------------------------------------------------------------------
    def generate(self, audio1, audio2, input_ids, max_len: int, top_p: float = 0.8, temperature: float = 1.0,
                 stop_id: int = 0, ignore_stop: bool = False, do_sample: bool = False, seed: Optional[int] = None,
                 row_offset: int = 0, return_logprobs: bool = False, num_return_sequences: int = 1,
                 num_beams: Optional[int] = None, length_penalty: float = 1.0, repetition_penalty: float = 1.0,
                 no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, logit_bias=None, _arm_neutral_rules: bool = False,
                 guidance_scale: float = 1.0, negative=None, keep_negative_rows: bool = False, top_logprobs: int = 0,
                 top_k: int = 0, min_p: float = 0.0, constraint=None, constraint_then_free: bool = False, stop_strings=None):
        """-> (tokens int32 [B, steps] on host, lengths [B], steps, first_token_ms)
        num_return_sequences = n > 1 (needs do_sample=True): n sampled answers per example from one encode and one prefill per
        example (mellow_generate_n).  Every array has B * n rows, row b * n + j = answer j of example b, and holds what this call
        returns for every example given n times in a row with the same seed and row_offset (bit-equal in "f32").  More than
        1024 rows run as consecutive calls of 1024 // n examples; n > 1024 is a ValueError.
        return_logprobs=True appends a fifth value, logprobs float32 [B, steps]: the model's log-softmax (temperature 1, no
        nucleus, also when sampling) at every recorded token, formed inside the decode step (mellow_generate_scored); exactly
        0.0 where tokens is -1.  Tokens, lengths and steps are the same either way.
        first_token_ms is measured from the C entry (inputs on the device); `last_first_token_host_ms` adds the time this
        call spent bringing host arrays to the device (latency from audio in HOST memory).
        do_sample=False (default): greedy, the reference's result for every top_p / temperature.  do_sample=True: seeded
        nucleus sampling (include/mellow_hip.h mellow_generate_sampled); row b draws from the stream of global row
        row_offset + b, so a shard or batch given its first row's offset reproduces the rows of one big call.
        input_ids of shape [B][Q][text_len] (3-D): Q questions about every example from one encode and one prefill of the clips'
        positions per example (mellow_generate_q).  Every array has B * Q rows, row b * Q + j = question j of example b, and holds
        what this call returns for the B * Q expanded examples (audio rows repeated Q times, ids flattened) with the same seed and
        row_offset (bit-equal in "f32").  At most 1024 rows per call; not together with num_return_sequences > 1.
        num_beams = k (1 .. 8; None: not a beam call): beam search (mellow_generate_beam; include/mellow_hip.h states the search).
        The m = num_return_sequences <= k best hypotheses per example are returned, m rows per example, best first: an example's
        hypotheses are ranked by score = logprob / tokens ** length_penalty (tokens counts the stop id), then beam index.  tokens
        [B * m, steps] hold a hypothesis up to its stop id and the stop id from there on; lengths as in the greedy call.
        return_logprobs=True appends token_logprobs [B * m, steps] (0.0 after the stop id) and scores float64 [B * m].  Not
        together with do_sample or several questions per example.  `last_beam` keeps the raw tables of the call.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens / logit_bias (dense float [vocab], finite or -inf): the repetition
        controls of include/mellow_hip.h (mellow_generate_rules), applied to every row's logits on the device before the token is
        chosen, whatever chooses it (arg-max, sampler, beam select); the history is the row's generated tokens.  With any of them
        set, a returned log-prob is that of the processed distribution, not the number score() returns.  All at their neutral
        values: nothing is armed and the call is the one without these keywords.
        guidance_scale = s != 1 with negative = (audio1, audio2, input_ids) of the same shapes: contrastive guidance (include/mellow_hip.h,
        mellow_generate_guidance).  Every example runs next to its negative (rows 2i, 2i + 1 of one batch of 2 * B rows); per step the
        two rows' log-softmax a, b are combined on the device to g = b + s * (a - b), which both rows then choose their token from
        (after the repetition controls, if set).  The B conditional rows are returned (keep_negative_rows=True: all 2 * B rows, rows
        2i and 2i + 1 equal).  row_offset counts PAIRS: answer i draws from the stream example i of the un-guided call draws from.  A
        returned log-prob is that of the processed distribution.  ValueError together with num_beams, num_return_sequences > 1 or
        3-D input_ids, for a scale that is not finite, or for s != 1 without `negative`.  s = 1 (default): nothing is armed, `negative`
        is ignored and the call is the one without these keywords.
        top_logprobs = k (1 .. 20; needs return_logprobs=True): the k likeliest tokens of every step (include/mellow_hip.h,
        mellow_generate_top_logprobs), taken on the device from exactly the row the token is chosen from -- after the guidance and the
        repetition controls, if set; at temperature 1 and without the nucleus, as `logprobs` is.  The result gains two values after
        logprobs: top_ids int32 [rows, steps, k] and top_logprobs float32 [rows, steps, k], best first (value descending, then index
        ascending); -1 / exactly 0.0 where tokens is -1.  Guided calls return the conditional rows, or all rows with
        keep_negative_rows=True.  ValueError with num_beams, without return_logprobs=True, or for k outside [0, 20].  0 (default):
        nothing is armed and the call is the one without the keyword.
        top_k = K / min_p = p (need do_sample=True): the sampler's candidate filters next to the nucleus (include/mellow_hip.h,
        mellow_generate_filters), applied on the device in Hugging Face's order temperature, top_k, top_p, min_p: the K likeliest
        tokens (ties cut by index), the nucleus inside them, and of those the tokens whose probability is at least p times the
        likeliest token's.  Seeds, row streams, num_return_sequences, question lists, repetition controls, guidance and the log-prob
        records (which stay unfiltered) work as without them.  ValueError without do_sample=True, with num_beams, for K < 0 or p
        outside [0, 1].  Both 0 (default; Hugging Face's top_k = 50 is not adopted): nothing is armed and the call is the one without
        the keywords.
        constraint = a list parallel to the EXAMPLES of phrase sets, each a list of token-id lists: constrained decoding
        (include/mellow_hip.h, mellow_generate_constraint; mellow_amd/constraint.py builds the trie).  Every answer of an example is
        one of its phrases followed by the stop id: tokens that do not continue a phrase are banned on the device inside the decode
        step, after the guidance and the repetition controls and before the top log-probs and whatever chooses the token, so the
        recorded log-probs are those of the constrained distribution (over the phrase set they sum to 1) -- not the numbers score()
        returns.  The engine expands the sets to the call's rows (num_return_sequences, questions, beams, both rows of a guided
        pair).  constraint_then_free=True: the set constrains only the start of the answer, which continues freely once a phrase is
        complete (a one-phrase set is a forced prefix).  ValueError for an empty set, an empty phrase, an id outside the vocabulary
        or a list of another length than the examples.  None (default): nothing is armed and the call is the one without the
        keywords.
        stop_strings = a list of 1 to 16 byte strings of 1 to 64 bytes: an answer ends once its text -- the concatenated bytes of
        its generated tokens, from the table of set_vocab_bytes -- contains one of them (include/mellow_hip.h,
        mellow_generate_stop_strings).  The match runs on the device inside the decode step, after the guidance, the repetition
        controls and the constraint and before the top log-probs and whatever chooses the token: the step after the token that
        completed a match, the row's only choice is the stop id (recorded log-prob exactly 0.0; it wins over min_new_tokens and over
        a constraint), so the row ends through the usual stop rule and a log-prob sum runs over the answer up to the end of the
        matching token.  Works on every route (sampling, num_return_sequences, questions, beams, guidance).  ValueError for an
        empty list, more than 16 strings or a string of 0 or more than 64 bytes; EngineError without set_vocab_bytes, or when the
        call knows no stop token (num_beams with ignore_stop).  None (default): nothing is armed and the call is the one without
        the keyword."""
        import time
        t_in = time.perf_counter()
        nseq = int(num_return_sequences)
        fk, fp = check_sample_filters(top_k, min_p)
        filters = None
        if fk or fp:
            if num_beams is not None:
                raise ValueError("top_k / min_p and num_beams do not combine: they filter a sampled draw, beam search is deterministic")
            if not do_sample:
                raise ValueError("top_k / min_p need do_sample=True: they filter the sampled draw, the greedy token is the arg-max whatever they are")
            self._need("mellow_generate_filters")
            filters = SampleFilters(size=C.sizeof(SampleFilters), top_k=fk, min_p=fp)
        topk = check_top_logprobs(top_logprobs)
        if topk:
            if num_beams is not None:
                raise ValueError("top_logprobs and num_beams do not combine: top log-probs of a beam hypothesis are not built")
            if not return_logprobs:
                raise ValueError("top_logprobs needs return_logprobs=True: the alternatives come with the log-prob record")
            self._need("mellow_generate_top_logprobs")
        gscale = check_guidance_scale(guidance_scale)
        multiq = has_question_axis(input_ids)
        if gscale != 1.0:
            if num_beams is not None:
                raise ValueError("guidance_scale and num_beams do not combine: beam search over pairs is not built")
            if nseq != 1:
                raise ValueError("guidance_scale and num_return_sequences > 1 do not combine: repeat the example (and its negative) in the batch")
            if multiq:
                raise ValueError("guidance_scale and several questions per example do not combine: pass an example per question")
            if negative is None:
                raise ValueError(f"guidance_scale = {gscale} needs `negative` = (audio1, audio2, input_ids): the input to contrast with")
            self._need("mellow_generate_guidance")
        con = None
        if constraint is not None:
            con = _CallConstraint(constraint, constraint_then_free, self.lm.vocab_size)
            self._need("mellow_generate_constraint")
        stop = None
        if stop_strings is not None:
            stop = _CallStopStrings(stop_strings)
            self._need("mellow_generate_stop_strings")
        opts = _CallOptions(self._make_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, logit_bias, _arm_neutral_rules, int(max_len)),
                            gscale if gscale != 1.0 else None, topk, filters, con, stop)
        if num_beams is not None:
            if do_sample:
                raise ValueError("num_beams and do_sample=True do not combine: beam search is deterministic")
            if multiq:
                raise ValueError("num_beams and several questions per example do not combine: ask each question in a call of its own")
            return self._generate_beam(audio1, audio2, input_ids, int(max_len), int(num_beams), nseq, float(length_penalty),
                                       int(stop_id), bool(ignore_stop), bool(return_logprobs), t_in, opts)
        if multiq:
            if nseq != 1:
                raise ValueError("num_return_sequences > 1 and several questions per example do not combine: ask each question in a "
                                 "call of its own with num_return_sequences, or repeat the question in the list")
            return self._generate_multiq(audio1, audio2, input_ids, int(max_len), float(top_p), float(temperature), int(stop_id),
                                         bool(ignore_stop), bool(do_sample), _seed64(seed) if do_sample else 0,
                                         int(row_offset) if do_sample else 0, bool(return_logprobs), t_in, opts)
        if nseq != 1:
            if nseq < 1:
                raise ValueError(f"num_return_sequences must be >= 1 (got {nseq})")
            if not do_sample:
                raise ValueError("num_return_sequences > 1 needs do_sample=True: greedy answers of one example are all the same")
            return self._generate_nseq(audio1, audio2, input_ids, int(max_len), nseq, float(top_p), float(temperature), int(stop_id),
                                       bool(ignore_stop), _seed64(seed), int(row_offset), bool(return_logprobs), t_in, opts)
        a1, a2, ids = self._f32(audio1), self._f32(audio2), self._prompt_ids(input_ids)
        rows = slice(None)
        opts.expand_constraint(a1.shape[0], 2 if opts.guide is not None else 1)      # (both rows of a guided pair carry the example's root)
        if opts.guide is not None:
            # rows 2i / 2i + 1 = example i / its negative
            n1, n2, nids = self._f32(negative[0]), self._f32(negative[1]), self._prompt_ids(negative[2])
            if n1.shape != a1.shape or n2.shape != a2.shape or nids.shape != ids.shape:
                raise ValueError(f"`negative` must have the shapes of the inputs: {tuple(n1.shape)}, {tuple(n2.shape)}, {tuple(nids.shape)} "
                                 f"against {tuple(a1.shape)}, {tuple(a2.shape)}, {tuple(ids.shape)}")
            a1 = torch.stack((a1, n1), dim=1).reshape(2 * a1.shape[0], -1).contiguous()
            a2 = torch.stack((a2, n2), dim=1).reshape(2 * a2.shape[0], -1).contiguous()
            ids = torch.stack((ids, nids), dim=1).reshape(2 * ids.shape[0], -1).contiguous()
            if not keep_negative_rows:
                rows = slice(None, None, 2)      # the conditional rows
        B, n = a1.shape
        assert a2.shape == a1.shape and ids.shape == (B, spec.TEXT_LEN), (a1.shape, a2.shape, ids.shape)
        out = torch.empty((B, max_len), dtype=torch.int32, device=self.tdev)
        top = self._top_record(topk, B, int(max_len))
        self._sync_inputs()
        t_up = (time.perf_counter() - t_in) * 1e3
        lp = None
        head = (_ptr(a1), _ptr(a2), n, _ptr(ids), B, int(max_len))
        tail = (int(stop_id), 1 if ignore_stop else 0, _ptr(out))
        if return_logprobs:
            self._need("mellow_generate_scored")
            lp = torch.empty((B, max_len), dtype=torch.float32, device=self.tdev)
            fn, args = self.lib.mellow_generate_scored, head + (1 if do_sample else 0, float(top_p), float(temperature), _seed64(seed) if do_sample else 0,
                                                                int(row_offset) if do_sample else 0) + tail + (_ptr(lp),)
        elif do_sample:
            fn, args = self.lib.mellow_generate_sampled, head + (float(top_p), float(temperature), _seed64(seed), int(row_offset)) + tail
        else:
            fn, args = self.lib.mellow_generate, head + (float(top_p), float(temperature)) + tail
        lens, steps, ftm = self._generate_call(opts, top, fn, B, *args)
        self.last_first_token_host_ms = t_up + ftm
        return self._result(out, lens, steps, ftm, lp, top, rows)

    def _generate_call(self, opts, top, fn, rows, *args, row0: int = 0):
        """ONE generation C call fn(h, *args, lens, &steps, &first_token_ms) on `rows` answer rows -- rows [row0, row0 + rows) of the
        generate() call -- armed from the call's options with the rows of the top record it fills (or None) -> (lengths int32 [rows],
        steps, first_token_ms)"""
        lens = (C.c_int32 * rows)()
        steps, ftm = C.c_int32(0), C.c_float(0.0)
        opts.arm(self, top, row0, rows)
        self._chk(fn(self.h, *args, lens, C.byref(steps), C.byref(ftm)))
        return np.asarray(list(lens), dtype=np.int32), int(steps.value), float(ftm.value)

    @staticmethod
    def _result(out, lens, steps, ftm, lp=None, top=None, rows=slice(None)):
        """the tuple generate() returns: the device records cut at `steps` columns (and to `rows`: the conditional rows of a guided
        call), with logprobs and the two top arrays where the call has them"""
        res = (out.cpu().numpy()[rows, :steps], lens[rows], steps, ftm)
        if lp is not None:
            res = res + (lp.cpu().numpy()[rows, :steps],)
        if top is not None:
            res = res + tuple(t.cpu().numpy()[rows, :steps] for t in top)
        return res

    def _top_record(self, k: int, rows: int, max_len: int):
        """the device record (ids int32, log-probs float32, [rows][max_len][k] each) of a generate() with top_logprobs=k, or None"""
        if not k:
            return None
        return (torch.empty((rows, max_len, k), dtype=torch.int32, device=self.tdev),
                torch.empty((rows, max_len, k), dtype=torch.float32, device=self.tdev))

    def _make_rules(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, logit_bias, arm_neutral, max_len):
        """the struct handed to mellow_generate_rules before every C call of this generate(), or None: nothing to arm"""
        t, n, m, bias = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, logit_bias,
                                          None if logit_bias is None else self.lm.vocab_size)
        if t == 1.0 and n == 0 and m == 0 and bias is None and not arm_neutral:
            return None
        if m > max_len:
            raise ValueError(f"min_new_tokens = {m} exceeds max_len = {max_len}")
        if max_len > RULES_MAX_LEN:
            raise ValueError(f"a call with logit rules takes max_len <= {RULES_MAX_LEN} (got {max_len})")
        self._need("mellow_generate_rules")
        r = LogitRules(size=C.sizeof(LogitRules), repetition_penalty=t, no_repeat_ngram_size=n, min_new_tokens=m,
                       logit_bias=None if bias is None else bias.ctypes.data)
        r._bias = bias               # keeps the vector alive while the struct points at it
        return r

    def logit_rules_apply(self, logits, history, hist_len, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                          min_new_tokens: int = 0, logit_bias=None, stop_id: int = 0, with_sum: bool = True):
        """The rules on caller data (numeric tap, mellow_logit_rules_apply): logits [B][vocab], history int [B][ld], hist_len int [B]
        -> dict of numpy arrays: "logits" [B][vocab] processed, "cand_val" / "cand_idx" [B][vocab / 32] the per-tile maximum and
        its first index, "cand_sum" [B][vocab / 32] the per-tile sum of exp(l - cand_val) (with_sum=False: absent)."""
        t, n, m, bias = check_logit_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, logit_bias, self.lm.vocab_size)
        self._need("mellow_logit_rules_apply")
        lg = self._f32(logits).clone()
        B, V = lg.shape
        h = self._i32(history).reshape(B, -1)
        ln = self._i32(hist_len).reshape(-1)
        if V != self.lm.vocab_size or ln.shape[0] != B:
            raise ValueError(f"logits {tuple(lg.shape)}, history {tuple(h.shape)}, hist_len {tuple(ln.shape)} do not describe B rows of the vocabulary")
        ld = int(h.shape[1])
        cv = torch.empty((B, V // 32), dtype=torch.float32, device=self.tdev)
        cx = torch.empty((B, V // 32), dtype=torch.int32, device=self.tdev)
        cs = torch.empty((B, V // 32), dtype=torch.float32, device=self.tdev) if with_sum else None
        r = LogitRules(size=C.sizeof(LogitRules), repetition_penalty=t, no_repeat_ngram_size=n, min_new_tokens=m,
                       logit_bias=None if bias is None else bias.ctypes.data)
        self._sync_inputs()
        self._chk(self.lib.mellow_logit_rules_apply(self.h, C.byref(r), _ptr(lg), B, _ptr(h) if ld else None, ld, _ptr(ln), int(stop_id),
                                                    _ptr(cv), _ptr(cx), None if cs is None else _ptr(cs)))
        out = {"logits": lg.cpu().numpy(), "cand_val": cv.cpu().numpy(), "cand_idx": cx.cpu().numpy()}
        if cs is not None:
            out["cand_sum"] = cs.cpu().numpy()
        return out

    def constraint_apply(self, logits, history, hist_len, constraint, then_free: bool = False, stop_id: int = 0, with_sum: bool = True):
        """The constraint on caller data (numeric tap, mellow_constraint_apply): logits [B][vocab], history int [B][ld], hist_len int
        [B], constraint = per ROW a list of token-id lists -> dict of numpy arrays: "logits" [B][vocab] processed, "state" int32 [B]
        the row's state after its history (a node of constraint.build_trie(constraint), or -1 DEAD / -2 FREE / -3 DONE), "cand_val" /
        "cand_idx" / "cand_sum" [B][vocab / 32] the tile partials (with_sum=False: no "cand_sum").  The launch leaves a row whose
        allowed set is everything, or empty, as it is, partials included: the partials start as those of the unprocessed rows (the
        neutral rules tap forms them)."""
        self._need("mellow_constraint_apply")
        lg = self._f32(logits).clone()
        B, V = lg.shape
        h = self._i32(history).reshape(B, -1)
        ln = self._i32(hist_len).reshape(-1)
        if V != self.lm.vocab_size or ln.shape[0] != B:
            raise ValueError(f"logits {tuple(lg.shape)}, history {tuple(h.shape)}, hist_len {tuple(ln.shape)} do not describe B rows of the vocabulary")
        con = _CallConstraint(constraint, then_free, V)
        con.expand(B, 1)
        ld = int(h.shape[1])
        before = self.logit_rules_apply(lg, np.zeros((B, 1), dtype=np.int32), np.zeros(B, dtype=np.int32), stop_id=-1, with_sum=with_sum)
        cv, cx = self._f32(before["cand_val"]).clone(), self._i32(before["cand_idx"]).clone()
        cs = self._f32(before["cand_sum"]).clone() if with_sum else None
        st = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_constraint_apply(self.h, C.byref(con.struct(0, B)), _ptr(lg), B, _ptr(h) if ld else None, ld, _ptr(ln),
                                                   int(stop_id), _ptr(cv), _ptr(cx), None if cs is None else _ptr(cs), _ptr(st)))
        out = {"logits": lg.cpu().numpy(), "state": st.cpu().numpy(), "cand_val": cv.cpu().numpy(), "cand_idx": cx.cpu().numpy()}
        if cs is not None:
            out["cand_sum"] = cs.cpu().numpy()
        return out

    def set_vocab_bytes(self, offsets, data):
        """The byte string of every token id, for stop_strings (mellow_set_vocab_bytes): offsets int [vocab + 1] from 0, never
        decreasing; data = the tokens' bytes back to back (bytes or uint8 array), token i = data[offsets[i] : offsets[i + 1]], at
        most 256 bytes, possibly none.  mellow_amd/stop_strings.py vocab_bytes builds the pair from a tokenizer.  The table
        belongs to the engine's shared state: set once on the engine or any fork, it serves all of them.  Setting it again replaces
        it -- never while a call runs on any context."""
        self._need("mellow_set_vocab_bytes")
        off, dat = check_vocab_bytes(offsets, data, self.lm.vocab_size)
        if dat.shape[0] == 0:
            dat = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.mellow_set_vocab_bytes(self.h, C.c_void_p(off.ctypes.data), C.c_void_p(dat.ctypes.data), int(off.shape[0] - 1)))

    def stop_strings_apply(self, logits, history, hist_len, stop_strings, stop_id: int = 0, with_sum: bool = True):
        """The stop strings on caller data (numeric tap, mellow_stop_strings_apply): logits [B][vocab], history int [B][ld], hist_len
        int [B], stop_strings = a list of byte strings -> dict of numpy arrays: "logits" [B][vocab] processed, "hit" int32 [B] (1:
        the text of the row's history holds a stop string), "cand_val" / "cand_idx" / "cand_sum" [B][vocab / 32] the tile partials
        (with_sum=False: no "cand_sum").  The launch leaves a row that is not hit as it is, partials included: the partials start as
        those of the unprocessed rows (the neutral rules tap forms them)."""
        self._need("mellow_stop_strings_apply")
        lg = self._f32(logits).clone()
        B, V = lg.shape
        h = self._i32(history).reshape(B, -1)
        ln = self._i32(hist_len).reshape(-1)
        if V != self.lm.vocab_size or ln.shape[0] != B:
            raise ValueError(f"logits {tuple(lg.shape)}, history {tuple(h.shape)}, hist_len {tuple(ln.shape)} do not describe B rows of the vocabulary")
        st = _CallStopStrings(stop_strings)
        ld = int(h.shape[1])
        before = self.logit_rules_apply(lg, np.zeros((B, 1), dtype=np.int32), np.zeros(B, dtype=np.int32), stop_id=-1, with_sum=with_sum)
        cv, cx = self._f32(before["cand_val"]).clone(), self._i32(before["cand_idx"]).clone()
        cs = self._f32(before["cand_sum"]).clone() if with_sum else None
        hit = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_stop_strings_apply(self.h, C.byref(st.struct), _ptr(lg), B, _ptr(h) if ld else None, ld, _ptr(ln),
                                                     int(stop_id), _ptr(cv), _ptr(cx), None if cs is None else _ptr(cs), _ptr(hit)))
        out = {"logits": lg.cpu().numpy(), "hit": hit.cpu().numpy(), "cand_val": cv.cpu().numpy(), "cand_idx": cx.cpu().numpy()}
        if cs is not None:
            out["cand_sum"] = cs.cpu().numpy()
        return out

    def guidance_apply(self, logits, scale: float, with_sum: bool = True):
        """Contrastive guidance on caller data (numeric tap, mellow_guidance_apply): logits [2 * P][vocab], rows 2i / 2i + 1 the
        conditional and the negative row of pair i -> dict of numpy arrays: "logits" [2 * P][vocab], both rows of a pair holding g,
        "cand_val" / "cand_idx" [2 * P][vocab / 32] the per-tile maximum of g and its first index, "cand_sum" [2 * P][vocab / 32] the
        per-tile sum of exp(g - cand_val) (with_sum=False: absent)."""
        s = check_guidance_scale(scale)
        self._need("mellow_guidance_apply")
        lg = self._f32(logits).clone()
        R, V = lg.shape
        if V != self.lm.vocab_size or R < 2 or R % 2:
            raise ValueError(f"logits {tuple(lg.shape)} do not describe pairs of rows of the vocabulary")
        cv = torch.empty((R, V // 32), dtype=torch.float32, device=self.tdev)
        cx = torch.empty((R, V // 32), dtype=torch.int32, device=self.tdev)
        cs = torch.empty((R, V // 32), dtype=torch.float32, device=self.tdev) if with_sum else None
        self._sync_inputs()
        self._chk(self.lib.mellow_guidance_apply(self.h, s, _ptr(lg), R // 2, _ptr(cv), _ptr(cx), None if cs is None else _ptr(cs)))
        out = {"logits": lg.cpu().numpy(), "cand_val": cv.cpu().numpy(), "cand_idx": cx.cpu().numpy()}
        if cs is not None:
            out["cand_sum"] = cs.cpu().numpy()
        return out

    def top_logprobs_apply(self, logits, cand_val, cand_sum, k: int):
        """The k likeliest tokens of caller rows (numeric tap, mellow_top_logprobs_apply): logits [B][vocab], cand_val / cand_sum
        [B][vocab / 32] the tile partials as logit_rules_apply or guidance_apply return them -> (ids int32 [B][k], lp float32 [B][k])
        as numpy arrays, best first."""
        k = check_top_logprobs(k)
        if k < 1:
            raise ValueError(f"top_logprobs_apply takes k = 1 to {TOP_LOGPROBS_MAX_K} (got {k})")
        self._need("mellow_top_logprobs_apply")
        lg, cv, cs = self._f32(logits), self._f32(cand_val), self._f32(cand_sum)
        B, V = lg.shape
        if V != self.lm.vocab_size or cv.shape != (B, V // 32) or cs.shape != (B, V // 32):
            raise ValueError(f"logits {tuple(lg.shape)}, cand_val {tuple(cv.shape)}, cand_sum {tuple(cs.shape)} do not describe B rows of the vocabulary")
        ids = torch.empty((B, k), dtype=torch.int32, device=self.tdev)
        lp = torch.empty((B, k), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_top_logprobs_apply(self.h, _ptr(lg), _ptr(cv), _ptr(cs), B, k, _ptr(ids), _ptr(lp)))
        return ids.cpu().numpy(), lp.cpu().numpy()

    def _generate_nseq(self, audio1, audio2, input_ids, max_len, nseq, top_p, temperature, stop_id, ignore_stop, seed, row_offset,
                       return_logprobs, t_in, opts):
        """generate(num_return_sequences=nseq > 1): one mellow_generate_n call per pass of plan_nseq_passes; a pass that stopped
        before the longest one is padded like the passes of a batch of more than 1024 rows (-1 tokens, 0.0 log-probs)."""
        import time
        self._need("mellow_generate_n")
        a1, a2, ids = self._f32(audio1), self._f32(audio2), self._prompt_ids(input_ids)
        B, ns = a1.shape
        assert a2.shape == a1.shape and ids.shape == (B, spec.TEXT_LEN), (a1.shape, a2.shape, ids.shape)
        passes = plan_nseq_passes(B, nseq, row_offset)
        N = B * nseq
        opts.expand_constraint(B, nseq)
        out = torch.empty((N, max_len), dtype=torch.int32, device=self.tdev)
        lp = torch.empty((N, max_len), dtype=torch.float32, device=self.tdev) if return_logprobs else None
        top = self._top_record(opts.top_k, N, max_len)
        self._sync_inputs()
        t_up = (time.perf_counter() - t_in) * 1e3
        lens = np.zeros((N,), dtype=np.int32)
        pass_steps, ftm0 = [], 0.0
        for k, (lo, hi, off) in enumerate(passes):
            r0, r1 = lo * nseq, hi * nseq
            lens[r0:r1], steps, ftm = self._generate_call(
                opts, None if top is None else (top[0][r0:r1], top[1][r0:r1]), self.lib.mellow_generate_n, r1 - r0,
                _ptr(a1[lo:hi]), _ptr(a2[lo:hi]), ns, _ptr(ids[lo:hi]), hi - lo, nseq, max_len, 1, top_p, temperature, seed, off, stop_id,
                1 if ignore_stop else 0, _ptr(out[r0:r1]), None if lp is None else _ptr(lp[r0:r1]), row0=r0)
            pass_steps.append(steps)
            if k == 0:
                ftm0 = ftm
        self.last_first_token_host_ms = t_up + ftm0
        res = self._result(out, lens, max(pass_steps), ftm0, lp, top)
        for (lo, hi, _), st in zip(passes, pass_steps):      # columns a pass never reached: never computed
            for rec, never in zip((res[0],) + res[4:], (-1, 0.0, -1, 0.0)):      # tokens, logprobs, top ids, top log-probs
                rec[lo * nseq:hi * nseq, st:] = never
        return res

    def _generate_beam(self, audio1, audio2, input_ids, max_len, k, m, length_penalty, stop_id, ignore_stop, return_logprobs, t_in, opts):
        """generate(num_beams=k): one mellow_generate_beam call, then the backtracking and the final ranking on the host"""
        import time
        a1, a2 = torch.as_tensor(audio1), torch.as_tensor(audio2)
        check_beam_request(a1.shape[0], k, max_len, m)
        if k > 1 and getattr(self, "precision", None) == "fp8":
            raise ValueError('num_beams > 1 is not available with precision="fp8": the bf16 K/V pages of that mode have no fan-out')
        self._need("mellow_generate_beam")
        a1, a2, ids = self._f32(a1), self._f32(a2), self._prompt_ids(input_ids)
        B, ns = a1.shape
        assert a2.shape == a1.shape and ids.shape == (B, spec.TEXT_LEN), (a1.shape, a2.shape, ids.shape)
        N = B * k
        opts.expand_constraint(B, k)
        par = np.zeros((max_len, N), dtype=np.int32)
        tok = np.zeros((max_len, N), dtype=np.int32)
        lp = np.zeros((max_len, N), dtype=np.float32)
        cum = np.zeros((N,), dtype=np.float32)
        self._sync_inputs()
        t_up = (time.perf_counter() - t_in) * 1e3
        steps, ftm = C.c_int32(0), C.c_float(0.0)
        vp = C.c_void_p
        opts.arm(self, None, 0, N)
        self._chk(self.lib.mellow_generate_beam(self.h, _ptr(a1), _ptr(a2), ns, _ptr(ids), B, k, max_len, stop_id, 1 if ignore_stop else 0,
                                                vp(par.ctypes.data), vp(tok.ctypes.data), vp(lp.ctypes.data), vp(cum.ctypes.data),
                                                C.byref(steps), C.byref(ftm)))
        st = int(steps.value)
        par, tok, lp = par[:st], tok[:st], lp[:st]
        self.last_beam = {"parent": par, "token": tok, "lp": lp, "cum": cum, "k": k}
        toks, lps = backtrack_beams(par, tok, lp, k)
        order, lengths, counts, scores = rank_beams(toks, lps, cum, k, stop_id, length_penalty, ignore_stop)
        rows = (np.arange(B)[:, None] * k + order[:, :m]).reshape(-1)
        self.last_first_token_host_ms = t_up + float(ftm.value)
        res = (toks[rows], lengths[rows], st, float(ftm.value))
        if return_logprobs:
            res = res + (lps[rows].astype(np.float32), scores[rows])
        self.last_beam.update(rows=rows, logprob=cum[rows].astype(np.float64))
        return res

    def beam_select(self, logits, cum, fin, k: int, stop_id: int = 0):
        """One selection step of the beam search on caller data (numeric tap, mellow_beam_select): logits [B * k][vocab], cum
        [B * k], fin [B * k] -> dict of parent / token int32 [B * k], cum / lp float32 [B * k] (row b * k + j = new beam j)."""
        self._need("mellow_beam_select")
        lg, cu, fi = self._f32(logits), self._f32(cum), self._i32(fin)
        N, k = lg.shape[0], int(k)
        if k < 1 or N % k != 0 or cu.shape != (N,) or fi.shape != (N,):
            raise ValueError(f"logits {tuple(lg.shape)}, cum {tuple(cu.shape)}, fin {tuple(fi.shape)} are not B * {k} rows")
        par = torch.empty((N,), dtype=torch.int32, device=self.tdev)
        tok = torch.empty((N,), dtype=torch.int32, device=self.tdev)
        oc = torch.empty((N,), dtype=torch.float32, device=self.tdev)
        ol = torch.empty((N,), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_beam_select(self.h, _ptr(lg), _ptr(cu), _ptr(fi), N // k, k, int(stop_id), _ptr(par), _ptr(tok),
                                              _ptr(oc), _ptr(ol)))
        return {"parent": par.cpu().numpy(), "token": tok.cpu().numpy(), "cum": oc.cpu().numpy(), "lp": ol.cpu().numpy()}

    def _generate_multiq(self, audio1, audio2, input_ids, max_len, top_p, temperature, stop_id, ignore_stop, do_sample, seed, row_offset,
                         return_logprobs, t_in, opts):
        """generate() with input_ids [B][Q][text_len]: one mellow_generate_q call on B * Q <= 1024 rows."""
        import time
        self._need("mellow_generate_q")
        a1, a2, ids = self._f32(audio1), self._f32(audio2), self._prompt_ids(input_ids)
        B, ns = a1.shape
        assert a2.shape == a1.shape and ids.dim() == 3 and ids.shape[0] == B and ids.shape[2] == spec.TEXT_LEN, (a1.shape, a2.shape, ids.shape)
        Q = int(ids.shape[1])
        if Q < 1:
            raise ValueError("every example needs at least one question (input_ids [B][0][text_len])")
        N = B * Q
        if N > NSEQ_PASS_ROWS:
            raise ValueError(f"{B} examples x {Q} questions = {N} answer rows exceed the {NSEQ_PASS_ROWS} one call takes: split the "
                             "examples over several calls, advancing row_offset by Q per example")
        if Q > 1 and self.precision == "fp8":
            raise ValueError('several questions per example are not available with precision="fp8": the bf16 K/V pages of that mode '
                             "have no fan-out (pass the pair once per question instead)")
        opts.expand_constraint(B, Q)
        out = torch.empty((N, max_len), dtype=torch.int32, device=self.tdev)
        lp = torch.empty((N, max_len), dtype=torch.float32, device=self.tdev) if return_logprobs else None
        top = self._top_record(opts.top_k, N, max_len)
        self._sync_inputs()
        t_up = (time.perf_counter() - t_in) * 1e3
        lens, steps, ftm = self._generate_call(opts, top, self.lib.mellow_generate_q, N, _ptr(a1), _ptr(a2), ns, _ptr(ids), B, Q, max_len,
                                               1 if do_sample else 0, top_p, temperature, seed, row_offset, stop_id, 1 if ignore_stop else 0,
                                               _ptr(out), None if lp is None else _ptr(lp))
        self.last_first_token_host_ms = t_up + ftm
        return self._result(out, lens, steps, ftm, lp, top)

    def stft_is_fft(self) -> bool:
        """the STFT runs as an FFT (f32x3 mode, windowed-DFT conv weights) instead of the DFT GEMM"""
        return bool(self.lib.mellow_stft_is_fft(self.h))

    def prefill_parts(self) -> int:
        """parts the f32x3 LM prefill runs as (2 = two half-batches on two streams MEASURED to overlap; 1 = one chain, also the
        fallback when this process's HIP runtime has no second hardware queue for the engine)"""
        return int(self.lib.mellow_prefill_parts(self.h))

    def last_row_repacks(self) -> int:
        """how often the last generate() call packed the still-running rows into fewer 32-row blocks"""
        return int(self.lib.mellow_last_row_repacks(self.h))

    def last_steps_enqueued(self) -> int:
        return int(self.lib.mellow_last_steps_enqueued(self.h))

    # ---- taps ----------------------------------------------------------------------------------------
    def logmel(self, wav, apply_bn: bool = False) -> torch.Tensor:
        w = self._f32(wav)
        n, ns = w.shape
        out = torch.empty((n, spec.frames_for(ns), spec.MEL_BINS), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_logmel(self.h, _ptr(w), n, ns, 1 if apply_bn else 0, _ptr(out)))
        return out

    def encode(self, wav) -> torch.Tensor:
        w = self._f32(wav)
        n, ns = w.shape
        out = torch.empty((n, spec.AUDIO_ROWS, spec.D_PROJ), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_encode(self.h, _ptr(w), n, ns, _ptr(out)))
        return out

    def prefix(self, audio1, audio2, input_ids) -> torch.Tensor:
        a1, a2, ids = self._f32(audio1), self._f32(audio2), self._prompt_ids(input_ids)
        B, n = a1.shape
        out = torch.empty((B, spec.PREFIX_LEN, spec.D_PROJ), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_prefix(self.h, _ptr(a1), _ptr(a2), n, _ptr(ids), B, _ptr(out)))
        return out

    def lm_prefill(self, prefix, reserve: int = 64) -> torch.Tensor:
        p = self._f32(prefix)
        B, T, H = p.shape
        out = torch.empty((B, self.lm.vocab_size), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_lm_prefill(self.h, _ptr(p), B, T, int(reserve), _ptr(out)))
        return out

    def lm_decode_step(self, token_ids) -> torch.Tensor:
        t = self._ids(token_ids).reshape(-1)
        out = torch.empty((t.shape[0], self.lm.vocab_size), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_lm_decode_step(self.h, _ptr(t), _ptr(out)))
        return out

    def embed_tokens(self, token_ids) -> torch.Tensor:
        """`lm.model.embed_tokens(ids)` (reference decoder.py:47, wrapper.py:237): (...,) ids -> (..., hidden) on the device"""
        t = self._ids(token_ids)
        out = torch.empty(tuple(t.shape) + (self.lm.hidden_size,), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_embed_tokens(self.h, _ptr(t), t.numel(), _ptr(out)))
        return out

    def lm_forward_logits(self, embeds, from_pos: int = 0) -> torch.Tensor:
        """`lm(inputs_embeds=embeds).logits[:, from_pos:]` (reference decoder.py:89): (B, T, hidden) -> (B, T - from_pos, vocab)"""
        p = self._f32(embeds)
        B, T, H = p.shape
        out = torch.empty((B, T - int(from_pos), self.lm.vocab_size), dtype=torch.float32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_lm_forward_logits(self.h, _ptr(p), B, T, int(from_pos), _ptr(out)))
        return out

    def lm_score(self, embeds, targets, from_pos: int = 0):
        """Teacher-forced scores of `lm(inputs_embeds=embeds).logits[:, from_pos:]` without materialising them (mellow_lm_score,
        the fused log-softmax head): embeds (B, T, hidden), targets int (B, T - from_pos) with -1 = not scored ->
        dict of device tensors {"logprob" f32, "argmax" i32, "lse" f32, "max" f32}, each (B, T - from_pos).
        A target outside [-1, vocab) raises IndexError."""
        p = self._f32(embeds)
        B, T, H = p.shape
        n = T - int(from_pos)
        t = torch.as_tensor(targets)
        if tuple(t.shape) != (B, n):
            raise ValueError(f"targets must be ({B}, {n}), got {tuple(t.shape)}")
        if t.numel() and (int(t.min()) < -1 or int(t.max()) >= self.lm.vocab_size):
            raise IndexError("index out of range in self")
        t = t.to(device=self.tdev, dtype=torch.int32).contiguous()
        out = {"logprob": torch.empty((B, n), dtype=torch.float32, device=self.tdev),
               "argmax": torch.empty((B, n), dtype=torch.int32, device=self.tdev),
               "lse": torch.empty((B, n), dtype=torch.float32, device=self.tdev),
               "max": torch.empty((B, n), dtype=torch.float32, device=self.tdev)}
        self._need("mellow_lm_score")
        self._sync_inputs()
        self._chk(self.lib.mellow_lm_score(self.h, _ptr(p), B, T, int(from_pos), _ptr(t), _ptr(out["logprob"]), _ptr(out["argmax"]),
                                           _ptr(out["lse"]), _ptr(out["max"])))
        return out

    def max_candidate_tokens(self) -> int:
        """largest candidate length L `score` takes: prefix 389 + L may not exceed the engine's max_positions"""
        return int(self.cfg.max_positions) - spec.PREFIX_LEN

    def score(self, audio1, audio2, input_ids, cand_ids, cand_len):
        """Teacher-forced log-probs of K candidate answers per example (mellow_score): audio1 / audio2 / input_ids as in
        `generate`; cand_ids int (B, K, L), cand_len int (B, K) with 1 <= cand_len <= L (ids at j >= cand_len are padding).
        -> (logprob f32 [B, K, L] (0 at j >= cand_len), sum f32 [B, K], argmax i32 [B, K, L]) as numpy arrays on the host.
        ValueError for a cand_len outside [1, L] or an L beyond max_candidate_tokens(); IndexError for a scored id outside the
        vocabulary."""
        a1, a2, ids = self._f32(audio1), self._f32(audio2), self._prompt_ids(input_ids)
        B, n = a1.shape
        assert a2.shape == a1.shape and ids.shape == (B, spec.TEXT_LEN), (a1.shape, a2.shape, ids.shape)
        c = torch.as_tensor(cand_ids)
        if c.dim() != 3 or c.shape[0] != B or c.shape[1] < 1 or c.shape[2] < 1:
            raise ValueError(f"cand_ids must be ({B}, K, L) with K, L >= 1, got {tuple(c.shape)}")
        K, L = int(c.shape[1]), int(c.shape[2])
        if L > self.max_candidate_tokens():
            raise ValueError(f"candidates of {L} tokens exceed the engine's page budget: prefix {spec.PREFIX_LEN} + L <= "
                             f"max_positions {int(self.cfg.max_positions)}, i.e. L <= {self.max_candidate_tokens()}")
        ln = np.ascontiguousarray(torch.as_tensor(cand_len).cpu().numpy(), dtype=np.int32)
        if ln.shape != (B, K):
            raise ValueError(f"cand_len must be ({B}, {K}), got {ln.shape}")
        if ln.min() < 1 or ln.max() > L:
            raise ValueError(f"cand_len must be in [1, {L}] (got {int(ln.min())} .. {int(ln.max())})")
        ch = c.cpu().numpy()
        scored = ch[np.arange(L)[None, None, :] < ln[:, :, None]]
        if scored.size and (int(scored.min()) < 0 or int(scored.max()) >= self.lm.vocab_size):
            raise IndexError("index out of range in self")
        c = c.clamp(0, self.lm.vocab_size - 1).to(device=self.tdev, dtype=torch.int32).contiguous()
        lp = torch.empty((B, K, L), dtype=torch.float32, device=self.tdev)
        sm = torch.empty((B, K), dtype=torch.float32, device=self.tdev)
        am = torch.empty((B, K, L), dtype=torch.int32, device=self.tdev)
        self._need("mellow_score")
        self._sync_inputs()
        self._chk(self.lib.mellow_score(self.h, _ptr(a1), _ptr(a2), n, _ptr(ids), B, _ptr(c), ln.ctypes.data_as(C.POINTER(C.c_int32)),
                                        K, L, _ptr(lp), _ptr(sm), _ptr(am)))
        return lp.cpu().numpy(), sm.cpu().numpy(), am.cpu().numpy()

    def forward(self, audio1, audio2, input_ids, answer_ids, from_pos: int = 0) -> torch.Tensor:
        """The training-time forward of the reference as inference arithmetic (`Mellow.forward`, mellow.py:89-98): logits of
        the sequence [audio1 | sep | audio2 | sep | prompt | answer] at every position >= from_pos.  The reference returns the
        HF output object; `.logits` of it is what this returns (no labels, no loss: decoder.py:84-89 passes labels=None)."""
        prefix = self.prefix(audio1, audio2, input_ids)
        ans = self.embed_tokens(answer_ids)
        return self.lm_forward_logits(torch.cat((prefix, ans), 1), from_pos)

    # -- the reference model object's call surface (wrapper.model is an nn.Module there: mellow.py:70-109) -------------------
    def generate_prefix_inference(self, input_dict):
        """`Mellow.generate_prefix_inference(input_dict)` (mellow.py:100-109): (prefix, None, None) -- the reference's second
        and third values are the encoder's output dicts, which the generation path never reads (wrapper.py:233)"""
        return self.prefix(input_dict["audio1"], input_dict["audio2"], input_dict["input"]["input_ids"]), None, None

    def __call__(self, input_dict):
        """`model(input_dict)` (mellow.py:89-98): an object whose `.logits` is (B, prefix + answer, vocab), like the HF
        CausalLMOutput the reference returns with labels=None (decoder.py:89: loss is None)"""
        from types import SimpleNamespace
        logits = self.forward(input_dict["audio1"], input_dict["audio2"], input_dict["input"]["input_ids"],
                              input_dict["answer"]["input_ids"])
        return SimpleNamespace(logits=logits, loss=None)

    def argmax(self, logits) -> torch.Tensor:
        l = self._f32(logits)
        out = torch.empty((l.shape[0],), dtype=torch.int32, device=self.tdev)
        self._sync_inputs()
        self._chk(self.lib.mellow_argmax(self.h, _ptr(l), l.shape[0], _ptr(out)))
        return out

    def sample_logits(self, logits, top_p: float, temperature: float, seed: int, step: int, row_ids=None, top_k: int = 0,
                      min_p: float = 0.0, filtered: Optional[bool] = None) -> torch.Tensor:
        """The decode step's draw on caller logits (B, vocab) -> tokens int32 (B,) on the device; row_ids (B,) = the global
        row index of each row (None: 0..B-1), step = the column of the token record the draw stands for.  top_k / min_p: the
        candidate filters (mellow_sample_logits_filtered, the sampler's filtered instantiation); filtered=True runs that
        instantiation also for neutral values, None (default) only when a filter is set."""
        fk, fp = check_sample_filters(top_k, min_p)
        if filtered is None:
            filtered = bool(fk or fp)
        elif not filtered and (fk or fp):
            raise ValueError("filtered=False with top_k / min_p set: the plain draw has no filters")
        l = self._f32(logits)
        if l.dim() != 2 or l.shape[1] != self.lm.vocab_size:
            raise ValueError(f"logits must be (B, {self.lm.vocab_size}), got {tuple(l.shape)}")
        B = l.shape[0]
        out = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        rid = None if row_ids is None else torch.as_tensor(row_ids).reshape(-1).to(device=self.tdev, dtype=torch.int32).contiguous()
        if rid is not None and rid.shape[0] != B:
            raise ValueError(f"row_ids has {rid.shape[0]} entries for {B} rows")
        self._sync_inputs()
        if filtered:
            self._need("mellow_sample_logits_filtered")
            f = SampleFilters(size=C.sizeof(SampleFilters), top_k=fk, min_p=fp)
            self._chk(self.lib.mellow_sample_logits_filtered(self.h, _ptr(l), B, None if rid is None else _ptr(rid), int(step), float(top_p),
                                                             float(temperature), _seed64(seed), C.byref(f), _ptr(out)))
            return out
        self._chk(self.lib.mellow_sample_logits(self.h, _ptr(l), B, None if rid is None else _ptr(rid), int(step), float(top_p),
                                                float(temperature), _seed64(seed), _ptr(out)))
        return out

    def resample(self, wav, orig_freq: int, new_freq: int) -> torch.Tensor:
        """(n, n_in) -> (n, ceil(new*n_in/orig)) on the device: the A0 resampler (twin of mellow_amd.audio.resample)."""
        w = self._f32(wav)
        if w.dim() == 1:
            w = w[None]
        n, n_in = w.shape
        n_out = C.c_int64(0)
        self._sync_inputs()
        self._chk(self.lib.mellow_resample(self.h, _ptr(w), n, n_in, int(orig_freq), int(new_freq), None, 0, C.byref(n_out)))
        out = torch.empty((n, n_out.value), dtype=torch.float32, device=self.tdev)
        self._chk(self.lib.mellow_resample(self.h, _ptr(w), n, n_in, int(orig_freq), int(new_freq), _ptr(out), n_out.value,
                                           C.byref(n_out)))
        return out

    def enable_taps(self, on: bool = True):
        self._chk(self.lib.mellow_debug_enable_taps(self.h, 1 if on else 0))

    def tap(self, name: str) -> torch.Tensor:
        n = C.c_int64(0)
        self._chk(self.lib.mellow_debug_tap(self.h, name.encode(), None, 0, C.byref(n)))
        out = torch.empty((n.value,), dtype=torch.float32, device=self.tdev)
        self._chk(self.lib.mellow_debug_tap(self.h, name.encode(), _ptr(out), n.value, C.byref(n)))
        return out

    # ---- measurement -----------------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        self._chk(self.lib.mellow_prof_enable(self.h, 1 if on else 0))

    def prof_reset(self):
        self._chk(self.lib.mellow_prof_reset(self.h))

    def prof_report(self):
        out = {}
        for i in range(self.lib.mellow_prof_num_families()):
            n, ms, fl, by = C.c_int64(0), C.c_double(0), C.c_double(0), C.c_double(0)
            self._chk(self.lib.mellow_prof_get(self.h, i, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
            out[self.lib.mellow_prof_family_name(i).decode()] = {
                "launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
        return out

    def last_phase_ms(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        self._chk(self.lib.mellow_last_phase_ms(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"encode_ms": a.value, "prefill_ms": b.value, "decode_ms": c.value}

    def set_graph(self, on: bool):
        self._chk(self.lib.mellow_set_graph(self.h, 1 if on else 0))


# ---- host-only helpers (usable without a GPU) ------------------------------------------------------------
def host_window_map(R: int, shift: int) -> np.ndarray:
    lib = load_library()
    out = (C.c_int32 * (R * R))()
    if lib.mellow_host_window_map(R, shift, out) != 0:
        raise EngineError(lib.mellow_last_error().decode())
    return np.asarray(list(out), dtype=np.int32)


def host_pack_weight(w: np.ndarray, npad: int = 128) -> np.ndarray:
    lib = load_library()
    w = np.ascontiguousarray(w, dtype=np.float32)
    N, K = w.shape
    NP, KP = (N + npad - 1) // npad * npad, (K + 31) // 32 * 32
    out = np.empty((NP // 32, KP // 8, 64, 4), dtype=np.float32)
    rc = lib.mellow_host_pack_weight(w.ctypes.data_as(C.POINTER(C.c_float)), N, K, npad,
                                     out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
    if rc != 0:
        raise EngineError(lib.mellow_last_error().decode())
    return out
