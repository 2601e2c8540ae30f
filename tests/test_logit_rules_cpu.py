"""CPU: the repetition controls (mellow_generate_rules, mellow_logit_rules_apply, Engine.generate(repetition_penalty=...),
MellowWrapper.generate(repetition_penalty=..., suppress_tokens=...)) as far as they go without a GPU: the exported symbols and the
struct, the host-side refusals, the float32 reference of tests/logit_rules_ref.py against hand-made rows, the wrapper's keyword rules
on a stub engine, and the pool's pass-through."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec
from mellow_amd.wrapper import MellowWrapper

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_rules_ref as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mellow_generate_rules", "mellow_logit_rules_apply")


def _lib():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    return E.load_library()


def _rules(**f):
    r = E.LogitRules(size=ctypes.sizeof(E.LogitRules), repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, logit_bias=None)
    for k, v in f.items():
        setattr(r, k, v)
    return r


def test_header_declares_and_library_exports_the_symbols_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    lib = _lib()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name, nargs in zip(NAMES, (2, 11)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_4 + E._ADDED_UNDER_MINOR_5
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    m = re.search(r"typedef struct mellow_logit_rules \{(.*?)\} mellow_logit_rules_t;", hdr, re.S)
    assert m, "the struct is not declared"
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == ["size", "repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "logit_bias"]
    assert [f[0] for f in E.LogitRules._fields_] == fields
    assert ctypes.sizeof(E.LogitRules) == 24 and E.LogitRules.logit_bias.offset == 16        # size first, the pointer aligned
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)   # detected by symbol lookup, not by the number
    assert "no longer" in hdr or "NOT the number" in hdr                                     # the log-prob note


def test_refusals_in_host_code():
    """no GPU here: every one of these returns before a device is touched"""
    lib = _lib()
    ok = _rules(repetition_penalty=1.2, no_repeat_ngram_size=2)
    assert lib.mellow_generate_rules(None, ctypes.byref(ok)) != 0
    assert "engine not finalized" in lib.mellow_last_error().decode()
    assert lib.mellow_generate_rules(None, None) != 0
    assert "engine not finalized" in lib.mellow_last_error().decode()
    assert lib.mellow_logit_rules_apply(None, ctypes.byref(ok), None, 1, None, 0, None, 0, None, None, None) != 0
    assert "engine not finalized" in lib.mellow_last_error().decode()
    bad = [(_rules(size=20), "size"), (_rules(size=0), "size"), (_rules(repetition_penalty=0.0), "repetition_penalty"),
           (_rules(repetition_penalty=-1.5), "repetition_penalty"), (_rules(repetition_penalty=math.nan), "repetition_penalty"),
           (_rules(repetition_penalty=math.inf), "repetition_penalty"), (_rules(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
           (_rules(min_new_tokens=-1), "min_new_tokens")]
    for r, word in bad:
        assert lib.mellow_generate_rules(None, ctypes.byref(r)) != 0
        assert word in lib.mellow_last_error().decode(), word
        assert lib.mellow_logit_rules_apply(None, ctypes.byref(r), None, 1, None, 0, None, 0, None, None, None) != 0
        assert word in lib.mellow_last_error().decode(), word


class OldLib:
    """a library built before mellow_generate_rules"""

    def mellow_last_error(self):
        return b""


def _bare_engine():
    e = object.__new__(E.Engine)
    e.lib, e.h = OldLib(), None
    e.tdev, e.lm = torch.device("cpu"), E.LMConfig.load()
    e._sync_inputs = lambda: None
    return e


def test_engine_argument_errors_need_no_gpu():
    e = _bare_engine()
    a = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, spec.TEXT_LEN), dtype=np.int64)
    V = e.lm.vocab_size
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(logit_bias=np.zeros(V)),
               dict(_arm_neutral_rules=True), dict(repetition_penalty=1.2, num_beams=2), dict(no_repeat_ngram_size=1, do_sample=True, seed=1)):
        with pytest.raises(E.EngineError, match="predates mellow_generate_rules"):
            e.generate(a, a, ids, max_len=4, **kw)
    with pytest.raises(E.EngineError, match="predates mellow_logit_rules_apply"):
        e.logit_rules_apply(np.zeros((1, V), dtype=np.float32), np.zeros((1, 4)), np.zeros(1), no_repeat_ngram_size=1)
    for kw, word in ((dict(repetition_penalty=0), "repetition_penalty"), (dict(repetition_penalty=math.nan), "repetition_penalty"),
                     (dict(repetition_penalty=math.inf), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                     (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=5), "max_len"),
                     (dict(logit_bias=np.zeros(V - 1)), "vocabulary"), (dict(logit_bias=np.full(V, np.nan)), "finite or -inf"),
                     (dict(logit_bias=np.where(np.arange(V) == 3, np.inf, 0.0)), "finite or -inf")):
        with pytest.raises(ValueError, match=word):
            e.generate(a, a, ids, max_len=4, **kw)
    with pytest.raises(ValueError, match="8192"):
        e.generate(a, a, ids, max_len=8193, no_repeat_ngram_size=2)
    assert E.check_logit_rules(1.5, 2, 3, np.full(V, -np.inf), V)[3].dtype == np.float32      # -inf everywhere is the caller's business


# ---- the reference by hand --------------------------------------------------------------------------------------------------------------
def test_reference_penalty_once_per_token_and_by_sign():
    l = np.array([2.0, -2.0, 0.0, 3.0, -0.0, 5.0], dtype=np.float32)
    out = LR.apply_row(l, [0, 1, 0, 0, 2, 4], repetition_penalty=2.0)
    assert out.dtype == np.float32
    assert out.tolist() == [1.0, -4.0, 0.0, 3.0, -0.0, 5.0]            # token 0 three times: divided once; the direction flips at 0
    assert np.signbit(out[4]) and not np.signbit(out[2])
    t = np.float32(1.3)
    out = LR.apply_row(np.array([0.7, -0.7], dtype=np.float32), [1, 0, 1], repetition_penalty=1.3)
    assert out[0] == np.float32(0.7) / t and out[1] == np.float32(-0.7) * t
    assert LR.apply_row(l, [], repetition_penalty=2.0).tolist() == l.tolist()
    assert LR.apply_row(l, [3], repetition_penalty=0.5).tolist() == [2.0, -2.0, 0.0, 6.0, -0.0, 5.0]


def test_reference_ngram_bans():
    l = np.zeros(8, dtype=np.float32)

    def banned(h, n):
        return np.nonzero(np.isneginf(LR.apply_row(l, h, no_repeat_ngram_size=n)))[0].tolist()

    assert banned([], 1) == [] and banned([5], 1) == [5] and banned([5, 2, 5], 1) == [2, 5]        # n = 1: the whole history
    assert banned([], 2) == [] and banned([3], 2) == []                                            # no earlier bigram start matches
    assert banned([1, 2, 1], 2) == [2]                                                             # ... 1 -> 2 seen: after 1, not 2
    assert banned([1, 2, 1, 3, 1], 2) == [2, 3]
    assert banned([1, 1], 2) == [1]
    assert banned([1], 3) == [] and banned([1, 2], 3) == []                                        # s = n - 1: nothing to match yet
    assert banned([1, 2, 4, 1, 2], 3) == [4]
    assert banned([1, 2, 4, 2, 1], 3) == []
    assert banned([7, 7, 7], 3) == [7]
    assert banned([1, 2, 3], 0) == []


def test_reference_min_new_tokens_boundary_and_bias():
    l = np.arange(6, dtype=np.float32)
    for s, hit in ((0, True), (2, True), (3, False), (4, False)):
        out = LR.apply_row(l, [1] * s, min_new_tokens=3, stop_id=4)
        assert np.isneginf(out[4]) == hit and np.isfinite(np.delete(out, 4)).all()
    assert np.isfinite(LR.apply_row(l, [], min_new_tokens=3, stop_id=-1)).all()                    # no stop id: nothing to ban
    bias = np.array([0.5, -np.inf, 0.0, -1.0, 0.0, 0.0], dtype=np.float32)
    out = LR.apply_row(l, [3], repetition_penalty=2.0, bias=bias)
    assert out.tolist() == [0.5, -np.inf, 2.0, 0.5, 4.0, 5.0]                                      # penalty first (3 / 2), then the bias
    val, idx = LR.tile_partials(np.concatenate([np.full(32, -np.inf), np.arange(32.0)]).astype(np.float32)[None])
    assert np.isneginf(val[0, 0]) and idx[0].tolist() == [0, 63]
    assert LR.merged_lse(val, np.array([[0.0, 1.5]])) == pytest.approx(31.0 + math.log(1.5))
    ls = LR.log_softmax64(out[None])[0]
    assert np.isneginf(ls[1]) and np.exp(ls).sum() == pytest.approx(1.0)


# ---- wrapper ----------------------------------------------------------------------------------------------------------------------------
class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(t) == self.STOP else f"t{int(t)}" for t in ids)


class StubEngine:
    tdev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def max_new_tokens_limit(self):
        return 1000

    def generate(self, audio1, audio2, input_ids, max_len, **kw):
        self.calls.append(dict(kw, max_len=max_len, examples=len(audio1)))
        rows = len(audio1) * int(kw.get("num_return_sequences", 1)) * (input_ids.shape[1] if input_ids.ndim == 3 else 1)
        toks = (1000 + np.arange(rows)[:, None] * 10 + np.arange(max_len)[None, :]).astype(np.int32)
        res = (toks, np.full(rows, max_len, dtype=np.int32), max_len, 1.5)
        if kw.get("return_logprobs"):
            lp = np.full(toks.shape, -0.5, dtype=np.float32)
            res = res + (lp, np.zeros(rows)) if "num_beams" in kw else res + (lp,)
        return res


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


EX = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]
RULE_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "logit_bias", "suppress_tokens")


def test_wrapper_neutral_values_arm_nothing():
    w = _wrapper()
    base = w.generate(EX, 5, 0.8, 1.0)
    same = w.generate(EX, 5, 0.8, 1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[], logit_bias={})
    assert same == base and w.model.calls[1] == w.model.calls[0]
    assert not any(k in w.model.calls[0] for k in RULE_KEYS)


def test_wrapper_passes_the_rules_on_every_route():
    w = _wrapper()
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2, suppress_tokens=[5, 9], logit_bias={9: 1.0, 11: -2.5, 12: -math.inf})
    w.generate(EX, 5, 0.8, 1.0, **kw)
    w.generate(EX, 5, 0.8, 1.0, do_sample=True, seed=1, num_return_sequences=2, return_logprobs=True, **kw)
    w.generate(EX, 5, 0.8, 1.0, num_beams=3, **kw)
    w.generate([["a.wav", "b.wav", ["q1", "q2"]]], 5, 0.8, 1.0, **kw)
    assert len(w.model.calls) == 4
    for c in w.model.calls:
        assert c["repetition_penalty"] == 1.2 and c["no_repeat_ngram_size"] == 3 and c["min_new_tokens"] == 2
        assert "suppress_tokens" not in c                                    # merged into the dense vector
        b = c["logit_bias"]
        assert b.dtype == np.float32 and b.shape == (49152,)
        assert np.isneginf(b[[5, 9, 12]]).all() and b[11] == np.float32(-2.5) and np.count_nonzero(b) == 4
    assert w.model.calls[2]["num_beams"] == 3 and w.model.calls[1]["num_return_sequences"] == 2
    only = _wrapper()
    only.generate(EX, 5, 0.8, 1.0, no_repeat_ngram_size=2)
    assert [k for k in RULE_KEYS if k in only.model.calls[0]] == ["no_repeat_ngram_size"]


def test_wrapper_keyword_errors():
    w = _wrapper()
    for kw, word in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1), "repetition_penalty"),
                     (dict(repetition_penalty=math.nan), "repetition_penalty"), (dict(repetition_penalty=math.inf), "repetition_penalty"),
                     (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(min_new_tokens=-1), "min_new_tokens"),
                     (dict(min_new_tokens=6), "max_len"), (dict(suppress_tokens=[49152]), "vocabulary"), (dict(suppress_tokens=[-1]), "vocabulary"),
                     (dict(logit_bias={49152: 1.0}), "vocabulary"), (dict(logit_bias={3: math.nan}), "finite or -inf"),
                     (dict(logit_bias={3: math.inf}), "finite or -inf")):
        with pytest.raises(ValueError, match=word):
            w.generate(EX, 5, 0.8, 1.0, **kw)
        with pytest.raises(ValueError, match=word):
            w.generate(EX, 5, 0.8, 1.0, num_beams=2, **kw)
    with pytest.raises(TypeError):
        w.generate(EX, 5, 0.8, 1.0, "<|endoftext|>", True, False, None, False, 1, 1, 1.0, 1.2)        # keyword-only
    assert w.model.calls == []


def test_pool_passes_the_keywords_through():
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from mellow_amd.serve import EnginePool
    pool = object.__new__(EnginePool)
    seen = []

    class Eng:
        def generate(self, a1, a2, ids, **kw):
            seen.append(kw)
            return len(a1)

    pool.engines, pool._locks, pool._pool = [Eng()], [threading.Lock()], ThreadPoolExecutor(max_workers=1)
    batches = [(np.zeros((2, 4)),) * 3, (np.zeros((3, 4)),) * 3]
    bias = np.zeros(49152, dtype=np.float32)
    assert pool.generate_many(batches, max_len=4, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=1, logit_bias=bias) == [2, 3]
    assert all(k["repetition_penalty"] == 1.3 and k["no_repeat_ngram_size"] == 2 and k["min_new_tokens"] == 1 and k["logit_bias"] is bias for k in seen)
    pool._pool.shutdown()
