"""CPU: several questions per example (mellow_generate_q, Engine.generate with input_ids [B][Q][text_len], MellowWrapper.generate
with a list of prompts) as far as it goes without a GPU: the exported symbol, and the wrapper's nesting, ragged padding, row
accounting and refusals against a stub engine."""
import ctypes
import os
import re
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec
from mellow_amd.wrapper import MellowWrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_generate_q():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    assert re.search(r"\bint\s+mellow_generate_q\s*\(", hdr)
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    lib = E.load_library()
    raw = ctypes.CDLL(E.LIB_PATH)
    assert "mellow_generate_q" in E.EXPORTED_SYMBOLS and "mellow_generate_q" in E._ADDED_UNDER_MINOR_4
    assert hasattr(raw, "mellow_generate_q")
    assert lib.mellow_generate_q.restype is ctypes.c_int
    assert len(lib.mellow_generate_q.argtypes) == 20          # mellow_generate_scored's nineteen plus Q
    assert lib.mellow_abi_minor() == 5                         # the current minor; added under minor 4: detected by symbol lookup


class OldLib:
    """a minor-4 library built before mellow_generate_q"""

    def mellow_last_error(self):
        return b""


def _bare_engine(precision="f32x3"):
    e = object.__new__(E.Engine)
    e.lib, e.h, e.precision = OldLib(), None, precision
    e.tdev, e.lm = torch.device("cpu"), E.LMConfig.load()
    e._sync_inputs = lambda: None
    return e


def test_engine_argument_errors_need_no_gpu():
    e = _bare_engine()
    a = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, 3, spec.TEXT_LEN), dtype=np.int64)
    with pytest.raises(E.EngineError, match="predates mellow_generate_q"):
        e.generate(a, a, ids, max_len=4)
    with pytest.raises(ValueError, match="num_return_sequences"):
        e.generate(a, a, ids, max_len=4, do_sample=True, seed=1, num_return_sequences=2)
    e.lib.mellow_generate_q = None                             # (present: the checks behind the lookup are reached)
    with pytest.raises(ValueError, match="at least one question"):
        e.generate(a, a, np.zeros((2, 0, spec.TEXT_LEN), dtype=np.int64), max_len=4)
    with pytest.raises(ValueError, match="1024"):
        e.generate(a, a, np.zeros((2, 513, spec.TEXT_LEN), dtype=np.int64), max_len=4)
    with pytest.raises(IndexError):
        e.generate(a, a, np.full((2, 3, spec.TEXT_LEN), e.lm.vocab_size, dtype=np.int64), max_len=4)
    e8 = _bare_engine("fp8")
    e8.lib.mellow_generate_q = None
    with pytest.raises(ValueError, match="fp8"):
        e8.generate(a, a, ids, max_len=4)


class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(t) == self.STOP else f"t{int(t)}" for t in ids)


class StubEngine:
    """row r of a call answers with tokens 1000 + 10 * (global row) + column; every third global row stops at column 2.  Rows per
    example: the second dimension of 3-D ids."""
    tdev = torch.device("cpu")
    precision = "f32x3"

    def __init__(self):
        self.calls = []

    def max_new_tokens_limit(self):
        return 1000

    def generate(self, audio1, audio2, input_ids, max_len, **kw):
        self.calls.append(dict(kw, max_len=max_len, examples=len(audio1), ids=input_ids))
        rows = len(audio1) * (input_ids.shape[1] if input_ids.ndim == 3 else 1)
        g = int(kw.get("row_offset", 0)) + np.arange(rows)
        toks = (1000 + 10 * g[:, None] + np.arange(max_len)[None, :]).astype(np.int32)
        toks[g % 3 == 0, 2] = Tok.STOP
        lens = np.where(g % 3 == 0, 2, max_len).astype(np.int32)
        lp = -(toks.astype(np.float32) % 7) / 8
        res = (toks, lens, max_len, 1.5)
        return res + (lp,) if kw.get("return_logprobs") else res


PROMPT_CODE = {}


def _code(prompt):
    """a distinct id per prompt string, so that the ids a stub call receives say which question sits in which row"""
    return PROMPT_CODE.setdefault(prompt, 1 + len(PROMPT_CODE))


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.tensor([[_code(p)] * spec.TEXT_LEN for p in prompts], dtype=torch.int64)}
    return w


@pytest.fixture
def wrapper():
    return _wrapper()


def _text(g, L=5):
    """what the stub's global row g decodes to"""
    t = [1000 + 10 * g + c for c in range(L)]
    return "t%d t%d " % (t[0], t[1]) if g % 3 == 0 else " ".join(f"t{x}" for x in t)


EXQ = [[f"a{i}.wav", f"b{i}.wav", [f"q{i}x", f"q{i}y", f"q{i}z"]] for i in range(2)]


def test_nested_strings_in_question_order(wrapper):
    out = wrapper.generate(EXQ, 5, 0.8, 1.0)
    c = wrapper.model.calls[0]
    assert tuple(c["ids"].shape) == (2, 3, spec.TEXT_LEN) and c["examples"] == 2           # one audio pair per example
    assert c["ids"][:, :, 0].tolist() == [[_code(f"q{i}{s}") for s in "xyz"] for i in range(2)]
    assert "do_sample" not in c and "num_return_sequences" not in c                         # greedy: today's keywords
    assert out == [[_text(3 * i + j) for j in range(3)] for i in range(2)]                  # row i * Q + j answers question j of example i
    t = wrapper.generate([EXQ[0][:2] + [tuple(EXQ[0][2])]], 5, 0.8, 1.0)                    # a tuple is a list of questions too
    assert t == [[_text(j) for j in range(3)]]


def test_ragged_counts_are_padded_with_the_first_question_and_trimmed(wrapper):
    ex = [["a0.wav", "b0.wav", ["only"]], ["a1.wav", "b1.wav", ["u", "v", "w"]], ["a2.wav", "b2.wav", "plain string"],
          ["a3.wav", "b3.wav", ["s", "t"]]]
    out = wrapper.generate(ex, 5, 0.9, 0.7, do_sample=True, seed=11)
    c = wrapper.model.calls[0]
    assert tuple(c["ids"].shape) == (4, 3, spec.TEXT_LEN)
    code = lambda *p: [_code(x) for x in p]
    assert c["ids"][:, :, 0].tolist() == [code("only", "only", "only"), code("u", "v", "w"),
                                          code("plain string", "plain string", "plain string"), code("s", "t", "s")]
    assert c["do_sample"] is True and c["seed"] == 11 and c["row_offset"] == 0
    # answer j of example i is global row i * Q + j of the PADDED layout (Q = 3), padded answers dropped
    assert out == [[_text(0)], [_text(3), _text(4), _text(5)], [_text(6)], [_text(9), _text(10)]]


def test_dicts_with_logprobs(wrapper):
    out = wrapper.generate(EXQ, 5, 0.8, 1.0, return_logprobs=True)
    assert wrapper.model.calls[0]["return_logprobs"] is True
    assert len(out) == 2 and all(len(o) == 3 for o in out)
    flat = _wrapper().generate([[f"a{i}.wav", f"b{i}.wav", "q"] for i in range(6)], 5, 0.8, 1.0, return_logprobs=True)
    assert [a for o in out for a in o] == flat               # the dicts of the expanded call, grouped per example
    assert sorted(out[0][0]) == ["logprob", "text", "token_ids", "token_logprobs", "tokens"]


def test_all_strings_is_todays_call(wrapper):
    ex = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]
    out = wrapper.generate(ex, 5, 0.8, 1.0)
    c = wrapper.model.calls[0]
    assert tuple(c["ids"].shape) == (3, spec.TEXT_LEN)                                      # 2-D ids
    assert sorted(k for k in c if k != "ids") == ["examples", "max_len", "stop_id", "temperature", "top_p"]
    assert out == [_text(0), _text(1), _text(2)]                                            # flat strings
    wrapper.generate(ex, 5, 0.9, 0.7, do_sample=True, seed=3)
    s = wrapper.model.calls[1]
    assert tuple(s["ids"].shape) == (3, spec.TEXT_LEN)
    assert sorted(k for k in s if k != "ids") == ["do_sample", "examples", "max_len", "row_offset", "seed", "stop_id", "temperature", "top_p"]


def test_refusals(wrapper, monkeypatch):
    with pytest.raises(ValueError, match="empty"):
        wrapper.generate([["a.wav", "b.wav", []]], 5, 0.8, 1.0)
    with pytest.raises(ValueError, match="num_return_sequences"):
        wrapper.generate(EXQ, 5, 0.9, 0.7, do_sample=True, seed=1, num_return_sequences=2)
    with pytest.raises(ValueError, match="1024"):
        wrapper.generate([["a.wav", "b.wav", ["q"] * 513], ["c.wav", "d.wav", "r"]], 5, 0.8, 1.0)
    monkeypatch.setattr(wrapper.model, "precision", "fp8")
    with pytest.raises(ValueError, match="fp8"):
        wrapper.generate(EXQ, 5, 0.8, 1.0)
    assert wrapper.generate([["a.wav", "b.wav", ["one"]]], 5, 0.8, 1.0) == [[_text(0)]]      # Q = 1 works there
    monkeypatch.setattr(wrapper.model, "precision", "f32x3")
    monkeypatch.setattr(wrapper, "_dp", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        wrapper.generate(EXQ, 5, 0.8, 1.0)
    assert len(wrapper.model.calls) == 1


def test_max_len_is_clamped_as_today(wrapper):
    with pytest.warns(UserWarning, match="clamped"):
        wrapper.generate(EXQ, 5000, 0.8, 1.0)
    assert wrapper.model.calls[0]["max_len"] == 1000


def test_pool_advances_row_offset_by_questions():
    from mellow_amd.serve import EnginePool
    pool = object.__new__(EnginePool)

    class Eng:
        def generate(self, a1, a2, ids, **kw):
            return kw["row_offset"]

    pool.engines, pool._locks, pool._pool = [Eng()], [threading.Lock()], ThreadPoolExecutor(max_workers=1)
    q = lambda B, Q: (np.zeros((B, 4)), np.zeros((B, 4)), np.zeros((B, Q, spec.TEXT_LEN), dtype=np.int64))
    plain = (np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((3, spec.TEXT_LEN), dtype=np.int64))
    assert pool.generate_many([q(2, 4), plain, q(1, 5), q(2, 1)], do_sample=True, seed=1, row_offset=10) == [10, 18, 21, 26]
    pool._pool.shutdown()
