"""CPU: log-probs of the generated tokens (mellow_generate_scored, Engine.generate(return_logprobs=True),
MellowWrapper.generate(return_logprobs=True)) as far as they go without a GPU: the exported symbols, and the wrapper's result
layout, stop-token counting rule and fp32 sum against a stub engine."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec
from mellow_amd.wrapper import MellowWrapper

NEW_SYMBOLS = ("mellow_generate_scored", "mellow_debug_dec_head_lse")


def test_library_exports_the_logprob_symbols():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    lib = E.load_library()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in E.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.mellow_abi_minor() == 5          # the current minor; added under minor 4: detected by symbol lookup


class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(t) == self.STOP else f"t{int(t)}" for t in ids)


# rows: stops at column 2; never stops; stops at once; its block left early (-1 = never computed)
TOKS = np.array([[11, 12, 7, 13, 14],
                 [21, 22, 23, 24, 25],
                 [7, 31, 32, 33, 34],
                 [41, 42, -1, -1, -1]], dtype=np.int32)
# values whose fp32 ascending sum differs from the fp64 sum rounded once and from the descending fp32 sum
LP = np.array([[-4e-8, -1.0, -4e-8, -9.0, -9.0],
               [-0.1, -0.2, -0.3, -0.4, -0.7],
               [-2.5, -9.0, -9.0, -9.0, -9.0],
               [-0.5, -0.25, 0.0, 0.0, 0.0]], dtype=np.float32)


class StubEngine:
    tdev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def max_new_tokens_limit(self):
        return 1000

    def generate(self, audio1, audio2, input_ids, max_len, **kw):
        self.calls.append(dict(kw, max_len=max_len))
        B = len(audio1)
        res = (TOKS[:B].copy(), np.array([2, 5, 0, 2], dtype=np.int32)[:B], 5, 1.5)
        return res + (LP[:B].copy(),) if kw.get("return_logprobs") else res


@pytest.fixture
def wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


EX = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(4)]


def test_return_logprobs_layout_and_stop_counting(wrapper):
    res = wrapper.generate(EX, 5, 0.8, 1.0, return_logprobs=True)
    assert wrapper.model.calls[0]["return_logprobs"] is True and wrapper.model.calls[0]["stop_id"] == Tok.STOP
    assert [sorted(r) for r in res] == [["logprob", "text", "token_ids", "token_logprobs", "tokens"]] * 4
    # the tokens before the first stop id plus the stop id itself (score()'s append_stop=True convention)
    assert res[0]["token_ids"] == [11, 12, 7] and res[0]["tokens"] == 3 and res[0]["text"] == "t11 t12 "
    # a row that never produced the stop id: everything it generated
    assert res[1]["token_ids"] == [21, 22, 23, 24, 25] and res[1]["tokens"] == 5
    # the stop id as the first token: one counted token, empty text
    assert res[2]["token_ids"] == [7] and res[2]["tokens"] == 1 and res[2]["text"] == ""
    # columns that were never computed (-1) are not counted
    assert res[3]["token_ids"] == [41, 42] and res[3]["tokens"] == 2 and res[3]["token_logprobs"] == [-0.5, -0.25]
    for r, lp in zip(res, LP):
        assert r["token_logprobs"] == [float(x) for x in lp[: r["tokens"]]]
        assert isinstance(r["logprob"], float) and all(isinstance(x, float) for x in r["token_logprobs"])


def test_logprob_is_the_fp32_ascending_sum(wrapper):
    res = wrapper.generate(EX, 5, 0.8, 1.0, return_logprobs=True)
    for r, lp in zip(res, LP):
        want = np.float32(0)
        for x in lp[: r["tokens"]]:
            want = np.float32(want + x)
        assert r["logprob"] == float(want)
    # row 0 tells the orders apart: (-4e-8 + -1) + -4e-8 = -1 in fp32; summed from the small end, or in fp64, it is below -1
    assert res[0]["logprob"] == -1.0
    assert float(np.float32(np.float32(LP[0, 2] + LP[0, 0]) + LP[0, 1])) != -1.0


def test_default_call_is_unchanged(wrapper):
    out = wrapper.generate(EX, 5, 0.8, 1.0)
    assert out == ["t11 t12 ", "t21 t22 t23 t24 t25", "", "t41 t42"]
    assert "return_logprobs" not in wrapper.model.calls[0]            # today's engine call, keyword for keyword
    assert wrapper.generate(EX, 5, 0.8, 1.0, return_logprobs=False) == out
    assert "return_logprobs" not in wrapper.model.calls[1]
    # sampling keywords behave as before, with and without the log-probs
    res = wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, return_logprobs=True)
    c = wrapper.model.calls[2]
    assert c["do_sample"] is True and c["seed"] == 11 and c["row_offset"] == 0 and wrapper.last_seed == 11
    assert [r["text"] for r in res] == out
    wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, return_logprobs=True)
    assert wrapper.model.calls[3]["seed"] == wrapper.last_seed


def test_return_logprobs_is_refused_under_data_parallel_sharding(wrapper, monkeypatch):
    monkeypatch.setattr(wrapper, "_dp", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        wrapper.generate(EX, 5, 0.8, 1.0, return_logprobs=True)
    assert wrapper.model.calls == []


class OldLib:
    """a minor-4 library built before the log-prob symbols"""

    def mellow_last_error(self):
        return b""


def test_an_older_library_raises_the_need_error():
    e = object.__new__(E.Engine)
    e.lib, e.h = OldLib(), None
    with pytest.raises(E.EngineError, match="predates mellow_generate_scored"):
        e._need("mellow_generate_scored")
    e.tdev, e.lm = torch.device("cpu"), E.LMConfig.load()
    with pytest.raises(E.EngineError, match="predates mellow_debug_dec_head_lse"):
        e.debug_dec_head_lse(torch.zeros((1, 576)))
    e._sync_inputs = lambda: None
    a = np.zeros((1, 8), dtype=np.float32)
    with pytest.raises(E.EngineError, match="predates mellow_generate_scored"):
        e.generate(a, a, np.zeros((1, spec.TEXT_LEN), dtype=np.int64), max_len=4, return_logprobs=True)
