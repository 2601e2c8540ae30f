"""CPU: n answers per example (mellow_generate_n, Engine.generate(num_return_sequences=n), MellowWrapper.generate(
num_return_sequences=n)) as far as it goes without a GPU: the exported symbol, the planning of the 1024-row passes, and the
wrapper's nested results, errors and data-parallel arithmetic against a stub engine."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec
from mellow_amd.wrapper import MellowWrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_generate_n():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    assert re.search(r"\bint\s+mellow_generate_n\s*\(", hdr)
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    lib = E.load_library()
    raw = ctypes.CDLL(E.LIB_PATH)
    assert "mellow_generate_n" in E.EXPORTED_SYMBOLS
    assert hasattr(raw, "mellow_generate_n")
    assert lib.mellow_generate_n.restype is ctypes.c_int
    assert len(lib.mellow_generate_n.argtypes) == 20          # mellow_generate_scored's nineteen plus n
    assert lib.mellow_abi_minor() == 5                         # the current minor; added under minor 4: detected by symbol lookup


def test_plan_nseq_passes():
    assert E.plan_nseq_passes(3, 400, 5) == [(0, 2, 5), (2, 3, 805)]
    assert E.plan_nseq_passes(7, 1, 0) == [(0, 7, 0)]
    assert E.plan_nseq_passes(1024, 1, 3) == [(0, 1024, 3)]
    assert E.plan_nseq_passes(5, 1024, 0) == [(i, i + 1, 1024 * i) for i in range(5)]
    assert E.plan_nseq_passes(130, 8, 2) == [(0, 128, 2), (128, 130, 1026)]
    with pytest.raises(ValueError):
        E.plan_nseq_passes(1, 1025, 0)
    with pytest.raises(ValueError):
        E.plan_nseq_passes(1, 0, 0)


class OldLib:
    """a minor-4 library built before mellow_generate_n"""

    def mellow_last_error(self):
        return b""


def test_engine_argument_errors_need_no_gpu():
    e = object.__new__(E.Engine)
    e.lib, e.h = OldLib(), None
    e.tdev, e.lm = torch.device("cpu"), E.LMConfig.load()
    e._sync_inputs = lambda: None
    a = np.zeros((1, 8), dtype=np.float32)
    ids = np.zeros((1, spec.TEXT_LEN), dtype=np.int64)
    with pytest.raises(E.EngineError, match="predates mellow_generate_n"):
        e.generate(a, a, ids, max_len=4, do_sample=True, seed=1, num_return_sequences=2)
    with pytest.raises(ValueError, match="do_sample"):
        e.generate(a, a, ids, max_len=4, num_return_sequences=2)
    with pytest.raises(ValueError):
        e.generate(a, a, ids, max_len=4, do_sample=True, seed=1, num_return_sequences=0)


class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(t) == self.STOP else f"t{int(t)}" for t in ids)


class StubEngine:
    """row r of a call answers with tokens 1000 + 10 * (global row) + column; every third global row stops at column 2"""
    tdev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def max_new_tokens_limit(self):
        return 1000

    def generate(self, audio1, audio2, input_ids, max_len, **kw):
        self.calls.append(dict(kw, max_len=max_len, examples=len(audio1)))
        rows = len(audio1) * int(kw.get("num_return_sequences", 1))
        g = int(kw.get("row_offset", 0)) + np.arange(rows)
        toks = (1000 + 10 * g[:, None] + np.arange(max_len)[None, :]).astype(np.int32)
        toks[g % 3 == 0, 2] = Tok.STOP
        lens = np.where(g % 3 == 0, 2, max_len).astype(np.int32)
        lp = -(toks.astype(np.float32) % 7) / 8
        res = (toks, lens, max_len, 1.5)
        return res + (lp,) if kw.get("return_logprobs") else res


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


@pytest.fixture
def wrapper():
    return _wrapper()


EX = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]


def _text(g, L=5):
    """what the stub's global row g decodes to"""
    t = [1000 + 10 * g + c for c in range(L)]
    return "t%d t%d " % (t[0], t[1]) if g % 3 == 0 else " ".join(f"t{x}" for x in t)


def test_nested_strings(wrapper):
    out = wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=2)
    c = wrapper.model.calls[0]
    assert c["num_return_sequences"] == 2 and c["do_sample"] is True and c["seed"] == 11 and c["row_offset"] == 0 and c["examples"] == 3
    assert isinstance(out, list) and len(out) == 3 and all(isinstance(o, list) and len(o) == 2 for o in out)
    assert out == [[_text(2 * i), _text(2 * i + 1)] for i in range(3)]          # row b * n + j is answer j of example b


def test_nested_dicts_with_logprobs(wrapper):
    out = wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=4, return_logprobs=True)
    c = wrapper.model.calls[0]
    assert c["num_return_sequences"] == 4 and c["return_logprobs"] is True
    assert len(out) == 3 and all(len(o) == 4 for o in out)
    flat = _wrapper().generate([EX[i // 4] for i in range(12)], 5, 0.9, 0.7, do_sample=True, seed=11, return_logprobs=True)
    assert [a for o in out for a in o] == flat               # the dicts of the repeated call, grouped per example
    for o in out:
        assert sorted(o[0]) == ["logprob", "text", "token_ids", "token_logprobs", "tokens"]
        best = max(o, key=lambda a: a["logprob"])            # the re-ranking idiom of the docstring
        assert best["logprob"] == max(a["logprob"] for a in o)
    assert out[0][0]["token_ids"][-1] == Tok.STOP and out[0][0]["tokens"] == 3
    assert out[0][1]["tokens"] == 5


def test_value_errors(wrapper):
    with pytest.raises(ValueError, match="do_sample"):
        wrapper.generate(EX, 5, 0.8, 1.0, num_return_sequences=2)
    for bad in (0, -3):
        with pytest.raises(ValueError, match=">= 1"):
            wrapper.generate(EX, 5, 0.8, 1.0, do_sample=True, seed=1, num_return_sequences=bad)
    with pytest.raises(ValueError, match="1024"):
        wrapper.generate(EX, 5, 0.8, 1.0, do_sample=True, seed=1, num_return_sequences=1025)
    with pytest.raises(TypeError):
        wrapper.generate(EX, 5, 0.8, 1.0, "<|endoftext|>", True, True, 1, False, 2)        # keyword-only
    assert wrapper.model.calls == []


def test_default_call_is_unchanged(wrapper):
    out = wrapper.generate(EX, 5, 0.8, 1.0)
    assert out == [_text(0), _text(1), _text(2)]
    assert "num_return_sequences" not in wrapper.model.calls[0]          # today's engine call, keyword for keyword
    assert wrapper.generate(EX, 5, 0.8, 1.0, num_return_sequences=1) == out
    assert wrapper.model.calls[1] == wrapper.model.calls[0]
    s = wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=1)
    assert s == out and "num_return_sequences" not in wrapper.model.calls[2] and wrapper.model.calls[2]["row_offset"] == 0
    d = wrapper.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=1, return_logprobs=True)
    assert [r["text"] for r in d] == out                                  # flat, one dict per example


def test_data_parallel_row_offset_and_per_rank(monkeypatch):
    """rank 1 of 2 over three examples (shards 2 + 1) with n = 3: its rows start at lo * n = 6, the gather is asked for
    n_total * n = 9 rows in blocks of n * ceil(3 / 2) = 6, and n is part of what the ranks agree on"""
    import torch.distributed as tdist
    from mellow_amd import dist as mdist
    w = _wrapper()
    monkeypatch.setattr(w, "_dp", lambda: (1, 2))
    agreed, gathered = [], []
    monkeypatch.setattr(w, "_check_same_examples", lambda examples, extra=b"": agreed.append(extra))
    monkeypatch.setattr(tdist, "get_backend", lambda *a: "gloo")

    def fake_gather(toks, lens, n_total, max_len, device=None, per_rank=0):
        gathered.append(dict(rows=toks.shape[0], n_total=n_total, max_len=max_len, per_rank=per_rank))
        g = np.arange(n_total)                       # every rank's rows, as the stub engine answers them
        full = (1000 + 10 * g[:, None] + np.arange(max_len)[None, :]).astype(np.int32)
        full[g % 3 == 0, 2] = Tok.STOP
        assert np.array_equal(full[6:9], toks)       # this rank's block is rows 6..8 of the whole
        return full, np.where(g % 3 == 0, 2, max_len).astype(np.int32)

    monkeypatch.setattr(mdist, "gather_tokens", fake_gather)
    out = w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=3)
    c = w.model.calls[0]
    assert c["examples"] == 1 and c["row_offset"] == 6 and c["num_return_sequences"] == 3
    assert gathered == [dict(rows=3, n_total=9, max_len=5, per_rank=6)]
    assert b"nseq" in agreed[0] and b"3" in agreed[0] and agreed[0] != repr(("sample", 11, 0.9, 0.7)).encode()
    assert out == [[_text(3 * i + j) for j in range(3)] for i in range(3)]
    with pytest.raises(NotImplementedError):         # the log-prob record stays refused under sharding
        w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, num_return_sequences=3, return_logprobs=True)


def test_pool_advances_row_offset_by_rows():
    from mellow_amd.serve import EnginePool
    pool = object.__new__(EnginePool)
    seen = []

    class Eng:
        def generate(self, a1, a2, ids, **kw):
            seen.append(kw["row_offset"])
            return kw["row_offset"]

    import threading
    from concurrent.futures import ThreadPoolExecutor
    pool.engines, pool._locks, pool._pool = [Eng()], [threading.Lock()], ThreadPoolExecutor(max_workers=1)
    batches = [(np.zeros((2, 4)),) * 3, (np.zeros((3, 4)),) * 3, (np.zeros((1, 4)),) * 3]
    assert pool.generate_many(batches, do_sample=True, seed=1, row_offset=10, num_return_sequences=4) == [10, 18, 30]
    assert pool.generate_many(batches, do_sample=True, seed=1, row_offset=10) == [10, 12, 15]
    pool._pool.shutdown()
