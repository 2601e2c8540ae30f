"""CPU: top log-probs (mellow_generate_top_logprobs, mellow_top_logprobs_apply, Engine.generate(top_logprobs=),
MellowWrapper.generate(top_logprobs=)) as far as it goes without a GPU: the exported symbols, the host-side refusals in their stated
order, the Engine's argument errors, the wrapper's keyword rules and the shaping of "top_logprobs" on a stub engine, the pool's
pass-through, and the numpy definition of tests/top_logprobs_ref.py against hand-made rows."""
import ctypes
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
import top_logprobs_ref as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mellow_generate_top_logprobs", "mellow_top_logprobs_apply")


def _lib():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    return E.load_library()


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    lib = _lib()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name, nargs in zip(NAMES, (4, 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)   # detected by symbol lookup, not by the number
    # the definition lines
    flat = " ".join(hdr.split())
    for line in ("Alternatives 0 .. k-1 are the first k tokens in the order (value descending, index ascending).",
                 "A -0 counts as +0", "Each alternative's log-prob is l[v] - lse, one fp32 subtraction.",
                 "lse = dec_lse_value(M, S)", "bit-equal to the call's out_logprob",
                 "A banned token (-inf) ranks last and reports -inf.", "reports NaN for all k log-probs",
                 "1 <= k <= 20 (TOP_LOGPROBS_MAX_K)", "1 << 24"):
        assert " ".join(line.replace("*", "").split()) in flat.replace(" * ", " "), line
    assert E.TOP_LOGPROBS_MAX_K == 20


def test_refusals_in_host_code_in_their_order():
    """no GPU here: every one of these returns before a device is touched.  The order: k, then the buffers, then the engine."""
    lib = _lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = lambda: lib.mellow_last_error().decode()      # noqa: E731
    for bad in (-1, 21, 1000):
        assert lib.mellow_generate_top_logprobs(None, bad, None, None) != 0 and "k must be" in err(), bad
        assert lib.mellow_top_logprobs_apply(None, None, None, None, 0, bad, None, None) != 0 and "k must be" in err(), bad
    for k in (1, 20):
        assert lib.mellow_generate_top_logprobs(None, k, None, p) != 0 and "null record buffer" in err()
        assert lib.mellow_generate_top_logprobs(None, k, p, None) != 0 and "null record buffer" in err()
        assert lib.mellow_top_logprobs_apply(None, p, p, p, 1, k, None, None) != 0 and "null record buffer" in err()
        assert lib.mellow_generate_top_logprobs(None, k, p, p) != 0 and "engine not finalized" in err()
        assert lib.mellow_top_logprobs_apply(None, p, p, p, 0, k, p, p) != 0 and "engine not finalized" in err()      # (before B <= 0)
    assert lib.mellow_generate_top_logprobs(None, 0, None, None) != 0 and "engine not finalized" in err()            # k = 0 needs no buffer


class OldLib:
    """a library built before mellow_generate_top_logprobs"""

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
    for kw in (dict(), dict(do_sample=True, seed=1), dict(num_return_sequences=2, do_sample=True, seed=1)):
        with pytest.raises(E.EngineError, match="predates mellow_generate_top_logprobs"):
            e.generate(a, a, ids, max_len=4, return_logprobs=True, top_logprobs=5, **kw)
    with pytest.raises(E.EngineError, match="predates mellow_generate_top_logprobs"):
        e.generate(a, a, np.zeros((2, 2, spec.TEXT_LEN), dtype=np.int64), max_len=4, return_logprobs=True, top_logprobs=5)
    with pytest.raises(E.EngineError, match="predates mellow_top_logprobs_apply"):
        e.top_logprobs_apply(np.zeros((2, V), dtype=np.float32), np.zeros((2, V // 32), dtype=np.float32), np.ones((2, V // 32), dtype=np.float32), 3)
    for kw, word in ((dict(top_logprobs=21, return_logprobs=True), "0 .off. to 20"), (dict(top_logprobs=-1, return_logprobs=True), "0 .off. to 20"),
                     (dict(top_logprobs=5), "return_logprobs"), (dict(top_logprobs=5, return_logprobs=True, num_beams=2), "num_beams")):
        with pytest.raises(ValueError, match=word):
            e.generate(a, a, ids, max_len=4, **kw)
    for k in (0, 21):
        with pytest.raises(ValueError):
            e.top_logprobs_apply(np.zeros((2, V), dtype=np.float32), np.zeros((2, V // 32), dtype=np.float32), np.ones((2, V // 32), dtype=np.float32), k)
    assert E.check_top_logprobs(0) == 0 and E.check_top_logprobs(20) == 20


# ---- the reference against hand-made rows ---------------------------------------------------------------------------------------------
def test_reference_orders_ties_by_index_and_zero_signs_together():
    row = np.array([1.0, 3.0, -0.0, 3.0, 0.0, 2.0, 3.0, -1.0], dtype=np.float32)
    ids, lp = TR.topk_rows(row, 8)
    assert ids.tolist() == [[1, 3, 6, 5, 0, 2, 4, 7]]              # the three 3.0 by index; -0 (index 2) before +0 (index 4): equal values
    assert lp.shape == (1, 8) and np.all(np.diff(lp[0]) <= 0)
    assert np.isclose(np.exp(TR.log_softmax64(row)).sum(), 1.0)
    assert lp[0, 0] == lp[0, 1] == lp[0, 2] and lp[0, 5] == lp[0, 6]
    ids3, lp3 = TR.topk_rows(np.stack([row, row[::-1]]), 3)
    assert ids3.tolist() == [[1, 3, 6], [1, 4, 6]] and np.array_equal(lp3[0], lp[0, :3])


def test_reference_fewer_than_k_finite_values():
    row = np.full(16, -np.inf, dtype=np.float32)
    row[[9, 2, 12]] = [0.5, 2.0, 0.5]
    ids, lp = TR.topk_rows(row, 6)
    assert ids.tolist() == [[2, 9, 12, 0, 1, 3]]                   # the finite ones in order, then the banned ones by index
    assert np.isfinite(lp[0, :3]).all() and np.isneginf(lp[0, 3:]).all()
    assert np.isclose(np.exp(lp[0, :3]).sum(), 1.0)


def test_reference_membership_check():
    L = np.array([5.0, 4.0, 3.0, 2.99, 0.0, -1.0], dtype=np.float32)
    assert TR.membership(L, [0, 1, 2], 0.05)[0] and TR.membership(L, [0, 1, 3], 0.05)[0]          # 2 and 3 lie within the band of each other
    assert not TR.membership(L, [0, 1, 4], 0.05)[0]                                             # (a): far below the k-th value
    assert not TR.membership(L, [0, 2, 3], 0.05)[0]                                             # (b): token 1 is clearly above it and missing
    assert not TR.membership(L, [0, 1, 1], 0.05)[0]                                             # an id twice
    assert not TR.membership(L, [0, 1, 3], 0.001)[0]
    assert TR.membership(L, [0, 1, 3], 0.05)[2] == 2


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
        toks[0, 2] = Tok.STOP                       # row 0 stops at its third token
        if max_len > 4:
            toks[1, 4:] = -1                        # row 1: its block exited after four tokens
        res = (toks, np.full(rows, max_len, dtype=np.int32), max_len, 1.5)
        if kw.get("return_logprobs"):
            res = res + (np.full(toks.shape, -0.5, dtype=np.float32),)
        k = int(kw.get("top_logprobs", 0))
        if k:
            ids = np.where(toks[:, :, None] >= 0, toks[:, :, None] + 100000 * np.arange(k)[None, None, :], -1).astype(np.int32)
            lp = np.where(toks[:, :, None] >= 0, -0.5 - np.arange(k, dtype=np.float32)[None, None, :], 0.0).astype(np.float32)
            res = res + (ids, lp)
        return res


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.stack([torch.full((8,), float(len(f))) for f in files])
    w.preprocess_text = lambda prompts: {"input_ids": torch.stack([torch.full((spec.TEXT_LEN,), len(p), dtype=torch.int64) for p in prompts])}
    return w


EX = [[f"a{i}.wav", f"b{i}.wav", "q" * (i + 1)] for i in range(3)]


def test_wrapper_zero_is_the_call_without_the_keyword():
    w = _wrapper()
    base = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True)
    same = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True, top_logprobs=0)
    text = w.generate(EX, 6, 0.8, 1.0, top_logprobs=0)
    assert same == base and all("top_logprobs" not in d for d in base) and all(isinstance(t, str) for t in text)
    assert all("top_logprobs" not in c for c in w.model.calls)
    assert sorted(w.model.calls[1]) == sorted(w.model.calls[0])


def test_wrapper_keyword_errors():
    w = _wrapper()
    for kw, word in ((dict(top_logprobs=5), "return_logprobs"), (dict(top_logprobs=21, return_logprobs=True), "0 .off. to 20"),
                     (dict(top_logprobs=-2, return_logprobs=True), "0 .off. to 20"),
                     (dict(top_logprobs=5, return_logprobs=True, num_beams=2), "num_beams")):
        with pytest.raises(ValueError, match=word):
            w.generate(EX, 6, 0.8, 1.0, **kw)
    with pytest.raises(TypeError):
        w.generate(EX, 6, 0.8, 1.0, "<|endoftext|>", True, False, None, True, 1, 1, 1.0, 1.0, 0, 0, None, None, 1.0, None, 5)      # keyword-only
    assert w.model.calls == []
    w._dp = lambda: (0, 2)
    with pytest.raises(NotImplementedError):          # return_logprobs is not sharded, with or without the alternatives
        w.generate(EX, 6, 0.8, 1.0, return_logprobs=True, top_logprobs=5)


def test_wrapper_shapes_the_alternatives_and_cuts_at_the_stop_token():
    w = _wrapper()
    plain = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True)
    out = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True, top_logprobs=3)
    assert w.model.calls[1]["top_logprobs"] == 3 and w.model.calls[1]["return_logprobs"]
    assert len(out) == 3
    for d, p in zip(out, plain):
        assert {k: v for k, v in d.items() if k != "top_logprobs"} == p          # everything else is the plain call's
        assert len(d["top_logprobs"]) == d["tokens"] == len(d["token_ids"])      # one list per counted token
        for tid, alts in zip(d["token_ids"], d["top_logprobs"]):
            assert [sorted(a) for a in alts] == [["logprob", "token", "token_id"]] * 3
            assert [a["token_id"] for a in alts] == [tid, tid + 100000, tid + 200000]      # best first, as the engine gave them
            assert [a["logprob"] for a in alts] == [-0.5, -1.5, -2.5]
            assert [a["token"] for a in alts] == [w.tokenizer.decode([a["token_id"]]) for a in alts]
    assert out[0]["tokens"] == 3 and out[0]["token_ids"][-1] == Tok.STOP         # the stop token is counted, nothing after it
    assert out[0]["top_logprobs"][-1][0]["token"] == "<|endoftext|>"
    assert out[1]["tokens"] == 4                                                 # never-computed columns give no list
    assert out[2]["tokens"] == 6


def test_wrapper_combines_with_the_other_keywords():
    w = _wrapper()
    negs = [[f"n{i}.wav", f"m{i}.wav", "x"] for i in range(3)]
    g = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True, top_logprobs=2, guidance_scale=2.0, negative_examples=negs,
                   no_repeat_ngram_size=2, do_sample=True, seed=3)
    c = w.model.calls[-1]
    assert c["top_logprobs"] == 2 and c["guidance_scale"] == 2.0 and c["no_repeat_ngram_size"] == 2 and c["do_sample"] and c["examples"] == 3
    assert len(g) == 3 and all(len(d["top_logprobs"]) == d["tokens"] and len(d["top_logprobs"][0]) == 2 for d in g)
    n = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True, top_logprobs=2, do_sample=True, seed=3, num_return_sequences=2)
    assert w.model.calls[-1]["num_return_sequences"] == 2 and w.model.calls[-1]["top_logprobs"] == 2
    assert [len(x) for x in n] == [2, 2, 2] and all(len(d["top_logprobs"]) == d["tokens"] for x in n for d in x)
    q = w.generate([["a.wav", "b.wav", ["q1", "q2 q"]], ["c.wav", "d.wav", "q3"]], 6, 0.8, 1.0, return_logprobs=True, top_logprobs=4)
    assert w.model.calls[-1]["top_logprobs"] == 4
    assert [len(x) for x in q] == [2, 1] and all(len(d["top_logprobs"][0]) == 4 for x in q for d in x)
    after = w.generate(EX, 6, 0.8, 1.0, return_logprobs=True)
    assert "top_logprobs" not in w.model.calls[-1] and all("top_logprobs" not in d for d in after)


def test_pool_passes_the_keyword_through():
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
    assert pool.generate_many(batches, max_len=4, return_logprobs=True, top_logprobs=8) == [2, 3]
    assert all(k["top_logprobs"] == 8 and k["return_logprobs"] for k in seen)
    assert "top_logprobs" in EnginePool.generate_many.__doc__
    pool._pool.shutdown()
