"""CPU: beam search (mellow_generate_beam, mellow_beam_select, Engine.generate(num_beams=k), MellowWrapper.generate(num_beams=k))
as far as it goes without a GPU: the exported symbols, the argument rules, the backtracking of the tables, the final ranking, and
the fp64 reference of tests/beam_ref.py against hand-made steps."""
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
import beam_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_beam_symbols():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    lib = E.load_library()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name, nargs in (("mellow_generate_beam", 16), ("mellow_beam_select", 11)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_4
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert lib.mellow_generate_beam.argtypes[5:10] == [ctypes.c_int] * 5          # B, k, max_len, stop_id, ignore_stop
    assert lib.mellow_beam_select.argtypes[4:7] == [ctypes.c_int] * 3             # B, k, stop_id
    assert lib.mellow_abi_minor() == 5                         # the current minor; added under minor 4: detected by symbol lookup
    assert "65536" in hdr and "NaN candidate ranks as the arg-max kernel ranks" in hdr


def test_both_entry_points_refuse_a_null_engine():
    lib = E.load_library()
    for name in ("mellow_generate_beam", "mellow_beam_select"):
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p or hasattr(t, "contents") else t(1) for t in fn.argtypes]
        assert fn(*args) != 0
        assert "engine not finalized" in lib.mellow_last_error().decode()


class OldLib:
    """a minor-4 library built before mellow_generate_beam"""

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
    with pytest.raises(E.EngineError, match="predates mellow_generate_beam"):
        e.generate(a, a, ids, max_len=4, num_beams=2)
    with pytest.raises(E.EngineError, match="predates mellow_beam_select"):
        e.beam_select(np.zeros((2, 8), dtype=np.float32), np.zeros(2), np.zeros(2), k=2)
    with pytest.raises(ValueError, match="do_sample"):
        e.generate(a, a, ids, max_len=4, num_beams=2, do_sample=True, seed=1)
    with pytest.raises(ValueError, match="questions"):
        e.generate(a, a, np.zeros((2, 2, spec.TEXT_LEN), dtype=np.int64), max_len=4, num_beams=2)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="num_beams"):
            e.generate(a, a, ids, max_len=4, num_beams=bad)
    for m in (0, 3):
        with pytest.raises(ValueError, match="num_return_sequences"):
            e.generate(a, a, ids, max_len=4, num_beams=2, num_return_sequences=m)
    e.precision = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        e.generate(a, a, ids, max_len=4, num_beams=2)


def test_row_and_staging_bounds():
    E.check_beam_request(128, 8, 64)                          # 1024 rows, 65536 rows x positions: the largest call
    E.check_beam_request(1024, 1, 300)                        # k = 1 stages nothing
    with pytest.raises(ValueError, match="1024"):
        E.check_beam_request(129, 8, 4)                       # 1032 rows
    with pytest.raises(ValueError, match="1024"):
        E.check_beam_request(1025, 1, 4)
    with pytest.raises(ValueError, match="65536"):
        E.check_beam_request(128, 8, 65)                      # 66560
    with pytest.raises(ValueError, match="65536"):
        E.check_beam_request(2, 2, 16385)
    E.check_beam_request(2, 2, 16384)
    assert E.BEAM_STAGE_ROWS * 30 * 3 * 64 * 4 == 1509949440  # the 1.5 GB per tensor of the header


def test_backtrack_displaced_and_reentered_beam():
    """k = 3, one example.  Step 0 expands beam 0.  Step 1: beam 1 is displaced (nobody continues it) and beam 0 is continued
    twice.  Step 2: the row that beam 1 lost is re-entered by a child of row 0, and rows swap."""
    parent = np.array([[0, 0, 0], [0, 0, 2], [2, 0, 1]])
    token = np.array([[10, 11, 12], [20, 21, 22], [30, 31, 32]])
    lp = -np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])
    toks, lps = E.backtrack_beams(parent, token, lp, 3)
    assert toks.tolist() == [[12, 22, 30], [10, 20, 31], [10, 21, 32]]
    assert np.allclose(lps, -np.array([[0.3, 0.6, 0.7], [0.1, 0.4, 0.8], [0.1, 0.5, 0.9]]))
    assert toks.dtype == np.int32 and lps.dtype == np.float64
    # two examples: the parent index is relative to the example
    p2 = np.concatenate([parent, parent], axis=1)
    t2 = np.concatenate([token, token + 100], axis=1)
    toks2, _ = E.backtrack_beams(p2, t2, np.concatenate([lp, lp], axis=1), 3)
    assert toks2[:3].tolist() == toks.tolist() and (toks2[3:] == toks + 100).all()
    with pytest.raises(ValueError):
        E.backtrack_beams(parent, token, lp, 2)
    with pytest.raises(ValueError):
        E.backtrack_beams(parent + 1, token, lp, 3)


def test_backtrack_finished_beam_frozen_with_lp_zero():
    """k = 2, stop id 7: beam 1 takes the stop id at step 1 and is then carried (parent = its own index, token 7, lp 0), moving to
    index 0 at step 3 when its frozen cum beats the running beam's"""
    parent = np.array([[0, 0], [0, 1], [0, 1], [1, 0]])
    token = np.array([[5, 6], [8, 7], [9, 7], [7, 3]])
    lp = np.array([[-1.0, -2.0], [-0.5, -0.25], [-0.5, 0.0], [0.0, -1.5]])
    toks, lps = E.backtrack_beams(parent, token, lp, 2)
    assert toks.tolist() == [[6, 7, 7, 7], [5, 8, 9, 3]]
    assert lps.tolist() == [[-2.0, -0.25, 0.0, 0.0], [-1.0, -0.5, -0.5, -1.5]]
    cum = lps.sum(axis=1)
    order, lengths, counts, scores = E.rank_beams(toks, lps, cum, 2, 7, 1.0)
    assert lengths.tolist() == [1, 4] and counts.tolist() == [2, 4]
    assert np.allclose(scores, [-2.25 / 2, -3.5 / 4]) and order.tolist() == [[1, 0]]


@pytest.mark.parametrize("lp_exp, want", [(0.0, [0, 2, 1]), (1.0, [1, 2, 0]), (2.0, [1, 2, 0])])
def test_final_ranking_with_length_penalty(lp_exp, want):
    """three hypotheses of one example, stop id 0, the stop id counted: 2 tokens / logprob -1.8, 6 tokens / -3.0, 3 tokens / -2.4;
    penalty 0 ranks by logprob, 1 by the mean per token (-0.9, -0.5, -0.8), 2 favours the long one further"""
    toks = np.array([[4, 0, 0, 0, 0, 0], [4, 5, 6, 7, 8, 0], [4, 5, 0, 0, 0, 0]])
    cum = np.array([-1.8, -3.0, -2.4])
    order, lengths, counts, scores = E.rank_beams(toks, np.zeros(toks.shape), cum, 3, 0, lp_exp)
    assert lengths.tolist() == [1, 5, 2] and counts.tolist() == [2, 6, 3]
    assert np.allclose(scores, cum / np.array([2.0, 6.0, 3.0]) ** lp_exp)
    assert order.tolist() == [want]
    assert scores.dtype == np.float64


def test_final_ranking_ties_go_to_the_beam_index_and_ignore_stop_counts_every_step():
    toks = np.array([[1, 0, 2], [3, 0, 4]])
    order, lengths, counts, scores = E.rank_beams(toks, np.zeros(toks.shape), np.array([-3.0, -3.0]), 2, 0, 1.0, ignore_stop=True)
    assert lengths.tolist() == [3, 3] and counts.tolist() == [3, 3] and order.tolist() == [[0, 1]] and np.allclose(scores, -1.0)


def test_reference_selection_step_by_hand():
    """V = 4, k = 2, one example: row 0 (cum -1) and row 1 (cum -1.5, uniform logits)"""
    l0 = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    l1 = np.zeros(4)
    parent, token, cum, lp, gaps = R.select_step(np.stack([l0, l1]), [-1.0, -1.5], [0, 0], 2, stop_id=3)
    assert parent.tolist() == [0, 0] and token.tolist() == [0, 1]
    assert np.allclose(cum, [-1.0 + np.log(0.5), -1.0 + np.log(0.25)]) and np.allclose(lp, np.log([0.5, 0.25]))
    # the third best: row 1's four tokens tie at -1.5 - log 4 = -2.886 against row 0's -1 + log 0.125 = -3.08
    assert np.isclose(gaps[0], min(np.log(2.0), (-1.0 + np.log(0.25)) - (-1.5 - np.log(4.0))))
    # a finished row offers one candidate with increment 0; ties on c go to the lower parent, then the lower token
    parent, token, cum, lp, _ = R.select_step(np.stack([l1, l1]), [-2.0, -2.0 - np.log(4.0)], [0, 1], 2, stop_id=3)
    assert parent.tolist() == [0, 0] and token.tolist() == [0, 1] and np.allclose(cum, -2.0 - np.log(4.0))
    parent, token, cum, lp, _ = R.select_step(np.stack([l1, l1]), [-2.0, -2.0], [0, 1], 2, stop_id=3)
    assert parent.tolist() == [1, 0] and token.tolist() == [3, 0] and lp.tolist()[0] == 0.0 and cum[0] == -2.0
    # cum = -inf never wins against a finite candidate
    parent, *_ = R.select_step(np.stack([l0, l0 + 50]), [0.0, -np.inf], [0, 0], 2, stop_id=3)
    assert parent.tolist() == [0, 0]


def test_reference_search_and_backtrack_agree():
    """a tiny model whose next-token logits depend on the history: the sequences the search tracks are the ones the tables give"""
    rng = np.random.default_rng(3)
    W = rng.standard_normal((7, 7)) * 2

    def fn(step, seqs):
        return np.stack([W[s[-1]] + 0.3 * len(s) * W[s[0]] if s else W[0] for s in seqs])

    out = R.search(fn, B=2, k=3, max_len=5, stop_id=6)
    toks, lps = E.backtrack_beams(out["parent"], out["token"], out["lp"], 3)
    assert np.allclose(lps.sum(axis=1), out["cum"])
    assert len(set(map(tuple, toks[:3].tolist()))) == 3        # an example's hypotheses are distinct
    for r in range(6):                                          # after a stop id only stop ids with increment 0
        hit = np.nonzero(toks[r] == 6)[0]
        if hit.size:
            assert (toks[r, hit[0]:] == 6).all() and (lps[r, hit[0] + 1:] == 0).all()


# ---- wrapper --------------------------------------------------------------------------------------------------------------
class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(t) == self.STOP else f"t{int(t)}" for t in ids)


class StubEngine:
    """hypothesis j of example b: tokens 1000 + 100 b + 10 j + column, stop at column 2 for j = 0"""
    tdev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def max_new_tokens_limit(self):
        return 1000

    def generate(self, audio1, audio2, input_ids, max_len, **kw):
        self.calls.append(dict(kw, max_len=max_len, examples=len(audio1)))
        m = int(kw.get("num_return_sequences", 1))
        B = len(audio1)
        b, j = np.divmod(np.arange(B * m), m)
        toks = (1000 + 100 * b[:, None] + 10 * j[:, None] + np.arange(max_len)[None, :]).astype(np.int32)
        toks[j == 0, 2:] = Tok.STOP
        lens = np.where(j == 0, 2, max_len).astype(np.int32)
        lp = np.where(toks == Tok.STOP, 0.0, -0.5).astype(np.float32)
        lp[j == 0, 2] = -0.25
        res = (toks, lens, max_len, 1.5)
        if kw.get("return_logprobs"):
            res = res + (lp, -(1.0 + j).astype(np.float64)) if "num_beams" in kw else res + (lp,)
        return res


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


EX = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]


def test_wrapper_strings_and_nesting():
    w = _wrapper()
    out = w.generate(EX, 5, 0.8, 1.0, num_beams=4, length_penalty=0.5)
    c = w.model.calls[0]
    assert c["num_beams"] == 4 and c["length_penalty"] == 0.5 and c["num_return_sequences"] == 1 and c["examples"] == 3
    assert c["stop_id"] == Tok.STOP and "do_sample" not in c
    assert out == ["t%d t%d " % (1000 + 100 * b, 1001 + 100 * b) for b in range(3)]
    out = w.generate(EX, 5, 0.8, 1.0, num_beams=4, num_return_sequences=2)
    assert len(out) == 3 and all(isinstance(o, list) and len(o) == 2 for o in out)
    assert out[1][1] == " ".join(f"t{1110 + c}" for c in range(5))


def test_wrapper_dicts_carry_the_score():
    w = _wrapper()
    out = w.generate(EX, 5, 0.8, 1.0, num_beams=3, num_return_sequences=3, return_logprobs=True)
    assert len(out) == 3 and all(len(o) == 3 for o in out)
    d = out[0][0]
    assert sorted(d) == ["logprob", "score", "text", "token_ids", "token_logprobs", "tokens"]
    assert d["token_ids"] == [1000, 1001, Tok.STOP] and d["tokens"] == 3 and d["logprob"] == -1.25 and d["score"] == -1.0
    assert out[2][1]["score"] == -2.0 and out[2][1]["tokens"] == 5
    flat = w.generate(EX, 5, 0.8, 1.0, num_beams=3, return_logprobs=True)
    assert [r["text"] for r in flat] == [o[0]["text"] for o in out]


def test_wrapper_errors():
    w = _wrapper()
    with pytest.raises(ValueError, match="do_sample"):
        w.generate(EX, 5, 0.8, 1.0, num_beams=2, do_sample=True, seed=1)
    with pytest.raises(ValueError, match="question"):
        w.generate([["a.wav", "b.wav", ["q1", "q2"]]], 5, 0.8, 1.0, num_beams=2)
    with pytest.raises(ValueError, match="num_beams"):
        w.generate(EX, 5, 0.8, 1.0, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match="num_beams"):
        w.generate(EX, 5, 0.8, 1.0, num_beams=9)
    with pytest.raises(ValueError, match="num_beams"):
        w.generate(EX, 5, 0.8, 1.0, num_beams=0)
    with pytest.raises(ValueError, match="65536"):
        w.generate([EX[0]] * 100, 900, 0.8, 1.0, num_beams=8)
    with pytest.raises(TypeError):
        w.generate(EX, 5, 0.8, 1.0, "<|endoftext|>", True, False, None, False, 1, 2)        # keyword-only
    assert w.model.calls == []
    w._dp = lambda: (0, 2)
    with pytest.raises(NotImplementedError):
        w.generate(EX, 5, 0.8, 1.0, num_beams=2)


def test_num_beams_one_is_the_call_without_the_keyword():
    w = _wrapper()
    base = w.generate(EX, 5, 0.8, 1.0)
    assert w.generate(EX, 5, 0.8, 1.0, num_beams=1, length_penalty=2.0) == base
    assert w.model.calls[1] == w.model.calls[0] and "num_beams" not in w.model.calls[0]


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
    assert pool.generate_many(batches, max_len=4, num_beams=4, length_penalty=0.0, num_return_sequences=2) == [2, 3]
    assert all(k["num_beams"] == 4 and k["length_penalty"] == 0.0 and k["num_return_sequences"] == 2 for k in seen)
    pool._pool.shutdown()
