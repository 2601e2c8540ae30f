"""CPU: the scoring interface (mellow_score / mellow_lm_score, Engine.score, MellowWrapper.score / choose) as far as it goes
without a GPU: exported symbols, the reference fixture tests/golden/score.npz against the CPU oracle, and the wrapper's
argument handling against a stub engine."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec
from mellow_amd.wrapper import MellowWrapper

SCORE_SYMBOLS = ("mellow_score", "mellow_lm_score")


def test_library_exports_the_scoring_symbols():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    lib = E.load_library()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name in SCORE_SYMBOLS:
        assert name in E.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.mellow_abi_minor() == 5          # the current minor; added under minor 4: detected by symbol lookup


def test_score_fixture_matches_the_cpu_oracle(synth_sd, golden_dir):
    """score.npz (the imported reference's `model(input_dict).logits`, reduced in fp64) against oracle.mellow_oracle.llama_forward
    + fp64 log_softmax on the reference's prefix: the oracle's logits are within 2e-3 of the reference's (test_oracle_golden.py),
    log-sum-exp is 1-Lipschitz in the max norm, so every statistic agrees within 4e-3 and the arg-max is equal (gaps >= 6e-3)."""
    from oracle import mellow_oracle as O
    g = np.load(os.path.join(golden_dir, "score.npz"))
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    cand, lens = torch.from_numpy(g["cand_ids"]), g["cand_len"]
    B, K, L = cand.shape
    assert (B, K, L) == (2, 3, 12) and lens.tolist() == [[12, 7, 1]] * 2
    assert float(g["top2_gap"].min()) >= 6e-3
    assert np.array_equal(g["cand_ids"][:, 0], np.load(os.path.join(golden_dir, "gen.npz"))["tokens"][:, :L])
    prefix = torch.from_numpy(e["prefix"])
    P = spec.PREFIX_LEN
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    for k in range(K):
        with torch.no_grad():
            seq = torch.cat((prefix, O.embed_tokens(synth_sd, cand[:, k])), 1)
            sc = O.llama_forward(synth_sd, O.LMParams(), seq)[:, P - 1: P - 1 + L].double()
        lse = torch.logsumexp(sc, -1)
        lp = torch.log_softmax(sc, -1).gather(-1, cand[:, k, :, None])[..., 0]
        assert float((lse - torch.from_numpy(g["lse"][:, k])).abs().max()) < 2e-3
        assert float((lp - torch.from_numpy(g["logprob"][:, k])).abs().max()) < 4e-3
        assert float((sc.max(-1).values - torch.from_numpy(g["max_logit"][:, k])).abs().max()) < 2e-3
        assert np.array_equal(sc.argmax(-1).numpy(), g["argmax"][:, k])


# ---- wrapper-level argument handling against a stub engine ---------------------------------------------------------------
class Tok:
    STOP = 7

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [100 + len(w) for w in s.split()]


class StubEngine:
    tdev = torch.device("cpu")

    def __init__(self, limit=20):
        self.limit = limit
        self.calls = []

    def max_candidate_tokens(self):
        return self.limit

    def score(self, audio1, audio2, input_ids, cand_ids, cand_len):
        cand_ids, cand_len = np.asarray(cand_ids), np.asarray(cand_len)
        self.calls.append((cand_ids.copy(), cand_len.copy()))
        lp = -(cand_ids % 10 + 1).astype(np.float32)            # token id -> a log-prob the test can predict
        lp = np.where(np.arange(cand_ids.shape[2])[None, None] < cand_len[..., None], lp, 0).astype(np.float32)
        return lp, lp.sum(-1), np.zeros_like(cand_ids, dtype=np.int32)


@pytest.fixture
def wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


EX = [["a.wav", "b.wav", "q1"], ["c.wav", "d.wav", "q2"]]


def test_score_pads_ragged_candidates_and_appends_stop(wrapper):
    res = wrapper.score(EX, [["a bb", "ccc"], ["dddd eeeee f"]])
    ids, lens = wrapper.model.calls[0]
    assert ids.shape == (2, 2, 4) and lens.tolist() == [[3, 2], [4, 4]]
    assert ids[0, 0].tolist() == [101, 102, 7, 0] and ids[0, 1].tolist() == [103, 7, 0, 0]
    assert ids[1, 0].tolist() == [104, 105, 101, 7] and ids[1, 1].tolist() == ids[1, 0].tolist()      # padded with the first candidate
    assert [len(r) for r in res] == [2, 1]                                                            # ... and dropped from the result
    assert res[0][0] == {"logprob": -(2 + 3 + 8), "tokens": 3, "token_logprobs": [-2.0, -3.0, -8.0]}
    assert res[0][1]["tokens"] == 2 and res[1][0]["tokens"] == 4
    assert all(isinstance(c["logprob"], float) for r in res for c in r)


def test_score_without_stop_and_choose(wrapper):
    res = wrapper.score(EX, [["a bb", "ccc"], ["dddd", "a"]], append_stop=False)
    ids, lens = wrapper.model.calls[0]
    assert lens.tolist() == [[2, 1], [1, 1]] and 7 not in ids
    assert [[c["logprob"] for c in r] for r in res] == [[-5.0, -4.0], [-5.0, -2.0]]
    assert wrapper.choose(EX, [["a bb", "ccc"], ["dddd", "a"]], append_stop=False) == [1, 1]
    # per token: -2.5 against -4 -> the longer answer wins; ties go to the lowest index
    assert wrapper.choose(EX, [["a bb", "ccc"], ["a", "a"]], normalize="mean", append_stop=False) == [0, 0]


def test_score_argument_errors(wrapper):
    with pytest.raises(ValueError, match="candidate lists"):
        wrapper.score(EX, [["a"]])
    with pytest.raises(ValueError, match="non-empty list"):
        wrapper.score(EX, [["a"], []])
    with pytest.raises(ValueError, match="non-empty list"):
        wrapper.score(EX, ["a", "b"])
    with pytest.raises(TypeError):
        wrapper.score(EX, [["a"], [3]])
    with pytest.raises(ValueError, match="no tokens"):
        wrapper.score(EX, [["a"], [""]], append_stop=False)
    with pytest.raises(ValueError, match="at most 20"):          # not clamped: the limit is named
        wrapper.score(EX, [["a"], [" ".join(["w"] * 20)]])
    with pytest.raises(ValueError, match="normalize"):
        wrapper.choose(EX, [["a"], ["b"]], normalize="max")
    with pytest.raises(RuntimeError):
        wrapper.score([], [])
    assert wrapper.model.calls == []


def test_score_is_refused_under_data_parallel_sharding(wrapper, monkeypatch):
    monkeypatch.setattr(wrapper, "_dp", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        wrapper.score(EX, [["a"], ["b"]])
    assert wrapper.model.calls == []
