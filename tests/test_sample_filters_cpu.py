"""CPU: the sampler's candidate filters top_k / min_p (include/mellow_hip.h, mellow_generate_filters) above the kernel -- the ABI, the
host-side errors of the C entry, the fp64 reference's own properties, what Engine.generate arms before every C call of every route
(against the recording fake library of tests/test_engine_calls_cpu.py, extended by the one arm symbol), and the wrapper's keywords."""
import ctypes as C
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
import sampler_filters_ref as F  # noqa: E402
import sampler_ref as R  # noqa: E402
import test_engine_calls_cpu as calls  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 49152
NEW = ("mellow_generate_filters", "mellow_sample_logits_filtered")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    return E.load_library()


def _f(top_k=0, min_p=0.0, size=None):
    return E.SampleFilters(size=C.sizeof(E.SampleFilters) if size is None else size, top_k=top_k, min_p=min_p)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_symbols_and_struct_are_declared_exported_and_under_minor_5(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)
    m = re.search(r"typedef struct mellow_sample_filters \{(.*?)\}\s*mellow_sample_filters_t;", hdr, re.S)
    assert m and re.findall(r"(int32_t|float)\s+(\w+);", m.group(1)) == [("int32_t", "size"), ("int32_t", "top_k"), ("float", "min_p")]
    assert C.sizeof(E.SampleFilters) == 12 and [f[0] for f in E.SampleFilters._fields_] == ["size", "top_k", "min_p"]
    raw = C.CDLL(E.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5 and hasattr(raw, name)
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.mellow_generate_filters.argtypes) == 2 and len(lib.mellow_sample_logits_filtered.argtypes) == 10
    # a library that predates them still loads; the Engine methods then say what is missing
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {"mellow_last_error": lambda self: b""})(), None
    e.tdev, e.lm, e._sync_inputs = torch.device("cpu"), E.LMConfig.load(), lambda: None
    a, ids = np.zeros((1, 8), dtype=np.float32), np.zeros((1, spec.TEXT_LEN), dtype=np.int64)
    with pytest.raises(E.EngineError, match="predates mellow_generate_filters"):
        e.generate(a, a, ids, max_len=4, do_sample=True, seed=1, top_k=5)
    with pytest.raises(E.EngineError, match="predates mellow_sample_logits_filtered"):
        e.sample_logits(np.zeros((1, V), dtype=np.float32), 1.0, 1.0, 1, 0, min_p=0.5)


def test_c_entry_errors_come_in_the_stated_order_without_a_device(lib):
    def err(fn, *a):
        assert fn(*a) != 0
        return lib.mellow_last_error().decode()

    arm = lib.mellow_generate_filters
    # value rules first (host code; the engine is NULL throughout), in the order size, top_k, min_p
    assert "size is 8" in err(arm, None, C.byref(_f(top_k=-1, min_p=2.0, size=8)))
    assert "top_k must be >= 0 (got -1)" in err(arm, None, C.byref(_f(top_k=-1, min_p=2.0)))
    for bad in (float("nan"), -0.25, 1.5, float("inf")):
        assert "min_p must be in [0, 1]" in err(arm, None, C.byref(_f(top_k=3, min_p=bad)))
    # then the engine
    for ok in (_f(), _f(top_k=50), _f(min_p=1.0), _f(top_k=2 ** 31 - 1, min_p=0.05)):
        assert "engine not finalized" in err(arm, None, C.byref(ok))
    assert "engine not finalized" in err(arm, None, None)
    tap = lib.mellow_sample_logits_filtered
    assert "top_k must be >= 0" in err(tap, None, None, 1, None, 0, 1.0, 1.0, 0, C.byref(_f(top_k=-7)), None)
    assert "min_p must be in [0, 1]" in err(tap, None, None, 1, None, 0, 1.0, 1.0, 0, C.byref(_f(min_p=1.25)), None)
    assert "engine not finalized" in err(tap, None, None, 1, None, 0, 1.0, 1.0, 0, C.byref(_f(top_k=4)), None)


def test_python_value_rules():
    assert E.check_sample_filters() == (0, 0.0) and E.check_sample_filters(50, 0.05) == (50, 0.05)
    assert E.check_sample_filters(np.int64(7), np.float32(0.5)) == (7, 0.5) and E.check_sample_filters(2 ** 40, 1)[0] == 2 ** 31 - 1
    for bad in (dict(top_k=-1), dict(top_k=2.5), dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan"))):
        with pytest.raises(ValueError):
            E.check_sample_filters(**bad)


# ---- the reference ----------------------------------------------------------------------------------------------------------

def _ref_rows():
    rng = np.random.default_rng(1)
    return [rng.standard_normal(V).astype(np.float32) * 8.0, rng.standard_normal(V).astype(np.float32) * 0.3,
            np.round(rng.standard_normal(V) * 2.0).astype(np.float32)]


def test_reference_neutral_filters_are_the_nucleus_reference():
    for b, row in enumerate(_ref_rows()):
        for (top_p, T, seed, step) in ((0.9, 1.0, 7, 0), (0.5, 0.7, 2 ** 40 + 3, 5), (1.0, 1.3, 99, 63), (0.0, 1.0, 1, 2)):
            tok, gap, mm = R.sample_ref(row, top_p, T, seed, 100 + b, step)
            for K in (0, V, V + 5):
                got = F.sample_ref(row, K, top_p, 0.0, T, seed, 100 + b, step)
                assert got[0] == tok and got[1] == pytest.approx(gap) and got[3] == np.inf, (b, top_p, K)
                assert (got[2] == np.inf) == (mm == np.inf) and (mm == np.inf or got[2] == pytest.approx(mm, rel=1e-6, abs=1e-9))
            k0 = F.kept_mask(row, 0, top_p, 0.0, T)
            k1, _ = R.nucleus_mask(R.scaled(row, T), top_p)
            assert np.array_equal(k0, k1)


def test_reference_top_k_1_and_min_p_1_are_the_arg_max():
    for row in _ref_rows():
        first = int(np.argmax(row))
        for seed in (0, 5, 2 ** 50):
            assert F.sample_ref(row, 1, 0.9, 0.0, 0.7, seed, 3, 4)[0] == first
        tied = np.nonzero(row == row.max())[0]
        assert np.array_equal(np.nonzero(F.kept_mask(row, 0, 1.0, 1.0, 1.0))[0], tied)
        assert F.sample_ref(row, 0, 1.0, 1.0, 1.0, 9, 0, 0)[0] in tied
    nan = _ref_rows()[0].copy()
    nan[[4000, 17]] = np.nan
    assert F.sample_ref(nan, 5, 0.5, 0.5, 1.0, 1, 0, 0) == (17, np.inf, np.inf, np.inf)


def test_reference_kept_sets_are_nested_prefixes_of_exact_size():
    for row in _ref_rows():
        order = np.lexsort((np.arange(V), -R.scaled(row, 0.9).astype(np.float64)))
        prev = None
        for K in (1, 2, 7, 40, 1000, V - 1, V):
            kept = F.kept_mask(row, K, 1.0, 0.0, 0.9)
            assert kept.sum() == K and kept[order[:K]].all()            # exactly K: a tie group on the K-th value is cut by index
            assert prev is None or not (prev & ~kept).any()
            prev = kept
        prev = None
        for mp in (1.0, 0.5, 0.1, 0.02, 1e-4, 0.0):
            kept = F.kept_mask(row, 0, 1.0, mp, 0.9)
            n = int(kept.sum())
            assert n >= 1 and kept[order[:n]].all()                     # a prefix of the order
            assert prev is None or not (prev & ~kept).any()
            prev = kept
        assert prev.all()
        # the intersection: the nucleus is taken INSIDE the top-k set, so it can only be smaller than either alone
        both = F.kept_mask(row, 40, 0.9, 0.02, 0.9)
        assert not (both & ~F.kept_mask(row, 40, 1.0, 0.0, 0.9)).any() and not (both & ~F.kept_mask(row, 0, 1.0, 0.02, 0.9)).any()
        n = int(both.sum())
        assert both[order[:n]].all()
        p = F.filtered_probs(row, 40, 0.9, 0.02, 0.9)
        assert abs(p.sum() - 1.0) < 1e-12 and np.array_equal(p > 0, both)


# ---- Engine.generate against the recording fake ---------------------------------------------------------------------------------

class FakeLib(calls.FakeLib):
    def mellow_generate_filters(self, h, ref):
        f = ref._obj
        self.calls.append(("mellow_generate_filters", (f.size, f.top_k, f.min_p), ()))
        self.armed["filters"] = True
        return 0


def _engine():
    e = calls._engine()
    e.lib = FakeLib(e.lm.vocab_size)
    return e


def _arm(top_k, min_p):
    return ("mellow_generate_filters", (12, top_k, float(np.float32(min_p))), ())


SAMPLED = dict(do_sample=True, seed=1)


def test_filters_are_armed_before_every_c_call_of_every_route():
    e = _engine()
    a1, a2, ids = calls._inputs(4)
    n1, n2, nids = calls._inputs(4, base=50.0)
    for kw, syms in ((dict(), ["mellow_generate_sampled"]),
                     (dict(return_logprobs=True), ["mellow_generate_scored"]),
                     (dict(num_return_sequences=2), ["mellow_generate_n"]),
                     (dict(guidance_scale=2.0, negative=(n1, n2, nids)), ["mellow_generate_guidance", "mellow_generate_sampled"]),
                     (dict(return_logprobs=True, top_logprobs=3, **calls.RULES),
                      ["mellow_generate_rules", "mellow_generate_top_logprobs", "mellow_generate_scored"])):
        e.lib.calls.clear()
        e.generate(a1, a2, ids, max_len=4, top_k=50, min_p=0.05, **SAMPLED, **kw)
        names = [c[0] for c in e.lib.calls]
        assert names[-1] == syms[-1] and names[-2] == "mellow_generate_filters" and sorted(names[:-2]) == sorted(syms[:-1]), kw
        assert e.lib.calls[-2] == _arm(50, 0.05), kw
    e.lib.calls.clear()
    q1, q2, qids = calls._inputs(2, Q=2)
    e.generate(q1, q2, qids, max_len=4, top_k=7, **SAMPLED)
    assert [c[0] for c in e.lib.calls] == ["mellow_generate_filters", "mellow_generate_q"] and e.lib.calls[0] == _arm(7, 0.0)
    # one value alone arms, too
    e.lib.calls.clear()
    e.generate(a1, a2, ids, max_len=4, min_p=0.25, **SAMPLED)
    assert e.lib.calls[0] == _arm(0, 0.25) and e.lib.calls[1][0] == "mellow_generate_sampled"
    # more than 1024 rows: B = 5, n = 400 run as three C calls, each behind its own arm call
    e.lib.calls.clear()
    b1, b2, bids = calls._inputs(5)
    res = e.generate(b1, b2, bids, max_len=4, stop_id=5, seed=11, do_sample=True, num_return_sequences=400, top_k=3, min_p=0.5)
    assert [c[0] for c in e.lib.calls] == ["mellow_generate_filters", "mellow_generate_n"] * 3
    assert all(c == _arm(3, 0.5) for c in e.lib.calls[0::2]) and res[0].shape == (2000, 4)
    # the generation calls themselves are those of the un-filtered call, argument for argument
    plain = _engine()
    plain.generate(b1, b2, bids, max_len=4, stop_id=5, seed=11, do_sample=True, num_return_sequences=400)
    assert calls._shape(plain.lib.calls) == calls._shape(e.lib.calls[1::2])


def test_neutral_values_arm_nothing_and_the_call_is_todays():
    a1, a2, ids = calls._inputs(3)
    for kw in (dict(), dict(do_sample=True, seed=2), dict(return_logprobs=True), dict(num_beams=2),
               dict(do_sample=True, seed=2, num_return_sequences=2)):
        e, p = _engine(), _engine()
        e.generate(a1, a2, ids, max_len=4, top_k=0, min_p=0.0, **kw)
        p.generate(a1, a2, ids, max_len=4, **kw)
        assert calls._shape(e.lib.calls) == calls._shape(p.lib.calls) and "mellow_generate_filters" not in [c[0] for c in e.lib.calls], kw


def test_engine_value_errors_come_before_any_c_call():
    e = _engine()
    a1, a2, ids = calls._inputs(2)
    with pytest.raises(ValueError, match="do_sample=True"):
        e.generate(a1, a2, ids, max_len=4, top_k=5)
    with pytest.raises(ValueError, match="do_sample=True"):
        e.generate(a1, a2, ids, max_len=4, min_p=0.1, return_logprobs=True)
    with pytest.raises(ValueError, match="num_beams"):
        e.generate(a1, a2, ids, max_len=4, num_beams=2, top_k=5)
    for bad in (dict(top_k=-1), dict(min_p=1.5), dict(min_p=-0.5), dict(min_p=float("nan")), dict(top_k=1.5)):
        with pytest.raises(ValueError):
            e.generate(a1, a2, ids, max_len=4, **SAMPLED, **bad)
    with pytest.raises(ValueError, match="filtered=False"):
        e.sample_logits(np.zeros((1, V), dtype=np.float32), 1.0, 1.0, 1, 0, top_k=4, filtered=False)
    assert e.lib.calls == []


def test_a_failing_filtered_call_leaves_nothing_armed():
    e = _engine()
    a1, a2, ids = calls._inputs(3)
    e.lib.fail = True
    with pytest.raises(E.EngineError, match="the fake library failed"):
        e.generate(a1, a2, ids, max_len=4, top_k=9, **SAMPLED)
    e.lib.calls.clear()
    e.generate(a1, a2, ids, max_len=4, **SAMPLED)
    assert [c[0] for c in e.lib.calls] == ["mellow_generate_sampled"] and e.lib.armed == {}


def test_sample_logits_picks_the_symbol():
    seen = []

    class Lib:
        def mellow_last_error(self):
            return b""

        def mellow_sample_logits(self, h, l, B, rid, step, top_p, T, seed, out):
            seen.append(("plain", B, step, top_p, T, seed))
            return 0

        def mellow_sample_logits_filtered(self, h, l, B, rid, step, top_p, T, seed, f, out):
            seen.append(("filtered", B, step, top_p, T, seed, f._obj.size, f._obj.top_k, f._obj.min_p))
            return 0

    e = calls._engine()
    e.lib = Lib()
    L = np.zeros((2, V), dtype=np.float32)
    e.sample_logits(L, 0.9, 0.7, 5, 3)
    e.sample_logits(L, 0.9, 0.7, 5, 3, top_k=40)
    e.sample_logits(L, 0.9, 0.7, 5, 3, min_p=0.5)
    e.sample_logits(L, 0.9, 0.7, 5, 3, filtered=True)
    assert seen == [("plain", 2, 3, 0.9, 0.7, 5), ("filtered", 2, 3, 0.9, 0.7, 5, 12, 40, 0.0), ("filtered", 2, 3, 0.9, 0.7, 5, 12, 0, 0.5),
                    ("filtered", 2, 3, 0.9, 0.7, 5, 12, 0, 0.0)]


# ---- the wrapper ------------------------------------------------------------------------------------------------------------

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
        toks = (1000 + 10 * np.arange(rows)[:, None] + np.arange(max_len)[None, :]).astype(np.int32)
        res = (toks, np.full((rows,), max_len, dtype=np.int32), max_len, 1.5)
        return res + (np.zeros_like(toks, dtype=np.float32),) if kw.get("return_logprobs") else res


def _wrapper():
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = Tok(), StubEngine(), False
    w.preprocess_audio = lambda files, resample: torch.zeros((len(files), 8))
    w.preprocess_text = lambda prompts: {"input_ids": torch.zeros((len(prompts), spec.TEXT_LEN), dtype=torch.int64)}
    return w


EX = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]


def test_wrapper_passes_the_keywords_on_every_route_and_is_off_by_default():
    w = _wrapper()
    out = w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, top_k=50, min_p=0.05)
    assert len(out) == 3 and all(isinstance(t, str) for t in out)
    c = w.model.calls[0]
    assert c["top_k"] == 50 and c["min_p"] == 0.05 and c["do_sample"] is True
    w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, top_k=4, num_return_sequences=2)
    assert w.model.calls[1]["top_k"] == 4 and w.model.calls[1]["min_p"] == 0.0 and w.model.calls[1]["num_return_sequences"] == 2
    w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, min_p=0.2, return_logprobs=True)
    assert w.model.calls[2]["min_p"] == 0.2 and w.model.calls[2]["return_logprobs"] is True
    q = [["a.wav", "b.wav", ["q one", "q two"]], ["c.wav", "d.wav", "q"]]
    ans = w.generate(q, 5, 0.9, 0.7, do_sample=True, seed=11, top_k=9, min_p=0.3)
    assert [len(a) if isinstance(a, list) else 1 for a in ans] == [2, 1]
    assert w.model.calls[3]["top_k"] == 9 and w.model.calls[3]["min_p"] == 0.3
    # off by default (Hugging Face's top_k = 50 is not adopted): the engine call has neither keyword
    for kw in (dict(), dict(do_sample=True, seed=11), dict(do_sample=True, seed=11, top_k=0, min_p=0.0)):
        w.generate(EX, 5, 0.9, 0.7, **kw)
        assert "top_k" not in w.model.calls[-1] and "min_p" not in w.model.calls[-1]


def test_wrapper_value_errors():
    w = _wrapper()
    with pytest.raises(ValueError, match="do_sample=True"):
        w.generate(EX, 5, 0.9, 0.7, top_k=5)
    with pytest.raises(ValueError, match="do_sample=True"):
        w.generate(EX, 5, 0.9, 0.7, min_p=0.1)
    with pytest.raises(ValueError, match="num_beams"):
        w.generate(EX, 5, 0.9, 0.7, num_beams=2, top_k=5)
    for bad in (dict(top_k=-2), dict(min_p=2.0), dict(min_p=float("nan"))):
        with pytest.raises(ValueError):
            w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=1, **bad)
    assert w.model.calls == []


def test_data_parallel_ranks_agree_on_the_filter_values(monkeypatch):
    import torch.distributed as tdist
    from mellow_amd import dist as mdist
    sigs = []
    for kw in (dict(), dict(top_k=50), dict(top_k=40), dict(min_p=0.05), dict(top_k=50, min_p=0.05), dict(top_k=50, min_p=0.1)):
        w = _wrapper()
        monkeypatch.setattr(w, "_dp", lambda: (0, 2))
        agreed = []
        monkeypatch.setattr(w, "_check_same_examples", lambda examples, extra=b"", _a=agreed: _a.append(extra))
        monkeypatch.setattr(tdist, "get_backend", lambda *a: "gloo")
        monkeypatch.setattr(mdist, "gather_tokens", lambda toks, lens, n_total, max_len, device=None, per_rank=0:
                            (np.zeros((n_total, max_len), dtype=np.int32), np.zeros((n_total,), dtype=np.int32)))
        w.generate(EX, 5, 0.9, 0.7, do_sample=True, seed=11, **kw)
        assert len(agreed) == 1
        sigs.append(agreed[0])
        assert w.model.calls[0].get("top_k", 0) == kw.get("top_k", 0) and w.model.calls[0].get("min_p", 0.0) == kw.get("min_p", 0.0)
    assert len(set(sigs)) == len(sigs)                                   # every pair of values is a signature of its own
    assert sigs[0] == repr(("sample", 11, 0.9, 0.7)).encode()            # without the keywords: today's signature
