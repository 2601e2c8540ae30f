"""CPU: constrained decoding (mellow_generate_constraint, mellow_constraint_apply, Engine.generate(constraint=...),
MellowWrapper.generate(choices=...)) as far as it goes without a GPU: the exported symbols and the struct, the host-side refusals in
their stated order, the trie builder against its inverse, the reference semantics of tests/constraint_ref.py by hand, the
sum-to-one property of the constrained distribution, the wrapper's keyword rules on a stub engine, the pool's pass-through and the
slicing under a stubbed two-rank shard."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from mellow_amd import constraint as MC
from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as CR  # noqa: E402
import logit_rules_ref as LR  # noqa: E402
from test_logit_rules_cpu import EX, Tok, _lib, _wrapper  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mellow_generate_constraint", "mellow_constraint_apply")
FIELDS = ["size", "n_nodes", "n_edges", "node_first", "node_flags", "edge_token", "edge_child", "n_rows", "row_root", "then_free"]


def test_header_declares_and_library_exports_the_symbols_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    lib = _lib()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name, nargs in zip(NAMES, (2, 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    m = re.search(r"typedef struct mellow_constraint \{(.*?)\} mellow_constraint_t;", hdr, re.S)
    assert m, "the struct is not declared"
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == FIELDS
    assert [f[0] for f in E.Constraint._fields_] == fields
    assert ctypes.sizeof(E.Constraint) == 72 and E.Constraint.node_first.offset == 16 and E.Constraint.row_root.offset == 56
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)   # detected by symbol lookup, not by the number
    assert "NOT the\n * numbers mellow_score returns" in hdr or "NOT the numbers mellow_score returns" in hdr      # the two consequences
    assert "min_new_tokens together with a set whose phrases are shorter" in hdr


# ---- the refusals of the C entry points, in host code ----------------------------------------------------------------------------------
def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _struct(first=(0, 2, 2, 2), flags=(0, 1, 1), tok=(5, 9), child=(1, 2), roots=(0,), then_free=0, **over):
    """a valid two-phrase trie ([5], [9]) unless told otherwise; the arrays are kept alive on the struct"""
    a = [_i32(first), _i32(flags), _i32(tok), _i32(child), _i32(roots)]
    c = E.Constraint(size=ctypes.sizeof(E.Constraint), n_nodes=len(flags), n_edges=len(tok), node_first=a[0].ctypes.data,
                     node_flags=a[1].ctypes.data, edge_token=a[2].ctypes.data, edge_child=a[3].ctypes.data, n_rows=len(roots),
                     row_root=a[4].ctypes.data, then_free=then_free)
    for k, v in over.items():
        setattr(c, k, v)
    c._keep = a
    return c


def _both(lib, c):
    """both entry points with a null engine -> the two messages"""
    out = []
    assert lib.mellow_generate_constraint(None, ctypes.byref(c)) != 0
    out.append(lib.mellow_last_error().decode())
    assert lib.mellow_constraint_apply(None, ctypes.byref(c), None, 1, None, 0, None, 0, None, None, None, None) != 0
    out.append(lib.mellow_last_error().decode())
    return out


def test_refusals_in_host_code_in_the_stated_order():
    """no GPU here: every one of these returns before a device is touched.  Each struct carries its own fault AND every fault the
    header lists after it, so the message shows which check came first."""
    lib = _lib()
    for msg in _both(lib, _struct()):
        assert "engine not finalized" in msg
    assert lib.mellow_generate_constraint(None, None) != 0 and "engine not finalized" in lib.mellow_last_error().decode()
    later = dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(9, 5, 49152), child=(0, 7, 2), roots=(3,))      # every later fault at once
    ladder = [
        (dict(later, size=8), "size"),
        (dict(later, n_nodes=-1), "counts"),
        (dict(later, n_edges=(1 << 20) + 1), "counts"),
        (dict(later, n_rows=0), "counts"),
        (dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(9, 5, 49152), child=(0, 7, 2), roots=(3,)), "sorted"),
        (dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(5, 9, 49152), child=(0, 7, 2), roots=(3,)), "child"),
        (dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(5, 9, 49152), child=(1, 7, 2), roots=(3,)), "child"),          # out of range
        (dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(5, 9, 49152), child=(1, 2, 2), roots=(3,)), "row_root"),       # root out of range
        (dict(first=(0, 2, 3, 3), flags=(1, 1, 1), tok=(5, 9, 49152), child=(1, 2, 2), roots=(0,)), "terminal"),
        (dict(first=(0, 2, 3, 3), flags=(0, 1, 1), tok=(5, 9, 49152), child=(1, 2, 2), roots=(0,)), "vocabulary"),
        (dict(first=(0, 2, 3, 3), flags=(0, 1, 1), tok=(-1, 9, 7), child=(1, 2, 2), roots=(0,)), "vocabulary"),
        (dict(first=(0, 2, 3, 3), flags=(0, 1, 1), tok=(5, 9, 7), child=(1, 2, 2), roots=(0,)), "engine not finalized"),
    ]
    for kw, word in ladder:
        for msg in _both(lib, _struct(**kw)):
            assert word in msg, (kw, word, msg)
    for kw, word in ((dict(then_free=2), "then_free"), (dict(first=(0, 2, 2, 1)), "node_first"), (dict(first=(0, 2, 1, 2)), "node_first"),
                     (dict(tok=(5, 5)), "sorted"), (dict(node_first=None), "null")):
        for msg in _both(lib, _struct(**kw)):
            assert word in msg, (kw, word, msg)


# ---- the trie builder ----------------------------------------------------------------------------------------------------------------------
SETS = [[[3, 4], [3], [3, 4, 5], [9]], [[7]], [[9], [3], [3, 4], [3, 4, 5], [3]], [[49151, 0], [0, 49151], [31], [32]]]


def test_build_trie_round_trip_sorted_edges_shared_roots_and_prefix_phrases():
    t = MC.build_trie(SETS)
    n = t["node_flags"].shape[0]
    assert all(t[k].dtype == np.int32 for k in t)
    assert t["node_first"].shape == (n + 1,) and t["node_first"][0] == 0 and t["node_first"][-1] == t["edge_token"].shape[0]
    for r, phrases in enumerate(SETS):
        assert CR.phrases_of(t, t["row_root"][r]) == sorted({tuple(p) for p in phrases}), r       # duplicates merged
        assert not CR.terminal(t, t["row_root"][r])
    for u in range(n):
        a, b = t["node_first"][u], t["node_first"][u + 1]
        assert (np.diff(t["edge_token"][a:b]) > 0).all()                                           # strictly ascending
        assert (t["edge_child"][a:b] > u).all() and (t["edge_child"][a:b] < n).all()
    assert t["row_root"][0] == t["row_root"][2] and len(set(t["row_root"].tolist())) == 3          # equal sets share one root
    u = CR.state_after(t, t["row_root"][0], [3])
    assert CR.terminal(t, u) and CR.edges(t, u)                                                    # [3] is a phrase and a prefix of [3, 4]
    # what the builder made passes the C entry's own checks
    lib = _lib()
    c = E._CallConstraint(SETS, False, 49152)
    c.expand(4, 2)
    assert c.roots.tolist() == np.repeat(t["row_root"], 2).tolist()
    assert lib.mellow_generate_constraint(None, ctypes.byref(c.struct())) != 0 and "engine not finalized" in lib.mellow_last_error().decode()
    assert c.struct(3, 4).n_rows == 4
    with pytest.raises(ValueError, match="one set per example"):
        c.expand(3, 1)


def test_check_constraint_refuses_in_host_code():
    for bad, word in (([], "phrase set per row"), ([[]], "empty phrase set"), ([[[1], []]], "empty phrase"), ([[[49152]]], "vocabulary"),
                      ([[[-1]]], "vocabulary"), ([[[1.5]]], "vocabulary"), ([["ab"]], "not a string")):
        with pytest.raises(ValueError, match=word):
            MC.check_constraint(bad)
        with pytest.raises(ValueError, match=word):
            MC.build_trie(bad)
    assert MC.check_constraint([[[2, 1], [1], [2, 1]]]) == [((1,), (2, 1))]


# ---- the reference by hand ---------------------------------------------------------------------------------------------------------------
def test_reference_edge_before_stop_absorbing_states_and_the_empty_set():
    t = MC.build_trie([[[3], [3, 7], [4, 5]]])          # 7 is also the stop id below: [3, 7] has an EDGE for it at the terminal node [3]
    root = int(t["row_root"][0])
    n3 = CR.step(t, root, 3, stop_id=7)
    assert n3 >= 0 and CR.terminal(t, n3)
    n37 = CR.step(t, n3, 7, stop_id=7)
    assert n37 >= 0 and n37 != n3                       # the edge wins: a node, not DONE
    assert CR.step(t, n37, 7, stop_id=7) == CR.DONE     # no edge there, terminal, the stop id
    assert CR.step(t, n3, 7, stop_id=-1) == n37 and CR.step(t, n37, 7, stop_id=-1) == CR.DEAD
    assert CR.step(t, root, 7, stop_id=7) == CR.DEAD    # the root is not terminal
    assert CR.step(t, root, 9, stop_id=7) == CR.DEAD
    n4 = CR.step(t, root, 4, stop_id=7)
    assert CR.step(t, n4, 7, stop_id=7) == CR.DEAD      # not terminal: the stop rule does not apply
    for s in (CR.DEAD, CR.FREE, CR.DONE):
        assert all(CR.step(t, s, tok, stop_id=7, then_free=tf) == s for tok in (3, 7, 9) for tf in (False, True))
    assert CR.step(t, root, 3, stop_id=7, then_free=True) == CR.FREE           # the child is terminal
    assert CR.step(t, root, 4, stop_id=7, then_free=True) == n4
    assert CR.state_after(t, root, [4, 5, 1, 2], 7, True) == CR.FREE and CR.state_after(t, root, [4, 5, 7, 7], 7) == CR.DONE
    assert CR.state_after(t, root, [4, 9, 5], 7) == CR.DEAD
    # allowed sets
    assert CR.allowed(t, root, 7) == [3, 4] and CR.allowed(t, n3, 7) == [7] and CR.allowed(t, n3, -1) == [7]
    assert CR.allowed(t, n4, 7) == [5] and CR.allowed(t, n37, 7) == [7] and CR.allowed(t, n37, -1) == []
    assert CR.allowed(t, CR.FREE, 7) is None and CR.allowed(t, CR.DEAD, 7) == [7] == CR.allowed(t, CR.DONE, 7)
    assert CR.allowed(t, CR.DEAD, -1) == [] == CR.allowed(t, CR.DONE, -1)
    # the empty allowed set constrains nothing; everything neither
    l = np.arange(24, dtype=np.float32).reshape(3, 8)
    out, states, con = CR.apply_rows(l, t, [root] * 3, [[9], [3], [3, 7]], stop_id=-1)
    assert states.tolist() == [CR.DEAD, n3, n37] and con.tolist() == [False, True, False]
    assert out[0].tobytes() == l[0].tobytes() and out[2].tobytes() == l[2].tobytes()
    assert np.isneginf(out[1, :7]).all() and out[1, 7] == l[1, 7]
    out, states, con = CR.apply_rows(l, t, [root] * 3, [[3], [], [4]], stop_id=2, then_free=True)
    assert states.tolist() == [CR.FREE, root, n4] and con.tolist() == [False, True, True] and out[0].tobytes() == l[0].tobytes()
    assert np.nonzero(np.isfinite(out[1]))[0].tolist() == [3, 4] and np.nonzero(np.isfinite(out[2]))[0].tolist() == [5]


def test_constrained_probabilities_multiply_to_one_over_the_phrase_set():
    """stop_id >= 0: along every phrase the constrained log-softmax of random logits, the stop step included, summed over the phrase
    set gives probability 1 in fp64 (the logits depend on the history, as a model's do)"""
    V, stop = 64, 7
    phrases = [[3], [3, 9], [3, 9, 9], [4, 5], [4, 6, 1], [12], [3, 8, 2]]      # prefixes of one another; no phrase holds the stop id
    t = MC.build_trie([phrases])
    root = int(t["row_root"][0])
    rng = np.random.default_rng(0)
    table = {}

    def logits(hist):
        if hist not in table:
            table[hist] = (rng.standard_normal(V) * 3).astype(np.float32)
        return table[hist]

    total = 0.0
    for p in CR.phrases_of(t, root):
        lp = 0.0
        for s, tok in enumerate(tuple(p) + (stop,)):
            hist = (tuple(p) + (stop,))[:s]
            out, _, con = CR.apply_rows(logits(hist)[None], t, [root], [hist], stop_id=stop)
            assert con[0]
            lp += LR.log_softmax64(out)[0, tok]
        total += np.exp(lp)
    assert abs(total - 1.0) <= 1e-12, total


# ---- wrapper -----------------------------------------------------------------------------------------------------------------------------
def test_wrapper_keyword_errors():
    w = _wrapper()
    for kw, word in ((dict(choices=[]), "empty set"), (dict(choices=[[], ["a"], ["b"]]), "empty set"), (dict(choices=["a", ""]), "empty string"),
                     (dict(choices=["a"], choices_then="loose"), "choices_then"), (dict(choices_then="loose"), "choices_then"),
                     (dict(choices=[["a"], ["b"]]), "one list per example"), (dict(choices="a b"), "list of strings"),
                     (dict(choices=["a", ["b"], ["c"]]), "mixes"),
                     (dict(choices=["a b c d e"]), "longest phrase"),                       # 5 tokens, max_len 5: no place for the stop token
                     (dict(choices=["a b c d e f"], choices_then="free"), "longest phrase"),
                     (dict(choices=["a", "bb", "c"], num_beams=3, num_return_sequences=3), "distinct phrases")):   # "a" and "c" are one phrase
        with pytest.raises(ValueError, match=word):
            w.generate(EX, 5, 0.8, 1.0, **kw)
    with pytest.raises(TypeError):
        w.generate(EX, 5, 0.8, 1.0, choices=[["a", 3], ["b"], ["c"]])
    assert w.model.calls == []
    w.generate(EX, 5, 0.8, 1.0, choices=["a b c d"])                                       # 4 tokens + the stop token fit
    w.generate(EX, 5, 0.8, 1.0, choices=["a b c d e"], choices_then="free")
    w.generate(EX, 5, 0.8, 1.0, choices=["a", "bb", "c"], num_beams=3, num_return_sequences=2)
    assert len(w.model.calls) == 3


def test_wrapper_neutral_call_arms_nothing():
    w = _wrapper()
    base = w.generate(EX, 5, 0.8, 1.0)
    same = w.generate(EX, 5, 0.8, 1.0, choices=None, choices_then="stop")
    assert same == base and w.model.calls[1] == w.model.calls[0]
    assert not any(k.startswith("constraint") for k in w.model.calls[0])


def test_wrapper_passes_the_keywords_on_every_route():
    w = _wrapper()
    flat = ["yes", "no way", "yes"]
    want = [[[103], [102, 103], [103]]] * 3                                 # Tok: a word is 100 + its length; _candidate_ids' convention
    w.generate(EX, 5, 0.8, 1.0, choices=flat)                                                              # plain
    w.generate(EX, 5, 0.8, 1.0, choices=flat, do_sample=True, seed=1)                                       # sampled
    w.generate(EX, 5, 0.8, 1.0, choices=flat, do_sample=True, seed=1, num_return_sequences=2, return_logprobs=True)   # nseq
    w.generate([["a.wav", "b.wav", ["q1", "q2"]]] * 3, 5, 0.8, 1.0, choices=flat)                           # questions
    w.generate(EX, 5, 0.8, 1.0, choices=flat, num_beams=3, num_return_sequences=2)                          # beams
    w.generate(EX, 5, 0.8, 1.0, choices=flat, guidance_scale=1.5, negative_examples="silence")              # guided
    assert len(w.model.calls) == 6
    for c in w.model.calls:
        assert c["constraint"] == want and c["constraint_then_free"] is False and c["examples"] == 3       # parallel to the EXAMPLES
    assert w.model.calls[2]["num_return_sequences"] == 2 and w.model.calls[4]["num_beams"] == 3 and w.model.calls[5]["guidance_scale"] == 1.5
    per = [["one"], ["two", "three four"], ["five"]]
    w.generate(EX, 5, 0.8, 1.0, choices=per, choices_then="free")
    assert w.model.calls[6]["constraint"] == [[[103]], [[103], [105, 104]], [[104]]] and w.model.calls[6]["constraint_then_free"] is True
    assert Tok().encode("three four") == [105, 104]


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
    batches = [(np.zeros((2, 4)),) * 3, (np.zeros((2, 4)),) * 3]
    con = [[[1], [2, 3]], [[4]]]
    assert pool.generate_many(batches, max_len=4, constraint=con, constraint_then_free=True) == [2, 2]
    assert all(k["constraint"] is con and k["constraint_then_free"] is True for k in seen)
    pool._pool.shutdown()


def test_data_parallel_shard_slices_the_sets_and_the_ranks_agree_on_them(monkeypatch):
    import torch.distributed as tdist
    from mellow_amd import dist as mdist
    per = [["one"], ["two", "three four"], ["five"]]
    ids = [[[103]], [[103], [105, 104]], [[104]]]
    sigs = {}
    for name, kw in (("none", dict()), ("per", dict(choices=per)), ("free", dict(choices=per, choices_then="free")),
                     ("other", dict(choices=[["one"], ["two"], ["five"]]))):
        for rank in (0, 1):
            w = _wrapper()
            monkeypatch.setattr(w, "_dp", lambda r=rank: (r, 2))
            agreed = []
            monkeypatch.setattr(w, "_check_same_examples", lambda examples, extra=b"", _a=agreed: _a.append(extra))
            monkeypatch.setattr(tdist, "get_backend", lambda *a: "gloo")
            monkeypatch.setattr(mdist, "gather_tokens", lambda toks, lens, n_total, max_len, device=None, per_rank=0:
                                (np.zeros((n_total, max_len), dtype=np.int32), np.zeros((n_total,), dtype=np.int32)))
            w.generate(EX, 5, 0.8, 1.0, **kw)
            lo, hi = mdist.shard_range(3, rank, 2)
            call = w.model.calls[0]
            assert call["examples"] == hi - lo
            if name in ("per", "free"):
                assert call["constraint"] == ids[lo:hi] and call["constraint_then_free"] is (name == "free")
            elif name == "other":
                assert len(call["constraint"]) == hi - lo
            else:
                assert "constraint" not in call
            assert len(agreed) == 1
            sigs.setdefault(name, agreed[0])
            assert sigs[name] == agreed[0]                                  # both ranks: the digest of ALL sets, not of the shard
    assert len(set(sigs.values())) == 4 and sigs["none"] == b""             # without the keyword: today's signature
