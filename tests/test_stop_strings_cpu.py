"""CPU: stop strings (mellow_set_vocab_bytes, mellow_generate_stop_strings, mellow_stop_strings_apply,
Engine.generate(stop_strings=...), MellowWrapper.generate(stop_strings=...)) as far as it goes without a GPU: the exported symbols
and the struct, the host-side refusals in their stated order, the incremental 63-byte-tail form against the brute force of
tests/stop_strings_ref.py, the vocabulary byte table on both routes, the text cut, the wrapper's keyword rules on a stub engine and
the data-parallel digest."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from mellow_amd import engine as E
from mellow_amd import stop_strings as MS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stop_strings_ref as SR  # noqa: E402
from test_logit_rules_cpu import EX, StubEngine, Tok, _lib, _wrapper  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mellow_set_vocab_bytes", "mellow_generate_stop_strings", "mellow_stop_strings_apply")
V = 49152


def test_header_declares_and_library_exports_the_symbols_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    lib = _lib()
    raw = ctypes.CDLL(E.LIB_PATH)
    for name, nargs in zip(NAMES, (4, 2, 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    m = re.search(r"typedef struct mellow_stop_strings \{(.*?)\} mellow_stop_strings_t;", hdr, re.S)
    assert m, "the struct is not declared"
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == ["size", "n_strings", "str_off", "str_bytes"] == [f[0] for f in E.StopStrings._fields_]
    assert ctypes.sizeof(E.StopStrings) == 24 and E.StopStrings.str_off.offset == 8
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)   # detected by symbol lookup, not by the number


# ---- the refusals of the C entry points, in host code ----------------------------------------------------------------------------------
def _struct(strings=(b"ab",), **over):
    c = E._CallStopStrings(list(strings)) if 1 <= len(strings) <= 16 and all(1 <= len(s) <= 64 for s in strings) else None
    if c is None:                      # what check_stop_strings refuses, built by hand
        c = E._CallStopStrings.__new__(E._CallStopStrings)
        c.off = np.zeros(len(strings) + 1, dtype=np.int32)
        c.off[1:] = np.cumsum([len(s) for s in strings])
        c.data = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8).copy()
        c.struct = E.StopStrings(size=ctypes.sizeof(E.StopStrings), n_strings=len(strings), str_off=c.off.ctypes.data, str_bytes=c.data.ctypes.data)
    for k, v in over.items():
        setattr(c.struct, k, v)
    return c


def _both(lib, c):
    out = []
    assert lib.mellow_generate_stop_strings(None, ctypes.byref(c.struct)) != 0
    out.append(lib.mellow_last_error().decode())
    assert lib.mellow_stop_strings_apply(None, ctypes.byref(c.struct), None, 1, None, 0, None, 0, None, None, None, None) != 0
    out.append(lib.mellow_last_error().decode())
    return out


def test_stop_strings_refusals_in_host_code_in_the_stated_order():
    """no GPU here: every one of these returns before a device is touched.  Each struct carries its own fault AND the faults the header
    lists after it, so the message shows which check came first."""
    lib = _lib()
    for msg in _both(lib, _struct()):
        assert "engine not finalized" in msg
    assert lib.mellow_generate_stop_strings(None, None) != 0 and "engine not finalized" in lib.mellow_last_error().decode()
    long65 = b"x" * 65
    ladder = [
        (_struct((b"a",) * 17 + (long65,), size=8), "size"),
        (_struct((b"a",) * 16 + (long65,)), "1 to 16 strings"),
        (_struct((), n_strings=0), "1 to 16 strings"),
        (_struct((b"a",), n_strings=-3), "1 to 16 strings"),
        (_struct((b"a", long65)), "string 1 has 65 bytes"),
        (_struct((b"a", b"", b"b")), "string 1 has 0 bytes"),
        (_struct((b"a", b"x" * 64)), "engine not finalized"),
        (_struct((b"a",) * 16), "engine not finalized"),
    ]
    for c, word in ladder:
        for msg in _both(lib, c):
            assert word in msg, (word, msg)
    for msg in _both(lib, _struct(str_off=None)):
        assert "null" in msg


def test_vocab_bytes_refusals_in_host_code_in_the_stated_order():
    lib = _lib()
    off = np.arange(V + 1, dtype=np.int32)
    data = np.zeros(V + 300, dtype=np.uint8)

    def call(o, d, n):
        rc = lib.mellow_set_vocab_bytes(None, None if o is None else o.ctypes.data, None if d is None else d.ctypes.data, n)
        assert rc != 0
        return lib.mellow_last_error().decode()

    bad = off.copy()
    bad[0] = 1            # does not start at 0 ...
    bad[100] = 50         # ... decreases ...
    bad[201:] += 300      # ... and token 200 has 301 bytes
    assert "null" in call(None, data, V - 1) and "null" in call(bad, None, V - 1)
    assert "n_tokens = 49151" in call(bad, data, V - 1)
    assert "start at 0" in call(bad, data, V)
    bad[0] = 0
    assert "decreases at token 99" in call(bad, data, V)
    bad[100] = 100
    assert "token 200 has 301 bytes" in call(bad, data, V)
    bad[201:] -= 300
    assert np.array_equal(bad, off) and "engine not finalized" in call(off, data, V)
    ok256 = off.copy()
    ok256[5:] += 255      # a token of exactly 256 bytes is fine
    assert "engine not finalized" in call(ok256, data, V)
    # the Python check says the same before the C call
    with pytest.raises(ValueError, match="token 200 has 301 bytes"):
        o = off.copy()
        o[201:] += 300
        E.check_vocab_bytes(o, np.zeros(int(o[-1]), dtype=np.uint8), V)
    with pytest.raises(ValueError, match="vocab \\+ 1"):
        E.check_vocab_bytes(off[:-1], data, V)
    with pytest.raises(ValueError, match="start at 0"):
        E.check_vocab_bytes(off + 1, data, V)


def test_check_stop_strings_refuses_in_host_code():
    for bad, word in (([], "1 to 16"), ([b"a"] * 17, "1 to 16"), ([b"a", b""], "stop string 1 has 0 bytes"), ([b"x" * 65], "has 65 bytes"),
                      (b"ab", "list of byte strings"), ("ab", "list of byte strings"), (["ab"], "bytes object"), ([3], "bytes object")):
        with pytest.raises(ValueError, match=word):
            E.check_stop_strings(bad)
    assert E.check_stop_strings([b"a", bytearray(b"x" * 64)]) == [b"a", b"x" * 64]
    c = E._CallStopStrings([b"ab", b"c"])
    assert c.off.tolist() == [0, 2, 3] and bytes(c.data) == b"abc" and c.struct.n_strings == 2


# ---- the definition: incremental == brute force ----------------------------------------------------------------------------------------
def _table(parts):
    off = np.zeros(len(parts) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off, np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def test_incremental_form_equals_the_brute_force_on_random_texts():
    rng = np.random.default_rng(0)
    hits = 0
    for trial in range(300):
        alpha = b"ab" if trial % 2 else b"abc"
        parts = [bytes(alpha[i] for i in rng.integers(0, len(alpha), size=rng.integers(0, 7))) for _ in range(40)]      # empty tokens too
        parts[0] = bytes(alpha[i] for i in rng.integers(0, len(alpha), size=256))                                         # and a 256-byte one
        table = _table(parts)
        strings = [bytes(alpha[i] for i in rng.integers(0, len(alpha), size=rng.integers(1, 13))) for _ in range(rng.integers(1, 5))]
        hist = rng.integers(-1, 41, size=rng.integers(0, 30)).tolist()       # -1 and 40: ids outside the table, no bytes
        for s in range(len(hist) + 1):
            a, b = SR.hit_brute(table, hist[:s], strings), SR.hit_incremental(table, hist[:s], strings)
            assert a == b, (trial, s)
            hits += a
    assert hits > 100
    # strings of exactly 64 bytes over 1-byte tokens: the tail of 63 bytes is exactly what such a match needs
    table = _table([bytes([97 + i]) for i in range(4)])
    for trial in range(50):
        hist = rng.integers(0, 4, size=200).tolist()
        x = SR.text_of(table, hist)
        at = int(rng.integers(0, 200 - 64))
        s64 = x[at:at + 64]
        first = x.find(s64) + 64
        for s in (first - 1, first, first + 1, 200):
            assert SR.hit_incremental(table, hist[:s], [s64]) == SR.hit_brute(table, hist[:s], [s64]) == (s >= first)
        near = s64[:63] + bytes([s64[63] ^ 1])                               # 63 of 64 bytes agree
        assert SR.hit_incremental(table, hist, [near]) == SR.hit_brute(table, hist, [near])
    assert SR.first_hit_step(table, [0, 1, 2, 3], [b"bc"]) == 3 and SR.first_hit_step(table, [0, 1], [b"bc"]) is None


def test_reference_rows_and_partials():
    l = np.arange(128, dtype=np.float32).reshape(2, 64)
    table = _table([b"a", b"b"])
    out, hit = SR.apply_rows(l, table, [[0, 1], [1, 0]], [b"ab"], stop_id=33)
    assert hit.tolist() == [True, False] and out[1].tobytes() == l[1].tobytes()
    assert out[0, 33] == 0.0 and np.isneginf(np.delete(out[0], 33)).all()
    val, idx, s = SR.hit_partials(64, 33)
    assert val.tolist() == [-np.inf, 0.0] and idx.tolist() == [0, 33] and s.tolist() == [0.0, 1.0]


# ---- the vocabulary's bytes ----------------------------------------------------------------------------------------------------------------
class BpeTok:
    """a byte-level BPE vocabulary as Hugging Face shows it: token strings in the GPT-2 alphabet, and specials outside it"""
    toks = ["Ġthe", "Ċ", ".Ċ", "Ã", "©", "<|endoftext|>", "a.b", "Ġ", "日本"]

    def __len__(self):
        return len(self.toks)

    def convert_ids_to_tokens(self, i):
        return self.toks[i]


class DecodeTok:
    def __len__(self):
        return 5

    def decode(self, ids):
        return "".join(["a", "é", "", " b", "<s>"][int(i)] for i in ids)


def test_vocab_bytes_on_both_routes():
    assert len(MS.BYTE_TO_UNICODE) == 256 == len(set(MS.BYTE_TO_UNICODE.values()))
    assert all(MS.BYTE_TO_UNICODE[b] == chr(b) for b in b"!~09AZaz") and MS.UNICODE_TO_BYTE["Ā"] == 0
    off, data = MS.vocab_bytes(BpeTok(), 12)
    table = (off, data)
    assert off.dtype == np.int32 and data.dtype == np.uint8 and off.shape == (13,) and off[0] == 0 and off[-1] == data.shape[0]
    assert SR.tok_bytes(table, 0) == b" the" and SR.tok_bytes(table, 1) == b"\n" and SR.tok_bytes(table, 2) == b".\n"
    assert SR.tok_bytes(table, 3) + SR.tok_bytes(table, 4) == "é".encode() and len(SR.tok_bytes(table, 3)) == 1      # one character over two tokens
    assert SR.tok_bytes(table, 5) == b"<|endoftext|>"                       # a special token: its characters are all in the alphabet
    assert SR.tok_bytes(table, 8) == "日本".encode()                         # outside the alphabet: the string's UTF-8
    assert all(SR.tok_bytes(table, i) == b"" for i in (9, 10, 11))          # ids past the tokenizer's size
    off, data = MS.vocab_bytes(DecodeTok(), 7)
    table = (off, data)
    assert [SR.tok_bytes(table, i) for i in range(7)] == [b"a", "é".encode(), b"", b" b", b"<s>", b"", b""]
    E.check_vocab_bytes(off, data, 7)

    class Long(DecodeTok):
        def decode(self, ids):
            return "x" * 257 if int(ids[0]) == 3 else "y"

    with pytest.raises(ValueError, match="token 3 has 257 bytes"):
        MS.vocab_bytes(Long(), 7)


# ---- the text cut ------------------------------------------------------------------------------------------------------------------------
def test_cut_text():
    assert MS.cut_text("xxabcyy", ["ab", "abc"]) == ("xx", "ab")                    # overlapping: "ab" ends first
    assert MS.cut_text("xxabcyy", ["abc", "ab"]) == ("xx", "ab")
    assert MS.cut_text("xxabcyy", ["bc", "abc"]) == ("xx", "abc")                   # equal end: the one that starts first
    assert MS.cut_text("xxabcyy", ["abc", "bc"]) == ("xx", "abc")
    assert MS.cut_text("xxabcyy", ["bc", "abc"], include=True) == ("xxabc", "abc")
    assert MS.cut_text("a dog barking and a dog", ["ark"]) == ("a dog b", "ark")    # inside a token
    assert MS.cut_text("a dog. a cat.", ["."], include=True) == ("a dog.", ".")
    assert MS.cut_text("a dog", [".", "\n"]) == ("a dog", None)
    assert MS.cut_text("", ["a"]) == ("", None)
    assert MS.cut_text("yy cat xx dog", ["dog", "cat"]) == ("yy ", "cat")           # the first occurrence, whatever the list's order


# ---- wrapper -----------------------------------------------------------------------------------------------------------------------------
class SizedTok(Tok):
    def __len__(self):
        return 1200


class StopStub(StubEngine):
    class lm:
        vocab_size = 2048

    def __init__(self):
        super().__init__()
        self.tables = []

    def set_vocab_bytes(self, offsets, data):
        self.tables.append((offsets, data))


def _stop_wrapper():
    w = _wrapper()
    w.tokenizer, w.model = SizedTok(), StopStub()
    return w


def test_wrapper_keyword_errors():
    w = _stop_wrapper()
    for kw, word in ((dict(stop_strings=[]), "empty list"), (dict(stop_strings=""), "empty string"), (dict(stop_strings=["a", ""]), "empty string"),
                     (dict(stop_strings=["a"] * 17), "1 to 16"), (dict(stop_strings=["x" * 65]), "65 bytes"),
                     (dict(stop_strings=["é" * 33]), "66 bytes")):                      # bytes count, not characters
        with pytest.raises(ValueError, match=word):
            w.generate(EX, 5, 0.8, 1.0, **kw)
    with pytest.raises(TypeError):
        w.generate(EX, 5, 0.8, 1.0, stop_strings=[b"a"])
    assert w.model.calls == [] and w.model.tables == []

    class LongTok(SizedTok):
        def decode(self, ids):
            return "z" * 300 if len(ids) == 1 and int(ids[0]) == 9 else super().decode(ids)

    w.tokenizer = LongTok()
    with pytest.raises(ValueError, match="token 9 has 300 bytes"):
        w.generate(EX, 5, 0.8, 1.0, stop_strings=["a"])
    assert w.model.calls == []


def test_wrapper_neutral_call_arms_nothing():
    w = _stop_wrapper()
    base = w.generate(EX, 5, 0.8, 1.0)
    same = w.generate(EX, 5, 0.8, 1.0, stop_strings=None, include_stop_str_in_output=True)
    assert same == base and w.model.calls[1] == w.model.calls[0]
    assert "stop_strings" not in w.model.calls[0] and w.model.tables == []
    dicts = w.generate(EX, 5, 0.8, 1.0, return_logprobs=True)
    assert all("stop_reason" not in d for d in dicts)


def test_wrapper_passes_the_keyword_on_every_route_builds_the_table_once_and_cuts():
    w = _stop_wrapper()
    one = w.generate(EX, 5, 0.8, 1.0, stop_strings="é.")                                                          # plain, a single string
    w.generate(EX, 5, 0.8, 1.0, stop_strings=["a", "bc"], do_sample=True, seed=1)                                # sampled
    w.generate(EX, 5, 0.8, 1.0, stop_strings=["a", "bc"], do_sample=True, seed=1, num_return_sequences=2, return_logprobs=True)
    w.generate([["a.wav", "b.wav", ["q1", "q2"]]] * 3, 5, 0.8, 1.0, stop_strings=["a", "bc"])                    # questions
    w.generate(EX, 5, 0.8, 1.0, stop_strings=["a", "bc"], num_beams=3, num_return_sequences=2)                   # beams
    w.generate(EX, 5, 0.8, 1.0, stop_strings=["a", "bc"], guidance_scale=1.5, negative_examples="silence")       # guided
    w.generate(EX, 5, 0.8, 1.0, stop_strings=["a", "bc"], choices=["x y"], min_new_tokens=2, top_k=4, do_sample=True, seed=2)
    assert len(w.model.calls) == 7
    assert w.model.calls[0]["stop_strings"] == ["é.".encode()] and all(c["stop_strings"] == [b"a", b"bc"] for c in w.model.calls[1:])
    assert w.model.calls[6]["constraint"] and w.model.calls[6]["min_new_tokens"] == 2 and w.model.calls[6]["top_k"] == 4
    assert len(w.model.tables) == 1                                                      # built lazily, handed over once
    off, data = w.model.tables[0]
    assert off.shape == (2049,) and SR.tok_bytes((off, data), 1001) == b"t1001" and SR.tok_bytes((off, data), 1200) == b""
    assert one == w.generate(EX, 5, 0.8, 1.0)                                            # "é." is in no text: uncut
    # the stub's texts are "t1000 t1001 ...": cut at the start of the match, or at its end
    assert w.generate(EX, 5, 0.8, 1.0, stop_strings=["1 t", "02"]) == ["t1000 t100", "t1010 t101", "t1"]
    assert w.generate(EX, 5, 0.8, 1.0, stop_strings=["1 t", "02"], include_stop_str_in_output=True) == ["t1000 t1001 t", "t1010 t1011 t", "t102"]
    dicts = w.generate(EX, 5, 0.8, 1.0, stop_strings=["1 t", "t1002", "zz"], return_logprobs=True)
    assert [d["text"] for d in dicts] == ["t1000 t100", "t1010 t101", "t1020 t102"] and [d["stop_reason"] for d in dicts] == ["1 t"] * 3
    assert all(d["stop_reason"] is None for d in w.generate(EX, 5, 0.8, 1.0, stop_strings=["zz"], return_logprobs=True))
    nested = w.generate(EX, 5, 0.8, 1.0, stop_strings=["0 t"], do_sample=True, seed=1, num_return_sequences=2, return_logprobs=True)
    assert len(nested) == 3 and all(len(x) == 2 and all(d["stop_reason"] == "0 t" for d in x) for x in nested)


def test_data_parallel_digest_changes_with_the_strings(monkeypatch):
    import torch.distributed as tdist
    from mellow_amd import dist as mdist
    sigs = {}
    for name, kw in (("none", dict()), ("a", dict(stop_strings=["a"])), ("ab", dict(stop_strings=["a", "b"])), ("b", dict(stop_strings="b"))):
        for rank in (0, 1):
            w = _stop_wrapper()
            monkeypatch.setattr(w, "_dp", lambda r=rank: (r, 2))
            agreed = []
            monkeypatch.setattr(w, "_check_same_examples", lambda examples, extra=b"", _a=agreed: _a.append(extra))
            monkeypatch.setattr(tdist, "get_backend", lambda *a: "gloo")
            monkeypatch.setattr(mdist, "gather_tokens", lambda toks, lens, n_total, max_len, device=None, per_rank=0:
                                (np.zeros((n_total, max_len), dtype=np.int32), np.zeros((n_total,), dtype=np.int32)))
            w.generate(EX, 5, 0.8, 1.0, **kw)
            assert ("stop_strings" in w.model.calls[0]) == (name != "none")
            assert len(agreed) == 1
            sigs.setdefault(name, agreed[0])
            assert sigs[name] == agreed[0]                                  # both ranks agree
    assert len(set(sigs.values())) == 4 and sigs["none"] == b""             # without the keyword: today's signature
    assert MS.stop_strings_digest([b"a", b"b"]) != MS.stop_strings_digest([b"ab"])
