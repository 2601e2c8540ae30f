"""GPU (-m gpu): stop strings inside the decode step (include/mellow_hip.h mellow_set_vocab_bytes / mellow_generate_stop_strings /
mellow_stop_strings_apply; Engine.generate(stop_strings=); mellow_amd/csrc/stop_strings.hip).

Yardstick: the transcription of the definition in tests/stop_strings_ref.py.  Everything the launch writes is exact -- a flag, 0.0,
-inf, an index, a sum of one 1.0 and zeros -- so every comparison is bit-equal; the loop tests compare with the same call un-armed,
whose tokens a stop string must not change before the hit.  Every test prints what it measured."""
import os
import sys

import numpy as np
import pytest

from mellow_amd import engine as E
from mellow_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_rules_ref as LR  # noqa: E402
import stop_strings_ref as SR  # noqa: E402
from test_gpu_logit_rules import _tap_rows  # noqa: E402

pytestmark = pytest.mark.gpu

V = 49152
ML = 16
_DATA = {}

# ---- the byte table: token i is a deterministic string of 1 to 5 lower-case letters, so matches cross token boundaries often; a few
# ids carry the shapes the tap cases need (upper case and bytes >= 128: no letter string holds them)
T_EMPTY, T_BIG, T_BIGMISS = 10, 11, 12
SPECIAL = {T_EMPTY: b"", T_BIG: b"q" * 100 + b"NEEDLE" + b"q" * 150, T_BIGMISS: b"q" * 100 + b"NEEDLF" + b"q" * 150,
           20: b"xA", 21: b"B", 22: b"Cy", 24: b"abc", 25: b"ab", 26: b"c", 27: b"C"}
SPECIAL.update({200 + k: bytes([128 + k]) for k in range(64)})
S64 = bytes(range(128, 192))
assert len(SPECIAL[T_BIG]) == 256


def _table():
    if "table" not in _DATA:
        parts = []
        for i in range(V):
            h = (i * 2654435761 + 12345) & 0xffffffff
            parts.append(SPECIAL[i] if i in SPECIAL else bytes(97 + ((h >> (4 + 5 * j)) % 26) for j in range(1 + h % 5)))
        off = np.zeros(V + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(p) for p in parts])
        _DATA["table"] = (off, np.frombuffer(b"".join(parts), dtype=np.uint8).copy())
    return _DATA["table"]


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    e = E.Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    e.set_vocab_bytes(*_table())
    yield e
    e.close()


# ---- 1. the tap against the definition ------------------------------------------------------------------------------------------
TAP_STRINGS = [b"NEEDLE", b"ABC", S64, b"ab", b"abc", b"Cyx"]
ONE_BYTE = list(range(200, 264))
# (history, hit) -- the flag is stated here and asserted from the reference, so the cases are what their names say
CASES = [([], False),                                      # empty
         ([24], True),                                     # inside one token; "ab" and "abc" together
         ([22, 20], True),                                 # across two tokens: Cy|xA
         ([20, 21, 22], True),                             # across three: xA|B|Cy
         ([20, 21, 27], True),                             # completed exactly at a token's last byte: xA|B|C
         (ONE_BYTE, True),                                 # a 64-byte string over 64 one-byte tokens
         (ONE_BYTE[:63] + [200], False),                   # ... and its 63-of-64 near miss
         ([26, T_BIG], True),                              # in the middle of a 256-byte token
         ([T_BIGMISS, 26], False),
         ([20, T_EMPTY, T_EMPTY, 21, T_EMPTY, 22], True),  # empty-bytes tokens in between
         ([25, T_EMPTY, 26], True),                        # "ab", then "abc"
         ([24, T_BIGMISS, T_BIGMISS, 26], True),           # an early hit, 500 bytes ago: sticky
         ([21, 22, T_BIGMISS, -1, V], False)]              # ids outside the vocabulary have no bytes
STOP_TAP = 33 * 32 + 5


@pytest.mark.parametrize("B", [1, 33])
def test_tap_against_the_definition(engine, B):
    rows = _tap_rows(engine, B)
    cases = [CASES[(b + (3 if B == 1 else 0)) % len(CASES)] for b in range(B)]
    hists = [c[0] for c in cases]
    hist = np.zeros((B, 64), dtype=np.int32)
    hl = np.array([len(h) for h in hists], dtype=np.int32)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = h
    out = engine.stop_strings_apply(rows, hist, hl, TAP_STRINGS, stop_id=STOP_TAP)
    again = engine.stop_strings_apply(rows, hist, hl, TAP_STRINGS, stop_id=STOP_TAP)
    base = engine.logit_rules_apply(rows, np.zeros((B, 1), dtype=np.int32), np.zeros(B, dtype=np.int32), stop_id=-1)    # what the head leaves
    table = _table()
    want, hit = SR.apply_rows(rows, table, hists, TAP_STRINGS, STOP_TAP)
    assert hit.tolist() == [c[1] for c in cases]
    assert all(SR.hit_incremental(table, h, TAP_STRINGS) == c for h, c in cases)
    hv, hx, hs = SR.hit_partials(V, STOP_TAP)
    lse = LR.merged_lse(out["cand_val"], out["cand_sum"])
    print(f"[{engine.precision}] tap B = {B}: hit {out['hit'].tolist()}; merged lse of the hit rows {sorted(set(lse[hit].tolist()))}")
    assert np.array_equal(out["hit"], hit.astype(np.int32))
    assert out["logits"].tobytes() == want.tobytes()
    for b in range(B):
        if hit[b]:
            assert out["cand_val"][b].tobytes() == hv.tobytes() and np.array_equal(out["cand_idx"][b], hx), b
            assert out["cand_sum"][b].tobytes() == hs.tobytes(), b
            assert lse[b] == 0.0
            assert out["cand_idx"][b, STOP_TAP // 32] == STOP_TAP and out["cand_sum"][b, STOP_TAP // 32] == 1.0
        else:                  # not hit: byte-identical to the input, partials included
            assert out["logits"][b].tobytes() == rows[b].tobytes()
            for k in ("cand_val", "cand_idx", "cand_sum"):
                assert out[k][b].tobytes() == base[k][b].tobytes(), (k, b)
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)
    if B == 33:
        assert hit.any() and (~hit).any()


def test_tap_refuses_a_stop_id_outside_the_vocabulary(engine):
    rows = _tap_rows(engine, 1)
    for bad in (-1, V):
        with pytest.raises(E.EngineError, match="stop_id"):
            engine.stop_strings_apply(rows, np.zeros((1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32), [b"a"], stop_id=bad)


# ---- 2. the loop ----------------------------------------------------------------------------------------------------------------------
def _free_stop(toks):
    """a stop id the un-armed answers never hold: every stop of the armed call is then a forced one"""
    used = set(np.asarray(toks).reshape(-1).tolist())
    return next(t for t in range(2, V) if t not in used and t not in SPECIAL)


def _tb(t):
    return SR.tok_bytes(_table(), t)


def _expect(toks, strings):
    """per row the step at which its text first holds a string (None: never), from the reference alone"""
    return [SR.first_hit_step(_table(), row.tolist(), strings) for row in np.asarray(toks)]


def _choose(toks, early=(), cand=None):
    """stop strings FROM the un-armed answers: bytes across tokens 2|3 of one row, bytes inside a token of another, bytes across three
    tokens of a third, the three rows taken from `cand` (and bytes across tokens 0|1 of the rows `early`: enough early stops to pack
    the rest into fewer row blocks).  The first choice, in a fixed order, for which the reference shows three rows hit at three different steps and a row that is not."""
    toks = np.asarray(toks)
    R = toks.shape[0]
    extra = [_tb(toks[r, 0])[-2:] + _tb(toks[r, 1])[:2] for r in early]
    cand = list(range(min(R, 6))) if cand is None else list(cand)
    for a in cand:
        sa = _tb(toks[a, 2])[-2:] + _tb(toks[a, 3])[:2]
        for b in cand:
            for pb in range(4, 9):
                sb = _tb(toks[b, pb])
                if b == a or len(sb) < 3:
                    continue
                for c in cand:
                    for pc in range(6, 11):
                        sc = _tb(toks[c, pc])[-1:] + _tb(toks[c, pc + 1]) + _tb(toks[c, pc + 2])[:1]
                        if c in (a, b) or len(sc) < 3 or not all(len(_tb(toks[c, pc + i])) for i in range(3)):
                            continue
                        strings = [sa, sb, sc] + extra
                        steps = _expect(toks, strings)
                        hit = {s for s in (steps[a], steps[b], steps[c])}
                        if None not in hit and len(hit) == 3 and any(s is None for s in steps):
                            return strings, steps
    raise AssertionError("no choice of strings from these answers meets the preconditions")


def _loop_case(engine, rows, kw, early=(), cand=None):
    b = synth.make_batch(rows)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1, **kw)
    stop = _free_stop(free)
    plain, _, psteps, _ = engine.generate(*b, max_len=ML, stop_id=stop, **kw)
    assert plain.tobytes() == free.tobytes() and psteps == ML
    strings, steps = _choose(plain, early, cand)
    hit = [s for s in steps if s is not None]
    assert len(set(hit)) >= 3 and len(hit) < rows, steps            # from the reference alone
    armed, lens, asteps, _ = engine.generate(*b, max_len=ML, stop_id=stop, stop_strings=strings, **kw)
    print(f"[{engine.precision}] loop rows = {rows} {kw}: stop id {stop}, strings {strings}, first hit per row {steps}, steps {asteps}, "
          f"repacks {engine.last_row_repacks()}")
    for r in range(rows):
        s = steps[r]
        if s is None:                                               # a row without a hit equals the un-armed call
            assert armed[r].tobytes() == plain[r].tobytes(), (r, armed[r], plain[r])
            continue
        want = plain[r, :s].tolist() + [stop] if s < ML else plain[r].tolist()
        assert armed[r, :len(want)].tolist() == want, (r, s, armed[r], plain[r])
        assert lens[r] == min(s, ML)
        assert all(t in (stop, -1) for t in armed[r, len(want):].tolist()), (r, armed[r])
    return steps


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_loop_five_rows(engine, mode):
    _loop_case(engine, 5, dict(do_sample=True, seed=11, top_p=0.9, temperature=0.8) if mode == "sampled" else {})


def test_loop_two_row_blocks_with_migration(engine):
    """40 rows = two row blocks; ten rows of the first block stop after their second token, so the eight rows of the second block are
    moved into the first, and the three later hits are found by rows that have moved: the state follows the example"""
    steps = _loop_case(engine, 40, {}, early=range(6, 16), cand=range(32, 38))
    assert engine.last_row_repacks() >= 1
    assert sum(s is not None and s <= 3 for s in steps[:32]) >= 8 and sum(s is not None and s > 3 for s in steps[32:]) >= 3


# ---- 3. log-probs and the top record ------------------------------------------------------------------------------------------------
def test_logprobs_and_top_record(engine):
    b = synth.make_batch(5)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1)
    stop = _free_stop(free)
    plain = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True, top_logprobs=3)
    strings, steps = _choose(plain[0])
    toks, lens, asteps, _, lp, tid, tlp = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True, top_logprobs=3, stop_strings=strings)
    n = 0
    for r, s in enumerate(steps):
        k = ML if s is None else s
        assert toks[r, :k].tobytes() == plain[0][r, :k].tobytes()
        assert lp[r, :k].tobytes() == plain[4][r, :k].tobytes()                    # the log-probs before the forced stop: byte-equal
        assert tid[r, :k].tobytes() == plain[5][r, :k].tobytes() and tlp[r, :k].tobytes() == plain[6][r, :k].tobytes()
        if s is not None and s < ML:
            assert toks[r, s] == stop and lp[r, s] == 0.0      # exactly zero (the greedy form records -log 1.0, the zero with the sign bit)
            assert tid[r, s, 0] == stop and tlp[r, s, 0] == 0.0
            n += 1
    print(f"[{engine.precision}] log-probs: first hit per row {steps}; {n} forced stops with log-prob 0.0 and (stop id, 0.0) first in the record")
    assert n >= 3


# ---- 4. beams -----------------------------------------------------------------------------------------------------------------------------
def test_beams(engine):
    b = synth.make_batch(2)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1, num_beams=3, num_return_sequences=3, ignore_stop=True)
    stop = _free_stop(free)
    # strings from the free hypotheses: bytes across tokens 2|3 of the best hypothesis of every example
    strings = [(_tb(free[r, 2])[-2:] + _tb(free[r, 3])[:2]) for r in (0, 3)]
    toks, lens, steps, _, lps, scores = engine.generate(*b, max_len=ML, stop_id=stop, num_beams=3, num_return_sequences=3, return_logprobs=True,
                                                        stop_strings=strings)
    forced = 0
    for r in range(toks.shape[0]):
        row = toks[r].tolist()
        n = row.index(stop) if stop in row else len(row)
        first = SR.first_hit_step(_table(), row[:n], strings)
        print(f"[{engine.precision}] beams: hypothesis {r}: tokens {row[:n + 1]}, first hit after {first} tokens, log-probs {lps[r][:n + 1].tolist()}")
        if n < len(row):             # the free hypotheses never hold the stop id: this stop is a forced one
            assert first == n, (r, row, first)                       # completed by the last token before the stop, not earlier
            assert lps[r][n] == 0.0
            forced += 1
        else:
            assert first is None or first == n, (r, row, first)      # no hypothesis continues past a hit
    assert forced >= 2
    with pytest.raises(E.EngineError, match="stop_id"):              # a beam call under ignore_stop knows no stop token
        engine.generate(*b, max_len=4, stop_id=stop, num_beams=3, ignore_stop=True, stop_strings=strings)


# ---- 5. combinations ------------------------------------------------------------------------------------------------------------------------
def test_wins_over_min_new_tokens(engine):
    b = synth.make_batch(3)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1, min_new_tokens=12)
    stop = _free_stop(free)
    strings = [_tb(free[0, 2])[-2:] + _tb(free[0, 3])[:2]]
    steps = _expect(free, strings)
    assert steps[0] is not None and steps[0] <= 4
    toks, lens, *_ = engine.generate(*b, max_len=ML, stop_id=stop, min_new_tokens=12, stop_strings=strings)
    print(f"[{engine.precision}] min_new_tokens = 12: first hit per row {steps}, lengths {lens.tolist()}")
    for r, s in enumerate(steps):
        if s is not None and s < ML:
            assert toks[r, :s].tolist() == free[r, :s].tolist() and toks[r, s] == stop, (r, toks[r])


def test_with_guidance_both_rows_of_a_pair_stop_together(engine):
    b = synth.make_batch(3)
    neg = (np.zeros_like(b[0]), np.zeros_like(b[1]), b[2])                      # "silence"
    kw = dict(guidance_scale=1.5, negative=neg, keep_negative_rows=True)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1, **kw)
    assert free.shape[0] == 6 and np.array_equal(free[0::2], free[1::2])
    stop = _free_stop(free)
    strings = [_tb(free[0, 2])[-2:] + _tb(free[0, 3])[:2]]
    steps = _expect(free, strings)
    toks, lens, *_ = engine.generate(*b, max_len=ML, stop_id=stop, stop_strings=strings, **kw)
    print(f"[{engine.precision}] guided: first hit per row {steps}, lengths {lens.tolist()}")
    assert steps[0] is not None and steps[0] == steps[1] and lens[0] == lens[1] == steps[0]
    assert np.array_equal(toks[0::2], toks[1::2])
    assert toks[0, steps[0]] == stop and toks[0, :steps[0]].tolist() == free[0, :steps[0]].tolist()


def test_with_a_constraint_then_free(engine):
    """the string is completed inside the forced phrase: the row stops there, with the rest of the phrase unsaid, and is not banned
    whole (the stop id is finite)"""
    b = synth.make_batch(2)
    phrase = [5000, 5001, 5002, 5003]
    stop = 2
    strings = [(_tb(5000) + _tb(5001))[-3:]]
    assert SR.first_hit_step(_table(), phrase, strings) == 2
    toks, lens, steps, _, lp = engine.generate(*b, max_len=8, stop_id=stop, constraint=[[phrase]] * 2, constraint_then_free=True,
                                               stop_strings=strings, return_logprobs=True)
    print(f"[{engine.precision}] constraint_then_free: tokens {toks.tolist()}, log-probs {lp.tolist()}")
    assert toks[:, :3].tolist() == [[5000, 5001, stop]] * 2 and lens.tolist() == [2, 2]
    assert (lp[:, 2] == 0.0).all() and np.isfinite(lp[:, :3]).all()


def test_fp8_the_token_after_the_hit_is_the_stop_id(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    e8.set_vocab_bytes(*_table())
    try:
        b = synth.make_batch(3)
        free, *_ = e8.generate(*b, max_len=ML, stop_id=-1)
        stop = _free_stop(free)
        strings = [_tb(free[0, 2])[-2:] + _tb(free[0, 3])[:2]]
        toks, lens, *_ = e8.generate(*b, max_len=ML, stop_id=stop, stop_strings=strings)
        n = 0
        for r in range(3):
            row = toks[r].tolist()
            k = row.index(stop) if stop in row else len([t for t in row if t >= 0])
            first = SR.first_hit_step(_table(), row[:k], strings)
            print(f"[fp8] row {r}: tokens {row}, first hit after {first} tokens")
            if stop in row:
                assert first == k
                n += 1
            else:
                assert first is None or first == k
        assert n >= 1
    finally:
        e8.close()


# ---- 6. arming clears; a fork shares the table ---------------------------------------------------------------------------------------
def test_an_unarmed_call_after_an_armed_one_is_what_it_was(engine):
    b = synth.make_batch(3)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1)
    stop = _free_stop(free)
    strings = [_tb(free[0, 2])[-2:] + _tb(free[0, 3])[:2]]
    pt, pl, ps, _, plp = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True)
    ct, *_ = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True, stop_strings=strings)
    at, al, as_, _, alp = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True)
    assert ct.tobytes() != pt.tobytes()
    assert at.tobytes() == pt.tobytes() and alp.tobytes() == plp.tobytes() and as_ == ps and np.array_equal(al, pl)
    # a fork has strings of its own, initially none, and sees the table set on its parent
    f = engine.fork()
    try:
        ft, *_ = f.generate(*b, max_len=ML, stop_id=stop)
        gt, *_ = f.generate(*b, max_len=ML, stop_id=stop, stop_strings=strings)
        assert ft.tobytes() == pt.tobytes() and gt.tobytes() == ct.tobytes()
    finally:
        f.close()


def test_without_the_table_the_call_is_refused(synth_sd):
    e = E.Engine(device=0, precision="f32")
    e.load_state_dict(synth_sd)
    try:
        b = synth.make_batch(1)
        with pytest.raises(E.EngineError, match="mellow_set_vocab_bytes"):
            e.generate(*b, max_len=2, stop_id=2, stop_strings=[b"a"])
    finally:
        e.close()


# ---- 7. the wrapper -------------------------------------------------------------------------------------------------------------------------
class ConcatTok:
    """decode(ids) is the concatenation of the per-token texts of the byte table"""
    def __len__(self):
        return V

    def encode(self, s):
        return [_DATA["stop"]] if s == "<|endoftext|>" else [0]

    def decode(self, ids):
        return "".join("<|endoftext|>" if int(t) == _DATA["stop"] else _tb(int(t)).decode("latin-1") for t in ids)


def test_wrapper_cuts_the_texts(engine):
    import torch
    from mellow_amd import spec
    from mellow_amd.stop_strings import cut_text
    from mellow_amd.wrapper import MellowWrapper
    b = synth.make_batch(3)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1)
    _DATA["stop"] = _free_stop(free)
    w = MellowWrapper.__new__(MellowWrapper)
    w.tokenizer, w.model, w._data_parallel = ConcatTok(), engine, False
    w._vocab_bytes = _table()            # the table the engine has: ConcatTok's texts are its tokens, as latin-1
    w.preprocess_audio = lambda files, resample, _n=iter((b[0], b[1]) * 8): torch.from_numpy(next(_n))
    w.preprocess_text = lambda prompts: {"input_ids": torch.from_numpy(b[2])}
    ex = [[f"a{i}.wav", f"b{i}.wav", f"q{i}"] for i in range(3)]
    plain = w.generate(ex, ML, 0.8, 1.0)
    s = (_tb(free[0, 2])[-2:] + _tb(free[0, 3])[:2]).decode("latin-1")
    assert s in plain[0]
    cut = w.generate(ex, ML, 0.8, 1.0, stop_strings=[s, "NEVER"])
    keep = w.generate(ex, ML, 0.8, 1.0, stop_strings=s, include_stop_str_in_output=True)
    dicts = w.generate(ex, ML, 0.8, 1.0, stop_strings=[s], return_logprobs=True)
    print(f"[{engine.precision}] wrapper: string {s!r}; plain {plain}; cut {cut}; kept {keep}; reasons {[d['stop_reason'] for d in dicts]}")
    assert cut == [cut_text(t, [s], False)[0] for t in plain] and keep == [cut_text(t, [s], True)[0] for t in plain]
    assert cut[0] == plain[0][:plain[0].index(s)] and keep[0] == cut[0] + s
    assert [d["text"] for d in dicts] == cut and dicts[0]["stop_reason"] == s
    assert [d["stop_reason"] for d in dicts] == [cut_text(t, [s])[1] for t in plain]
    hit = _expect(free, [s.encode("latin-1")])
    assert dicts[0]["tokens"] == hit[0] + 1 and dicts[0]["token_logprobs"][-1] == 0.0      # the sum ends at the matching token (+ 0.0)
