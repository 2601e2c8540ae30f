"""GPU (-m gpu): constrained decoding inside the decode step (include/mellow_hip.h mellow_generate_constraint / mellow_constraint_apply;
Engine.generate(constraint=, constraint_then_free=); mellow_amd/csrc/constrain.hip).

Yardsticks: the numpy transcription of tests/constraint_ref.py for the tap (bit-equal: the launch stores -inf or leaves a value as
it is), membership in the phrase set for the generation loop (exact whatever the rounding), and Engine.forward (teacher forced, all
positions, no K/V cache) for decisions and log-probs.  TOL = 6e-3 is the bound tests/test_gpu_nseq.py derives for a log-prob of the
decode step against the reference; two routes that are each within TOL of it differ by at most 2 * TOL.  Every test prints what it
measured."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from mellow_amd import constraint as MC
from mellow_amd import engine as E
from mellow_amd import spec, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as CR  # noqa: E402
import logit_rules_ref as LR  # noqa: E402
from test_gpu_logit_rules import _tap_rows  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 6e-3
V = 49152
T = spec.PREFIX_LEN


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    e = E.Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


# ---- 1. the tap against the definition ------------------------------------------------------------------------------------------
# one arena: the root of BIG has 1500 edges (more than one stride of the 1024 threads) with the edge tokens 0, 31, 32 and 49151, all of
# tile 3 (96 .. 127, allowed whole) and none of tile 2 (64 .. 95, banned whole); [0] is terminal with children; [0, 5, 6] has one edge
_SINGLE = sorted({0, 31, 32, 49151} | set(range(96, 128)) | set(range(1000, 1000 + 30 * 1464, 30)))
assert len(_SINGLE) == 1500 and not any(64 <= t < 96 for t in _SINGLE)
BIG = [[t] for t in _SINGLE] + [[0, 5], [0, 5, 6, 7]]
SMALL = [[31, 32], [49151]]
STOPPY = [[7, 9]]                      # 7 is the stop id of half the cases: the root has an EDGE for it
# (phrase set, history): length 0, 1, phrase length, phrase length + 1 (past the stop), one that leaves the trie, a terminal node with
# children, the one-edge node, one that is dead at its first token
COMBOS = [(BIG, []), (BIG, [0]), (BIG, [0, 5, 6, 7]), (BIG, [0, 5, 6, 7, 7]), (BIG, [0, 99]), (BIG, [0, 5]), (BIG, [0, 5, 6]),
          (SMALL, [5]), (SMALL, []), (SMALL, [31]), (SMALL, [31, 32]), (SMALL, [49151, 7]), (STOPPY, []), (STOPPY, [7]), (STOPPY, [7, 9]), (STOPPY, [7, 9, 7])]


@pytest.mark.parametrize("then_free", [False, True])
@pytest.mark.parametrize("stop_id", [7, -1])
@pytest.mark.parametrize("B", [1, 33])
def test_tap_against_the_definition(engine, B, stop_id, then_free):
    rows = _tap_rows(engine, B)
    combos = [COMBOS[b % len(COMBOS)] for b in range(B)]
    sets, hists = [c[0] for c in combos], [c[1] for c in combos]
    hist = np.zeros((B, 8), dtype=np.int32)
    hl = np.array([len(h) for h in hists], dtype=np.int32)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = h
    out = engine.constraint_apply(rows, hist, hl, sets, then_free=then_free, stop_id=stop_id)
    again = engine.constraint_apply(rows, hist, hl, sets, then_free=then_free, stop_id=stop_id)
    base = engine.logit_rules_apply(rows, np.zeros((B, 1), dtype=np.int32), np.zeros(B, dtype=np.int32), stop_id=-1)    # what the head leaves
    trie = MC.build_trie(sets)
    assert max(np.diff(trie["node_first"])) == 1500 and min(np.diff(trie["node_first"])[np.diff(trie["node_first"]) > 0]) == 1
    want, states, con = CR.apply_rows(rows, trie, trie["row_root"], hists, stop_id=stop_id, then_free=then_free)
    val, idx = LR.tile_partials(want)
    lse = LR.merged_lse(out["cand_val"], out["cand_sum"])
    d = float(np.abs(lse - LR.logsumexp64(want)).max())
    dead = np.isneginf(val)
    print(f"[{engine.precision}] tap B = {B}, stop id {stop_id}, then_free {then_free}: states {states.tolist()}; {int(con.sum())} rows constrained, "
          f"{int(np.isneginf(want).sum())} logits banned, {int(dead.sum())} tiles banned whole; merged lse vs fp64 logsumexp: max|d| {d:.3e}")
    assert np.array_equal(out["state"], states)
    assert out["logits"].tobytes() == want.tobytes()
    assert out["cand_val"].tobytes() == val.tobytes() and np.array_equal(out["cand_idx"], idx)
    assert d <= 1e-4 and np.isfinite(lse).all()
    assert (out["cand_sum"][dead] == 0.0).all() and (out["cand_sum"][~dead] >= 1.0).all()
    assert con[0] and dead[0, 2] and not dead[0, 3] and out["logits"][0, 96:128].tobytes() == rows[0, 96:128].tobytes()   # tile 2 banned whole, tile 3 allowed whole
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)
    # rows whose allowed set is everything, or empty: byte-identical, partials included
    free = ~con
    if B == 33:
        assert con.any() and free.any() == (then_free or stop_id < 0)
        assert (states[free] == CR.FREE).any() == then_free
        assert any(CR.allowed(trie, int(u), stop_id) == [] for u in states[free]) == (stop_id < 0)
    for k in ("logits", "cand_val", "cand_idx", "cand_sum"):
        src = rows if k == "logits" else base[k]
        assert out[k][free].tobytes() == src[free].tobytes(), k


# ---- 2. membership, exact ---------------------------------------------------------------------------------------------------------------
# per example 2-5 phrases of 1-4 tokens; phrases share first tokens, and [1000] is a prefix of two others
SETS = [[[1000, 2000], [1000, 2001, 2002], [1000], [3000, 3001, 3002, 3003], [40000]],
        [[500], [600, 601]],
        [[7000, 7001, 7002], [7000, 7001, 7003, 7004], [31, 32], [49151]]]
STOP = 2
ML = 4 + 2                             # the longest phrase + 2


def _check_membership(toks, per_row_sets, label):
    toks = np.asarray(toks)
    for r, row in enumerate(toks):
        row = row.tolist()
        assert STOP in row, (label, r, row)
        n = row.index(STOP)
        assert row[:n] in per_row_sets[r], (label, r, row)                  # exactly one of its example's phrases
        assert all(t == STOP for t in row[n:]), (label, r, row)             # every token after that is the stop id
    print(f"[{label}] {toks.shape[0]} rows, {toks.shape[1]} steps: answers {[row.tolist()[:row.tolist().index(STOP)] for row in toks]}")


def _modes():
    b = synth.make_batch(3)
    ids2 = np.stack([b[2], synth.make_batch(3, first=3)[2]], axis=1)          # [3][2][129]: two questions per example
    neg = (np.zeros_like(b[0]), np.zeros_like(b[1]), b[2])                      # "silence"
    return {"greedy": (b, {}, 1), "sampled": (b, dict(do_sample=True, seed=3), 1),
            "nseq": (b, dict(do_sample=True, seed=3, num_return_sequences=3), 3), "questions": ((b[0], b[1], ids2), {}, 2),
            "beams": (b, dict(num_beams=3, num_return_sequences=2), 2), "guided": (b, dict(guidance_scale=1.5, negative=neg), 1)}


@pytest.mark.parametrize("mode", ["greedy", "sampled", "nseq", "questions", "beams", "guided"])
def test_every_answer_is_one_of_its_phrases(engine, mode):
    batch, kw, per = _modes()[mode]
    toks, lens, steps, _ = engine.generate(*batch, max_len=ML, stop_id=STOP, constraint=SETS, **kw)
    assert toks.shape[0] == 3 * per
    sets = [SETS[r // per] for r in range(3 * per)]
    _check_membership(toks, sets, f"{engine.precision} {mode}")
    assert all(lens[r] == toks[r].tolist().index(STOP) for r in range(3 * per))
    if mode == "beams":                                                       # the two hypotheses of an example differ
        assert all(toks[2 * e].tolist() != toks[2 * e + 1].tolist() for e in range(3))


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_then_free_constrains_only_the_start(engine, mode):
    batch, kw, _ = _modes()[mode]
    toks, lens, steps, _ = engine.generate(*batch, max_len=ML, stop_id=-1, constraint=SETS, constraint_then_free=True, **kw)
    assert toks.shape == (3, ML)                                              # no stop id: the answer is max_len tokens long
    for r in range(3):
        row = toks[r].tolist()
        assert any(row[:len(p)] == p for p in SETS[r]), (r, row)
    plain, *_ = engine.generate(*batch, max_len=ML, stop_id=-1, **kw)
    print(f"[{engine.precision}] then_free {mode}: {toks.tolist()}; the call without the set: {plain.tolist()}")
    assert not any(any(plain[r].tolist()[:len(p)] == p for p in SETS[r]) for r in range(3)), "the free call already starts with a phrase: the test shows nothing"


def test_fp8_greedy_and_guided_answers_are_phrases(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        for mode in ("greedy", "guided"):
            batch, kw, _ = _modes()[mode]
            toks, *_ = e8.generate(*batch, max_len=ML, stop_id=STOP, constraint=SETS, **kw)
            _check_membership(toks, SETS, f"fp8 {mode}")
    finally:
        e8.close()


# ---- 3. decisions and log-probs against Engine.forward ------------------------------------------------------------------------------
def test_greedy_decisions_and_logprobs_against_the_teacher_forced_forward(engine):
    """synth.make_batch(3) with SETS, stop id 2, max_len 6 (the loop ends after the step at which every row has stopped: 3 steps, 9
    decisions).  The phrase ids were chosen without a GPU: on the fp32 oracle
    (oracle/mellow_oracle.py on the same checkpoint, the mask of tests/constraint_ref.py on its logits) the gap between the best and
    the second allowed logit is 0.6306 (example 0, step 0: it picks [40000]), 60.5019 (example 1, step 0: [500]) and 0.8861 (example 2,
    step 0: [31, 32]); every other decision has ONE allowed token (gap inf).  The smallest, 0.6306, is 52 times the 2 * TOL = 0.012
    under which a decision may be skipped: the reference alone skips none."""
    b = synth.make_batch(3)
    toks, lens, steps, _, lp = engine.generate(*b, max_len=ML, stop_id=STOP, return_logprobs=True, constraint=SETS)
    trie = MC.build_trie(SETS)
    checked, skipped, dmax = np.zeros(3, dtype=int), 0, 0.0
    for s in range(steps):
        ans = np.concatenate([toks[:, :s], np.zeros((3, 1), dtype=toks.dtype)], axis=1).astype(np.int64)      # (a dummy last token)
        lg = engine.forward(*b, ans, from_pos=T - 1 + s)[:, 0].cpu().numpy()
        p, states, _ = CR.apply_rows(lg, trie, trie["row_root"], [toks[r, :s] for r in range(3)], stop_id=STOP)
        ls = LR.log_softmax64(p)
        for r in range(3):
            o = np.sort(p[r].astype(np.float64))[::-1]
            gap, want = float(o[0] - o[1]), LR.first_argmax(p[r])
            d = abs(float(lp[r, s]) - float(ls[r, toks[r, s]]))
            print(f"[{engine.precision}] step {s} example {r}: state {states[r]}, masked top-2 gap {gap:.4f}, chosen {int(toks[r, s])} == masked arg-max "
                  f"{want}: {int(toks[r, s]) == want}; |lp - masked log-softmax| {d:.3e}")
            if gap > 2 * TOL:
                assert int(toks[r, s]) == want, (s, r, int(toks[r, s]), want)
                checked[r] += 1
            else:
                skipped += 1
            assert d <= 2 * TOL, (s, r, d)
            dmax = max(dmax, d)
    print(f"[{engine.precision}] constrained greedy: {steps} steps, decisions skipped {skipped} of {3 * steps}; max|lp - masked log-softmax of the forward| "
          f"{dmax:.3e} (bound {2 * TOL:.1e})")
    assert skipped * 8 <= 3 * steps and (checked >= 1).all()


# ---- 4. exhaustive beams --------------------------------------------------------------------------------------------------------------
BEAM_SET = [[11, 12], [11, 13, 14], [15], [15, 16]]      # four phrases, two distinct first tokens


def test_exhaustive_beams_return_every_phrase_once_and_their_probabilities_sum_to_one(engine):
    """k = 4 over 4 phrases that start with only 2 distinct tokens: at step 0 the row has two finite candidates, so two of the four
    beams are filled with candidates of value -inf (include/mellow_hip.h: c descending, then parent, then token); they rank last,
    their rows go DEAD and offer the stop id at -inf, and the four finite continuations of step 1 displace them."""
    b = synth.make_batch(1)
    toks, lens, steps, _, lps, scores = engine.generate(*b, max_len=ML, stop_id=STOP, num_beams=4, num_return_sequences=4, return_logprobs=True,
                                                        constraint=[BEAM_SET])
    got = sorted(toks[r].tolist()[:lens[r]] for r in range(4))
    logprob = np.asarray(engine.last_beam["logprob"], dtype=np.float64)
    L = max(len(p) for p in BEAM_SET) + 1
    total, bound = float(np.exp(logprob).sum()), math.exp(L * TOL) - 1
    print(f"[{engine.precision}] beams: hypotheses {[toks[r].tolist()[:lens[r]] for r in range(4)]}, log-probs {logprob.tolist()}, sum of probabilities {total:.9f} "
          f"(|sum - 1| bound {bound:.3e})")
    assert got == sorted(BEAM_SET)
    assert np.isfinite(logprob).all()
    assert abs(total - 1.0) <= bound


# ---- 5. arming clears -------------------------------------------------------------------------------------------------------------------
def test_an_unarmed_call_after_an_armed_one_is_what_it_was(engine):
    b = synth.make_batch(3)
    pt, pl, ps, _, plp = engine.generate(*b, max_len=ML, stop_id=STOP, return_logprobs=True)
    ct, *_ = engine.generate(*b, max_len=ML, stop_id=STOP, return_logprobs=True, constraint=SETS)
    at, al, as_, _, alp = engine.generate(*b, max_len=ML, stop_id=STOP, return_logprobs=True)
    assert not np.array_equal(ct[:, :1], pt[:, :1])
    assert at.tobytes() == pt.tobytes() and alp.tobytes() == plp.tobytes() and as_ == ps and np.array_equal(al, pl)
    # armed for another row count: the call fails with a message, and takes the constraint with it
    con = E._CallConstraint(SETS[:2], False, V)
    con.expand(2, 1)
    assert engine.lib.mellow_generate_constraint(engine.h, C.byref(con.struct())) == 0
    with pytest.raises(E.EngineError, match="n_rows"):
        engine.generate(*b, max_len=ML, stop_id=STOP)
    after, *_ = engine.generate(*b, max_len=ML, stop_id=STOP)
    assert after.tobytes() == pt.tobytes()
    # NULL disarms
    con.expand(2, 1)
    assert engine.lib.mellow_generate_constraint(engine.h, C.byref(con.struct())) == 0
    assert engine.lib.mellow_generate_constraint(engine.h, None) == 0
    assert engine.generate(*b, max_len=ML, stop_id=STOP)[0].tobytes() == pt.tobytes()


# ---- 6. more than one pass ------------------------------------------------------------------------------------------------------------
def test_a_call_of_more_than_1024_rows_advances_through_the_roots_pass_by_pass(engine):
    """1027 rows (eight 2 s examples tiled) run as passes of 1024 and 3 rows; the sets cycle with period 3, so the second pass's rows
    1024 .. 1026 carry the sets of rows 1, 2, 0: a pass that started at the call's first root again would answer from the wrong set"""
    B = 1027
    a1, a2, ids = (np.tile(x, (B // 8 + 1, 1))[:B] for x in synth.make_batch(8, n_samples=2 * 32000))
    one = [[[100 + r]] for r in range(3)]
    toks, lens, steps, _ = engine.generate(a1, a2, ids, max_len=3, stop_id=STOP, constraint=[one[r % 3] for r in range(B)])
    assert toks.shape == (B, 2) and steps == 2
    assert toks[:, 0].tolist() == [100 + r % 3 for r in range(B)] and (toks[:, 1] == STOP).all() and (lens == 1).all()
