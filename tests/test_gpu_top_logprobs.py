"""GPU (-m gpu): top log-probs inside the decode step (include/mellow_hip.h mellow_generate_top_logprobs / mellow_top_logprobs_apply;
Engine.generate(top_logprobs=); mellow_amd/csrc/top_logprobs.hip).

Yardsticks: the numpy definition of tests/top_logprobs_ref.py for the tap -- the ids exactly, the log-probs against fp64 within
1e-4 + 2 ulp (1e-4 is the bound the merged lse is held to against fp64 in tests/test_gpu_guidance.py (d)); properties that hold exactly
whatever the rounding for the generation loop; and Engine.forward (teacher forced, all positions, no K/V cache) for the recorded
alternatives.  TOL = 6e-3 is the project's logit tolerance (tests/test_gpu_nseq.py derives it); a log-prob is held to 2 * TOL as in
tests/test_gpu_logit_rules.py, and a comparison of two log-probs to 4 * TOL.  Every test prints what it measured."""
import os
import sys

import numpy as np
import pytest

from mellow_amd import engine as E
from mellow_amd import spec, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import top_logprobs_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 6e-3
V = 49152
T = spec.PREFIX_LEN
NEG = np.float32(-np.inf)


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    e = E.Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


_DATA = {}


def _real_logits(engine):
    """eight rows of prefill logits (computed once, by whichever engine asks first: they are test data here)"""
    if "l" not in _DATA:
        a1, a2, ids = synth.make_batch(8)
        _DATA["l"] = engine.lm_prefill(engine.prefix(a1, a2, ids), reserve=4).cpu().numpy()
    return _DATA["l"]


def _partials(engine, rows, bias=None):
    """(logits, cand_val, cand_sum) of the rows as the rules launch leaves them: neutral rules, or a bias for all of them"""
    B = rows.shape[0]
    out = engine.logit_rules_apply(rows, np.zeros((B, 1), dtype=np.int32), np.zeros(B, dtype=np.int32), logit_bias=bias)      # (empty histories)
    return out["logits"], out["cand_val"], out["cand_sum"]


# ---- 1. the tap against the definition ------------------------------------------------------------------------------------------
FINITE3 = (40001, 17, 49151)


def _tap_rows(engine):
    """34 rows (past one 32-row block) and their partials; row 0 is the heavily tied one, the row of the B = 1 case"""
    if "tap" in _DATA:
        return _DATA["tap"]
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(7):
        rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))    # heavy exact ties
        rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)              # peaked
        rows.append(rng.standard_normal(V).astype(np.float32) * 0.3)              # flat
    rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)
    rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))
    # the 20 largest values all in the registers of ONE thread: thread 77 of the 1024 holds the float4 groups q * 1024 + 77, so its
    # groups q = 0 .. 4 are 20 values (a float4 group itself holds four).  Descending in index order inside a group, ascending over
    # the groups, two of them equal
    one = rng.standard_normal(V).astype(np.float32)
    for q in range(5):
        for j in range(4):
            one[4 * (q * 1024 + 77) + j] = 20.0 + q - 0.25 * j
    one[4 * (2 * 1024 + 77) + 1] = one[4 * (2 * 1024 + 77) + 0]
    rows.append(one)
    # the largest values at the last indices (49151, 49150, ...), two of them tied; then three zeros, the middle one a -0, in index
    # order; everything else negative
    last = (-1.0 - np.abs(rng.standard_normal(V))).astype(np.float32)
    last[V - 10:] = 30.0 + np.arange(10, dtype=np.float32)
    last[V - 2] = last[V - 1]
    last[[50, 200]] = 0.0
    last[100] = -0.0
    rows.append(last)
    rows.append(rng.standard_normal(V).astype(np.float32))                        # all but 3 tokens banned (below)
    rows += list(_real_logits(engine))
    rows = np.stack(rows)
    assert rows.shape == (34, V)
    lg, cv, cs = _partials(engine, rows)
    assert lg.tobytes() == rows.tobytes()                                         # neutral rules leave the rows as they are
    bias = np.full(V, NEG, dtype=np.float32)
    bias[list(FINITE3)] = 0.0
    bl, bv, bs = _partials(engine, rows[25:26], bias)
    lg, cv, cs = lg.copy(), cv.copy(), cs.copy()
    lg[25], cv[25], cs[25] = bl[0], bv[0], bs[0]
    assert int(np.isfinite(lg[25]).sum()) == 3
    ref = {k: TR.topk_rows(lg, k) for k in (1, 5, 20)}                            # computed once, shared, left unchanged
    _DATA["tap"] = (lg, cv, cs, ref)
    return _DATA["tap"]


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("B", [1, 34])
def test_tap_against_the_definition(engine, B, k):
    lg, cv, cs, ref = _tap_rows(engine)
    ids, lp = engine.top_logprobs_apply(lg[:B], cv[:B], cs[:B], k)
    ids2, lp2 = engine.top_logprobs_apply(lg[:B], cv[:B], cs[:B], k)
    want_ids, want_lp = ref[k][0][:B], ref[k][1][:B]
    fin = np.isfinite(want_lp)
    with np.errstate(invalid="ignore"):                 # (-inf entries: checked below, not through their difference)
        err = np.abs(lp.astype(np.float64) - want_lp)
    bound = 1e-4 + 2 * np.spacing(np.abs(want_lp[fin]).astype(np.float32)).astype(np.float64)
    ties = int((lp[:, 1:] == lp[:, :-1]).sum()) if k > 1 else 0
    print(f"[{engine.precision}] tap B = {B}, k = {k}: ids equal {np.array_equal(ids, want_ids)}; max |lp - fp64| on finite entries "
          f"{float(err[fin].max()):.3e} (bound 1e-4 + 2 ulp); -inf entries {int((~fin).sum())}; adjacent equal log-probs {ties}")
    assert ids.shape == (B, k) and lp.shape == (B, k) and ids.dtype == np.int32 and lp.dtype == np.float32
    assert np.array_equal(ids, want_ids), "(a) the ids are not those of the definition"
    assert (err[fin] <= bound).all(), "(b)"
    assert np.isneginf(lp[~fin]).all(), "(c)"
    assert ids.tobytes() == ids2.tobytes() and lp.tobytes() == lp2.tobytes(), "(d) two calls differ"
    if B == 34 and k == 20:
        assert sorted(ids[25, :3].tolist()) == sorted(FINITE3)
        assert ids[25, 3:].tolist() == [i for i in range(40) if i not in FINITE3][:17]      # the banned ones follow by index
        assert set(ids[23].tolist()) == {4 * (q * 1024 + 77) + j for q in range(5) for j in range(4)}
        assert ids[24, :2].tolist() == [V - 2, V - 1] and ids[24, 10:13].tolist() == [50, 100, 200]      # -0 counts as +0


def test_tap_survives_nan_and_inf(engine):
    """runs once: one row with a NaN logit, one with +inf.  All log-probs NaN, all ids inside the vocabulary, nothing else is defined"""
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((2, V)).astype(np.float32)
    rows[0, 12345] = np.nan
    rows[1, 777] = np.inf
    lg, cv, cs = _partials(engine, rows)
    ids, lp = engine.top_logprobs_apply(lg, cv, cs, 5)
    print(f"[{engine.precision}] NaN / +inf rows: ids {ids.tolist()}, lp {lp.tolist()}")
    assert np.isnan(lp).all()
    assert ((ids >= 0) & (ids < V)).all()


# ---- 2. the greedy loop; 5. against the teacher-forced forward -----------------------------------------------------------------------
ML2, K2 = 6, 5


def _greedy(engine):
    """the armed and the un-armed greedy call on 3 synthetic examples, and the teacher-forced logits at every generated position"""
    key = ("greedy", engine.precision)
    if key not in _DATA:
        b = synth.make_batch(3)
        plain = engine.generate(*b, max_len=ML2, stop_id=-1, return_logprobs=True)
        armed = engine.generate(*b, max_len=ML2, stop_id=-1, return_logprobs=True, top_logprobs=K2)
        toks = armed[0]
        L = []
        for st in range(ML2):
            ans = np.concatenate([toks[:, :st], np.zeros((3, 1), dtype=toks.dtype)], axis=1).astype(np.int64)      # (a dummy last token)
            L.append(engine.forward(*b, ans, from_pos=T - 1 + st)[:, 0].cpu().numpy())
        _DATA[key] = (b, plain, armed, np.stack(L, axis=1))       # L [3][ML2][V]
    return _DATA[key]


def _ordered(ids, lp):
    """top_lp non-increasing along k, equal values in ascending id (over the computed entries)"""
    ok = True
    for i, x in zip(ids.reshape(-1, ids.shape[-1]), lp.reshape(-1, lp.shape[-1])):
        if i[0] < 0:
            continue
        ok &= bool((np.diff(x) <= 0).all())
        eq = np.diff(x) == 0
        ok &= bool((np.diff(i)[eq] > 0).all())
    return ok


def test_greedy_loop(engine):
    """|top_lp[..., 0] - logprobs| <= 1e-5: the greedy kernel records -log S, the record M - (M + log S).  The two differ by two roundings,
    that of lse = M + log S and that of the subtraction, each at most half an ulp at the magnitude of lse: below 128 that is 2^-18 =
    3.8e-6 each, 7.6e-6 together.  The precondition asserted is therefore max(|M|, |lse|) < 128 over the rows, M and lse taken from
    Engine.forward.  (Below 64, the figure this test was first written with, the two roundings give 3.8e-6 together; the synthetic
    checkpoint does not meet it: measured on the MI355X, M = 117.5 and lse = 117.8 at the largest, and the difference 3.81e-6, one
    half-ulp at that magnitude.  The bound itself is unchanged.)"""
    b, plain, armed, L = _greedy(engine)
    assert len(plain) == 5 and len(armed) == 7
    toks, lens, steps, _, lp, tid, tlp = armed
    for x, y in zip(plain[:3], armed[:3]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "tokens / lengths / steps changed with the record armed"
    assert plain[4].tobytes() == lp.tobytes(), "the log-probs changed with the record armed"
    assert tid.shape == (3, steps, K2) and tlp.shape == (3, steps, K2) and tid.dtype == np.int32 and tlp.dtype == np.float32
    lmax = float(np.abs(L).max())
    mmax = float(max(np.abs(L.max(axis=-1)).max(), np.abs(TR.logsumexp64(L)).max()))
    d0 = float(np.abs(tlp[..., 0] - lp)[toks >= 0].max())
    print(f"[{engine.precision}] greedy, 3 examples, max_len {ML2}, k = {K2}: steps {steps}; alternative 0 == token at {int((tid[..., 0] == toks).sum())} of "
          f"{toks.size}; max |top_lp[0] - logprob| {d0:.3e} (bound 1e-5); max(|M|, |lse|) over the rows of the forward {mmax:.2f} (precondition < 128); "
          f"max |logit| of the forward {lmax:.2f}")
    assert mmax < 128.0
    assert (tid[..., 0] == toks)[toks >= 0].all()
    assert d0 <= 1e-5
    assert _ordered(tid, tlp)
    assert (tid[toks < 0] == -1).all() and (tlp[toks < 0] == 0.0).all()
    assert ((tid >= 0) & (tid < V))[toks >= 0].all() and np.isfinite(tlp).all()


def test_against_the_teacher_forced_forward(engine):
    """every recorded alternative of the greedy answers against Engine.forward on the same answers: membership within 4 * TOL of the
    k-th largest log-softmax value, both ways, and the log-probs within 2 * TOL.  No decision is left out."""
    b, plain, armed, L = _greedy(engine)
    toks, _, steps, _, lp, tid, tlp = armed
    dmax, low, near = 0.0, 0.0, 0
    for r in range(3):
        for st in range(steps):
            ok, lo, nb = TR.membership(L[r, st], tid[r, st], 4 * TOL)
            ls = TR.log_softmax64(L[r, st])
            d = float(np.abs(tlp[r, st].astype(np.float64) - ls[tid[r, st].astype(np.int64)]).max())
            print(f"[{engine.precision}] row {r} step {st}: lowest recorded value - k-th value {lo:+.3e}, tokens within the band of the k-th {nb}, "
                  f"max |top_lp - log-softmax of the forward| {d:.3e}")
            assert ok, (r, st, tid[r, st].tolist())
            dmax, low, near = max(dmax, d), min(low, lo), near + nb
    print(f"[{engine.precision}] {3 * steps} records checked, none skipped: max |top_lp - forward| {dmax:.3e} (bound {2 * TOL:.1e}); lowest margin {low:+.3e}")
    assert dmax <= 2 * TOL


# ---- 3. the sampled loop -------------------------------------------------------------------------------------------------------------
def test_sampled_loop(engine):
    b, _, garmed, _ = _greedy(engine)
    kw = dict(max_len=ML2, stop_id=-1, return_logprobs=True, do_sample=True, seed=7, top_p=0.9, temperature=0.7)
    plain = engine.generate(*b, **kw)
    toks, lens, steps, _, lp, tid, tlp = engine.generate(*b, top_logprobs=K2, **kw)
    assert plain[0].tobytes() == toks.tobytes() and plain[4].tobytes() == lp.tobytes() and np.array_equal(plain[1], lens) and plain[2] == steps
    among = tid == toks[..., None]
    hit = among.any(axis=-1)
    got = np.where(among, tlp, 0.0).sum(axis=-1, dtype=np.float32)
    print(f"[{engine.precision}] sampled (seed 7, top_p 0.9, T 0.7): drawn token among the {K2} alternatives at {int(hit.sum())} of {toks.size} steps, "
          f"not the best one at {int((hit & ~among[..., 0]).sum())}; bit-equal log-prob at {int((got.view(np.uint32) == lp.view(np.uint32))[hit].sum())}")
    assert hit.any()
    assert (got.view(np.uint32) == lp.view(np.uint32))[hit].all(), "a drawn token's entry is not bit-equal to the call's log-prob"
    assert np.array_equal(tid[:, 0], garmed[5][:, 0]), "step 0: the alternatives are not those of the temperature-1 row"
    assert tlp[:, 0].tobytes() == garmed[6][:, 0].tobytes()
    assert _ordered(tid, tlp)


# ---- 4. rows and slots -----------------------------------------------------------------------------------------------------------------
def test_rows_and_slots(engine):
    """34 examples (two row blocks), max_len 4, k = 3, a stop id that some rows produce early: block exit and row migration.  Every
    row's record equals that of the same example run alone."""
    B, ML, k = 34, 4, 3
    b = synth.make_batch(B)
    free, *_ = engine.generate(*b, max_len=ML, stop_id=-1)
    vals, counts = np.unique(free[:, :2], return_counts=True)
    stop = int(vals[np.argmax(counts)])
    toks, lens, steps, _, lp, tid, tlp = engine.generate(*b, max_len=ML, stop_id=stop, return_logprobs=True, top_logprobs=k)
    repacks = engine.last_row_repacks()
    early = int((lens < steps - 1).sum())
    print(f"[{engine.precision}] B = {B}, stop id {stop}: steps {steps}, rows stopped before the last step {early}, repacks {repacks}, "
          f"never-computed entries {int((toks < 0).sum())}")
    assert early >= 1 and steps >= 2
    assert (tid[toks < 0] == -1).all() and (tlp[toks < 0] == 0.0).all()
    assert (tid[toks >= 0] >= 0).all() and (tid[..., 0] == toks)[toks >= 0].all()
    L = []
    if engine.precision != "f32":
        for st in range(steps):
            ans = np.concatenate([np.maximum(toks[:, :st], 0), np.zeros((B, 1), dtype=toks.dtype)], axis=1).astype(np.int64)
            L.append(engine.forward(*b, ans, from_pos=T - 1 + st)[:, 0].cpu().numpy())
    dmax, same, parted = 0.0, 0, 0
    for r in range(B):
        one = engine.generate(*(x[r:r + 1] for x in b), max_len=ML, stop_id=stop, return_logprobs=True, top_logprobs=k)
        n = min(int(lens[r]) + 1, steps, one[2])            # the row's own tokens, the stop id included
        assert n >= 1
        if engine.precision == "f32":
            assert np.array_equal(one[0][0, :n], toks[r, :n]), (r, one[0], toks[r])
        else:
            # f32x3 arithmetic depends on the batch: should the two runs ever choose different tokens, their records are comparable up
            # to and including that step (the histories are equal until then)
            diff = np.nonzero(one[0][0, :n] != toks[r, :n])[0]
            if diff.size:
                parted += 1
                n = int(diff[0]) + 1
        if engine.precision == "f32":
            assert np.array_equal(one[5][0, :n], tid[r, :n]), (r, one[5][0, :n], tid[r, :n])
        else:
            for st in range(n):
                assert TR.membership(L[st][r], tid[r, st], 4 * TOL)[0] and TR.membership(L[st][r], one[5][0, st], 4 * TOL)[0], (r, st)
        eq = one[5][0, :n] == tid[r, :n]
        same += int(eq.all())
        if eq.any():
            dmax = max(dmax, float(np.abs(one[6][0, :n] - tlp[r, :n])[eq].max()))
    print(f"[{engine.precision}] rows whose ids equal those of the run alone: {same} of {B}; rows whose tokens part from the run alone {parted}; "
          f"max |lp - lp alone| {dmax:.3e} (bound {2 * TOL:.1e})")
    assert dmax <= 2 * TOL


def test_more_than_1024_rows_advance_through_the_record(engine):
    """1026 rows = a pass of 1024 and a pass of 2 (examples 0 .. 7 in turn, then example 0 twice).  The stop id is example 0's first
    token, so the second pass ends after one step while the first goes on: its rows' later columns are padded like the token record."""
    ML, k = 3, 2
    b8 = synth.make_batch(8)
    free = engine.generate(*b8, max_len=ML, stop_id=-1, return_logprobs=True, top_logprobs=k)
    stop = int(free[0][0, 0])
    order = [i % 8 for i in range(1024)] + [0, 0]
    big = tuple(np.ascontiguousarray(x[order]) for x in b8)
    toks, lens, steps, _, lp, tid, tlp = engine.generate(*big, max_len=ML, stop_id=stop, return_logprobs=True, top_logprobs=k)
    print(f"[{engine.precision}] 1026 rows, stop id {stop}: steps {steps}; tail rows: tokens {toks[1024:].tolist()}, ids {tid[1024:].tolist()}; "
          f"step-0 |lp - lp of the 8-row call| {float(np.abs(tlp[1024:, 0] - free[6][0, 0]).max()):.3e}")
    assert toks.shape == (1026, steps) and tid.shape == (1026, steps, k) and tlp.shape == (1026, steps, k) and steps >= 2
    assert (toks[1024:, 0] == stop).all() and (toks[1024:, 1:] == -1).all() and (lens[1024:] == 0).all()
    assert (tid[toks < 0] == -1).all() and (tlp[toks < 0] == 0.0).all()
    assert (tid[..., 0] == toks)[toks >= 0].all() and np.isfinite(tlp).all() and _ordered(tid, tlp)
    if engine.precision == "f32":           # (encoder and prefill do not depend on the batch in this mode: rows 0 and 8 of the first pass
        #                                      and row 0 of the 8-row call are the same example)
        assert tid[1024:, 0].tobytes() == tid[0:16:8, 0].tobytes() and tlp[1024:, 0].tobytes() == tlp[0:16:8, 0].tobytes()
        assert np.array_equal(tid[1024:, 0], np.repeat(free[5][0:1, 0], 2, axis=0))
    assert float(np.abs(tlp[1024:, 0] - free[6][0, 0]).max()) <= 2 * TOL


# ---- 6. combinations ---------------------------------------------------------------------------------------------------------------------
def test_with_rules(engine):
    b = synth.make_batch(2)
    toks, _, steps, _, lp, tid, tlp = engine.generate(*b, max_len=5, stop_id=-1, return_logprobs=True, top_logprobs=5, no_repeat_ngram_size=1)
    bad = 0
    for r in range(2):
        assert len(set(toks[r].tolist())) == steps                      # (the rule itself: no token twice)
        for st in range(steps):
            hist = set(toks[r, :st].tolist())
            bad += sum(1 for v, x in zip(tid[r, st].tolist(), tlp[r, st].tolist()) if np.isfinite(x) and v in hist)
    print(f"[{engine.precision}] no_repeat_ngram_size = 1: alternatives with a finite log-prob that are tokens of the row's history: {bad}")
    assert bad == 0 and (tid[..., 0] == toks).all() and _ordered(tid, tlp)


def test_with_guidance(engine):
    b = synth.make_batch(2)
    neg = (b[1], b[0], b[2])
    res = engine.generate(*b, max_len=5, stop_id=-1, return_logprobs=True, top_logprobs=5, guidance_scale=2.0, negative=neg, keep_negative_rows=True)
    toks, tid, tlp = res[0], res[5], res[6]
    assert tid.shape == (4, res[2], 5)
    assert tid[0::2].tobytes() == tid[1::2].tobytes() and tlp[0::2].tobytes() == tlp[1::2].tobytes(), "the two rows of a pair differ"
    half = engine.generate(*b, max_len=5, stop_id=-1, return_logprobs=True, top_logprobs=5, guidance_scale=2.0, negative=neg)
    assert half[5].tobytes() == tid[0::2].tobytes() and half[6].tobytes() == tlp[0::2].tobytes()
    assert (tid[..., 0] == toks).all() and _ordered(tid, tlp)
    print(f"[{engine.precision}] guided, s = 2: pair rows byte-equal over {res[2]} steps; the conditional rows are what is returned")


def test_with_num_return_sequences_and_question_lists(engine):
    b = synth.make_batch(4)
    two = tuple(x[:2] for x in b)
    kw = dict(max_len=5, stop_id=-1, return_logprobs=True, top_logprobs=5)
    S = dict(do_sample=True, seed=11, top_p=0.9, temperature=0.8)
    n2 = engine.generate(*two, num_return_sequences=2, **S, **kw)
    ex = engine.generate(*(np.repeat(x, 2, axis=0) for x in two), **S, **kw)
    q_ids = np.asarray(b[2]).reshape(2, 2, -1)                      # questions (0, 1) about pair 0, (2, 3) about pair 1
    q2 = engine.generate(two[0], two[1], q_ids, **kw)
    qx = engine.generate(np.repeat(two[0], 2, axis=0), np.repeat(two[1], 2, axis=0), np.asarray(b[2]), **kw)
    for name, got, want in (("num_return_sequences = 2", n2, ex), ("2 questions", q2, qx)):
        assert got[5].shape == (4, got[2], 5) and got[6].shape == (4, got[2], 5)
        assert _ordered(got[5], got[6])
        same = got[0].tobytes() == want[0].tobytes() and got[5].tobytes() == want[5].tobytes() and got[6].tobytes() == want[6].tobytes()
        print(f"[{engine.precision}] {name}: tokens and records byte-equal to the expanded list: {same}")
        if engine.precision == "f32":
            assert same, name


def test_fp8_properties(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        b = synth.make_batch(2)
        toks, _, steps, _, lp, tid, tlp = e8.generate(*b, max_len=5, stop_id=-1, return_logprobs=True, top_logprobs=5)
        print(f"[fp8] greedy: steps {steps}, max |top_lp[0] - logprob| {float(np.abs(tlp[..., 0] - lp).max()):.3e}")
        assert tid.shape == (2, steps, 5) and (tid[..., 0] == toks).all() and np.isfinite(tlp).all() and _ordered(tid, tlp)
    finally:
        e8.close()


# ---- 7. disarm ---------------------------------------------------------------------------------------------------------------------------
def test_a_plain_call_after_an_armed_one_is_the_plain_call(engine):
    b = synth.make_batch(3)

    def plain():
        engine.prof_enable(True)
        engine.prof_reset()
        try:
            res = engine.generate(*b, max_len=ML2, stop_id=-1, return_logprobs=True)
            return res, {k: v["launches"] for k, v in engine.prof_report().items()}
        finally:
            engine.prof_enable(False)

    before, n0 = plain()
    armed = engine.generate(*b, max_len=ML2, stop_id=-1, return_logprobs=True, top_logprobs=20)
    after, n1 = plain()
    greedy, *_ = engine.generate(*b, max_len=ML2, stop_id=-1)
    print(f"[{engine.precision}] launches of the plain call before / after an armed one: {sum(n0.values())} / {sum(n1.values())}")
    assert len(armed) == 7 and len(after) == 5
    assert before[0].tobytes() == after[0].tobytes() and before[4].tobytes() == after[4].tobytes() and before[2] == after[2]
    assert n0 == n1
    assert greedy.tobytes() == before[0].tobytes()
    # the raw ABI: a call that records no log-probs refuses an armed record and disarms it
    import ctypes as C
    import torch
    lib, h, p = engine.lib, engine.h, E._ptr
    a1, a2, ids = engine._f32(b[0]), engine._f32(b[1]), engine._prompt_ids(b[2])
    out = torch.zeros((3, ML2), dtype=torch.int32, device=engine.tdev)
    rid = torch.zeros((3, ML2, 4), dtype=torch.int32, device=engine.tdev)
    rlp = torch.zeros((3, ML2, 4), dtype=torch.float32, device=engine.tdev)
    lens, steps, ftm = (C.c_int32 * 3)(), C.c_int32(0), C.c_float(0.0)
    engine._sync_inputs()
    assert lib.mellow_generate_top_logprobs(h, 4, p(rid), p(rlp)) == 0, lib.mellow_last_error().decode()
    assert lib.mellow_generate(h, p(a1), p(a2), int(a1.shape[1]), p(ids), 3, ML2, 0.8, 1.0, -1, 0, p(out), lens, C.byref(steps), C.byref(ftm)) != 0
    assert "records no log-probs" in lib.mellow_last_error().decode()
    assert lib.mellow_generate(h, p(a1), p(a2), int(a1.shape[1]), p(ids), 3, ML2, 0.8, 1.0, -1, 0, p(out), lens, C.byref(steps), C.byref(ftm)) == 0
    assert out.cpu().numpy()[:, : steps.value].tobytes() == greedy.tobytes() and int(rid.abs().sum()) == 0
