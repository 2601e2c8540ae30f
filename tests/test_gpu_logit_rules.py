"""GPU (-m gpu): repetition controls inside the decode step (include/mellow_hip.h mellow_generate_rules / mellow_logit_rules_apply;
Engine.generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, logit_bias=); mellow_amd/csrc/logit_rules.hip).

Yardsticks: the float32 transcription of tests/logit_rules_ref.py for the tap (bit-equal: every rule is one correctly rounded fp32
operation or a store of -inf), properties that hold exactly whatever the rounding for the generation loop, and Engine.forward
(teacher forced, all positions, no K/V cache) for the decisions.  TOL = 6e-3 is the bound tests/test_gpu_nseq.py derives for a log-prob
of the decode step against the reference; two routes that are each within TOL of it differ by at most 2 * TOL.  Every test prints
what it measured."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from mellow_amd import engine as E
from mellow_amd import spec, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import logit_rules_ref as LR  # noqa: E402

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


_REAL = {}


def _real_logits(engine):
    """eight rows of prefill logits (computed once, by whichever engine asks first: they are test data here)"""
    if "l" not in _REAL:
        a1, a2, ids = synth.make_batch(8)
        _REAL["l"] = engine.lm_prefill(engine.prefix(a1, a2, ids), reserve=4).cpu().numpy()
    return _REAL["l"]


# ---- 1. the tap against the definition ------------------------------------------------------------------------------------------
def _tap_rows(engine, B):
    rng = np.random.default_rng(1)
    if B == 1:
        return np.round(rng.standard_normal((1, V)) * 2.0).astype(np.float32)
    rows = []
    for _ in range(8):
        rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)              # peaked
        rows.append(rng.standard_normal(V).astype(np.float32) * 0.3)              # flat
        rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))    # heavy exact ties
    rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))
    rows += list(_real_logits(engine))
    assert len(rows) == 33
    return np.stack(rows)


def _histories(rows, n, ld=300):
    """per row a history of length 0, 1, n - 1, n, 40 or 300 (B = 1: 40) over a small alphabet -- the row's six best and six worst
    tokens and a few of tile 2 -- so that tokens and n-grams repeat and both signs of the penalty occur"""
    rng = np.random.default_rng(2)
    B = rows.shape[0]
    lens = [0, 1, max(n - 1, 0), n, 40, 300]
    hist = np.zeros((B, ld), dtype=np.int32)
    hl = np.zeros(B, dtype=np.int32)
    for b in range(B):
        order = np.argsort(rows[b], kind="stable")
        alpha = np.concatenate([order[-6:], order[:6], np.array([64, 65, 95])])
        L = 40 if B == 1 else lens[b % 6]
        h = rng.choice(alpha, size=L)
        if L >= 8:
            h[-3:] = h[2:5]                      # a forced repeat of the last (n - 1)-gram for n <= 4
        hist[b, :L] = h
        hl[b] = L
    return hist, hl


def _bias():
    rng = np.random.default_rng(4)
    bias = np.zeros(V, dtype=np.float32)
    at = rng.choice(V, 500, replace=False)
    bias[at] = rng.standard_normal(500).astype(np.float32) * 3
    bias[64:96] = NEG                            # tile 2 banned whole
    bias[1000] = NEG
    return bias


CASES = {
    "all": dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5, logit_bias=_bias(), stop_id=7),
    "ngram1": dict(repetition_penalty=0.7, no_repeat_ngram_size=1, stop_id=7),
    "ngram2": dict(no_repeat_ngram_size=2, min_new_tokens=1, stop_id=-1),
    "ngram4_bias": dict(no_repeat_ngram_size=4, logit_bias=np.where(np.isinf(_bias()), 0, _bias()).astype(np.float32), stop_id=3),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("B", [1, 33])
def test_tap_against_the_definition(engine, B, case):
    kw = dict(CASES[case])
    rows = _tap_rows(engine, B)
    hist, hl = _histories(rows, kw.get("no_repeat_ngram_size", 0))
    out = engine.logit_rules_apply(rows, hist, hl, **kw)
    again = engine.logit_rules_apply(rows, hist, hl, **kw)
    rk = dict(kw)
    rk["bias"] = rk.pop("logit_bias", None)
    want = LR.apply_rows(rows, [hist[b, :hl[b]] for b in range(B)], **rk)
    val, idx = LR.tile_partials(want)
    lse = LR.merged_lse(out["cand_val"], out["cand_sum"])
    d = float(np.abs(lse - LR.logsumexp64(want)).max())
    changed = int((want.view(np.int32) != rows.view(np.int32)).sum())
    dead = np.isneginf(val)
    print(f"[{engine.precision}] tap {case}, B = {B}: {changed} logits changed, {int(np.isneginf(want).sum())} banned, {int(dead.sum())} tiles banned "
          f"whole; merged lse vs fp64 logsumexp of the processed row: max|d| {d:.3e}")
    assert changed > 0
    assert out["logits"].tobytes() == want.tobytes()
    assert out["cand_val"].tobytes() == val.tobytes() and np.array_equal(out["cand_idx"], idx)
    assert d <= 1e-4 and np.isfinite(lse).all()
    assert (out["cand_sum"][dead] == 0.0).all() and (out["cand_sum"][~dead] >= 1.0).all()
    if "logit_bias" in kw and np.isinf(kw["logit_bias"]).any():
        assert dead[:, 2].all()
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)


def test_tap_neutral_rules_leave_the_logits_unchanged(engine):
    rows = _tap_rows(engine, 33)
    hist, hl = _histories(rows, 0)
    out = engine.logit_rules_apply(rows, hist, hl)
    val, idx = LR.tile_partials(rows)
    assert out["logits"].tobytes() == rows.tobytes()
    assert out["cand_val"].tobytes() == val.tobytes() and np.array_equal(out["cand_idx"], idx)
    d = float(np.abs(LR.merged_lse(out["cand_val"], out["cand_sum"]) - LR.logsumexp64(rows)).max())
    print(f"[{engine.precision}] neutral tap: merged lse vs fp64 logsumexp, max|d| {d:.3e}")
    assert d <= 1e-4


# ---- 2. exact properties end to end --------------------------------------------------------------------------------------------------
MODES = {"greedy": {}, "sampled": dict(do_sample=True, seed=3, top_p=0.9, temperature=0.8), "beam": dict(num_beams=3, num_return_sequences=3)}


def _properties(engine, modes, label):
    b = synth.make_batch(3)
    plain, *_ = engine.generate(*b, max_len=12, stop_id=-1)
    sup = np.zeros(V, dtype=np.float32)
    sup[np.unique(plain)] = NEG
    for name in modes:
        kw = dict(MODES[name], max_len=12, stop_id=-1)
        t1, *_ = engine.generate(*b, no_repeat_ngram_size=1, **kw)
        t2, *_ = engine.generate(*b, no_repeat_ngram_size=2, **kw)
        t3, *_ = engine.generate(*b, logit_bias=sup, **kw)
        rows = 9 if name == "beam" else 3
        assert t1.shape == t2.shape == t3.shape == (rows, 12)
        for r in range(rows):
            assert len(set(t1[r].tolist())) == 12, (name, r, t1[r])
            bigrams = list(zip(t2[r, :-1].tolist(), t2[r, 1:].tolist()))
            assert len(set(bigrams)) == 11, (name, r, t2[r])
        assert not np.isin(t3, np.unique(plain)).any(), name
        print(f"[{label}] {name}: 12 distinct tokens per row with n = 1, 11 distinct bigrams with n = 2, none of the {np.unique(plain).size} "
              f"suppressed tokens; rows equal to the plain greedy rows: n = 1 {int((t1[:3] == plain).all(1).sum())}, suppressed 0 of {rows}")


@pytest.mark.parametrize("mode", list(MODES))
def test_exact_properties_end_to_end(engine, mode):
    _properties(engine, [mode], engine.precision)


def test_min_new_tokens_end_to_end(engine):
    """the stop id is the plain call's most frequent first token (the device of tests/test_gpu_nseq.py): the plain call gives length 0"""
    b = synth.make_batch(3)
    free, *_ = engine.generate(*b, max_len=12, stop_id=-1)
    vals, counts = np.unique(free[:, 0], return_counts=True)
    stop = int(vals[np.argmax(counts)])
    pt, pl, ps, _ = engine.generate(*b, max_len=12, stop_id=stop)
    toks, lens, steps, _ = engine.generate(*b, max_len=12, stop_id=stop, min_new_tokens=5)
    print(f"[{engine.precision}] stop id {stop}: plain lengths {pl.tolist()} (steps {ps}), with min_new_tokens = 5 {lens.tolist()} (steps {steps})")
    assert (pl == 0).any()
    assert steps >= 5 and (toks[:, :5] != stop).all() and (lens >= 5).all()
    bt, bl, bs, _ = engine.generate(*b, max_len=12, stop_id=stop, min_new_tokens=5, num_beams=2)
    assert (bt[:, :5] != stop).all() and (bl >= 5).all()


# ---- 3. armed-neutral equals plain ---------------------------------------------------------------------------------------------------
def test_neutral_rules_equal_the_plain_call(engine):
    b = synth.make_batch(3)
    pt, pl, ps, _, plp = engine.generate(*b, max_len=16, stop_id=-1, return_logprobs=True)
    nt, nl, ns, _, nlp = engine.generate(*b, max_len=16, stop_id=-1, return_logprobs=True, _arm_neutral_rules=True)
    at, al, as_, _, alp = engine.generate(*b, max_len=16, stop_id=-1, return_logprobs=True)
    d = float(np.abs(nlp - plp).max())
    print(f"[{engine.precision}] B = 3: neutral rules vs plain: tokens equal {np.array_equal(nt, pt)}, max|lp - plain lp| {d:.3e}")
    assert np.array_equal(nt, pt) and np.array_equal(nl, pl) and ns == ps
    assert d <= 1e-4
    assert np.array_equal(at, pt) and alp.tobytes() == plp.tobytes()          # a plain call after a ruled one: what it was before
    ruled, *_ = engine.generate(*b, max_len=16, stop_id=-1, repetition_penalty=1.5, no_repeat_ngram_size=1)
    after, *_ = engine.generate(*b, max_len=16, stop_id=-1)
    assert np.array_equal(after, pt) and ruled.shape == pt.shape


def test_neutral_rules_equal_the_plain_call_across_row_blocks(engine):
    """B = 40: two row blocks, the per-block exit and row migration on (the stop id is the most frequent early token of the free run)"""
    b = synth.make_batch(40)
    free, *_ = engine.generate(*b, max_len=24, stop_id=0, ignore_stop=True)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])
    pt, pl, ps, _ = engine.generate(*b, max_len=24, stop_id=stop)
    reps0 = engine.last_row_repacks()
    nt, nl, ns, _ = engine.generate(*b, max_len=24, stop_id=stop, _arm_neutral_rules=True)
    print(f"[{engine.precision}] B = 40, stop id {stop}: steps {ps} / {ns}, repacks {reps0} / {engine.last_row_repacks()}, rows stopped early {int((pl < ps).sum())}")
    assert np.array_equal(nt, pt) and np.array_equal(nl, pl) and ns == ps and engine.last_row_repacks() == reps0


# ---- 4. against an independent forward -----------------------------------------------------------------------------------------------
RULES4 = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
FIRST4 = 6


def _rep(batch, n):
    return tuple(np.repeat(x, n, axis=0) for x in batch)


def test_greedy_decisions_against_the_teacher_forced_forward(engine):
    """B = 2 (synthetic examples 6 and 7), max_len 8, repetition_penalty 1.3 and no_repeat_ngram_size 2 together, stop id -1: 16
    decisions.  The batch was chosen without a GPU: the fp32 oracle (oracle/mellow_oracle.py on the same checkpoint, the rules of
    tests/logit_rules_ref.py on its logits) puts the margin between the best and the second processed logit, for (step 0, example 0),
    (step 0, example 1), (step 1, example 0) ..., at
        1.1423 1.8874 | 4.7076 13.0586 | 1.5521 10.6136 | 3.6007 0.7375 | 1.6291 1.6838 | 0.9756 2.1031 | 3.8976 1.3782 | 11.6384 0.5792
    against the band 4 * TOL * (s + 1) = 0.024 ... 0.192 under which a decision may be skipped: none is below it (the closest, step 7
    of example 1, is 3.0 times the band).  Examples 2 and 3 have one margin below the band (0.1112 at step 6)."""
    B, ML = 2, 8
    b = synth.make_batch(B, first=FIRST4)
    toks, lens, steps, _, lp = engine.generate(*b, max_len=ML, stop_id=-1, return_logprobs=True, **RULES4)
    assert toks.shape == (B, ML)
    skipped, dmax = 0, 0.0
    for s in range(ML):
        ans = np.concatenate([toks[:, :s], np.zeros((B, 1), dtype=toks.dtype)], axis=1).astype(np.int64)      # (a dummy last token)
        lg = engine.forward(*b, ans, from_pos=T - 1 + s)[:, 0].cpu().numpy()
        p = LR.apply_rows(lg, [toks[r, :s] for r in range(B)], **RULES4)
        ls = LR.log_softmax64(p)
        for r in range(B):
            o = np.sort(p[r].astype(np.float64))[::-1]
            margin, band = float(o[0] - o[1]), 4 * TOL * (s + 1)
            want = LR.first_argmax(p[r])
            print(f"[{engine.precision}] step {s} example {r}: reference margin {margin:.4f} (band {band:.3f}), chosen == reference: {int(toks[r, s]) == want}")
            if margin < band:
                skipped += 1
            else:
                assert int(toks[r, s]) == want, (s, r, int(toks[r, s]), want)
            dmax = max(dmax, abs(float(lp[r, s]) - float(ls[r, toks[r, s]])))
    print(f"[{engine.precision}] greedy with rules: decisions skipped {skipped} of {B * ML}; max|lp - processed log-softmax of the forward| {dmax:.3e} "
          f"(bound {2 * TOL:.1e})")
    assert skipped <= 1
    assert dmax <= 2 * TOL


def test_beam_decisions_against_the_teacher_forced_forward(engine):
    """The same two examples and rules, k = 3: 16 decisions.  The oracle's own search (tests/beam_ref.py on the processed logits) puts
    the margin between the k-th and the (k + 1)-th candidate at
        0.1954 1.6140 | 1.3455 3.1974 | 0.2897 2.2998 | 0.1906 0.4963 | 0.8758 0.8031 | 0.3479 1.3810 | 2.9423 0.7846 | 0.7849 0.5198
    none below the band (the closest, step 3 of example 0, is 2.0 times it), and moves rows at every step from 1 on (parents
    [0, 1, 1 | 0, 1, 2] at step 1, ten (step, row) pairs in all).  Examples 0 and 1 have two margins below the band."""
    B, k, ML = 2, 3, 8
    N = B * k
    b = synth.make_batch(B, first=FIRST4)
    engine.generate(*b, max_len=ML, stop_id=-1, num_beams=k, **RULES4)
    tab = engine.last_beam
    par, tok, lp = tab["parent"], tab["token"], tab["lp"]
    assert par.shape == (ML, N)
    rb = _rep(b, k)
    seqs = [[] for _ in range(N)]
    ref_cum = np.where(np.arange(N) % k == 0, 0.0, -np.inf)
    dmax, skipped, moved = 0.0, 0, 0
    for s in range(ML):
        ans = np.array([q + [0] for q in seqs], dtype=np.int64)
        lg = engine.forward(*rb, ans, from_pos=T - 1 + s)[:, 0].cpu().numpy()
        p = LR.apply_rows(lg, seqs, **RULES4).astype(np.float64)
        ls = LR.log_softmax64(p)
        prow = np.arange(N) // k * k + par[s]
        want_lp = ls[prow, tok[s]]
        dmax = max(dmax, float(np.abs(lp[s] - want_lp).max()))
        cands = BR.candidates(p, ref_cum, np.zeros(N, dtype=np.int64), k, -1)
        for e in range(B):
            c = cands[e]
            margin, band = float(c[k - 1, 0] - c[k, 0]), 4 * TOL * (s + 1)
            got = {(int(par[s, e * k + j]), int(tok[s, e * k + j])) for j in range(k)}
            want = {(int(c[j, 1]), int(c[j, 2])) for j in range(k)}
            print(f"[{engine.precision}] step {s} example {e}: reference margin k-th / (k+1)-th {margin:.4f} (band {band:.3f}), chosen == reference: {got == want}")
            if margin < band:
                skipped += 1
            else:
                assert got == want, (s, e, got, want)
        moved += int((par[s] != np.arange(N) % k).sum()) if s >= 1 else 0
        ref_cum = ref_cum[prow] + want_lp
        seqs = [seqs[prow[r]] + [int(tok[s, r])] for r in range(N)]
    print(f"[{engine.precision}] beams with rules: max|lp - processed log-softmax of the forward| {dmax:.3e} (bound {2 * TOL:.1e}); decisions skipped "
          f"{skipped} of {B * ML}; (step, row) pairs whose parent is another row: {moved}")
    assert dmax <= 2 * TOL
    assert skipped <= 1
    assert moved >= 1, "every row kept its own history at every step: the history ping-pong was not exercised"


# ---- 5. the history follows the example, not the slot ---------------------------------------------------------------------------------
def test_history_follows_the_example_through_row_migration(engine):
    a1, a2, ids = synth.make_batch(40)
    kw = dict(do_sample=True, top_p=0.8, temperature=1.0, seed=5, no_repeat_ngram_size=1)
    free, *_ = engine.generate(a1, a2, ids, max_len=24, stop_id=0, ignore_stop=True, **kw)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    toks, lens, steps, _ = engine.generate(a1, a2, ids, max_len=24, stop_id=stop, **kw)
    reps = engine.last_row_repacks()
    print(f"[{engine.precision}] B = 40, stop id {stop}: steps {steps}, {reps} repacks, rows stopped early {int((lens < steps).sum())}")
    assert reps >= 1, "no row repack happened: pick a stop id that stops more rows"
    for r in range(40):
        row = toks[r][toks[r] >= 0]
        assert len(set(row.tolist())) == row.size, (r, row)


# ---- 6. refusals through the raw ABI ----------------------------------------------------------------------------------------------------
def _arm_raw(e, **f):
    r = E.LogitRules(size=C.sizeof(E.LogitRules), repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, logit_bias=None)
    for k, v in f.items():
        setattr(r, k, v)
    rc = e.lib.mellow_generate_rules(e.h, C.byref(r))
    return rc, e.lib.mellow_last_error().decode()


def test_refusals_through_the_raw_abi(engine):
    for f, word in ((dict(size=8), "size"), (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                    (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                    (dict(min_new_tokens=-2), "min_new_tokens")):
        rc, msg = _arm_raw(engine, **f)
        assert rc != 0 and word in msg, (f, msg)
    b = synth.make_batch(3)
    plain, *_ = engine.generate(*b, max_len=12, stop_id=-1)
    ruled, *_ = engine.generate(*b, max_len=12, stop_id=-1, logit_bias=np.where(np.isin(np.arange(V), plain[:, 0]), NEG, 0).astype(np.float32))
    assert not np.array_equal(ruled, plain)
    # armed, then consumed by a call that fails in its argument check: the next call runs without rules
    sup = np.where(np.isin(np.arange(V), plain[:, 0]), NEG, 0).astype(np.float32)
    rc, msg = _arm_raw(engine, logit_bias=sup.ctypes.data)
    assert rc == 0, msg
    rc = engine.lib.mellow_generate(engine.h, None, None, 0, None, 0, 0, 0.8, 1.0, -1, 0, None, None, None, None)
    assert rc != 0
    after, *_ = engine.generate(*b, max_len=12, stop_id=-1)
    assert np.array_equal(after, plain)
    # NULL disarms
    assert _arm_raw(engine, no_repeat_ngram_size=1)[0] == 0
    assert engine.lib.mellow_generate_rules(engine.h, None) == 0
    assert np.array_equal(engine.generate(*b, max_len=12, stop_id=-1)[0], plain)


# ---- 7. fp8 ------------------------------------------------------------------------------------------------------------------------------
def test_fp8_greedy_obeys_the_exact_properties(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        _properties(e8, ["greedy"], "fp8")
    finally:
        e8.close()
