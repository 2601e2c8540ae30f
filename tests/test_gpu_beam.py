"""GPU (-m gpu): beam search inside the decode step (include/mellow_hip.h mellow_generate_beam / mellow_beam_select;
Engine.generate(num_beams=k); mellow_amd/csrc/beam.hip).

Yardsticks: the fp64 definition of tests/beam_ref.py for the selection, and existing code for the search -- Engine.forward (teacher
forced, all positions, no K/V cache) and Engine.score.  TOL = 6e-3 is the bound tests/test_gpu_nseq.py derives for a log-prob of
the decode step against the reference; two routes that are each within TOL of it differ by at most 2 * TOL.  A wrong or missing K/V
move shifts a log-prob by order 1.  Every test prints what it measured (DESIGN.md section 6k is where the figures belong)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402

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


def _rep(batch, n):
    return tuple(np.repeat(x, n, axis=0) for x in batch)


# ---- 1. the select tap against the fp64 definition ----------------------------------------------------------------------------
def select_case(B, k, scale, seed=0):
    """N = B * k rows of randn * scale logits with, in example 0: row 0 holding its maximum twice (token order), row 1 finished,
    row 2 with cum = -inf; and two bit-identical rows with equal cum (parent order) in example 1 (example 0 when B = 1)."""
    g = np.random.default_rng(seed)
    N = B * k
    logits = (g.standard_normal((N, V)) * scale).astype(np.float32)
    cum = (-g.uniform(0.0, 3.0, N)).astype(np.float32)
    fin = np.zeros(N, dtype=np.int32)
    stop_id = 11
    cum[0] = np.float32(-0.125)
    top = int(logits[0].argmax())
    logits[0, (top + 977) % V] = logits[0, top]
    fin[1] = 1
    cum[1] = np.float32(-0.25) - np.float32(np.log(V) * (0.1 if scale > 1 else 0.8))
    cum[2] = -np.inf
    a = k if B > 1 else 3
    logits[a + 1] = logits[a]
    cum[a] = cum[a + 1] = np.float32(-0.5)
    return logits, cum, fin, stop_id


_SELECT_REF = {}


def _select_ref(B, k, scale):
    if (B, k, scale) not in _SELECT_REF:
        lg, cum, fin, stop = select_case(B, k, scale)
        _SELECT_REF[(B, k, scale)] = (lg, cum, fin, stop) + R.select_step(lg, cum, fin, k, stop)
    return _SELECT_REF[(B, k, scale)]


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("B,k", [(2, 3), (1, 8), (5, 7)])
def test_select_tap_against_the_definition(engine, B, k, scale):
    """(parent, token) exact, cum / lp within 2e-4: the 1e-4 lse bound of DESIGN.md 6g plus the fp32 rounding of the sum.  The
    seed (0 for every case, chosen without a GPU) leaves the smallest gap between consecutive distinct candidate values among each
    example's best k + 1 at 1.29e-3 or more, five times the tolerance: fp32 arithmetic cannot reorder them."""
    lg, cum, fin, stop, parent, token, rcum, rlp, gaps = _select_ref(B, k, scale)
    assert min(gaps) >= 1e-3, gaps
    out = engine.beam_select(lg, cum, fin, k, stop)
    dc = float(np.abs(out["cum"].astype(np.float64) - rcum).max())
    dl = float(np.abs(out["lp"].astype(np.float64) - rlp).max())
    print(f"[{engine.precision}] select B = {B}, k = {k}, randn x {scale}: smallest reference gap {min(gaps):.3e}; max|cum - ref| {dc:.3e}, "
          f"max|lp - ref| {dl:.3e}; finished row chosen: {bool(((parent[:k] == 1) & (token[:k] == stop)).any())}")
    assert np.array_equal(out["parent"], parent) and np.array_equal(out["token"], token)
    assert dc <= 2e-4 and dl <= 2e-4
    again = engine.beam_select(lg, cum, fin, k, stop)
    assert all(out[n].tobytes() == again[n].tobytes() for n in out)


# ---- 2. one beam is the greedy call --------------------------------------------------------------------------------------------
def test_one_beam_equals_the_greedy_call(engine):
    b = synth.make_batch(3)
    gt, gl, gs, _, glp = engine.generate(*b, max_len=8, return_logprobs=True)
    toks, lens, steps, _, lp, score = engine.generate(*b, max_len=8, num_beams=1, return_logprobs=True)
    d = 0.0
    for r in range(3):
        n = min(int(gl[r]) + 1, gs)                      # up to and including the row's stop id: a finished beam is frozen after it
        assert np.array_equal(toks[r, :n], gt[r, :n])
        d = max(d, float(np.abs(lp[r, :n] - glp[r, :n]).max()))
    print(f"[{engine.precision}] num_beams = 1 vs greedy: steps {steps} ({gs}), lengths {lens.tolist()} ({gl.tolist()}), max|lp - greedy lp| {d:.3e}")
    assert steps == gs and np.array_equal(lens, gl) and toks.shape == gt.shape
    if (gl == gs).all():
        assert np.array_equal(toks, gt)
    assert d <= 2e-4
    plain = engine.generate(*b, max_len=8, num_beams=1)
    assert len(plain) == 4 and np.array_equal(plain[0], toks)


# ---- 3. the search against an independent forward -----------------------------------------------------------------------------
def test_search_against_the_teacher_forced_forward(engine):
    """B = 2 (synthetic examples 6 and 7), k = 3, max_len 6, stop id -1: 12 decisions.  The batch was chosen without a GPU: the
    fp32 oracle (oracle/mellow_oracle.py on the same checkpoint, the search of tests/beam_ref.py in fp64 on its logits) puts the
    margin between the k-th and the (k + 1)-th candidate, for (step 0, example 0), (step 0, example 1), (step 1, example 0) ..., at
        0.1954 1.6140 | 1.3455 3.1974 | 0.2897 2.2998 | 0.5235 0.4963 | 0.2054 0.8031 | 0.2765 1.3810
    against the band 4 * TOL * (s + 1) = 0.024, 0.048, 0.072, 0.096, 0.120, 0.144 under which a decision may be skipped: none is
    below it (the closest, step 4 of example 0, is 1.7 times the band), and the oracle's search moves rows at steps 1, 2, 3 and 5
    (parents [0, 1, 1 | 0, 1, 2] at step 1).  Examples 0 and 1 have one margin below the band (0.0491 at step 4), examples 4
    and 5 two."""
    B, k, ML = 2, 3, 6
    N = B * k
    b = synth.make_batch(B, first=6)
    engine.generate(*b, max_len=ML, stop_id=-1, num_beams=k)
    tab = engine.last_beam
    par, tok, lp = tab["parent"], tab["token"], tab["lp"]
    assert par.shape == (ML, N) and tok.shape == (ML, N)
    rb = _rep(b, k)
    seqs = [[] for _ in range(N)]
    ref_cum = np.where(np.arange(N) % k == 0, 0.0, -np.inf)
    dmax, skipped, moved = 0.0, 0, 0
    for s in range(ML):
        ans = np.array([q + [0] for q in seqs], dtype=np.int64)            # (a dummy last token: its own logits are not read)
        lg = engine.forward(*rb, ans, from_pos=T - 1 + s)[:, 0].double().cpu().numpy()
        ls = R.log_softmax64(lg)
        prow = np.arange(N) // k * k + par[s]
        want_lp = ls[prow, tok[s]]
        if s == 0:
            assert (par[0] == 0).all()
        dmax = max(dmax, float(np.abs(lp[s] - want_lp).max()))
        cands = R.candidates(lg, ref_cum, np.zeros(N, dtype=np.int64), k, -1)
        for e in range(B):
            c = cands[e]
            margin = float(c[k - 1, 0] - c[k, 0])
            band = 4 * TOL * (s + 1)
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
    d_cum = float(np.abs(tab["cum"] - ref_cum).max())
    print(f"[{engine.precision}] search B = 2, k = 3: max|lp - forward| {dmax:.3e} (bound {2 * TOL:.1e}); |cum - reference cum| {d_cum:.3e}; "
          f"decisions skipped {skipped} of {B * ML}; (step, row) pairs whose parent is another row: {moved}")
    assert dmax <= 2 * TOL
    assert skipped <= 2
    assert moved >= 1, "every row kept its own page at every step: the reorder was not exercised"


# ---- 4. across a row block ------------------------------------------------------------------------------------------------------
def test_across_a_row_block_against_score(engine):
    """33 rows: example 10's beams are rows 30, 31 (block 0) and 32 (block 1)"""
    b = synth.make_batch(11)
    toks, lens, steps, _, lp, score = engine.generate(*b, max_len=8, stop_id=-1, num_beams=3, num_return_sequences=3, return_logprobs=True)
    assert toks.shape == (33, 8) and lp.shape == (33, 8) and steps == 8 and score.shape == (33,)
    ref, sums, _ = engine.score(*b, toks.reshape(11, 3, 8), np.full((11, 3), 8))
    logprob = engine.last_beam["logprob"]
    d_tok = float(np.abs(lp.astype(np.float64) - ref.reshape(33, 8)).max())
    d_sum = float(np.abs(logprob - sums.reshape(33).astype(np.float64)).max())
    print(f"[{engine.precision}] B = 11, k = 3: token log-probs vs score(): max|d| {d_tok:.3e} (bound {2 * TOL:.1e}); hypothesis logprob vs score(): "
          f"max|d| {d_sum:.3e} (bound {8 * 2 * TOL:.2e})")
    assert d_tok <= 2 * TOL and d_sum <= 8 * 2 * TOL
    assert np.allclose(score, logprob / 8.0)
    for e in range(11):
        rows = toks[3 * e:3 * e + 3]
        assert len({tuple(r.tolist()) for r in rows}) == 3
        sc = score[3 * e:3 * e + 3]
        assert sc[0] >= sc[1] >= sc[2]


# ---- 5. the stop rule --------------------------------------------------------------------------------------------------------------
def test_stop_rule(engine):
    """One example, two beams.  The stop id is a frequent early token of the free-running search, as in tests/test_gpu_nseq.py; a
    beam call ends early only when EVERY beam has taken the stop id, which on the synthetic checkpoint few tokens achieve, so the
    early tokens are tried in the order (frequency descending, id ascending) and the first whose call ends before max_len is the
    one tested (none: the test fails)."""
    B, k, ML = 1, 2, 24
    b = synth.make_batch(B)
    engine.generate(*b, max_len=ML, stop_id=0, ignore_stop=True, num_beams=k)
    free = engine.last_beam["token"]
    assert free.shape == (ML, B * k)
    vals, counts = np.unique(free[1:6], return_counts=True)
    steps = ML
    for stop in [int(v) for v in vals[np.argsort(-counts, kind="stable")]]:
        toks, lens, steps, _, lp, score = engine.generate(*b, max_len=ML, stop_id=stop, num_beams=k, num_return_sequences=k, return_logprobs=True)
        if steps < ML:
            break
    enq = engine.last_steps_enqueued()
    tab = engine.last_beam
    print(f"[{engine.precision}] B = {B}, k = {k}, stop id {stop}: steps {steps} of {ML}, enqueued {enq}, lengths {lens.tolist()}")
    assert steps < ML, "no early end: pick a stop id that every beam reaches"
    assert enq <= steps + 1
    assert toks.shape == (B * k, steps) and (tab["token"][steps - 1] == stop).all()
    at, alp = E.backtrack_beams(tab["parent"], tab["token"], tab["lp"], k)
    run = np.cumsum(alp, axis=1)
    for r in range(B * k):
        hit = np.nonzero(toks[r] == stop)[0]
        assert hit.size and lens[r] == hit[0]                       # the length is the first stop position
        assert (toks[r, hit[0]:] == stop).all() and (lp[r, hit[0] + 1:] == 0).all()
    for r in range(B * k):                                          # a finished hypothesis's logprob does not change after its stop id
        h = int(np.nonzero(at[r] == stop)[0][0])
        assert np.all(run[r, h:] == run[r, h]) and abs(run[r, h] - float(tab["cum"][r])) <= 1e-4


# ---- 6. graph reuse and determinism -----------------------------------------------------------------------------------------------
def test_graph_reuse_and_determinism(engine):
    b2, b6 = synth.make_batch(2), synth.make_batch(6)
    S = dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7)

    def beam():
        r = engine.generate(*b2, max_len=8, stop_id=-1, num_beams=3, num_return_sequences=3, return_logprobs=True)
        t = engine.last_beam
        return [r[0], r[1], r[4], t["parent"], t["token"], t["lp"], t["cum"]]

    calls = [beam,
             lambda: list(engine.generate(*b6, max_len=8, stop_id=-1)[:2]),
             lambda: list(engine.generate(*b2, max_len=8, stop_id=-1, num_return_sequences=3, **S)[:2]),
             beam]

    def same(r, w):
        assert len(r) == len(w) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(r, w))

    first = [c() for c in calls]
    same(first[3], first[0])
    try:
        for on in (True, False):
            engine.set_graph(on)
            for c, w in zip(calls, first):
                same(c(), w)
    finally:
        engine.set_graph(True)


# ---- 7. refusals through the raw ABI ------------------------------------------------------------------------------------------------
def _raw_call(e, b, B, k, max_len):
    a1, a2, ids = e._f32(b[0]), e._f32(b[1]), e._prompt_ids(b[2])
    n = 16
    par, tok = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lp, cum = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    steps, ftm = C.c_int32(0), C.c_float(0)
    e._sync_inputs()
    vp = C.c_void_p
    rc = e.lib.mellow_generate_beam(e.h, E._ptr(a1), E._ptr(a2), a1.shape[1], E._ptr(ids), B, k, max_len, -1, 0, vp(par.ctypes.data),
                                    vp(tok.ctypes.data), vp(lp.ctypes.data), vp(cum.ctypes.data), C.byref(steps), C.byref(ftm))
    return rc, e.lib.mellow_last_error().decode()


def test_refusals_through_the_raw_abi(engine, synth_sd):
    """host-side checks: nothing is launched, the small output arrays are never written"""
    b = synth.make_batch(1)
    rc, msg = _raw_call(engine, b, 1, 9, 2)
    assert rc != 0 and "1 to 8 beams" in msg
    rc, msg = _raw_call(engine, b, 1, 0, 2)
    assert rc != 0 and "1 to 8 beams" in msg
    rc, msg = _raw_call(engine, b, 205, 5, 2)
    assert rc != 0 and "1025" in msg and "1024" in msg
    rc, msg = _raw_call(engine, b, 1025, 1, 2)
    assert rc != 0 and "1024" in msg
    rc, msg = _raw_call(engine, b, 2, 2, 16385)
    assert rc != 0 and "65536" in msg and "65540" in msg
    if engine.precision == "f32x3":
        e8 = E.Engine(device=0, precision="fp8")
        e8.load_state_dict(synth_sd)
        try:
            rc, msg = _raw_call(e8, b, 1, 2, 2)
            assert rc != 0 and "not available in MELLOW_PRECISION_FP8" in msg and "mellow_generate_beam" in msg
        finally:
            e8.close()


# ---- 8. next to the greedy answer (printed, not asserted: beam search does not guarantee the inequality) -------------------------------
def test_best_hypothesis_next_to_the_greedy_answer(engine):
    b = synth.make_batch(8)
    gt, gl, gs, _, glp = engine.generate(*b, max_len=16, stop_id=-1, return_logprobs=True)
    toks, lens, steps, _, lp, score = engine.generate(*b, max_len=16, stop_id=-1, num_beams=4, length_penalty=0.0, return_logprobs=True)
    best = engine.last_beam["logprob"]
    greedy = glp.astype(np.float64).sum(axis=1)
    print(f"[{engine.precision}] B = 8, k = 4, max_len 16: mean logprob of the best hypothesis {best.mean():.4f}, of the greedy answer {greedy.mean():.4f}; "
          f"examples where the beam's is higher {int((best > greedy).sum())}, equal tokens {int((toks == gt).all(1).sum())} of 8")
    assert toks.shape == (8, 16) and np.isfinite(best).all() and np.allclose(score, best)
