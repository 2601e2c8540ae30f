"""GPU (-m gpu): contrastive guidance inside the decode step (include/mellow_hip.h mellow_generate_guidance / mellow_guidance_apply;
Engine.generate(guidance_scale=, negative=); mellow_amd/csrc/guidance.hip).

Yardsticks: the fp64 definition of tests/guidance_ref.py for the tap, with the fp32 rounding bound of the formula; properties that hold
exactly whatever the rounding for the generation loop (the two rows of a pair are bit-equal); and Engine.forward (teacher forced, all
positions, no K/V cache) on the conditional and on the negative inputs for the decisions.  TOL = 6e-3 is the project's logit tolerance
(tests/test_gpu_nseq.py derives it); g = b + s * (a - b) carries the error of a with weight |s| and that of b with weight |s - 1|, and a
log-softmax value carries at most twice a logit's error, hence the factor 4 * (|s| + |s - 1|) (the step factor as in the rules test).
Every test prints what it measured."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import spec, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as GR  # noqa: E402

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


_DATA = {}


def _pairs2():
    """2 pairs: conditional rows = synthetic examples 0, 1; negative rows = the clips of examples 2, 3 under the prompts of 0, 1"""
    if "p2" not in _DATA:
        bc = synth.make_batch(2)
        n1, n2, _ = synth.make_examples([2, 3])
        _DATA["p2"] = (bc, (n1, n2, bc[2]))
    return _DATA["p2"]


def _pairs17():
    """17 pairs = 34 rows, past one 32-row block: examples 0 .. 16, each against its own clips swapped"""
    if "p17" not in _DATA:
        bc = synth.make_batch(17)
        _DATA["p17"] = (bc, (bc[1], bc[0], bc[2]))
    return _DATA["p17"]


def _real_logits(engine):
    """eight rows of prefill logits (computed once, by whichever engine asks first: they are test data here)"""
    if "l" not in _DATA:
        a1, a2, ids = synth.make_batch(8)
        _DATA["l"] = engine.lm_prefill(engine.prefix(a1, a2, ids), reserve=4).cpu().numpy()
    return _DATA["l"]


def _pair_equal(x):
    x = np.asarray(x)
    return x[0::2].tobytes() == x[1::2].tobytes()


# ---- 1. the tap against the definition ------------------------------------------------------------------------------------------
def _tap_rows(engine, P):
    rng = np.random.default_rng(1)
    if P == 1:
        return np.stack([rng.standard_normal(V).astype(np.float32) * 8.0, np.round(rng.standard_normal(V) * 2.0).astype(np.float32)])
    rows = []
    for _ in range(8):
        rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)              # peaked
        rows.append(rng.standard_normal(V).astype(np.float32) * 0.3)              # flat
        rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))    # heavy exact ties
    rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))
    rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))
    rows += list(_real_logits(engine))
    assert len(rows) == 34
    return np.stack(rows)


@pytest.mark.parametrize("scale", [0.0, 1.5, 3.0])
@pytest.mark.parametrize("P", [1, 17])
def test_tap_against_the_definition(engine, P, scale):
    rows = _tap_rows(engine, P)
    out = engine.guidance_apply(rows, scale)
    again = engine.guidance_apply(rows, scale)
    nosum = engine.guidance_apply(rows, scale, with_sum=False)
    g = out["logits"]
    want = GR.guide_rows(rows, scale)
    bound = GR.bound(rows, scale)
    err = np.abs(g[0::2].astype(np.float64) - want).max(axis=1)
    val, idx = GR.tile_partials(g)
    sums = GR.tile_sums64(g)
    rel = float(np.abs(out["cand_sum"] / sums - 1.0).max())
    M = out["cand_val"].astype(np.float64).max(axis=1, keepdims=True)
    lse = (M + np.log((out["cand_sum"].astype(np.float64) * np.exp(out["cand_val"].astype(np.float64) - M)).sum(axis=1, keepdims=True)))[:, 0]
    dl = float(np.abs(lse - GR.logsumexp64(g)).max())
    top2 = np.sort(g.reshape(2 * P, -1, 32), axis=2)[:, :, -2:]
    tied = int((top2[:, :, 0] == top2[:, :, 1]).sum())
    print(f"[{engine.precision}] tap P = {P}, s = {scale}: max |g - g_fp64| / bound over the pairs {float((err / bound).max()):.3f} "
          f"(largest |d| {float(err.max()):.3e}, its bound {float(bound[np.argmax(err)]):.3e}); cand_sum rel. error {rel:.3e}; "
          f"merged lse vs fp64 logsumexp of g {dl:.3e}; tiles with a tied maximum {tied}")
    assert g.shape == rows.shape and np.isfinite(g).all()
    assert _pair_equal(g), "(a) the two stored rows of a pair differ"
    assert (err <= bound).all(), "(b)"
    assert out["cand_val"].tobytes() == val.tobytes() and np.array_equal(out["cand_idx"], idx), "(c)"
    assert _pair_equal(out["cand_val"]) and _pair_equal(out["cand_idx"]) and _pair_equal(out["cand_sum"])
    assert rel <= 1e-4 and dl <= 1e-4, "(d)"
    assert "cand_sum" not in nosum and all(nosum[k].tobytes() == out[k].tobytes() for k in nosum), "(e)"
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)


# ---- 2. greedy decisions against the teacher-forced forward --------------------------------------------------------------------------
def test_greedy_decisions_against_the_teacher_forced_forward(engine):
    """B = 2 pairs, max_len 8, stop id -1, s = 3.0: 16 decisions.  Conditional rows: synthetic examples 0, 1; negative rows: the clips of
    examples 2, 3 under the prompts of 0, 1.  The batch was chosen without a GPU: the fp32 oracle (oracle/mellow_oracle.py on the same
    checkpoint, a guided greedy loop with tests/guidance_ref.py on its logits) puts the margin between the best and the second guided
    value, for (step 0, example 0), (step 0, example 1), (step 1, example 0) ..., at
        3.2776 1.4663 | 4.8520 7.6795 | 2.3816 2.6072 | 7.3230 4.6961 | 6.1087 19.0723 | 1.5219 15.2741 | 14.6363 7.9934 | 8.2718 6.6066
    against the band 4 * TOL * (step + 1) * (|s| + |s - 1|) = 0.12 * (step + 1) under which a decision may be skipped: none is below it
    (the closest, step 5 of example 0, is 2.1 times the band), and the oracle's guided answer differs from its plain greedy answer at 11
    of the 16 positions: an implementation that ignores the negative fails.  (The count printed below is another one: the guided
    reference token against the arg-max of the conditional row on the GUIDED history, 9 of 16 when this was written.)"""
    B, ML, s = 2, 8, 3.0
    w = abs(s) + abs(s - 1)
    bc, bn = _pairs2()
    toks, lens, steps, _, lp = engine.generate(*bc, max_len=ML, stop_id=-1, return_logprobs=True, guidance_scale=s, negative=bn)
    assert toks.shape == (B, ML) and lp.shape == (B, ML)
    skipped, dmax, differ = 0, 0.0, 0
    for st in range(ML):
        ans = np.concatenate([toks[:, :st], np.zeros((B, 1), dtype=toks.dtype)], axis=1).astype(np.int64)      # (a dummy last token)
        lc = engine.forward(*bc, ans, from_pos=T - 1 + st)[:, 0].cpu().numpy()
        lu = engine.forward(*bn, ans, from_pos=T - 1 + st)[:, 0].cpu().numpy()
        g = GR.guide(lc, lu, s)
        ls = GR.log_softmax64(g)
        for r in range(B):
            o = np.sort(g[r])[::-1]
            margin, band = float(o[0] - o[1]), 4 * TOL * (st + 1) * w
            want = GR.first_argmax(g[r])
            differ += want != GR.first_argmax(lc[r])
            print(f"[{engine.precision}] step {st} example {r}: reference margin {margin:.4f} (band {band:.3f}), chosen == reference: {int(toks[r, st]) == want}")
            if margin < band:
                skipped += 1
            else:
                assert int(toks[r, st]) == want, (st, r, int(toks[r, st]), want)
            dmax = max(dmax, abs(float(lp[r, st]) - float(ls[r, toks[r, st]])))
    print(f"[{engine.precision}] guided greedy, s = {s}: decisions skipped {skipped} of {B * ML}; guided reference token != plain arg-max at {differ} of "
          f"{B * ML}; max|lp - log-softmax of the guided forward| {dmax:.3e} (bound {4 * TOL * w:.2e})")
    assert skipped <= 1
    assert dmax <= 4 * TOL * w


# ---- 3. exact properties ----------------------------------------------------------------------------------------------------------------
PROPS = {"greedy": {}, "sampled": dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7), "logprobs": dict(return_logprobs=True),
         "ngram2": dict(no_repeat_ngram_size=2)}


def _pair_rows_equal(engine, label, name, bc, bn, **kw):
    res = engine.generate(*bc, guidance_scale=3.0, negative=bn, keep_negative_rows=True, **kw)
    toks, lens = res[0], res[1]
    P = bc[0].shape[0]
    assert toks.shape[0] == 2 * P and lens.shape == (2 * P,)
    assert _pair_equal(toks) and _pair_equal(lens), (name, toks)
    if kw.get("return_logprobs"):
        assert res[4].shape == toks.shape and _pair_equal(res[4]), name
    half = engine.generate(*bc, guidance_scale=3.0, negative=bn, **kw)
    assert np.array_equal(half[0], toks[0::2]) and np.array_equal(half[1], lens[0::2])          # the conditional rows are what is returned
    print(f"[{label}] {name}: rows 2i + 1 bit-equal to rows 2i over {P} pairs, {res[2]} steps")
    return res


@pytest.mark.parametrize("mode", list(PROPS))
def test_both_rows_of_a_pair_are_bit_equal(engine, mode):
    bc, bn = _pairs2()
    res = _pair_rows_equal(engine, engine.precision, mode, bc, bn, max_len=8, stop_id=-1, **PROPS[mode])
    if mode == "ngram2":
        for r in range(4):
            bigrams = list(zip(res[0][r, :-1].tolist(), res[0][r, 1:].tolist()))
            assert len(set(bigrams)) == 7, (r, res[0][r])


def test_pairs_stay_equal_across_row_blocks_with_block_exit(engine):
    """17 pairs = 34 rows: pair 16 is alone in the second row block.  The stop id is a token that pair produces early in the free run,
    so its block exits while the first one goes on."""
    bc, bn = _pairs17()
    free, *_ = engine.generate(*bc, max_len=6, stop_id=-1, guidance_scale=3.0, negative=bn, keep_negative_rows=True)
    assert free.shape == (34, 6) and _pair_equal(free)
    stop, at = None, None
    for j in range(0, 4):
        cand = int(free[32, j])
        if (~(free[:32, : j + 1] == cand).any(axis=1)).any():       # some row of block 0 has not produced it by then
            stop, at = cand, j
            break
    assert stop is not None, "pair 16 offers no early token the first block has not also produced"
    toks, lens, steps, _ = _pair_rows_equal(engine, engine.precision, "17 pairs, real stop id", bc, bn, max_len=6, stop_id=stop)
    print(f"[{engine.precision}] stop id {stop} (pair 16 produces it at step {at}): steps {steps}, lengths of pair 16 {lens[32:].tolist()}, "
          f"rows stopped before the last step {int((lens < steps).sum())}")
    assert lens[32] == at and steps > at + 1
    assert (toks[32:, at + 2:] == -1).all(), "the second row block went on after both of its rows had stopped"
    assert np.array_equal(toks[:32, : at + 1], free[:32, : at + 1])


def test_fp8_pairs_are_bit_equal(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        bc, bn = _pairs2()
        _pair_rows_equal(e8, "fp8", "greedy", bc, bn, max_len=8, stop_id=-1)
    finally:
        e8.close()


# ---- 4. the random stream goes by pair ---------------------------------------------------------------------------------------------------
def test_random_stream_by_pair(synth_sd):
    """precision "f32" (a row's arithmetic does not depend on the batch it is in): pairs [0, 1, 2] sampled in one call are bit-equal to
    three single-pair calls with row_offset 0, 1, 2"""
    e = E.Engine(device=0, precision="f32")
    e.load_state_dict(synth_sd)
    try:
        bc = synth.make_batch(3)
        bn = (bc[1], bc[0], bc[2])
        kw = dict(max_len=8, stop_id=-1, do_sample=True, seed=7, top_p=0.9, temperature=0.7, guidance_scale=3.0, keep_negative_rows=True)
        whole, *_ = e.generate(*bc, negative=bn, **kw)
        greedy, *_ = e.generate(*bc, negative=bn, max_len=8, stop_id=-1, guidance_scale=3.0, keep_negative_rows=True)
        assert whole.shape == (6, 8) and _pair_equal(whole)
        for i in range(3):
            one, *_ = e.generate(*(x[i:i + 1] for x in bc), negative=tuple(x[i:i + 1] for x in bn), row_offset=i, **kw)
            assert np.array_equal(one, whole[2 * i:2 * i + 2]), (i, one, whole[2 * i:2 * i + 2])
        other, *_ = e.generate(*(x[1:2] for x in bc), negative=tuple(x[1:2] for x in bn), row_offset=0, **kw)
        print(f"[f32] pairs 0 .. 2 in one call == three calls with row_offset 0, 1, 2; sampled != greedy in {int((whole != greedy).sum())} of 48 "
              f"tokens; pair 1 at row_offset 0 differs from pair 1 at row_offset 1 in {int((other != whole[2:4]).sum())} of 16 tokens")
        assert not np.array_equal(whole, greedy), "the sampled call gave the greedy tokens: the test does not see the stream"
    finally:
        e.close()


# ---- 5. nothing changes when nothing is armed -------------------------------------------------------------------------------------------
def test_scale_one_is_the_plain_call_and_the_armed_state_is_consumed(engine):
    bc, bn = _pairs2()
    pt, pl, ps, _ = engine.generate(*bc, max_len=8, stop_id=-1)
    ot, ol, os_, _ = engine.generate(*bc, max_len=8, stop_id=-1, guidance_scale=1.0, negative=bn)
    assert ot.tobytes() == pt.tobytes() and np.array_equal(ol, pl) and os_ == ps
    gt, *_ = engine.generate(*bc, max_len=8, stop_id=-1, guidance_scale=3.0, negative=bn)
    at, al, as_, _ = engine.generate(*bc, max_len=8, stop_id=-1)
    print(f"[{engine.precision}] scale 1 == plain; guided differs from plain in {int((gt != pt).sum())} of {pt.size} tokens; plain after guided == plain")
    assert not np.array_equal(gt, pt)
    assert at.tobytes() == pt.tobytes() and np.array_equal(al, pl) and as_ == ps
    # a sampled plain call after a guided one draws from the stream of the ROW again
    kw = dict(max_len=8, stop_id=-1, do_sample=True, seed=7, top_p=0.9, temperature=0.7)
    s0, *_ = engine.generate(*bc, **kw)
    engine.generate(*bc, guidance_scale=3.0, negative=bn, **kw)
    s1, *_ = engine.generate(*bc, **kw)
    assert s1.tobytes() == s0.tobytes()


# ---- 6. refusals through the raw ABI ----------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi(engine):
    lib, h = engine.lib, engine.h
    bc, _ = _pairs2()
    plain, *_ = engine.generate(*bc, max_len=4, stop_id=-1)
    a1, a2 = engine._f32(np.repeat(bc[0], 2, axis=0)[:3]), engine._f32(np.repeat(bc[1], 2, axis=0)[:3])
    ids = engine._i32(np.repeat(bc[2], 6, axis=0))                     # enough for [3] and for [3][2] prompts
    ns, ML = int(a1.shape[1]), 4
    out = torch.zeros((64, ML), dtype=torch.int32, device=engine.tdev)
    lp = torch.zeros((64, ML), dtype=torch.float32, device=engine.tdev)
    par, cum = np.zeros((ML, 8), dtype=np.int32), np.zeros(8, dtype=np.float32)
    btok, blp = np.zeros((ML, 8), dtype=np.int32), np.zeros((ML, 8), dtype=np.float32)
    lens, steps, ftm = (C.c_int32 * 64)(), C.c_int32(0), C.c_float(0.0)
    p, vp = E._ptr, C.c_void_p
    engine._sync_inputs()

    def arm():
        assert lib.mellow_generate_guidance(h, 2.0) == 0, lib.mellow_last_error().decode()

    def still_plain(what):
        after, *_ = engine.generate(*bc, max_len=ML, stop_id=-1)
        assert after.tobytes() == plain.tobytes(), what

    for bad in (float("nan"), float("inf")):
        assert lib.mellow_generate_guidance(h, bad) != 0 and "finite" in lib.mellow_last_error().decode()
    arm()
    assert lib.mellow_generate(h, p(a1), p(a2), ns, p(ids), 3, ML, 0.8, 1.0, -1, 0, p(out), lens, C.byref(steps), C.byref(ftm)) != 0
    msg = lib.mellow_last_error().decode()
    assert "guidance" in msg and "even" in msg, msg
    still_plain("odd B")
    arm()
    assert lib.mellow_generate_n(h, p(a1), p(a2), ns, p(ids), 2, 2, ML, 1, 0.9, 1.0, 7, 0, -1, 0, p(out), p(lp), lens, C.byref(steps), C.byref(ftm)) != 0
    msg = lib.mellow_last_error().decode()
    assert "guidance" in msg and "mellow_generate_n" in msg, msg
    still_plain("mellow_generate_n")
    arm()
    assert lib.mellow_generate_q(h, p(a1), p(a2), ns, p(ids), 2, 2, ML, 0, 0.9, 1.0, 0, 0, -1, 0, p(out), p(lp), lens, C.byref(steps), C.byref(ftm)) != 0
    msg = lib.mellow_last_error().decode()
    assert "guidance" in msg and "mellow_generate_q" in msg, msg
    still_plain("mellow_generate_q")
    arm()
    assert lib.mellow_generate_beam(h, p(a1), p(a2), ns, p(ids), 2, 2, ML, -1, 0, vp(par.ctypes.data), vp(btok.ctypes.data), vp(blp.ctypes.data),
                                    vp(cum.ctypes.data), C.byref(steps), C.byref(ftm)) != 0
    msg = lib.mellow_last_error().decode()
    assert "guidance" in msg and "mellow_generate_beam" in msg, msg
    still_plain("mellow_generate_beam")
    # scale 1 arms nothing, and disarms
    arm()
    assert lib.mellow_generate_guidance(h, 1.0) == 0
    assert lib.mellow_generate(h, p(a1), p(a2), ns, p(ids), 3, ML, 0.8, 1.0, -1, 0, p(out), lens, C.byref(steps), C.byref(ftm)) == 0      # odd B: un-guided
    still_plain("scale 1")
