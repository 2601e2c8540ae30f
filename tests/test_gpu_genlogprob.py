"""GPU (-m gpu): log-probs of the generated tokens, formed inside the decode step (include/mellow_hip.h mellow_generate_scored;
Engine.generate(return_logprobs=True), Engine.debug_dec_head_lse).

Bounds.  lse of the head tap against an fp64 logsumexp of the logits the same launch stored: 1e-4, the bound tests/test_gpu_score.py
holds the scoring head to (a tiled fp32 sum of 49152 terms in (0, 1]; here 32-wide tiles and chains of at most 16 + 6 + 8 additions).
A token's log-prob against the reference (tests/golden/score.npz): 6e-3 = test_gpu_score.py's TOL (3e-3 on the logit + 3e-3 for the
1-Lipschitz log-sum-exp).  Against Engine.score of the same tokens: both routes are within 6e-3 of the reference, so 1.2e-2.
Every test prints its measured maximum; DESIGN.md section 6h records them.

The tap runs the exact-fp32 / e4m3 head kernel on caller rows (the twin of debug_dec_head); the streaming f32x3 head of the
default mode is reached through generate(): one row block at B = 2 / 3, two with the per-block exit and row migration at B = 40."""
import math
import os

import numpy as np
import pytest
import torch

from mellow_amd import spec, synth

pytestmark = pytest.mark.gpu

TOL = 6e-3
V = 49152


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    from mellow_amd.engine import Engine
    e = Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch3():
    return synth.make_batch(3)


def _rows(B, synth_sd, seed):
    """seeded randn rows at a few scales; the last row all zero, row 0 proportional to a head weight row (a peaked distribution:
    its top logit is 30, every other one c * <w_j, w_k>)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 576), generator=g) * torch.tensor([0.25, 1.0, 4.0])[torch.arange(B) % 3, None]
    w = synth_sd[spec.LM + "lm_head.weight"][1234].float()
    kinds = ["randn"] * B
    if B >= 3:
        x[0] = w * (30.0 / float(w @ w))
        x[B - 1] = 0.0
        kinds[0], kinds[B - 1] = "peaked", "zero"
    return x, kinds


def _check_tap(engine, x, kinds, act_fp8=False):
    out = engine.debug_dec_head_lse(x, act_fp8=act_fp8)
    again = engine.debug_dec_head_lse(x, act_fp8=act_fp8)
    plain = engine.debug_dec_head(x, act_fp8=act_fp8)
    for k in out:
        assert torch.equal(out[k], again[k]), k                                     # two identical calls: identical bytes
    assert torch.equal(out["logits"], plain)                                        # the non-LSE kernel's logits, bit for bit
    assert torch.equal(out["max"], out["logits"].max(-1).values)
    assert torch.equal(out["argmax"], engine.argmax(out["logits"]))
    lse64 = torch.logsumexp(out["logits"].double(), -1)
    d = (out["lse"].double() - lse64).abs()
    assert torch.isfinite(out["lse"]).all()
    for i, kind in enumerate(kinds):
        if kind == "zero":
            dz = abs(float(out["lse"][i]) - math.log(V))
            print(f"  zero row: |lse - log(49152)| = {dz:.3e}")
            assert float(out["max"][i]) == 0.0 and dz <= 1e-6
        if kind == "peaked":
            assert float(out["max"][i]) > 25.0
    return float(d.max())


# 1: one live row of a block; 33: two row blocks; 97: three blocks and a partial one; 161: six blocks
@pytest.mark.parametrize("B", [1, 33, 97, 161])
def test_head_tap(engine, synth_sd, B):
    if B == 1:
        x3, kinds = _rows(3, synth_sd, 1)
        d = max(_check_tap(engine, x3[i: i + 1], kinds[i: i + 1]) for i in (0, 1, 2))       # peaked, randn and zero, one row each
    else:
        x, kinds = _rows(B, synth_sd, B)
        d = _check_tap(engine, x, kinds)
    print(f"[{engine.precision}] B = {B}: tap lse vs fp64 logsumexp of its logits, max|d| {d:.3e}")
    assert d <= 1e-4


def test_head_tap_fp8(synth_sd):
    from mellow_amd.engine import Engine
    e8 = Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        x, kinds = _rows(33, synth_sd, 8)
        kinds[0] = "randn"                # (an e4m3 head need not keep the peak exactly where the fp32 one has it)
        for act in (False, True):
            d = _check_tap(e8, x, kinds, act_fp8=act)
            print(f"[fp8, act_fp8={act}] tap lse vs fp64 logsumexp of its own logits, max|d| {d:.3e}")
            assert d <= 1e-4
    finally:
        e8.close()


def test_generate_matches_the_reference(engine, golden_dir):
    gen = np.load(os.path.join(golden_dir, "gen.npz"))
    sc = np.load(os.path.join(golden_dir, "score.npz"))
    a1, a2, ids = synth.make_batch(2)
    assert np.array_equal(ids, sc["input_ids"]) and np.array_equal(sc["cand_ids"][:, 0], gen["tokens"][:, :12])
    toks, lens, steps, _, lp = engine.generate(a1, a2, ids, max_len=12, stop_id=-1, return_logprobs=True)
    assert steps == 12 and lp.shape == (2, 12) and lp.dtype == np.float32
    assert np.array_equal(toks, gen["tokens"][:, :12])
    d = np.abs(lp.astype(np.float64) - sc["logprob"][:, 0])
    l0 = torch.log_softmax(torch.from_numpy(gen["logits_step0"]).double(), -1).numpy()
    d0 = np.abs(lp[:, 0].astype(np.float64) - l0[np.arange(2), toks[:, 0]])
    print(f"[{engine.precision}] generated log-probs vs the reference: max|d| {d.max():.3e}; step 0 vs its fp64 log-softmax {d0.max():.3e}")
    assert d.max() <= TOL
    assert d0.max() <= TOL


@pytest.mark.parametrize("sampled", [False, True])
def test_generate_matches_score(engine, batch3, sampled):
    """the recorded number is the raw model log-softmax of the token, greedy or drawn at top_p 0.9 / temperature 0.7: what score()
    returns for the same tokens (both within 6e-3 of the reference: 1.2e-2)"""
    a1, a2, ids = batch3
    kw = dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7) if sampled else {}
    toks, _, steps, _, lp = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, return_logprobs=True, **kw)
    assert toks.shape == (3, 16) and lp.shape == (3, 16)
    ref, _, am = engine.score(a1, a2, ids, toks[:, None, :], np.full((3, 1), 16))
    d = np.abs(lp.astype(np.float64) - ref[:, 0]).max()
    print(f"[{engine.precision}] {'sampled' if sampled else 'greedy'}: log-probs vs score() of the same tokens, max|d| {d:.3e}; "
          f"tokens off the arg-max: {int((am[:, 0] != toks).sum())} of 48")
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert d <= 2 * TOL
    if not sampled:
        assert np.array_equal(am[:, 0], toks)


# the streaming f32x3 head serves 1, 2 or 4 row blocks per pass: 97 rows = one pass of four with a partial group, 161 rows = six
# blocks, a second pass (in the f32 engine: the fp32 head at several row blocks inside generate)
@pytest.mark.parametrize("B", [97, 161])
def test_generate_matches_score_at_many_row_blocks(engine, B):
    a1, a2, ids = synth.make_batch(B)
    toks, _, steps, _, lp = engine.generate(a1, a2, ids, max_len=3, stop_id=-1, return_logprobs=True)
    base, *_ = engine.generate(a1, a2, ids, max_len=3, stop_id=-1)
    ref, _, am = engine.score(a1, a2, ids, toks[:, None, :], np.full((B, 1), 3))
    d = np.abs(lp.astype(np.float64) - ref[:, 0]).max()
    print(f"[{engine.precision}] B = {B}: log-probs vs score() of the same tokens, max|d| {d:.3e}")
    assert np.array_equal(toks, base) and np.array_equal(am[:, 0], toks)
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert d <= 2 * TOL


def test_nothing_else_moved(engine, batch3):
    a1, a2, ids = batch3
    for kw in ({}, dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7)):
        base = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, **kw)
        with_lp = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, return_logprobs=True, **kw)
        after = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, **kw)        # the step graph of a call without, after one with
        again = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, return_logprobs=True, **kw)      # ... and the reverse
        assert len(base) == 4 and len(with_lp) == 5
        for r in (with_lp, after, again):
            assert np.array_equal(r[0], base[0]) and np.array_equal(r[1], base[1]) and r[2] == base[2]
        assert np.array_equal(with_lp[4], again[4])
        engine.set_graph(False)
        try:
            eager = engine.generate(a1, a2, ids, max_len=16, stop_id=-1, return_logprobs=True, **kw)
        finally:
            engine.set_graph(True)
        assert np.array_equal(eager[0], base[0])
        assert np.array_equal(eager[4].view(np.int32), with_lp[4].view(np.int32))       # graph replay == eager launches, bit for bit


def test_logprobs_follow_their_example_through_row_migration(engine, synth_sd):
    from mellow_amd.engine import Engine
    a1, a2, ids = synth.make_batch(40)
    kw = dict(do_sample=True, top_p=0.8, temperature=1.0, seed=5)
    free, *_ = engine.generate(a1, a2, ids, max_len=24, stop_id=0, ignore_stop=True, **kw)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    plain, lp0, n0, _ = engine.generate(a1, a2, ids, max_len=24, stop_id=stop, **kw)
    mig, lm, nm, _, lpm = engine.generate(a1, a2, ids, max_len=24, stop_id=stop, return_logprobs=True, **kw)
    reps = engine.last_row_repacks()
    other = Engine(device=0, precision=engine.precision, options={"row_migration": 0})
    other.load_state_dict(synth_sd)
    try:
        nomig, ln, nn, _, lpn = other.generate(a1, a2, ids, max_len=24, stop_id=stop, return_logprobs=True, **kw)
    finally:
        other.close()
    assert reps > 0, "no row repack happened: pick a stop id that stops more rows"
    assert nm == nn == n0 and np.array_equal(lm, ln) and np.array_equal(lm, lp0) and np.array_equal(mig, plain)
    worst = 0.0
    for r in range(40):
        n = lm[r] + 1 if lm[r] < nm else nm
        assert np.array_equal(mig[r, :n], nomig[r, :n]), r
        if engine.precision == "f32":
            assert np.array_equal(lpm[r, :n], lpn[r, :n]), r
        worst = max(worst, float(np.abs(lpm[r, :n] - lpn[r, :n]).max()))
    print(f"[{engine.precision}] {reps} repacks; log-probs with / without row migration: max|d| {worst:.3e}")
    assert worst <= 1e-3
    assert (mig == -1).any()                                           # a repack drops the rows that have stopped
    for t, lp in ((mig, lpm), (nomig, lpn)):
        assert np.all(lp[t == -1] == 0.0)                              # never computed: exactly 0.0
        assert np.isfinite(lp).all() and (lp[t >= 0] <= 0).all()


def test_three_pickers_share_the_step_bookkeeping(engine):
    """The arg-max, the sampler and the beam merge run the same step epilogue (token / log-prob record, stop count, block-exit countdown,
    publish, embedding gather).  B = 33 is two row blocks; the stop id is chosen as in the migration test above, so rows stop at
    different steps, a block empties and rows migrate.  A sampler at top_p = 0 keeps the arg-max alone, and one beam is the greedy
    search: the three calls must tell the same story.  The greedy log-prob is -log S, the sampler's and the beam's l[id] - lse:
    2e-4 is the bound test_gpu_beam.py holds the two forms to."""
    B, ML = 33, 12
    a1, a2, ids = synth.make_batch(B)
    free, *_ = engine.generate(a1, a2, ids, max_len=ML, stop_id=0, ignore_stop=True)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    gt, gl, gs, _, glp = engine.generate(a1, a2, ids, max_len=ML, stop_id=stop, return_logprobs=True)
    reps_g = engine.last_row_repacks()
    st, sl, ss, _, slp = engine.generate(a1, a2, ids, max_len=ML, stop_id=stop, return_logprobs=True, do_sample=True, top_p=0.0, seed=5)
    reps_s = engine.last_row_repacks()
    bt, bl, bs, _, blp, _ = engine.generate(a1, a2, ids, max_len=ML, stop_id=stop, return_logprobs=True, num_beams=1)
    d_s = float(np.abs(slp - glp).max())
    d_b = 0.0
    for r in range(B):
        n = min(int(gl[r]) + 1, gs)                      # up to and including the row's stop id: a finished beam is frozen after it
        assert np.array_equal(bt[r, :n], gt[r, :n]), r
        d_b = max(d_b, float(np.abs(blp[r, :n] - glp[r, :n]).max()))
    print(f"[{engine.precision}] stop id {stop}: steps {gs} / {ss} / {bs}, repacks {reps_g} / {reps_s}, rows dropped {int((gt == -1).any(1).sum())}; "
          f"max|lp - greedy lp|: sampled {d_s:.3e}, one beam {d_b:.3e}")
    assert reps_g >= 1 and reps_s >= 1, "no row repack happened: pick a stop id that stops more rows"
    assert np.array_equal(st, gt) and np.array_equal(sl, gl) and ss == gs        # (the -1 columns of dropped rows included)
    assert d_s <= 2e-4
    assert bs == gs and np.array_equal(bl, gl) and bt.shape == gt.shape
    assert d_b <= 2e-4


@pytest.mark.parametrize("engine", ["f32"], indirect=True)
def test_scored_batches_beyond_1024_rows_pad_every_record(engine, golden_dir):
    """A scored batch of more than 1024 rows runs as passes (tests/test_gpu_parity.py test_batches_beyond_1024_rows_run_as_passes has
    the construction: 1024 rows cycling over examples that stop at steps 8 / 17 / 3 / never, then six copies of the one that stops
    at step 3).  Every record of the one call -- tokens, lengths, log-probs, top ids, top log-probs -- equals the engine's own
    single-pass calls on the two parts bit for bit ("f32": the routes are bit-equal), and where the second pass stopped before the
    first the records are padded: -1 in the tokens and the top ids, exactly 0.0 in the log-probs and the top log-probs."""
    g = np.load(os.path.join(golden_dir, "eos_mixed.npz"))
    stop, L = int(g["stop_id"]), int(g["max_len"])
    ex = g["one_never_examples"].tolist()
    rows = [ex[i % 4] for i in range(1024)] + [ex[2]] * 6
    a1, a2, ids = synth.make_examples(ex)
    pick = [ex.index(r) for r in rows]
    a1, a2, ids = a1[pick], a2[pick], ids[pick]
    kw = dict(max_len=L, stop_id=stop, return_logprobs=True, top_logprobs=2)
    toks, lens, n, _, lp, tid, tlp = engine.generate(a1, a2, ids, **kw)
    assert toks.shape == lp.shape == (1030, L) and tid.shape == tlp.shape == (1030, L, 2) and n == L
    for sel in (slice(0, 1024), slice(1024, 1030)):
        t, ln, st, _, p, ti, tp = engine.generate(a1[sel], a2[sel], ids[sel], **kw)
        print(f"rows {sel.start}..{sel.stop}: {st} steps alone, {n} in the call of all rows")
        assert np.array_equal(toks[sel, :st], t) and np.array_equal(lens[sel], ln)
        assert np.array_equal(lp[sel, :st].view(np.int32), p.view(np.int32))
        assert np.array_equal(tid[sel, :st], ti) and np.array_equal(tlp[sel, :st].view(np.int32), tp.view(np.int32))
    assert st < 5 < L                                        # pass 1 stopped after step 3 (step 4 may still have been enqueued)
    assert (toks[1024:, 5:] == -1).all() and (tid[1024:, 5:] == -1).all()
    assert (lp[1024:, 5:] == 0.0).all() and (tlp[1024:, 5:] == 0.0).all()
