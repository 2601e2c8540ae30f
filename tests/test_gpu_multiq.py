"""GPU (-m gpu): Q questions per example from one encode and one prefill of the clips' 256 positions per example (include/mellow_hip.h
mellow_generate_q; Engine.generate with input_ids [B][Q][text_len]).

The yardstick is the existing code: the plain call on the B * Q expanded examples (audio rows repeated Q times, ids flattened), with
the same seed and row_offset.  In the "f32" engine the two are bit-identical: that mode's GEMMs do not depend on the batch, the cut
at position 256 is a multiple of the attention's query tile, and both forms run the last prefix position, the head and the decode
loop on the same B * Q rows.  In the default "f32x3" engine the prefill's last bits depend on how many rows share a launch (ABI
minor 1), so there the share of equal rows is printed, not asserted, and the log-probs are held to Engine.score of the same tokens:
2 * TOL = 1.2e-2, the bound and derivation of tests/test_gpu_genlogprob.py test_generate_matches_score (both routes within 6e-3 of
the reference).  The questions of one example differ, so a tail prefilled at the wrong position, or K/V fanned out to the wrong
row, moves a row's log-probs by order 1 (test_scoring_separates_the_questions measures that).  Every test prints what it measured
(DESIGN.md section 6j is where the figures belong)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import synth

pytestmark = pytest.mark.gpu

TOL = 6e-3
S = dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7)
VOCAB = 49152


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    e = E.Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


def _questions(B, Q):
    """(audio1, audio2, ids [B][Q][text_len]): question j of example b is the example's synthetic prompt with every id moved by
    1009 * j + 17 * b inside the vocabulary -- the questions of an example all differ"""
    a1, a2, ids = synth.make_batch(B)
    off = 1009 * np.arange(Q)[None, :, None] + 17 * np.arange(B)[:, None, None]
    return a1, a2, ((ids[:, None, :].astype(np.int64) + off) % VOCAB).astype(ids.dtype)


def _expand(batch):
    """the B * Q examples of the plain call: audio rows repeated Q times, ids flattened"""
    a1, a2, ids = batch
    Q = ids.shape[1]
    return np.repeat(a1, Q, axis=0), np.repeat(a2, Q, axis=0), ids.reshape(-1, ids.shape[2])


def _equal(r, w, with_lp):
    assert r[0].tobytes() == w[0].tobytes() and r[0].shape == w[0].shape
    assert r[1].tobytes() == w[1].tobytes() and r[2] == w[2]
    if with_lp:
        assert r[4].view(np.int32).tobytes() == w[4].view(np.int32).tobytes()


def test_smallest_case(engine):
    b = _questions(1, 2)
    toks, lens, steps, _ = engine.generate(*b, max_len=8, stop_id=-1)
    assert toks.shape == (2, 8) and toks.dtype == np.int32 and lens.dtype == np.int32 and steps == 8 and lens.tolist() == [8, 8]
    assert not np.array_equal(toks[0], toks[1])                  # two questions about one pair: two answers
    want, *_ = engine.generate(*_expand(b), max_len=8, stop_id=-1)
    print(f"[{engine.precision}] B = 1, Q = 2: rows equal to the expanded call: {int((toks == want).all(1).sum())} of 2")
    if engine.precision == "f32":
        assert toks.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def case11(engine):
    """B = 11, Q = 3: 33 rows, example 10's rows sit in row blocks 0 and 1.  Greedy and sampled, with the log-prob record; the
    expanded calls; and score() of the question-list calls' tokens on the expanded examples."""
    b = _questions(11, 3)
    x = _expand(b)
    out = {"batch": b, "expanded": x}
    for name, kw in (("greedy", {}), ("sampled", dict(row_offset=5, **S))):
        kw = dict(max_len=8, stop_id=-1, return_logprobs=True, **kw)
        got, want = engine.generate(*b, **kw), engine.generate(*x, **kw)
        ref, rsum, _ = engine.score(*x, got[0].reshape(33, 1, 8), np.full((33, 1), 8))
        out[name] = (got, want, ref.reshape(33, 8), rsum.reshape(33))
    return out


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_rows_across_a_row_block_boundary(engine, case11, mode):
    got, want, ref, _ = case11[mode]
    toks, lens, steps, _, lp = got
    assert toks.shape == (33, 8) and lp.shape == (33, 8) and lp.dtype == np.float32 and steps == 8
    same = (toks == want[0]).all(1)
    dlp = float(np.abs(lp[same] - want[4][same]).max()) if same.any() else float("nan")
    d = float(np.abs(lp.astype(np.float64) - ref).max())
    print(f"[{engine.precision}] B = 11, Q = 3, {mode}: rows whose tokens equal the expanded call's: {float(same.mean()):.3f}; log-probs of "
          f"those rows vs the expanded call: max|d| {dlp:.3e}; log-probs vs score() of the same tokens: max|d| {d:.3e}")
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert len({r.tobytes() for r in toks}) > 11                 # the questions of an example get answers of their own
    assert d <= 2 * TOL
    if engine.precision == "f32":
        _equal(got, want, True)


def test_scoring_separates_the_questions(engine, case11):
    """the check above can tell a right tail from a wrong one: the tokens of (example b, question j) scored under question j + 1 of
    the same example -- same clips, same head K/V, another tail -- are far from their own log-probs"""
    got, _, _, rsum = case11["greedy"]
    a1, a2, ids = case11["expanded"]
    wrong_ids = np.roll(ids.reshape(11, 3, -1), -1, axis=1).reshape(33, -1)
    _, wsum, _ = engine.score(a1, a2, wrong_ids, got[0].reshape(33, 1, 8), np.full((33, 1), 8))
    gap = np.abs(wsum.reshape(33).astype(np.float64) - rsum)
    print(f"[{engine.precision}] log-prob sum of a row's 8 tokens under the next question of its example: |gap| min {gap.min():.3f} "
          f"median {np.median(gap):.3f} max {gap.max():.3f} (the bound of the comparison is {2 * TOL})")
    assert np.median(gap) > 10 * 2 * TOL


def test_stop_rule_early_exit_and_migration(engine):
    b = _questions(5, 8)
    x = _expand(b)
    free, *_ = engine.generate(*b, max_len=24, stop_id=0, ignore_stop=True, **S)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    toks, lens, steps, _ = engine.generate(*b, max_len=24, stop_id=stop, **S)
    reps = engine.last_row_repacks()
    want, wlens, wsteps, _ = engine.generate(*x, max_len=24, stop_id=stop, **S)
    wreps = engine.last_row_repacks()
    print(f"[{engine.precision}] B = 5, Q = 8, stop id {stop}: steps {steps} (expanded call {wsteps}), repacks {reps} ({wreps}), "
          f"-1 entries {int((toks == -1).sum())} ({int((want == -1).sum())}), rows equal {int((toks == want).all(1).sum())} of 40")
    assert toks.shape == (40, steps) and lens.shape == (40,)
    for r in range(40):                                 # a row's length is its first stop id; -1 only after it
        hit = np.nonzero(toks[r] == stop)[0]
        assert lens[r] == (hit[0] if hit.size else steps)
        assert (toks[r, : min(lens[r] + 1, steps)] >= 0).all()
    if engine.precision == "f32":
        assert wreps > 0, "no row repack happened: pick a stop id that stops more rows"
        assert steps == wsteps and np.array_equal(lens, wlens)
        assert toks.tobytes() == want.tobytes()         # the -1 columns included
        assert reps == wreps


@pytest.mark.parametrize("with_lp", [False, True])
def test_graph_reuse(engine, with_lp):
    """a question-list call, a plain call and an n-call of the same 6 rows share the step graph (the key holds the row count): none
    may see stale state"""
    q, b6, b3 = _questions(2, 3), synth.make_batch(6), synth.make_batch(3)
    kw = dict(max_len=8, stop_id=-1, return_logprobs=with_lp, **S)
    calls = [lambda: engine.generate(*q, **kw),
             lambda: engine.generate(*b6, **kw),
             lambda: engine.generate(*b3, num_return_sequences=2, **kw),
             lambda: engine.generate(*q, **kw)]
    first = [c() for c in calls]
    _equal(first[3], first[0], with_lp)
    assert not np.array_equal(first[0][0], first[1][0]) and not np.array_equal(first[0][0], first[2][0])
    try:
        for on in (True, False):
            engine.set_graph(on)
            for c, w in zip(calls, first):
                _equal(c(), w, with_lp)
    finally:
        engine.set_graph(True)


def _raw(engine, batch, out_rows, max_len=4):
    """mellow_generate_q through ctypes on device copies of `batch` (ids [B][Q][text_len]); call(B, Q) -> return code"""
    a1, a2, ids = engine._f32(batch[0]), engine._f32(batch[1]), torch.as_tensor(batch[2]).to(device=engine.tdev, dtype=torch.int32).contiguous()
    out = torch.empty((out_rows, max_len), dtype=torch.int32, device=engine.tdev)
    lens, steps, ftm = (C.c_int32 * 1100)(), C.c_int32(0), C.c_float(0)
    engine._sync_inputs()

    def call(B, Q, do_sample=0, seed=0, row_offset=0):
        return engine.lib.mellow_generate_q(engine.h, E._ptr(a1), E._ptr(a2), a1.shape[1], E._ptr(ids), B, Q, max_len, do_sample, 0.9, 0.7,
                                            seed, row_offset, -1, 0, E._ptr(out), None, lens, C.byref(steps), C.byref(ftm))
    return call, out, lens, steps


def test_one_question_is_the_plain_call(engine):
    a1, a2, ids = synth.make_batch(3)
    for kw in (dict(max_len=8, stop_id=-1), dict(max_len=8, stop_id=-1, row_offset=2, return_logprobs=True, **S)):
        base = engine.generate(a1, a2, ids, **kw)
        one = engine.generate(a1, a2, ids[:, None, :], **kw)
        _equal(one, base, "return_logprobs" in kw)
    # ... and the C entry point with Q = 1 returns the bytes of mellow_generate_sampled
    base = engine.generate(a1, a2, ids, max_len=4, stop_id=-1, row_offset=2, **S)
    call, out, lens, steps = _raw(engine, (a1, a2, ids[:, None, :]), 3)
    assert call(3, 1, do_sample=1, seed=7, row_offset=2) == 0
    assert np.array_equal(out.cpu().numpy(), base[0]) and list(lens)[:3] == base[1].tolist() and steps.value == base[2]


def test_argument_errors_of_the_entry_point(engine):
    b = _questions(2, 2)
    call, out, lens, steps = _raw(engine, b, 4)
    assert call(2, 2) == 0
    good = out.cpu().numpy().copy()
    # host-side checks: nothing is launched
    assert call(2, 0) != 0 and b"Q must be >= 1" in engine.lib.mellow_last_error()
    assert call(2, -1) != 0
    assert call(25, 41) != 0 and b"1024" in engine.lib.mellow_last_error()          # 25 * 41 = 1025 rows
    # an id outside the vocabulary in question 1 of example 1: flagged on the device, raised as by the plain call
    bad = b[2].copy()
    bad[1, 1, 5] = VOCAB
    ids = torch.as_tensor(bad).to(device=engine.tdev, dtype=torch.int32)
    with pytest.raises(IndexError, match="index out of range in self"):
        engine.generate(b[0], b[1], ids, max_len=4, stop_id=-1)
    with pytest.raises(IndexError, match="index out of range in self"):
        engine.generate(*_expand((b[0], b[1], ids.cpu().numpy()))[:2], ids.reshape(4, -1), max_len=4, stop_id=-1)
    assert call(2, 2) == 0 and np.array_equal(out.cpu().numpy(), good)              # the engine is fine afterwards


def test_fp8_engine_refuses_several_questions(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        b = _questions(2, 2)
        with pytest.raises(ValueError, match="fp8"):
            e8.generate(*b, max_len=4, stop_id=-1)
        call, *_ = _raw(e8, b, 4)
        assert call(2, 2) != 0 and b"not available in MELLOW_PRECISION_FP8" in e8.lib.mellow_last_error()
        base = e8.generate(b[0], b[1], b[2][:, 0], max_len=4, stop_id=-1)
        one = e8.generate(b[0], b[1], b[2][:, :1], max_len=4, stop_id=-1)
        assert np.array_equal(one[0], base[0]) and one[0].shape == (2, 4)
    finally:
        e8.close()


def test_encode_and_prefill_cost_less_than_the_expanded_call(engine):
    """B = 8, Q = 4: front-end and encoder work is 1/4 of the expanded call's, prefill rows 8 * 256 + 32 * 133 = 6304 against
    32 * 389 = 12448 (0.51).  Median of three each in this process, after one warm-up of each."""
    b = _questions(8, 4)
    x = _expand(b)
    dev = lambda t: tuple(torch.as_tensor(v).to(engine.tdev) for v in t)
    b, x = dev((b[0], b[1], b[2].astype(np.int32))), dev((x[0], x[1], x[2].astype(np.int32)))

    def phases(batch):
        engine.generate(*batch, max_len=8, stop_id=-1)
        runs = []
        for _ in range(3):
            engine.generate(*batch, max_len=8, stop_id=-1)
            p = engine.last_phase_ms()
            runs.append((p["encode_ms"], p["prefill_ms"]))
        return float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))

    qe, qp = phases(b)
    xe, xp = phases(x)
    print(f"[{engine.precision}] B = 8, Q = 4, max_len 8: question lists encode {qe:.2f} ms + prefill {qp:.2f} ms = {qe + qp:.2f} ms; "
          f"expanded call encode {xe:.2f} ms + prefill {xp:.2f} ms = {xe + xp:.2f} ms; ratio {(qe + qp) / (xe + xp):.2f}")
    assert qe + qp < xe + xp
