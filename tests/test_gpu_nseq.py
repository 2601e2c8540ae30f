"""GPU (-m gpu): n sampled answers per example from one encode and one prefill per example (include/mellow_hip.h
mellow_generate_n; Engine.generate(num_return_sequences=n)).

The yardstick is the existing code: the same call on every example given n times in a row, with the same seed and row_offset.
In the "f32" engine the two are bit-identical (that mode's prefill does not depend on the batch, and both forms run the last prefix
position, the head and the decode loop on the same B * n rows); in the default "f32x3" engine the prefill's last bits depend on
how many examples share the call (ABI minor 1), so there the share of equal rows is printed, not asserted, and the log-probs are
held to Engine.score of the same tokens: 2 * TOL = 1.2e-2, the bound and derivation of tests/test_gpu_genlogprob.py
test_generate_matches_score (both routes within 6e-3 of the reference).  A wrong or missing K/V copy of a row moves its
log-probs by order 1.  Every test prints what it measured (DESIGN.md section 6i is where the figures belong)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from mellow_amd import synth

pytestmark = pytest.mark.gpu

TOL = 6e-3
S = dict(do_sample=True, seed=7, top_p=0.9, temperature=0.7)


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    e = E.Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


def _rep(batch, n):
    """every example n times in a row"""
    return tuple(np.repeat(x, n, axis=0) for x in batch)


def test_smallest_case(engine):
    b = synth.make_batch(1)
    toks, lens, steps, _ = engine.generate(*b, max_len=8, stop_id=-1, num_return_sequences=2, **S)
    assert toks.shape == (2, 8) and toks.dtype == np.int32 and steps == 8 and lens.tolist() == [8, 8]
    assert not np.array_equal(toks[0], toks[1])                  # two rows of one example: two random streams
    want, *_ = engine.generate(*_rep(b, 2), max_len=8, stop_id=-1, **S)
    print(f"[{engine.precision}] B = 1, n = 2: rows equal to the repeated call: {int((toks == want).all(1).sum())} of 2")
    if engine.precision == "f32":
        assert np.array_equal(toks, want)


def test_copies_across_a_row_block_boundary(engine):
    """33 rows; n = 3 does not divide 32, so example 10's copies are rows 30, 31 (block 0) and 32 (block 1)"""
    b = synth.make_batch(11)
    kw = dict(max_len=8, stop_id=-1, row_offset=5, return_logprobs=True, **S)
    toks, lens, steps, _, lp = engine.generate(*b, num_return_sequences=3, **kw)
    assert toks.shape == (33, 8) and lp.shape == (33, 8) and lp.dtype == np.float32 and steps == 8
    want, wlens, wsteps, _, wlp = engine.generate(*_rep(b, 3), **kw)
    share = float((toks == want).all(1).mean())
    same = (toks == want).all(1)
    dlp = float(np.abs(lp[same] - wlp[same]).max()) if same.any() else float("nan")
    ref, _, _ = engine.score(*b, toks.reshape(11, 3, 8), np.full((11, 3), 8))
    d = float(np.abs(lp.astype(np.float64) - ref.reshape(33, 8)).max())
    print(f"[{engine.precision}] B = 11, n = 3: rows whose tokens equal the repeated call's: {share:.3f}; log-probs of those rows vs the "
          f"repeated call: max|d| {dlp:.3e}; log-probs vs score() of the same tokens: max|d| {d:.3e}")
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert d <= 2 * TOL
    if engine.precision == "f32":
        assert np.array_equal(toks, want) and np.array_equal(lens, wlens) and steps == wsteps
        assert np.array_equal(lp.view(np.int32), wlp.view(np.int32))


def test_stop_rule_early_exit_and_migration_on_fanned_out_rows(engine):
    b = synth.make_batch(5)
    free, *_ = engine.generate(*b, max_len=24, stop_id=0, ignore_stop=True, num_return_sequences=8, **S)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    toks, lens, steps, _ = engine.generate(*b, max_len=24, stop_id=stop, num_return_sequences=8, **S)
    reps = engine.last_row_repacks()
    want, wlens, wsteps, _ = engine.generate(*_rep(b, 8), max_len=24, stop_id=stop, **S)
    wreps = engine.last_row_repacks()
    print(f"[{engine.precision}] B = 5, n = 8, stop id {stop}: steps {steps} (repeated call {wsteps}), repacks {reps} ({wreps}), "
          f"-1 entries {int((toks == -1).sum())} ({int((want == -1).sum())}), rows equal {int((toks == want).all(1).sum())} of 40")
    assert toks.shape == (40, steps) and lens.shape == (40,)
    for r in range(40):                                 # a row's length is its first stop id; -1 only after it
        hit = np.nonzero(toks[r] == stop)[0]
        assert lens[r] == (hit[0] if hit.size else steps)
        assert (toks[r, : min(lens[r] + 1, steps)] >= 0).all()
    if engine.precision == "f32":
        assert wreps > 0, "no row repack happened: pick a stop id that stops more rows"
        assert steps == wsteps and np.array_equal(lens, wlens)
        assert np.array_equal(toks, want)               # the -1 columns included
        assert reps == wreps


@pytest.mark.parametrize("with_lp", [False, True])
def test_graph_reuse(engine, with_lp):
    """an n-call and a plain call of the same 6 rows share the step graph (the key holds the row count): none may see stale state"""
    b2, b3, b6 = synth.make_batch(2), synth.make_batch(3), synth.make_batch(6)
    kw = dict(max_len=8, stop_id=-1, return_logprobs=with_lp, **S)
    calls = [lambda: engine.generate(*b2, num_return_sequences=3, **kw),
             lambda: engine.generate(*b6, **kw),
             lambda: engine.generate(*b3, num_return_sequences=2, **kw),
             lambda: engine.generate(*b2, num_return_sequences=3, **kw)]

    def same(r, w):
        assert r[0].tobytes() == w[0].tobytes() and r[1].tobytes() == w[1].tobytes() and r[2] == w[2]
        if with_lp:
            assert r[4].tobytes() == w[4].tobytes()

    first = [c() for c in calls]
    same(first[3], first[0])
    assert not np.array_equal(first[0][0], first[1][0]) and not np.array_equal(first[0][0], first[2][0])
    try:
        for on in (True, False):
            engine.set_graph(on)
            for c, w in zip(calls, first):
                same(c(), w)
    finally:
        engine.set_graph(True)


def test_n_equal_one_is_the_plain_call(engine):
    b = synth.make_batch(3)
    kw = dict(max_len=8, stop_id=-1, row_offset=2, **S)
    base = engine.generate(*b, **kw)
    one = engine.generate(*b, num_return_sequences=1, **kw)
    assert one[0].tobytes() == base[0].tobytes() and one[1].tobytes() == base[1].tobytes() and one[2] == base[2]
    # ... and the C entry point with n = 1 returns the bytes of mellow_generate_sampled
    a1, a2, ids = engine._f32(b[0]), engine._f32(b[1]), engine._prompt_ids(b[2])
    out = torch.empty((3, 8), dtype=torch.int32, device=engine.tdev)
    lens, steps, ftm = (C.c_int32 * 3)(), C.c_int32(0), C.c_float(0)
    engine._sync_inputs()

    def call(B, n, do_sample=1):
        return engine.lib.mellow_generate_n(engine.h, E._ptr(a1), E._ptr(a2), a1.shape[1], E._ptr(ids), B, n, 8, do_sample, 0.9, 0.7, 7, 2, -1, 0,
                                            E._ptr(out), None, lens, C.byref(steps), C.byref(ftm))

    assert call(3, 1) == 0
    assert np.array_equal(out.cpu().numpy(), base[0]) and list(lens) == base[1].tolist() and steps.value == base[2]
    # argument errors of the entry point (host-side checks: nothing is launched)
    assert call(3, 2, do_sample=0) != 0 and b"do_sample" in engine.lib.mellow_last_error()
    assert call(3, 342) != 0 and b"1024" in engine.lib.mellow_last_error()
    assert call(3, 0) != 0


def test_host_passes_of_a_large_call(engine, monkeypatch):
    """B * n beyond one pass is cut into consecutive calls with row_offset advanced by n per example (here with the pass size
    lowered to 4 rows: passes of 2 + 1 examples): the rows of the one-pass call"""
    b = synth.make_batch(3)
    kw = dict(max_len=6, stop_id=-1, row_offset=3, return_logprobs=True, num_return_sequences=2, **S)
    whole = engine.generate(*b, **kw)
    monkeypatch.setattr(E, "NSEQ_PASS_ROWS", 4)
    assert E.plan_nseq_passes(3, 2, 3) == [(0, 2, 3), (2, 3, 7)]
    cut = engine.generate(*b, **kw)
    assert cut[0].shape == (6, 6) and cut[2] == whole[2]
    print(f"[{engine.precision}] passes of 2 + 1 examples vs one pass: rows equal {int((cut[0] == whole[0]).all(1).sum())} of 6")
    if engine.precision == "f32":
        assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1])
        assert np.abs(cut[4] - whole[4]).max() <= 1e-3         # (one row block either way: the same decode kernels)


def test_fp8_engine_refuses_n_above_one(synth_sd):
    e8 = E.Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    try:
        b = synth.make_batch(2)
        with pytest.raises(E.EngineError, match="not available in MELLOW_PRECISION_FP8"):
            e8.generate(*b, max_len=4, stop_id=-1, num_return_sequences=2, **S)
        base = e8.generate(*b, max_len=4, stop_id=-1, **S)
        one = e8.generate(*b, max_len=4, stop_id=-1, num_return_sequences=1, **S)
        assert np.array_equal(one[0], base[0]) and one[0].shape == (2, 4)
    finally:
        e8.close()


def test_1024_rows_offsets_past_32_bits(engine):
    """32 examples x 32 answers: the pages of 1024 rows hold 2.6e9 floats per tensor, so a 32-bit element or byte offset in the
    fan-out would wrap.  The first and the last example's 64 rows are held to score() of their tokens."""
    b = synth.make_batch(32)
    toks, lens, steps, _, lp = engine.generate(*b, max_len=3, stop_id=-1, num_return_sequences=32, return_logprobs=True, **S)
    assert toks.shape == (1024, 3) and (toks >= 0).all() and np.isfinite(lp).all() and (lp <= 0).all()
    pick = [0, 31]
    ref, _, _ = engine.score(b[0][pick], b[1][pick], b[2][pick], toks.reshape(32, 32, 3)[pick], np.full((2, 32), 3))
    d = float(np.abs(lp.reshape(32, 32, 3)[pick].astype(np.float64) - ref).max())
    print(f"[{engine.precision}] B = 32, n = 32: log-probs of examples 0 and 31 vs score(): max|d| {d:.3e}; distinct first tokens "
          f"of example 31: {len(set(toks[31 * 32:, 0].tolist()))}")
    assert d <= 2 * TOL
