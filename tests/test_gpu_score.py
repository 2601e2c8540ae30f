"""GPU (-m gpu): teacher-forced scoring -- mellow_score / mellow_lm_score through Engine.score / Engine.lm_score and
MellowWrapper.score / choose -- against the imported reference (tests/golden/score.npz, made by make_golden_score.py), against
the engine's own materialised logits, and against its own generation path.

Tolerances.  A token's log-prob against the reference: 6e-3 = the 3e-3 the project holds all-position logits to
(test_gpu_parity.py::test_all_position_forward_matches_reference) for the target logit plus 3e-3 for the log-sum-exp, which is
1-Lipschitz in the max norm.  lse of the fused head against an fp64 logsumexp of the materialised fp32 logits: 1e-4 (a tiled fp32
sum of 49152 terms in (0, 1], 64-wide groups, 768 merged partials: relative error below about 840 x 2^-24 = 5e-5, the rest is
expf / logf rounding); the measured maximum is printed by the test and recorded in DESIGN.md."""
import os
import wave

import numpy as np
import pytest
import torch

from mellow_amd import spec, synth

pytestmark = pytest.mark.gpu

TOL = 6e-3


@pytest.fixture(scope="module", params=["f32x3", "f32"])
def engine(request, synth_sd):
    from mellow_amd.engine import Engine
    e = Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch2():
    return synth.make_batch(2)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "score.npz"))


def _mask(lens, L):
    return np.arange(L)[None, None, :] < np.asarray(lens)[..., None]


def _same(engine, a, b, what):
    """layout independence: bit-equal on the exact fp32 path; f32x3 last bits depend on the batch (mellow_hip.h, minor 1): 1e-3"""
    if engine.precision == "f32":
        assert np.array_equal(a, b), f"{what}: max|d| {np.abs(a - b).max():.3e}"
    else:
        assert np.abs(a - b).max() <= 1e-3, f"{what}: max|d| {np.abs(a - b).max():.3e}"


def test_score_matches_the_reference(engine, batch2, fixture):
    a1, a2, ids = batch2
    g = fixture
    assert np.array_equal(ids, g["input_ids"])
    lp, sm, am = engine.score(a1, a2, ids, g["cand_ids"], g["cand_len"])
    assert lp.shape == (2, 3, 12) and sm.shape == (2, 3) and am.shape == (2, 3, 12) and lp.dtype == np.float32
    m = _mask(g["cand_len"], 12)
    d = np.abs(lp.astype(np.float64) - g["logprob"])[m]
    ref_sum = np.where(m, g["logprob"], 0).sum(-1)
    ds = np.abs(sm.astype(np.float64) - ref_sum)
    print(f"[{engine.precision}] token log-prob max|d| vs reference {d.max():.3e}; sum max|d| {ds.max():.3e}")
    assert np.isfinite(lp).all()
    assert d.max() <= TOL
    assert (ds <= TOL * g["cand_len"]).all(), ds
    assert np.array_equal(am, g["argmax"])                    # every position, padding included (reference gaps >= 6e-3)
    assert np.all(lp[~m] == 0.0)                              # padding entries exactly 0
    # out_sum is the fp32 sum over j < cand_len in ascending j
    want = np.zeros((2, 3), dtype=np.float32)
    for j in range(12):
        want = np.where(j < g["cand_len"], want + lp[:, :, j], want).astype(np.float32)
    assert np.array_equal(sm, want)


def test_fused_head_equals_materialised_logits(engine, fixture, golden_dir):
    g = fixture
    pre = torch.from_numpy(np.load(os.path.join(golden_dir, "enc10.npz"))["prefix"])
    seq = torch.cat((pre.to(engine.tdev), engine.embed_tokens(g["cand_ids"][:, 0])), 1)
    f0 = 380
    n = seq.shape[1] - f0
    rng = np.random.default_rng(5)
    tg = rng.integers(0, 49152, (2, n))
    tg[0, 3] = tg[1, 0] = -1
    logits = engine.lm_forward_logits(seq, from_pos=f0)
    out = {k: v.cpu().numpy() for k, v in engine.lm_score(seq, tg, from_pos=f0).items()}
    L = logits.cpu().numpy()
    assert np.array_equal(out["max"], L.max(-1))                                     # bit-equal accumulators
    assert np.array_equal(out["argmax"].reshape(-1), engine.argmax(logits.reshape(2 * n, -1)).cpu().numpy())
    tl = np.take_along_axis(L, np.maximum(tg, 0)[..., None], -1)[..., 0]
    want = np.where(tg >= 0, tl - out["lse"], np.float32(0)).astype(np.float32)      # one fp32 subtraction, as on the device
    assert np.array_equal(out["logprob"], want)                                      # <=> the target logit is bit-equal
    lse64 = torch.logsumexp(logits.double(), -1).cpu().numpy()
    d = np.abs(out["lse"].astype(np.float64) - lse64).max()
    print(f"[{engine.precision}] fused lse vs fp64 logsumexp of the materialised logits: max|d| {d:.3e}")
    assert d <= 1e-4


def test_teacher_forcing_reproduces_greedy_generation(engine, batch2):
    a1, a2, ids = batch2
    toks, _, steps, _ = engine.generate(a1, a2, ids, max_len=16, stop_id=-1)
    assert toks.shape == (2, 16)
    lp, sm, am = engine.score(a1, a2, ids, toks[:, None, :], np.full((2, 1), 16))
    assert np.array_equal(am[:, 0], toks)
    assert (lp <= 0).all() and (np.exp(lp) <= 1).all()


def test_layout_independence(engine, batch2, fixture):
    a1, a2, ids = batch2
    g = fixture
    c, ln = g["cand_ids"], g["cand_len"]
    lp, sm, am = engine.score(a1, a2, ids, c, ln)
    # K = 1, every candidate alone (its slot and K change, the other candidates are gone)
    for k in range(3):
        lp1, sm1, am1 = engine.score(a1, a2, ids, c[:, k:k + 1], ln[:, k:k + 1])
        _same(engine, lp1[:, 0], lp[:, k], f"candidate {k} alone")
        _same(engine, sm1[:, 0], sm[:, k], f"sum of candidate {k} alone")
        assert np.array_equal(am1[:, 0], am[:, k])
    # another slot order, and one example alone (the other rows of the batch are gone)
    perm = [2, 0, 1]
    lpp, smp, _ = engine.score(a1[1:], a2[1:], ids[1:], c[1:, perm], ln[1:, perm])
    _same(engine, lpp[0], lp[1, perm], "permuted slots, example 1 alone")
    _same(engine, smp[0], sm[1, perm], "permuted sums")
    # L padding: the same candidates in 20 slots (padding ids are arbitrary)
    pad = np.random.default_rng(9).integers(0, 49152, (2, 3, 8))
    lpl, sml, _ = engine.score(a1, a2, ids, np.concatenate((c, pad), 2), ln)
    _same(engine, lpl[:, :, :12], lp, "L = 20")
    assert np.all(lpl[:, :, 12:] == 0)
    _same(engine, sml, sm, "sums at L = 20")


def test_determinism_errors_and_generate_afterwards(engine, batch2, fixture, golden_dir):
    a1, a2, ids = batch2
    g = fixture
    c, ln = g["cand_ids"], g["cand_len"]
    r1 = engine.score(a1, a2, ids, c, ln)
    r2 = engine.score(a1, a2, ids, c, ln)
    for x, y in zip(r1, r2):
        assert x.tobytes() == y.tobytes()
    # -1 at a scored position of `score` is an id outside the vocabulary; in lm_score it means "not scored"
    bad = c.copy(); bad[1, 1, 2] = -1
    with pytest.raises(IndexError):
        engine.score(a1, a2, ids, bad, ln)
    bad = c.copy(); bad[0, 2, 0] = 49152
    with pytest.raises(IndexError):
        engine.score(a1, a2, ids, bad, ln)
    bad[0, 2, 0] = c[0, 2, 0]; bad[0, 2, 5] = 49152          # beyond cand_len = 1: padding, never scored
    r3 = engine.score(a1, a2, ids, bad, ln)
    assert r3[0].tobytes() == r1[0].tobytes()
    for wrong in (0, 13):
        l2 = ln.copy(); l2[1, 0] = wrong
        with pytest.raises(ValueError, match="cand_len"):
            engine.score(a1, a2, ids, c, l2)
    seq = torch.from_numpy(np.load(os.path.join(golden_dir, "enc10.npz"))["prefix"][:1])       # (1, 389, 576)
    with pytest.raises(IndexError):
        engine.lm_score(seq, np.asarray([[0, 49152]]), from_pos=387)
    with pytest.raises(IndexError):
        engine.lm_score(seq, np.asarray([[-2, 5]]), from_pos=387)
    out = engine.lm_score(seq, np.asarray([[-1, 5]]), from_pos=387)
    assert float(out["logprob"][0, 0]) == 0.0 and float(out["logprob"][0, 1]) < 0 and np.isfinite(out["lse"].cpu().numpy()).all()
    # the raw ABI refuses the same things without the binding's checks
    import ctypes as C
    from mellow_amd.engine import _ptr
    t = torch.tensor([[0, 49152]], dtype=torch.int32, device=engine.tdev)
    lpb = torch.empty((1, 2), dtype=torch.float32, device=engine.tdev)
    seq_d = seq.to(engine.tdev).contiguous()
    torch.cuda.synchronize()
    rc = engine.lib.mellow_lm_score(engine.h, _ptr(seq_d), 1, 389, 387, _ptr(t), _ptr(lpb), None, None, None)
    assert rc != 0 and b"index out of range" in engine.lib.mellow_last_error()
    # a generate call after score is undisturbed
    toks, *_ = engine.generate(a1, a2, ids, max_len=12, stop_id=-1)
    assert np.array_equal(toks, np.load(os.path.join(golden_dir, "gen.npz"))["tokens"])


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_candidate_length_budget(synth_sd, batch2, fixture, precision):
    """389 + L <= max_positions: one over is a ValueError naming the limit, the limit itself runs"""
    from mellow_amd.engine import Engine, EngineError, _ptr
    e = Engine(device=0, precision=precision, max_positions=400)
    e.load_state_dict(synth_sd)
    try:
        a1, a2, ids = batch2
        g = fixture
        assert e.max_candidate_tokens() == 11
        with pytest.raises(ValueError, match="L <= 11"):
            e.score(a1, a2, ids, g["cand_ids"], g["cand_len"])
        ln = np.minimum(g["cand_len"], 11)
        lp, sm, am = e.score(a1, a2, ids, g["cand_ids"][:, :, :11], ln)
        m = _mask(ln, 11)
        assert np.abs(lp.astype(np.float64) - g["logprob"][:, :, :11])[m].max() <= TOL
        # the raw ABI refuses L = 12 too
        c = torch.as_tensor(g["cand_ids"]).to(device=e.tdev, dtype=torch.int32).contiguous()
        lens = np.ascontiguousarray(g["cand_len"], dtype=np.int32)
        x1, x2, xi = e._f32(a1), e._f32(a2), e._prompt_ids(ids)
        o1 = torch.empty((2, 3, 12), dtype=torch.float32, device=e.tdev)
        o2 = torch.empty((2, 3), dtype=torch.float32, device=e.tdev)
        torch.cuda.synchronize()
        import ctypes as C
        rc = e.lib.mellow_score(e.h, _ptr(x1), _ptr(x2), x1.shape[1], _ptr(xi), 2, _ptr(c), lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                3, 12, _ptr(o1), _ptr(o2), None)
        assert rc != 0 and b"max_positions" in e.lib.mellow_last_error()
    finally:
        e.close()


def test_more_than_1024_rows_run_as_passes(engine):
    B, K, L = 9, 128, 2
    a1, a2, ids = synth.make_batch(B)
    rng = np.random.default_rng(11)
    c = rng.integers(0, 49152, (B, K, L))
    ln = rng.integers(1, L + 1, (B, K))
    lp, sm, am = engine.score(a1, a2, ids, c, ln)              # 1152 rows: a pass of 1024 and one of 128
    assert np.isfinite(lp).all() and np.all(lp[~_mask(ln, L)] == 0)
    h = K // 2
    for s in (slice(0, h), slice(h, K)):                       # 576 rows each: one pass
        lph, smh, amh = engine.score(a1, a2, ids, c[:, s], ln[:, s])
        _same(engine, lph, lp[:, s], "half of the candidates")
        _same(engine, smh, sm[:, s], "sums of half of the candidates")
        if engine.precision == "f32":
            assert np.array_equal(amh, am[:, s])


class Tok:
    """tokenizer stand-in in the style of tests/test_gpu_example_flow.py::Tok (the SmolLM2 files are not available offline); the
    stop token has an id inside the vocabulary here, because score() appends it to every candidate"""
    STOP = 2

    def encode(self, s):
        return [self.STOP] if s == "<|endoftext|>" else [17 + (sum(w.encode()) * 7919 + i * 104729) % 49000 for i, w in enumerate(s.split())]

    def encode_plus(self, text, max_length=129, **kw):
        ids = self.encode(text)[:max_length]
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([[1] * max_length])}

    def decode(self, ids):
        return " ".join(f"t{int(i)}" for i in ids)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_wrapper_score_and_choose(synth_sd, golden_dir, tmp_path, precision):
    from mellow import MellowWrapper
    g = np.load(os.path.join(golden_dir, "example.npz"))
    paths = []
    for name in ("1", "2"):
        p = tmp_path / f"{name}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(g[f"sr{name}"])); w.writeframes(np.asarray(g[f"pcm{name}"], dtype="<i2").tobytes())
        paths.append(str(p))
    mellow = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=synth_sd, tokenizer=Tok(), precision=precision)
    # 1.wav is shorter than 10 s (tiled: no random crop), so both examples preprocess deterministically
    examples = [[paths[0], paths[0], str(g["prompt"])], [paths[0], paths[0], "which clip is louder?"]]
    cands = [["dog barking", "chirping birds", "car engine", "clapping"], ["the first one", "the second"]]
    res = mellow.score(examples, cands)
    assert [len(r) for r in res] == [4, 2]
    tok = Tok()
    for r, cs in zip(res, cands):
        for c, text in zip(r, cs):
            assert c["tokens"] == len(text.split()) + 1 and len(c["token_logprobs"]) == c["tokens"]
            assert all(x <= 0 for x in c["token_logprobs"])
            assert abs(c["logprob"] - sum(c["token_logprobs"])) <= 1e-3 * max(1.0, abs(c["logprob"]))
    sums = [[c["logprob"] for c in r] for r in res]
    assert mellow.choose(examples, cands) == [int(np.argmax(s)) for s in sums]
    means = [[c["logprob"] / c["tokens"] for c in r] for r in res]
    assert mellow.choose(examples, cands, normalize="mean") == [int(np.argmax(s)) for s in means]
    # equality with Engine.score on the same ids
    ids, lens, counts = mellow._candidate_ids(cands, True, "<|endoftext|>")
    a = mellow.preprocess_audio([paths[0], paths[0]], resample=True)
    pid = mellow.preprocess_text([e[2] for e in examples])["input_ids"]
    lp, sm, _ = mellow.model.score(a, a, pid, ids, lens)
    for b in range(2):
        for k in range(counts[b]):
            assert res[b][k]["logprob"] == float(sm[b, k])
            assert res[b][k]["token_logprobs"] == [float(x) for x in lp[b, k, : lens[b, k]]]
    assert np.array_equal(ids[1, 2], ids[1, 0])               # ragged K: padded with the first candidate
    with pytest.raises(ValueError, match="at most"):
        mellow.score(examples[:1], [[" ".join(["w"] * mellow.model.max_candidate_tokens())]])


def test_fp8_mode_scores(synth_sd, batch2, fixture):
    """fp8 mode: runs, finite, the arg-max path is exercised.  No agreement floor is asserted here (tools/score_bench.py
    --precision fp8 --structured measures the teacher-forced distance to the f32x3 engine)."""
    from mellow_amd.engine import Engine
    e = Engine(device=0, precision="fp8")
    e.load_state_dict(synth_sd)
    try:
        a1, a2, ids = batch2
        g = fixture
        lp, sm, am = e.score(a1, a2, ids, g["cand_ids"], g["cand_len"])
        m = _mask(g["cand_len"], 12)
        assert np.isfinite(lp).all() and np.isfinite(sm).all() and (lp[m] < 0).all() and np.all(lp[~m] == 0)
        assert am.min() >= 0 and am.max() < 49152
        print(f"[fp8] arg-max agreement with the reference at {am.size} positions: {(am == g['argmax']).mean():.3f}; "
              f"token log-prob mean|d| {np.abs(lp - g['logprob'])[m].mean():.3e}")
        r2 = e.score(a1, a2, ids, g["cand_ids"], g["cand_len"])
        assert r2[0].tobytes() == lp.tobytes()
    finally:
        e.close()
