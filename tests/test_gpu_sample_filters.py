"""GPU (-m gpu): the sampler's candidate filters top_k / min_p (include/mellow_hip.h mellow_generate_filters /
mellow_sample_logits_filtered; Engine.generate(top_k=, min_p=); the FILT instantiations of mellow_amd/csrc/sample.hip).

The kernel is held to the fp64 definition of tests/sampler_filters_ref.py draw by draw (draws whose margins are below rounding are
gated and counted), to exact cases that no rounding touches, its draws to the renormalised kept distribution, and the generation loop
to the reference applied to teacher-forced logits.  Keying and capture: one captured step serves every (top_k, min_p); a call without
the keywords is the call it was.  The sampler is one workgroup per 49152-wide row, so the batch is the only size there is to choose."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import synth
from mellow_amd.engine import Engine, EngineError, SampleFilters, _ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_filters_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu
V = 49152
GATE = 1e-5


@pytest.fixture(scope="module")
def eng(synth_sd):
    e = Engine(device=0, precision="f32")
    e.load_state_dict(synth_sd)
    yield e
    e.close()


def _fresh(synth_sd, precision="f32"):
    e = Engine(device=0, precision=precision)
    e.load_state_dict(synth_sd)
    return e


_DATA = {}


def _rows(eng):
    """the 57 synthetic rows of tests/test_gpu_sampling.py (seed 1: peaked, flat, heavy ties) and 8 rows of prefill logits; built once"""
    if "rows" not in _DATA:
        rng = np.random.default_rng(1)
        rows = []
        for k in range(19):
            rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)              # peaked
            rows.append(rng.standard_normal(V).astype(np.float32) * 0.3)              # flat
            rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))    # heavy exact ties
        a1, a2, ids = synth.make_batch(8)
        rows += list(eng.lm_prefill(eng.prefix(a1, a2, ids), reserve=4).cpu().numpy())
        L = np.stack(rows)
        assert L.shape == (65, V)
        _DATA["rows"] = (L, torch.from_numpy(L).cuda())
    return _DATA["rows"]


# ---- 1. draw by draw against the reference ---------------------------------------------------------------------------------------
CASES = [(50, 1.0, 0.0, 1.0, 7, 0), (1, 0.9, 0.0, 1.0, 3, 1), (40, 0.9, 0.0, 0.7, 2 ** 40 + 3, 5), (0, 1.0, 0.05, 1.0, 99, 63),
         (0, 0.95, 0.1, 1.3, 12345, 2), (1000, 0.8, 0.02, 1.0, 2 ** 63 + 11, 17), (49152, 1.0, 0.0, 1.0, 5, 4), (7, 0.5, 0.5, 0.9, 11, 9)]
_GATED = {}


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_matches_fp64_reference(eng, case):
    top_k, top_p, min_p, T, seed, step = CASES[case]
    L, lt = _rows(eng)
    B = L.shape[0]
    row_ids = np.arange(B, dtype=np.int32) * 3 + 100
    got = eng.sample_logits(lt, top_p, T, seed, step, row_ids=row_ids, top_k=top_k, min_p=min_p, filtered=True).cpu().numpy()
    n_gated, sizes = 0, []
    for b in range(B):
        tok, gap, mm, mq = F.sample_ref(L[b], top_k, top_p, min_p, T, seed, int(row_ids[b]), step)
        if gap <= GATE or mm <= GATE or mq <= GATE:
            n_gated += 1
            continue
        assert got[b] == tok, (CASES[case], b, int(got[b]), tok, gap, mm, mq)
    _GATED[case] = (n_gated, B)
    print(f"case {CASES[case]}: gated {n_gated} / {B} draws")


def test_gated_share_of_the_reference_comparison():
    """the share of gated draws over the eight cases above (they ran before this test, in this module)"""
    assert sorted(_GATED) == list(range(len(CASES))), "the eight cases did not all run"
    n_gated, n_all = sum(g for g, _ in _GATED.values()), sum(n for _, n in _GATED.values())
    print(f"gated {n_gated} / {n_all} draws")
    assert n_all == 8 * 65 and n_gated < 0.01 * n_all


# ---- 2. exact cases ---------------------------------------------------------------------------------------------------------------
def test_neutral_filters_and_the_whole_vocabulary_are_the_plain_draw(eng):
    L, lt = _rows(eng)
    row_ids = np.arange(L.shape[0], dtype=np.int32) * 3 + 100
    for (top_p, T, seed, step) in ((0.9, 1.0, 7, 0), (0.5, 0.7, 2 ** 40 + 3, 5), (1.0, 1.0, 12345, 1), (0.0, 1.0, 1, 2)):
        plain = eng.sample_logits(lt, top_p, T, seed, step, row_ids=row_ids).cpu().numpy()
        for kw in (dict(), dict(top_k=V), dict(top_k=V + 1), dict(top_k=2 ** 31 - 1)):
            filt = eng.sample_logits(lt, top_p, T, seed, step, row_ids=row_ids, filtered=True, **kw).cpu().numpy()
            assert filt.tobytes() == plain.tobytes(), (top_p, T, seed, step, kw)


def test_top_k_1_is_the_arg_max(eng):
    rng = np.random.default_rng(3)
    L = np.round(rng.standard_normal((8, V)) * 2.0).astype(np.float32)      # ties at the maximum
    L[2, 777] = np.nan                                                      # (the NaN rows of tests/test_gpu_sampling.py test_edge_cases)
    L[5, [9, 3000]] = np.nan
    lt = torch.from_numpy(L).cuda()
    want = torch.argmax(lt, dim=1).int().cpu().numpy()
    for seed in (0, 1, 2 ** 62):
        for top_p, min_p in ((1.0, 0.0), (0.9, 0.0), (0.3, 0.5)):
            got = eng.sample_logits(lt, top_p, 1.0, seed, 3, top_k=1, min_p=min_p).cpu().numpy()
            assert np.array_equal(got, want), (seed, top_p, min_p, got, want)


def test_min_p_1_keeps_exactly_the_tokens_tied_at_the_maximum(eng):
    rng = np.random.default_rng(4)
    row = rng.standard_normal(V).astype(np.float32)
    tied = np.sort(rng.choice(V, 5, replace=False))
    row[tied] = row.max() + 0.5
    lt = torch.from_numpy(np.tile(row, (1024, 1))).cuda()
    d = np.concatenate([eng.sample_logits(lt, 1.0, 1.0, 21, s, min_p=1.0).cpu().numpy() for s in range(2)])
    assert np.isin(d, tied).all() and len(set(d.tolist())) > 1, set(d.tolist())


def test_an_all_equal_row_is_cut_by_index(eng):
    lt = torch.zeros((1024, V), dtype=torch.float32).cuda()
    d = np.concatenate([eng.sample_logits(lt, 1.0, 1.0, 8, s, top_k=37).cpu().numpy() for s in range(4)])
    assert d.min() >= 0 and d.max() <= 36 and len(set(d.tolist())) == 37, sorted(set(d.tolist()))


def test_top_k_inside_a_tie_group(eng):
    rng = np.random.default_rng(1)
    for _ in range(2):
        rng.standard_normal(V)
    row = np.round(rng.standard_normal(V) * 2.0).astype(np.float32)          # the first ties-heavy row of _rows
    order = np.lexsort((np.arange(V), -row.astype(np.float64)))
    lt = torch.from_numpy(np.tile(row, (1024, 1))).cuda()
    for K in (3, 100, 5000):
        assert row[order[K - 1]] == row[order[K]], "K does not fall inside a tie group"
        first = np.zeros(V, dtype=bool)
        first[order[:K]] = True
        for top_p in (1.0, 0.97):
            d = eng.sample_logits(lt, top_p, 1.0, 13, K, top_k=K).cpu().numpy()
            assert first[d].all(), (K, top_p)
            if top_p == 1.0 and K > 3:            # the tail of the set is reached: the cut is not short of K either
                assert np.isin(d, order[K // 2:K]).any(), K


def test_bad_values_raise_engine_error(eng):
    lt = torch.zeros((2, V), dtype=torch.float32).cuda()
    out = torch.zeros((2,), dtype=torch.int32).cuda()
    for f in (SampleFilters(size=8, top_k=1, min_p=0.0), SampleFilters(size=12, top_k=-1, min_p=0.0),
              SampleFilters(size=12, top_k=0, min_p=float("nan")), SampleFilters(size=12, top_k=0, min_p=1.5),
              SampleFilters(size=12, top_k=0, min_p=-0.5)):
        with pytest.raises(EngineError):
            eng._chk(eng.lib.mellow_sample_logits_filtered(eng.h, _ptr(lt), 2, None, 0, 1.0, 1.0, 1, C.byref(f), _ptr(out)))
        with pytest.raises(EngineError):
            eng._chk(eng.lib.mellow_generate_filters(eng.h, C.byref(f)))
    for bad in (dict(top_p=0.9, temperature=0.0), dict(top_p=float("nan"), temperature=1.0)):
        with pytest.raises(EngineError):
            eng.sample_logits(lt, seed=1, step=0, top_k=5, **bad)
    # a greedy call and a beam call refuse armed filters, and disarm them
    a1, a2, ids = synth.make_batch(2)
    f = SampleFilters(size=12, top_k=5, min_p=0.0)
    want, *_ = eng.generate(a1, a2, ids, max_len=3, stop_id=-1)
    for kw in (dict(), dict(num_beams=2)):
        eng._chk(eng.lib.mellow_generate_filters(eng.h, C.byref(f)))
        with pytest.raises(EngineError, match="sample filters are armed"):
            eng.generate(a1, a2, ids, max_len=3, stop_id=-1, **kw)
        got, *_ = eng.generate(a1, a2, ids, max_len=3, stop_id=-1)
        assert np.array_equal(got, want)


# ---- 3. distribution --------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_renormalised_kept_distribution(eng):
    rng = np.random.default_rng(5)
    row = np.full(V, -30.0, dtype=np.float32)
    hot = rng.choice(V, 40, replace=False)
    row[hot] = rng.uniform(0.0, 3.0, 40).astype(np.float32)                 # (the 40-hot row of tests/test_gpu_sampling.py)
    top_k, min_p, T, n = 12, 0.1, 0.8, 8192
    p = F.filtered_probs(row, top_k, 1.0, min_p, T)
    lt = torch.from_numpy(np.tile(row, (1024, 1))).cuda()
    draws = np.concatenate([eng.sample_logits(lt, 1.0, T, seed=42, step=s, top_k=top_k, min_p=min_p).cpu().numpy() for s in range(n // 1024)])
    assert np.all(p[draws] > 0), "a token outside the kept set was drawn"
    support = np.nonzero(p)[0]
    assert 2 <= len(support) <= top_k
    obs = np.bincount(draws, minlength=V)[support].astype(np.float64)
    exp = p[support] * n
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    df = len(support) - 1
    print(f"kept {len(support)} tokens; chi2 {chi2:.1f}, df {df}")
    assert chi2 < df + 6.0 * np.sqrt(2.0 * df) + 10.0, (chi2, df)


# ---- 4. the loop against teacher-forced logits -----------------------------------------------------------------------------------
def test_generation_matches_teacher_forced_reference(eng):
    B, L, top_k, top_p, min_p, T, seed = 4, 16, 20, 0.9, 0.02, 0.8, 31337
    a1, a2, ids = synth.make_batch(B)
    toks, *_ = eng.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True, do_sample=True, top_p=top_p, temperature=T, seed=seed,
                            top_k=top_k, min_p=min_p)
    pre = eng.prefix(a1, a2, ids)
    prefill = eng.lm_prefill(pre, reserve=L).cpu().numpy()
    # teacher-forced: the whole sequence [prefix | embed(sampled tokens)] in one forward, logits of every generated position
    emb = eng.embed_tokens(torch.from_numpy(toks[:, : L - 1].astype(np.int64)))
    tf = eng.lm_forward_logits(torch.cat((pre, emb), 1), from_pos=pre.shape[1] - 1).cpu().numpy()
    assert np.abs(tf[:, 0] - prefill).max() < 5e-3
    n_all = n_gated = 0
    for b in range(B):
        for t in range(L):
            tok, gap, mm, mq = F.sample_ref(tf[b, t], top_k, top_p, min_p, T, seed, b, t, mass_tol=2e-3, minp_tol=2e-3)
            n_all += 1
            # the decode step's logits differ from the forward's by summation order: gate on that size
            if gap <= 2e-3 / T or mm <= 2e-3 or mq <= 2e-3:
                n_gated += 1
                continue
            assert toks[b, t] == tok, (b, t, int(toks[b, t]), tok, gap, mm, mq)
    print(f"gated {n_gated} / {n_all}")
    assert n_gated <= 0.05 * n_all


# ---- 5. keying and capture ----------------------------------------------------------------------------------------------------------
def test_keying_and_capture(eng, synth_sd, golden_dir):
    a1, a2, ids = synth.make_batch(8)
    kw = dict(max_len=8, stop_id=-1, do_sample=True, top_p=0.9, temperature=1.0, seed=77)
    f1, f2 = dict(top_k=50, min_p=0.05), dict(top_k=5, min_p=0.3)
    full, *_ = eng.generate(a1, a2, ids, **kw, **f1)
    again, *_ = eng.generate(a1, a2, ids, **kw, **f1)
    assert np.array_equal(full, again)
    eng.set_graph(False)
    try:
        eager, *_ = eng.generate(a1, a2, ids, **kw, **f1)
    finally:
        eng.set_graph(True)
    assert np.array_equal(full, eager), "graph on and graph off differ"
    part, *_ = eng.generate(a1[2:6], a2[2:6], ids[2:6], row_offset=2, **kw, **f1)
    assert np.array_equal(part, full[2:6])
    # two calls with different values on one engine (one capture) == the same calls on a fresh engine each
    second, *_ = eng.generate(a1, a2, ids, **kw, **f2)
    assert (second != full).any()
    for f, want in ((f1, full), (f2, second)):
        fresh = _fresh(synth_sd)
        got, *_ = fresh.generate(a1, a2, ids, **kw, **f)
        fresh.close()
        assert np.array_equal(got, want), f
    # an un-filtered sampled call after filtered ones is that call on a fresh engine; greedy still reproduces the golden tokens
    plain, *_ = eng.generate(a1, a2, ids, **kw)
    fresh = _fresh(synth_sd)
    want, *_ = fresh.generate(a1, a2, ids, **kw)
    fresh.close()
    assert np.array_equal(plain, want)
    g = np.load(os.path.join(golden_dir, "b32.npz"))
    b32 = synth.make_batch(32)
    gr, *_ = eng.generate(*b32, max_len=int(g["steps"]), stop_id=-1)
    assert np.array_equal(gr, g["tokens"])


# ---- 6. combinations ------------------------------------------------------------------------------------------------------------------
S6 = dict(max_len=6, stop_id=-1, do_sample=True, seed=11, top_p=0.9, temperature=0.8, top_k=5, min_p=0.3)


def test_num_return_sequences_and_question_lists_equal_the_expanded_lists(eng):
    b = synth.make_batch(6)
    three = tuple(x[:3] for x in b)
    n2, *_ = eng.generate(*three, num_return_sequences=2, **S6)
    ex, *_ = eng.generate(*(np.repeat(x, 2, axis=0) for x in three), **S6)
    assert n2.shape == (6, 6) and n2.tobytes() == ex.tobytes()
    q_ids = np.asarray(b[2]).reshape(3, 2, -1)                      # questions (0, 1) about pair 0, (2, 3) about pair 1, (4, 5) about pair 2
    q2, *_ = eng.generate(three[0], three[1], q_ids, **S6)
    qx, *_ = eng.generate(np.repeat(three[0], 2, axis=0), np.repeat(three[1], 2, axis=0), np.asarray(b[2]), **S6)
    assert q2.shape == (6, 6) and q2.tobytes() == qx.tobytes()


def test_return_logprobs_leaves_the_tokens_and_records_the_unfiltered_log_softmax(eng):
    b = synth.make_batch(3)
    toks, lens, steps, _ = eng.generate(*b, **S6)
    st, sl, ss, _, lp = eng.generate(*b, return_logprobs=True, **S6)
    assert st.tobytes() == toks.tobytes() and np.array_equal(sl, lens) and ss == steps
    res = eng.generate(*b, return_logprobs=True, top_logprobs=3, **S6)
    assert res[0].tobytes() == toks.tobytes() and res[4].tobytes() == lp.tobytes()
    # the record is the model's log-softmax at temperature 1 without any filter: what the un-filtered call records for the same tokens
    # at step 0 (same prefill row), and what the teacher-forced forward gives at every step
    pt, _, _, _, plp, ptid, ptlp = eng.generate(*b, return_logprobs=True, top_logprobs=3, **dict(S6, top_k=0, min_p=0.0))
    assert res[5][:, 0].tobytes() == ptid[:, 0].tobytes() and res[6][:, 0].tobytes() == ptlp[:, 0].tobytes()
    pre = eng.prefix(*b)
    emb = eng.embed_tokens(torch.from_numpy(toks[:, :-1].astype(np.int64)))
    tf = eng.lm_forward_logits(torch.cat((pre, emb), 1), from_pos=pre.shape[1] - 1).cpu().numpy().astype(np.float64)
    ls = tf - (tf.max(-1, keepdims=True) + np.log(np.exp(tf - tf.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    want = np.take_along_axis(ls, toks[..., None].astype(np.int64), axis=-1)[..., 0]
    err = float(np.abs(lp - want).max())
    print(f"max |logprob - log-softmax of the forward| {err:.3e} (bound 1.2e-2, the project's log-prob tolerance)")
    assert err <= 1.2e-2


def test_with_guidance_and_repetition_penalty(eng):
    b = synth.make_batch(3)
    neg = (b[1], b[0], b[2])
    kw = dict(S6, guidance_scale=2.0, negative=neg, repetition_penalty=1.3)
    toks, *_ = eng.generate(*b, keep_negative_rows=True, **kw)
    assert toks.shape == (6, 6) and toks[0::2].tobytes() == toks[1::2].tobytes(), "the two rows of a pair differ"
    half, *_ = eng.generate(*b, **kw)
    assert half.tobytes() == toks[0::2].tobytes() and half.min() >= 0 and half.max() < V


def test_engine_pool_equals_one_engine(eng, synth_sd):
    from mellow_amd.serve import EnginePool
    batches = [synth.make_batch(n, first=f) for n, f in ((3, 0), (2, 3), (3, 5))]
    pool = EnginePool(synth_sd, n_contexts=2, precision="f32")
    try:
        res = pool.generate_many(batches, **S6)
    finally:
        pool.close()
    off = 0
    for (b1, b2, bi), r in zip(batches, res):
        want, *_ = eng.generate(b1, b2, bi, row_offset=off, **S6)
        assert np.array_equal(r[0], want)
        off += len(b1)


def test_fp8_mode(synth_sd):
    e = _fresh(synth_sd, "fp8")
    try:
        b = synth.make_batch(3)
        greedy, *_ = e.generate(*b, max_len=6, stop_id=-1)
        k1, *_ = e.generate(*b, max_len=6, stop_id=-1, do_sample=True, seed=4, top_p=0.9, temperature=1.0, top_k=1)
        s, *_ = e.generate(*b, **S6)
        assert np.array_equal(k1, greedy)
        assert s.shape == (3, 6) and s.min() >= 0 and s.max() < V
    finally:
        e.close()


# ---- 7. the wrapper -------------------------------------------------------------------------------------------------------------------
class Tok:
    def encode(self, s):
        return [0] if s == "<|endoftext|>" else [17 + (sum(s.encode()) * 7919 + i * 104729) % 49000 for i, _ in enumerate(s.split())]

    def encode_plus(self, text, max_length=129, **kw):
        ids = self.encode(text)[:max_length]
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([[1] * max_length])}

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(i) == 0 else f"t{int(i)}" for i in ids)


def test_wrapper_generate_with_filters(synth_sd):
    from mellow_amd import MellowWrapper
    rng = np.random.default_rng(0)
    examples = [[rng.standard_normal(32000 * 3).astype(np.float32) * 0.1, rng.standard_normal(32000 * 4).astype(np.float32) * 0.1, p]
                for p in ("compare the two", "which is higher")]
    m = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=synth_sd, tokenizer=Tok(), data_parallel=False)
    kw = dict(examples=examples, max_len=5, top_p=0.9, temperature=1.0, audio_resample=False)
    out = m.generate(do_sample=True, seed=7, top_k=50, min_p=0.05, **kw)
    assert len(out) == 2 and all(isinstance(t, str) and t for t in out)
    assert out == m.generate(do_sample=True, seed=7, top_k=50, min_p=0.05, **kw)
    k1 = m.generate(do_sample=True, seed=7, top_k=1, **kw)
    assert k1 == m.generate(**kw), "top_k = 1 is not the greedy answer"
    nested = m.generate(do_sample=True, seed=7, top_k=50, min_p=0.05, num_return_sequences=2, **kw)
    assert [len(x) for x in nested] == [2, 2]
    with pytest.raises(ValueError, match="do_sample=True"):
        m.generate(top_k=5, **kw)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(num_beams=2, min_p=0.1, **kw)
    with pytest.raises(ValueError):
        m.generate(do_sample=True, seed=7, min_p=1.5, **kw)
