"""GPU (-m gpu): opt-in seeded nucleus sampling (include/mellow_hip.h mellow_generate_sampled, mellow_amd/csrc/sample.hip).

The kernel is held to the fp64 definition of tests/sampler_ref.py draw by draw (draws whose margins are below rounding are
gated and counted), its draws to the nucleus distribution, and the generation loop to the sampler applied to teacher-forced
logits.  Keying: a row's stream depends on (seed, global row, step) only -- not on batch slot, row migration, engine context or
shard.  Greedy stays what it was: top_p = 0 reproduces the greedy goldens, and a sampled call leaves the greedy graph intact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mellow_amd import synth
from mellow_amd.engine import Engine, EngineError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 49152
GATE = 1e-5


@pytest.fixture(scope="module")
def eng_f32(synth_sd):
    e = Engine(device=0, precision="f32")
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def eng(request, synth_sd):
    e = Engine(device=0, precision=request.param)
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def real_logits(eng_f32):
    a1, a2, ids = synth.make_batch(8)
    pre = eng_f32.prefix(a1, a2, ids)
    return eng_f32.lm_prefill(pre, reserve=4).cpu().numpy()


def _rows(real_logits):
    rng = np.random.default_rng(1)
    rows = []
    for k in range(19):
        rows.append(rng.standard_normal(V).astype(np.float32) * 8.0)              # peaked
        rows.append(rng.standard_normal(V).astype(np.float32) * 0.3)              # flat
        rows.append(np.round(rng.standard_normal(V) * 2.0).astype(np.float32))    # heavy exact ties
    rows += list(real_logits)
    return np.stack(rows)


def test_kernel_matches_fp64_reference(eng_f32, real_logits):
    L = _rows(real_logits)
    B = L.shape[0]
    assert B >= 64
    lt = torch.from_numpy(L).cuda()
    n_all = n_gated = 0
    for (top_p, T, seed, step) in [(0.9, 1.0, 7, 0), (0.5, 0.7, 2 ** 40 + 3, 5), (0.95, 1.3, 99, 63), (0.0, 1.0, 1, 2),
                                   (1.0, 1.0, 12345, 1), (0.8, 1.0, 2 ** 63 + 11, 17)]:
        row_ids = np.arange(B, dtype=np.int32) * 3 + 100
        got = eng_f32.sample_logits(lt, top_p, T, seed, step, row_ids=row_ids).cpu().numpy()
        for b in range(B):
            tok, gap, mm = R.sample_ref(L[b], top_p, T, seed, int(row_ids[b]), step)
            n_all += 1
            if gap <= GATE or mm <= GATE:
                n_gated += 1
                continue
            assert got[b] == tok, (top_p, T, seed, step, b, int(got[b]), tok, gap, mm)
    print(f"gated {n_gated} / {n_all} draws")
    assert n_gated < 0.01 * n_all


def test_draws_follow_the_nucleus_distribution(eng_f32):
    rng = np.random.default_rng(5)
    row = np.full(V, -30.0, dtype=np.float32)
    hot = rng.choice(V, 40, replace=False)
    row[hot] = rng.uniform(0.0, 3.0, 40).astype(np.float32)
    top_p, T, n = 0.9, 0.8, 8192
    p = R.nucleus_probs(row, top_p, T)
    lt = torch.from_numpy(np.tile(row, (1024, 1))).cuda()
    draws = []
    for s in range(n // 1024):
        draws.append(eng_f32.sample_logits(lt, top_p, T, seed=42, step=s).cpu().numpy())
    draws = np.concatenate(draws)
    assert np.all(p[draws] > 0), "a token outside the nucleus was drawn"
    support = np.nonzero(p)[0]
    obs = np.bincount(draws, minlength=V)[support].astype(np.float64)
    exp = p[support] * n
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    df = len(support) - 1
    print(f"chi2 {chi2:.1f}, df {df}")
    assert chi2 < df + 6.0 * np.sqrt(2.0 * df) + 10.0, (chi2, df)


def test_edge_cases(eng_f32):
    rng = np.random.default_rng(3)
    L = np.round(rng.standard_normal((8, V)) * 2.0).astype(np.float32)      # ties at the maximum
    L[2, 777] = np.nan
    L[5, [9, 3000]] = np.nan
    lt = torch.from_numpy(L).cuda()
    want = torch.argmax(lt, dim=1).int().cpu().numpy()
    for seed in (0, 1, 2 ** 62):
        got = eng_f32.sample_logits(lt, 0.0, 1.0, seed, 3).cpu().numpy()
        assert np.array_equal(got, want), (got, want)
    # top_p = 1 reaches the tail that every smaller nucleus cuts; a tie group on the boundary is cut by index
    row = np.zeros(V, dtype=np.float32)
    row[0] = 10.0
    lt = torch.from_numpy(np.tile(row, (1024, 1))).cuda()
    kept999, _ = R.nucleus_mask(R.scaled(row, 1.0), 0.999)
    d1 = np.concatenate([eng_f32.sample_logits(lt, 1.0, 1.0, 11, s).cpu().numpy() for s in range(8)])
    assert np.any(~kept999[d1]), "top_p = 1 never left the 0.999 nucleus"
    kept5, _ = R.nucleus_mask(R.scaled(row, 1.0), 0.5)
    cut = int(np.nonzero(kept5)[0].max())
    assert 100 < cut < V - 100
    d5 = np.concatenate([eng_f32.sample_logits(lt, 0.5, 1.0, 11, s).cpu().numpy() for s in range(4)])
    assert np.all(kept5[d5]) and d5.max() > 0.9 * cut, (cut, d5.max())
    for bad in [dict(top_p=0.9, temperature=0.0), dict(top_p=0.9, temperature=-1.0), dict(top_p=0.9, temperature=float("inf")),
                dict(top_p=float("nan"), temperature=1.0)]:
        with pytest.raises(EngineError):
            eng_f32.sample_logits(lt[:2], seed=1, step=0, **bad)
    # rows permuted together with their row ids: the tokens permute, bit for bit
    L = (rng.standard_normal((16, V)) * 3.0).astype(np.float32)
    ids = np.arange(16, dtype=np.int32) + 1000
    perm = rng.permutation(16)
    a = eng_f32.sample_logits(torch.from_numpy(L).cuda(), 0.9, 1.0, 5, 4, row_ids=ids).cpu().numpy()
    b = eng_f32.sample_logits(torch.from_numpy(L[perm]).cuda(), 0.9, 1.0, 5, 4, row_ids=ids[perm]).cpu().numpy()
    assert np.array_equal(a[perm], b)


def test_top_p_zero_is_greedy_end_to_end(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, "b32.npz"))
    a1, a2, ids = synth.make_batch(32)
    steps = int(g["steps"])
    toks, lens, n, _ = eng.generate(a1, a2, ids, max_len=steps, stop_id=-1, do_sample=True, top_p=0.0, temperature=1.0,
                                    seed=2024)
    assert n == steps and np.array_equal(toks, g["tokens"])


def test_generation_matches_teacher_forced_reference(eng_f32):
    B, L, top_p, T, seed = 8, 32, 0.9, 0.8, 31337
    a1, a2, ids = synth.make_batch(B)
    toks, *_ = eng_f32.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True, do_sample=True, top_p=top_p,
                                temperature=T, seed=seed)
    pre = eng_f32.prefix(a1, a2, ids)
    prefill = eng_f32.lm_prefill(pre, reserve=L).cpu().numpy()
    # teacher-forced: the whole sequence [prefix | embed(sampled tokens)] in one forward, logits of every generated position
    emb = eng_f32.embed_tokens(torch.from_numpy(toks[:, : L - 1].astype(np.int64)))
    tf = eng_f32.lm_forward_logits(torch.cat((pre, emb), 1), from_pos=pre.shape[1] - 1).cpu().numpy()
    assert np.abs(tf[:, 0] - prefill).max() < 5e-3
    n_all = n_gated = 0
    for b in range(B):
        for t in range(L):
            tok, gap, mm = R.sample_ref(tf[b, t], top_p, T, seed, b, t, mass_tol=2e-3)
            n_all += 1
            # the decode step's logits differ from the forward's by summation order: gate on that size
            if gap <= 2e-3 / T or mm <= 2e-3:
                n_gated += 1
                continue
            assert toks[b, t] == tok, (b, t, int(toks[b, t]), tok, gap, mm)
    print(f"gated {n_gated} / {n_all}")
    assert n_gated <= 0.05 * n_all


def test_determinism_and_graph_cache(eng_f32, synth_sd, golden_dir):
    g = np.load(os.path.join(golden_dir, "b32.npz"))
    a1, a2, ids = synth.make_batch(32)
    kw = dict(max_len=16, stop_id=-1, do_sample=True, top_p=0.9, temperature=1.0)
    t1, *_ = eng_f32.generate(a1, a2, ids, seed=1, **kw)
    t2, *_ = eng_f32.generate(a1, a2, ids, seed=1, **kw)
    assert np.array_equal(t1, t2)
    eng_f32.set_graph(False)
    try:
        t3, *_ = eng_f32.generate(a1, a2, ids, seed=1, **kw)
    finally:
        eng_f32.set_graph(True)
    assert np.array_equal(t1, t3)
    t4, *_ = eng_f32.generate(a1, a2, ids, seed=2, **kw)
    assert (t4 != t1).any(axis=1).mean() > 0.5
    gr, *_ = eng_f32.generate(a1, a2, ids, max_len=64, stop_id=-1)
    assert np.array_equal(gr, g["tokens"])            # greedy after sampled calls: the greedy graph is the greedy graph
    t5, *_ = eng_f32.generate(a1, a2, ids, seed=3, **kw)
    fresh = Engine(device=0, precision="f32")
    fresh.load_state_dict(synth_sd)
    t6, *_ = fresh.generate(a1, a2, ids, seed=3, **kw)
    fresh.close()
    assert np.array_equal(t5, t6)


def test_keying_across_layouts(eng_f32, synth_sd):
    a1, a2, ids = synth.make_batch(32)
    kw = dict(stop_id=-1, do_sample=True, top_p=0.9, temperature=1.0, seed=77)
    full, *_ = eng_f32.generate(a1, a2, ids, max_len=12, **kw)
    part, *_ = eng_f32.generate(a1[8:12], a2[8:12], ids[8:12], max_len=12, row_offset=8, **kw)
    assert np.array_equal(part, full[8:12])
    # 64 rows under the stop rule: row migration on (default) == off, and rows did migrate
    a1, a2, ids = synth.make_batch(64)
    kw = dict(do_sample=True, top_p=0.8, temperature=1.0, seed=5)
    free, *_ = eng_f32.generate(a1, a2, ids, max_len=24, stop_id=0, ignore_stop=True, **kw)
    vals, counts = np.unique(free[:, 1:6], return_counts=True)
    stop = int(vals[np.argmax(counts)])                 # the most frequent early token: several rows stop early
    mig, lm, nm, _ = eng_f32.generate(a1, a2, ids, max_len=24, stop_id=stop, **kw)
    reps = eng_f32.last_row_repacks()
    other = Engine(device=0, precision="f32", options={"row_migration": 0})
    other.load_state_dict(synth_sd)
    nomig, ln, nn, _ = other.generate(a1, a2, ids, max_len=24, stop_id=stop, **kw)
    other.close()
    assert nm == nn and np.array_equal(lm, ln)
    for r in range(64):
        assert np.array_equal(mig[r, : lm[r] + 1 if lm[r] < nm else nm], nomig[r, : lm[r] + 1 if lm[r] < nm else nm]), r
    assert reps > 0, "no row repack happened: pick a stop id that stops more rows"
    # EnginePool over 3 batches == one engine with the matching offsets
    from mellow_amd.serve import EnginePool
    batches = [synth.make_batch(n, first=f) for n, f in ((5, 0), (3, 5), (6, 8))]
    kw = dict(max_len=8, stop_id=-1, do_sample=True, top_p=0.9, temperature=1.0, seed=9)
    pool = EnginePool(synth_sd, n_contexts=2, precision="f32")
    try:
        res = pool.generate_many(batches, **kw)
    finally:
        pool.close()
    off = 0
    for (b1, b2, bi), r in zip(batches, res):
        want, *_ = eng_f32.generate(b1, b2, bi, row_offset=off, **kw)
        assert np.array_equal(r[0], want)
        off += len(b1)


def test_fp8_mode_samples(synth_sd):
    e = Engine(device=0, precision="fp8")
    e.load_state_dict(synth_sd)
    try:
        a1, a2, ids = synth.make_batch(8)
        greedy, *_ = e.generate(a1, a2, ids, max_len=12, stop_id=-1)
        z, *_ = e.generate(a1, a2, ids, max_len=12, stop_id=-1, do_sample=True, top_p=0.0, temperature=1.0, seed=4)
        s, *_ = e.generate(a1, a2, ids, max_len=12, stop_id=-1, do_sample=True, top_p=0.9, temperature=1.0, seed=4)
        assert np.array_equal(z, greedy)
        assert s.shape == (8, 12) and s.min() >= 0 and s.max() < V
    finally:
        e.close()


_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from mellow_amd import synth
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
_COLL = ("all_gather", "all_gather_into_tensor", "all_gather_object", "all_reduce", "broadcast", "broadcast_object_list", "gather",
         "scatter", "reduce", "reduce_scatter", "reduce_scatter_tensor", "all_to_all", "all_to_all_single", "barrier", "send", "recv")
_calls = []
def _count(name, fn):
    def w(*a, **k):
        _calls.append(name)
        return fn(*a, **k)
    return w
for _n in _COLL:
    if hasattr(dist, _n):
        setattr(dist, _n, _count(_n, getattr(dist, _n)))
sd = synth.make_state_dict(0)
from mellow_amd import MellowWrapper
class Tok:
    def encode(self, s): return [0] if s == "<|endoftext|>" else [17 + (sum(s.encode()) * 7919 + i * 104729) % 49000 for i, _ in enumerate(s.split())]
    def encode_plus(self, text, max_length=129, **kw):
        ids = self.encode(text)[:max_length]
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([[1] * max_length])}
    def decode(self, ids): return " ".join("<|endoftext|>" if int(i) == 0 else f"t{int(i)}" for i in ids)
rng = np.random.default_rng(0)
examples = [[rng.standard_normal(32000 * 3).astype(np.float32) * 0.1, rng.standard_normal(32000 * 4).astype(np.float32) * 0.1, p]
            for p in ("compare the two", "which is higher", "describe")]
m = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=sd, tokenizer=Tok(), data_parallel=True)
del _calls[:]
sharded = m.generate(examples=examples, max_len=6, top_p=0.9, temperature=1.0, audio_resample=False, do_sample=True, seed=7)
assert _calls == ["all_gather"], _calls
for bad in (None, 7 + rank):
    try:
        m.generate(examples=examples, max_len=6, top_p=0.9, temperature=1.0, audio_resample=False, do_sample=True, seed=bad)
        raise SystemExit(f"seed {bad} was accepted")
    except ValueError as e:
        pass
m1 = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=sd, tokenizer=Tok(), data_parallel=False)
alone = m1.generate(examples=examples, max_len=6, top_p=0.9, temperature=1.0, audio_resample=False, do_sample=True, seed=7)
assert sharded == alone, (rank, sharded, alone)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_data_parallel_sampling(tmp_path):
    script = tmp_path / "dp_sample_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29757", OMP_NUM_THREADS="8", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29757", str(script), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count("ok") == 2
