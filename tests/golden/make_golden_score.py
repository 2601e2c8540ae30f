#!/usr/bin/env python3
"""Generate tests/golden/score.npz: teacher-forced scoring statistics of the IMPORTED reference (build container only, like
make_golden.py, whose model construction this script imports and does not edit).

    python tests/golden/make_golden_score.py

For the two synthetic examples of the "enc10" / "forward" cases, K = 3 candidate answers of L = 12 token slots, lengths
(12, 7, 1): candidate 0 = the first 12 reference greedy tokens of gen.npz (a high-probability path), candidates 1 and 2 (and
every slot beyond a candidate's length) = seeded random ids.  One `model(input_dict).logits` call per candidate slot on the
CPU; from its fp32 logits, in fp64: log-softmax at the candidate ids, log-sum-exp, arg-max, maximum logit and top-2 gap of
every position 388 + j, j < L (position 388 + j predicts token j).

The GPU test compares arg-max at every position and holds the engine's logits to 3e-3, so the script asserts that NO position
has a reference top-2 gap below 6e-3; if the first seed has one it steps the seed (+1, at most 16 times) and records the
seed used.  Only arrays are stored.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository, the shims and the reference on sys.path)

from mellow_amd import spec, synth  # noqa: E402

K, L = 3, 12
CAND_LEN = (12, 7, 1)
SEED0 = MG.SEED + 177
MIN_GAP = 6e-3
MAX_SEED_STEPS = 16


def candidates(seed, greedy):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 49152, (greedy.shape[0], K, L), generator=g)
    c[:, 0, :] = torch.from_numpy(greedy[:, :L])
    return c


def reference_stats(model, a1t, a2t, idst, cand):
    B = cand.shape[0]
    P = spec.PREFIX_LEN
    out = {k: np.zeros((B, K, L), dtype=np.float64) for k in ("logprob", "lse", "max_logit", "top2_gap")}
    out["argmax"] = np.zeros((B, K, L), dtype=np.int64)
    for k in range(K):
        with torch.no_grad():
            logits = model({"audio1": a1t, "audio2": a2t, "input": {"input_ids": idst}, "answer": {"input_ids": cand[:, k]}}).logits
        assert logits.shape == (B, P + L, 49152) and logits.dtype == torch.float32
        sc = logits[:, P - 1: P - 1 + L].double()
        lse = torch.logsumexp(sc, -1)
        top2 = torch.topk(sc, 2, dim=-1).values
        out["logprob"][:, k] = (sc.gather(-1, cand[:, k, :, None])[..., 0] - lse).numpy()
        out["lse"][:, k] = lse.numpy()
        out["max_logit"][:, k] = top2[..., 0].numpy()
        out["top2_gap"][:, k] = (top2[..., 0] - top2[..., 1]).numpy()
        out["argmax"][:, k] = sc.argmax(-1).numpy()
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    t0 = time.time()
    sd = synth.make_state_dict(MG.SEED)
    model, _ = MG.build_reference(sd)
    a1, a2, ids = synth.make_batch(2)
    a1t, a2t, idst = torch.from_numpy(a1), torch.from_numpy(a2), torch.from_numpy(ids)
    greedy = np.load(os.path.join(HERE, "gen.npz"))["tokens"]
    assert greedy.shape[0] == 2 and greedy.shape[1] >= L
    for step in range(MAX_SEED_STEPS + 1):
        seed = SEED0 + step
        cand = candidates(seed, greedy)
        st = reference_stats(model, a1t, a2t, idst, cand)
        gap = float(st["top2_gap"].min())
        print(f"seed {seed}: min top-2 gap over {st['top2_gap'].size} positions {gap:.5f} ({time.time() - t0:.1f}s)")
        if gap >= MIN_GAP:
            break
    else:
        raise SystemExit(f"no seed in {SEED0}..{SEED0 + MAX_SEED_STEPS} keeps every top-2 gap >= {MIN_GAP}")
    assert float(st["top2_gap"].min()) >= MIN_GAP
    # candidate 0 is the greedy path: teacher forcing reproduces it
    assert np.array_equal(st["argmax"][:, 0], greedy[:, :L])
    lens = np.tile(np.asarray(CAND_LEN, dtype=np.int32), (2, 1))
    np.savez_compressed(os.path.join(HERE, "score.npz"), seed=seed, seed0=SEED0, input_ids=ids, cand_ids=cand.numpy(), cand_len=lens,
                        logprob=st["logprob"], lse=st["lse"], max_logit=st["max_logit"], top2_gap=st["top2_gap"], argmax=st["argmax"])
    print(f"score.npz: candidate sums {np.where(np.arange(L) < lens[..., None], st['logprob'], 0).sum(-1).tolist()} ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
