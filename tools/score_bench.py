#!/usr/bin/env python3
"""Scoring benchmark: Engine.score (the fused log-softmax head, candidates assembled on the device) against the route the
engine offered before it -- prefix + cat + lm_forward_logits + torch log_softmax + gather -- for the same numbers.

    python tools/score_bench.py [--precision f32x3|f32|fp8] [--reps 7] [--out profiles/score_bench.json]
    python tools/score_bench.py --precision fp8 --structured      # teacher-forced |d logprob| of the fp8 engine vs f32x3

Shapes: B = 32, K = 4, L = 16 and B = 32, K = 1, L = 64 on the seeded synthetic checkpoint and batch.  Every call ends in a
drained engine stream and a device synchronise, so a call's time is the host clock around it; both routes are warmed, then
alternated, and the median of the repetitions is reported with min / max.  The head phase comes from a separate profiled
pass (family "lm_head_all_positions": HIP events on the engine's stream; for the old route the torch log_softmax + gather is
added from torch events).  Bytes are computed from the shapes.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _opts import engine_options  # noqa: E402

from mellow_amd import spec, synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

SHAPES = ((32, 4, 16), (32, 1, 64))
V = 49152


def route_new(eng, a1, a2, ids, cand, lens):
    return eng.score(a1, a2, ids, cand, lens)[0]


def route_old(eng, a1, a2, ids, cand, lens, ev=None):
    B, K, L = cand.shape
    prefix = eng.prefix(a1, a2, ids)
    emb = eng.embed_tokens(cand[:, :, : L - 1]) if L > 1 else torch.empty((B, K, 0, spec.D_PROJ), device=eng.tdev)
    seq = torch.cat((prefix[:, None].expand(B, K, spec.PREFIX_LEN, spec.D_PROJ), emb), 2).reshape(B * K, spec.PREFIX_LEN + L - 1, spec.D_PROJ)
    logits = eng.lm_forward_logits(seq, from_pos=spec.PREFIX_LEN - 1)
    if ev:
        ev[0].record()
    lp = torch.log_softmax(logits, -1).gather(-1, cand.reshape(B * K, L, 1).long())[..., 0]
    if ev:
        ev[1].record()
    return lp.reshape(B, K, L).cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def head_ms(eng, fn):
    eng.prof_enable(True)
    eng.prof_reset()
    fn()
    ms = eng.prof_report()["lm_head_all_positions"]["ms"]
    eng.prof_enable(False)
    return ms


def bench(args, opts):
    sd = synth.make_state_dict(0, structured=args.structured)
    eng = Engine(device=0, precision=args.precision, options=opts)
    eng.load_state_dict(sd)
    res = {"box": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "precision": args.precision,
           "reps": args.reps, "shapes": []}
    for B, K, L in SHAPES:
        a1, a2, ids = synth.make_batch(B)
        a1, a2, ids = eng._f32(a1), eng._f32(a2), eng._prompt_ids(ids)
        cand = torch.from_numpy(np.random.default_rng(B * 1000 + K * 100 + L).integers(0, V, (B, K, L))).to(eng.tdev)
        lens = np.full((B, K), L, dtype=np.int32)
        new = lambda: route_new(eng, a1, a2, ids, cand, lens)
        old = lambda: route_old(eng, a1, a2, ids, cand, lens)
        for _ in range(2):
            r_new, r_old = new(), old()
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        h_new = head_ms(eng, new)
        h_old = head_ms(eng, lambda: route_old(eng, a1, a2, ids, cand, lens, ev))
        torch.cuda.synchronize()
        h_old_torch = ev[0].elapsed_time(ev[1])
        rows = B * K * L
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        entry = {
            "B": B, "K": K, "L": L, "scored_positions": rows,
            "score_ms": {"median": round(m_new, 3), "min": round(min(t_new), 3), "max": round(max(t_new), 3)},
            "old_route_ms": {"median": round(m_old, 3), "min": round(min(t_old), 3), "max": round(max(t_old), 3)},
            "candidates_per_s": {"score": round(B * K / m_new * 1e3, 1), "old_route": round(B * K / m_old * 1e3, 1)},
            "head_phase_ms": {"score": round(h_new, 3), "old_route": round(h_old + h_old_torch, 3),
                              "old_route_gemm": round(h_old, 3), "old_route_log_softmax_gather": round(h_old_torch, 3)},
            # the head's HBM writes, from the shapes: partials (768 groups x 12 B) + log-prob + arg-max per position, against the
            # logits and their log_softmax (vocab x 4 B each) + the gathered value
            "head_bytes_written_per_position": {"score": V // 64 * 12 + 4 + 8, "old_route": 2 * V * 4 + 4},
            "max_abs_diff_between_routes": float(np.abs(r_new - r_old).max()),
        }
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    eng.close()
    return res


def fp8_distance(args, opts):
    """teacher-forced |d logprob| of the fp8 engine against the f32x3 engine over the 32 x 64 greedy positions (f32x3 tokens) of
    the structured checkpoint: the deterministic instrument for the fp8 mode (no token coin flips)"""
    sd = synth.make_state_dict(0, structured=True)
    ref = Engine(device=0, precision="f32x3")
    ref.load_state_dict(sd)
    a1, a2, ids = synth.make_batch(32)
    toks, *_ = ref.generate(a1, a2, ids, max_len=64, stop_id=-1)
    lens = np.full((32, 1), 64, dtype=np.int32)
    lp_ref, _, am_ref = ref.score(a1, a2, ids, toks[:, None, :], lens)
    ref.close()
    e8 = Engine(device=0, precision="fp8", options=opts)
    e8.load_state_dict(sd)
    lp8, _, am8 = e8.score(a1, a2, ids, toks[:, None, :], lens)
    e8.close()
    d = np.abs(lp8.astype(np.float64) - lp_ref)
    out = {"box": torch.cuda.get_device_name(0), "checkpoint": "structured", "positions": int(d.size),
           "fp8_vs_f32x3_abs_dlogprob": {"mean": float(d.mean()), "max": float(d.max()), "median": float(np.median(d))},
           "f32x3_mean_logprob_of_its_greedy_tokens": float(lp_ref.mean()),
           "teacher_forced_argmax_agreement": float((am8 == am_ref).mean())}
    print(json.dumps(out), flush=True)
    return out


def main():
    opts = engine_options()
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32x3", choices=("f32x3", "f32", "fp8"))
    ap.add_argument("--structured", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/score_bench.py needs an MI355X: no GPU is visible")
    res = fp8_distance(args, opts) if (args.precision == "fp8" and args.structured) else bench(args, opts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
