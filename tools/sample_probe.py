#!/usr/bin/env python3
"""Developer tool (GPU box): decode ms per step of greedy vs seeded nucleus sampling (do_sample=True, top_p 0.9, T 1.0) on the
same engine at B = 32, 64, 128 (max_len 64, fixed length, best of 3 passes each).  Under `rocprofv3 --kernel-trace --stats`
it also gives the sampler's own time (dec_sample_kernel) and that of the lm_head with its logits store.

    python tools/sample_probe.py [B ...] [--top-k K] [--min-p P] [--reps N] [--json PATH] [--dump PATH] [--lib PATH] [--tag NAME]

--top-k / --min-p: a third column, the sampled call with the candidate filters (the sampler's filtered instantiation), and its price
over the un-filtered sampled call.  --reps N: the whole measurement N times over (every repeat printed: the spread).  --lib: another
build of the library (a parent commit's, say) for a same-session A/B; a library that predates the filters measures the first two
columns.  --dump: the sampled call's tokens of every B as .npz (token equality of two builds on one seed).  --json: every figure."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _opts import engine_options  # noqa: E402  (--opt KEY=VALUE -> engine options)
OPTS = engine_options()
ap = argparse.ArgumentParser()
ap.add_argument("batches", nargs="*", type=int, default=[32, 64, 128])
ap.add_argument("--top-k", type=int, default=0)
ap.add_argument("--min-p", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--json")
ap.add_argument("--dump")
ap.add_argument("--lib")
ap.add_argument("--tag", default="")
A = ap.parse_args()
if A.lib:
    os.environ["MELLOW_HIP_LIB"] = os.path.abspath(A.lib)
import numpy as np  # noqa: E402
from mellow_amd import synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

L = 64
eng = Engine(device=0, precision=os.environ.get("MELLOW_PRECISION", "f32x3"), options=OPTS)
eng.load_state_dict(synth.make_state_dict(0))
SAMPLED = dict(do_sample=True, top_p=0.9, temperature=1.0, seed=1234)
modes = [("greedy", {}), ("sampled", SAMPLED)]
if (A.top_k or A.min_p) and hasattr(eng.lib, "mellow_generate_filters"):
    modes.append(("filtered", dict(SAMPLED, top_k=A.top_k, min_p=A.min_p)))
records, dumps = [], {}
for rep in range(A.reps):
    for B in A.batches:
        a1, a2, ids = synth.make_batch(B)
        a1d, a2d, idsd = eng._f32(a1), eng._f32(a2), eng._i32(ids)
        res = {}
        for mode, kw in modes:
            dec = []
            for _ in range(3):
                toks, *_ = eng.generate(a1d, a2d, idsd, max_len=L, stop_id=0, ignore_stop=True, **kw)
                dec.append(eng.last_phase_ms()["decode_ms"] / (L - 1))
            res[mode] = min(dec)
            if mode != "greedy":
                dumps[f"{mode}_B{B}"] = toks
        g, s = res["greedy"], res["sampled"]
        line = f"{A.tag + ' ' if A.tag else ''}B {B:4d}  decode ms/step  greedy {g:.4f}  sampled {s:.4f}  (+{(s - g) * 1e3:.1f} us, +{100 * (s / g - 1):.1f} %)"
        if "filtered" in res:
            f = res["filtered"]
            line += f"  filtered (top_k {A.top_k}, min_p {A.min_p:g}) {f:.4f}  (+{(f - s) * 1e3:.1f} us over sampled, +{100 * (f / s - 1):.1f} %)"
        print(line, flush=True)
        records.append(dict(tag=A.tag, rep=rep, B=B, top_k=A.top_k, min_p=A.min_p, **{k + "_ms_per_step": v for k, v in res.items()}))
if A.dump:
    np.savez(A.dump, **dumps)
if A.json:
    with open(A.json, "w") as fh:
        json.dump(records, fh, indent=1)
