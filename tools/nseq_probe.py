#!/usr/bin/env python3
"""Developer tool (GPU box): phase times of generate(num_return_sequences=n) against the call it replaces, the same examples
given n times in a row (include/mellow_hip.h mellow_generate_n).

    python tools/nseq_probe.py nseq      [--examples 8] [--n 4] [--max-len 64] [--passes 7] [--out FILE]
    python tools/nseq_probe.py repeated  ...

One side per process, so that the repeated side can run on another build of the library (MELLOW_HIP_LIB=path: the parent commit's
for the comparison in DESIGN.md).  f32x3 unless MELLOW_PRECISION says otherwise; sampled (seed 7, top_p 0.9, T 0.7), fixed length;
two warm-up calls, then the phase times (mellow_last_phase_ms: encode, prefill -- which holds the fan-out -- and decode) and the
host clock around the call, best and median of the passes.  Under `rocprofv3 --kernel-trace --stats` the nseq side also gives
kv_fanout_kernel's own time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from mellow_amd import synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", choices=("nseq", "repeated"))
ap.add_argument("--examples", type=int, default=8)
ap.add_argument("--n", type=int, default=4)
ap.add_argument("--max-len", type=int, default=64)
ap.add_argument("--passes", type=int, default=7)
ap.add_argument("--out")
a = ap.parse_args()

eng = Engine(device=0, precision=os.environ.get("MELLOW_PRECISION", "f32x3"))
eng.load_state_dict(synth.make_state_dict(0))
a1, a2, ids = synth.make_batch(a.examples)
kw = dict(max_len=a.max_len, stop_id=0, ignore_stop=True, do_sample=True, seed=7, top_p=0.9, temperature=0.7)
if a.side == "nseq":
    kw["num_return_sequences"] = a.n
else:
    a1, a2, ids = (np.repeat(x, a.n, axis=0) for x in (a1, a2, ids))
a1d, a2d, idsd = eng._f32(a1), eng._f32(a2), eng._i32(ids)
rec = {"encode_ms": [], "prefill_ms": [], "decode_ms": [], "call_ms": []}
for i in range(2 + a.passes):
    t0 = time.perf_counter()
    toks, *_ = eng.generate(a1d, a2d, idsd, **kw)
    t1 = time.perf_counter()
    if i >= 2:
        for k, v in eng.last_phase_ms().items():
            rec[k].append(v)
        rec["call_ms"].append((t1 - t0) * 1e3)
assert toks.shape == (a.examples * a.n, a.max_len)
res = {"side": a.side, "examples": a.examples, "n": a.n, "rows": a.examples * a.n, "max_len": a.max_len, "precision": eng.precision,
       "library": os.environ.get("MELLOW_HIP_LIB", "default"), "passes": a.passes,
       "best": {k: min(v) for k, v in rec.items()}, "median": {k: statistics.median(v) for k, v in rec.items()}}
b, m = res["best"], res["median"]
print(f"{a.side:9s} {a.examples} x {a.n} = {res['rows']} rows, max_len {a.max_len}, {eng.precision}: best (median) ms  "
      f"encode {b['encode_ms']:.2f} ({m['encode_ms']:.2f})  prefill {b['prefill_ms']:.2f} ({m['prefill_ms']:.2f})  "
      f"decode {b['decode_ms']:.2f} ({m['decode_ms']:.2f})  call {b['call_ms']:.2f} ({m['call_ms']:.2f})", flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
