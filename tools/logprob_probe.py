#!/usr/bin/env python3
"""Developer tool (GPU box): what log-probs of the generated tokens cost inside the decode step (generate(return_logprobs=True),
include/mellow_hip.h mellow_generate_scored).  One engine, f32x3 unless MELLOW_PRECISION says otherwise, max_len 64, fixed length,
B = 32 / 64 / 128 (or the batch sizes given); the four modes are alternated and the best of 5 passes each is reported:
  decode ms per step: greedy, greedy + log-probs, sampled (top_p 0.9, T 1.0), sampled + log-probs;
  the route it replaces: generate() followed by score() of the returned tokens, host clock around both calls, against one
  generate(return_logprobs=True) call.
--out FILE writes the table as JSON (profiles/logprob_probe.json).  Under `rocprofv3 --kernel-trace --stats` it also gives the
head's and the arg-max kernel's own time in both variants (the kernel names carry the template arguments)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _opts import engine_options  # noqa: E402  (--opt KEY=VALUE -> engine options)
OPTS = engine_options()
import numpy as np  # noqa: E402
from mellow_amd import synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

L = 64
args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i: i + 2]
eng = Engine(device=0, precision=os.environ.get("MELLOW_PRECISION", "f32x3"), options=OPTS)
eng.load_state_dict(synth.make_state_dict(0))
MODES = (("greedy", {}), ("greedy_lp", dict(return_logprobs=True)),
         ("sampled", dict(do_sample=True, top_p=0.9, temperature=1.0, seed=1234)),
         ("sampled_lp", dict(do_sample=True, top_p=0.9, temperature=1.0, seed=1234, return_logprobs=True)))
rows = []
for B in [int(b) for b in (args or ["32", "64", "128"])]:
    a1, a2, ids = synth.make_batch(B)
    a1d, a2d, idsd = eng._f32(a1), eng._f32(a2), eng._i32(ids)
    dec = {m: [] for m, _ in MODES}
    wall = {"generate_lp": [], "generate_then_score": []}
    for _ in range(5):
        for mode, kw in MODES:
            t0 = time.perf_counter()
            r = eng.generate(a1d, a2d, idsd, max_len=L, stop_id=0, ignore_stop=True, **kw)
            t1 = time.perf_counter()
            dec[mode].append(eng.last_phase_ms()["decode_ms"] / (L - 1))
            if mode == "greedy_lp":
                wall["generate_lp"].append((t1 - t0) * 1e3)
        t0 = time.perf_counter()
        toks, *_ = eng.generate(a1d, a2d, idsd, max_len=L, stop_id=0, ignore_stop=True)
        eng.score(a1d, a2d, idsd, toks[:, None, :], np.full((B, 1), L))
        wall["generate_then_score"].append((time.perf_counter() - t0) * 1e3)
    res = {m: min(v) for m, v in dec.items()}
    res.update({k: min(v) for k, v in wall.items()})
    res["spread_greedy"] = [min(dec["greedy"]), max(dec["greedy"])]
    res["B"] = B
    rows.append(res)
    g, gl, s, sl = res["greedy"], res["greedy_lp"], res["sampled"], res["sampled_lp"]
    print(f"B {B:4d}  decode ms/step  greedy {g:.4f} (passes {res['spread_greedy'][0]:.4f}-{res['spread_greedy'][1]:.4f})  + log-probs {gl:.4f} "
          f"(+{(gl - g) * 1e3:.1f} us, x{gl / g:.4f})  sampled {s:.4f}  + log-probs {sl:.4f} (+{(sl - s) * 1e3:.1f} us, x{sl / s:.4f})", flush=True)
    print(f"        call ms  generate(return_logprobs) {res['generate_lp']:.2f}  generate + score {res['generate_then_score']:.2f}  "
          f"(x{res['generate_lp'] / res['generate_then_score']:.3f})", flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"precision": eng.precision, "max_len": L, "best_of": 5, "rows": rows}, f, indent=1)
        f.write("\n")
