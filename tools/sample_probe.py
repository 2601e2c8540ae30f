#!/usr/bin/env python3
"""Developer tool (GPU box): decode ms per step of greedy vs seeded nucleus sampling (do_sample=True, top_p 0.9, T 1.0) on the
same engine at B = 32, 64, 128 (max_len 64, fixed length, best of 3 passes each).  Under `rocprofv3 --kernel-trace --stats`
it also gives the sampler's own time (dec_sample_kernel) and that of the lm_head with its logits store."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _opts import engine_options  # noqa: E402  (--opt KEY=VALUE -> engine options)
OPTS = engine_options()
from mellow_amd import synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

L = 64
eng = Engine(device=0, precision=os.environ.get("MELLOW_PRECISION", "f32x3"), options=OPTS)
eng.load_state_dict(synth.make_state_dict(0))
for B in [int(b) for b in (sys.argv[1:] or ["32", "64", "128"])]:
    a1, a2, ids = synth.make_batch(B)
    a1d, a2d, idsd = eng._f32(a1), eng._f32(a2), eng._i32(ids)
    res = {}
    for mode, kw in (("greedy", {}), ("sampled", dict(do_sample=True, top_p=0.9, temperature=1.0, seed=1234))):
        dec = []
        for _ in range(3):
            eng.generate(a1d, a2d, idsd, max_len=L, stop_id=0, ignore_stop=True, **kw)
            dec.append(eng.last_phase_ms()["decode_ms"] / (L - 1))
        res[mode] = min(dec)
    g, s = res["greedy"], res["sampled"]
    print(f"B {B:4d}  decode ms/step  greedy {g:.4f}  sampled {s:.4f}  (+{(s - g) * 1e3:.1f} us, +{100 * (s / g - 1):.1f} %)", flush=True)
