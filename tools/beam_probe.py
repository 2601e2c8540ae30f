#!/usr/bin/env python3
"""Developer tool (GPU box): what beam search costs inside the decode step (generate(num_beams=k), include/mellow_hip.h
mellow_generate_beam).  One engine, f32x3 unless MELLOW_PRECISION says otherwise, max_len 64, fixed length (ignore_stop), k = 4 and
N = B * k = 32 / 64 / 128 rows (or the row counts given); the three modes are alternated and the best of 5 passes each is reported:
  decode ms per step: a beam call of N rows next to the greedy and the sampled (top_p 0.9, T 1.0) step of a plain call of N rows;
  the bytes the reorder moved per step, from the parent table of the call: a row whose parent at step s is another row reads and
  writes s positions x 30 layers x 3 kv heads x 64 floats of K and of V, once into the staging buffer and once out of it.
--out FILE writes the table as JSON (profiles/beam_probe.json).  Under `rocprofv3 --kernel-trace --stats` it also gives the own
time of beam_rows_kernel, beam_merge_kernel and the two beam_kv_move_kernel launches."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _opts import engine_options  # noqa: E402  (--opt KEY=VALUE -> engine options)
OPTS = engine_options()
import numpy as np  # noqa: E402
from mellow_amd import synth  # noqa: E402
from mellow_amd.engine import Engine  # noqa: E402

L, K = 64, 4
args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i: i + 2]
eng = Engine(device=0, precision=os.environ.get("MELLOW_PRECISION", "f32x3"), options=OPTS)
eng.load_state_dict(synth.make_state_dict(0))
rows = []
for N in [int(b) for b in (args or ["32", "64", "128"])]:
    B = N // K
    big = tuple(eng._f32(x) if i < 2 else eng._i32(x) for i, x in enumerate(synth.make_batch(N)))
    small = tuple(x[:B].contiguous() for x in big)
    modes = (("greedy", big, {}), ("sampled", big, dict(do_sample=True, top_p=0.9, temperature=1.0, seed=1234)),
             ("beam", small, dict(num_beams=K)))
    dec = {m: [] for m, _, _ in modes}
    for _ in range(5):
        for mode, batch, kw in modes:
            eng.generate(*batch, max_len=L, stop_id=0, ignore_stop=True, **kw)
            dec[mode].append(eng.last_phase_ms()["decode_ms"] / (L - 1))
    par = eng.last_beam["parent"]                       # [L][N]
    moved = par[1:] != (np.arange(N) % K)[None, :]      # (step, row): the parent is another row
    pos = (np.arange(1, L)[:, None] * moved).sum()      # positions moved over the call
    per_step = float(pos) * 30 * 3 * 64 * 4 * 2 * 4 / (L - 1)     # K and V, gather + scatter, read + write
    res = {m: min(v) for m, v in dec.items()}
    res.update(rows=N, examples=B, k=K, spread_greedy=[min(dec["greedy"]), max(dec["greedy"])], spread_beam=[min(dec["beam"]), max(dec["beam"])],
               moved_row_steps=int(moved.sum()), row_steps=int(moved.size), reorder_bytes_per_step=per_step)
    rows.append(res)
    g, s, b = res["greedy"], res["sampled"], res["beam"]
    print(f"N {N:4d} (B {B} x k {K})  decode ms/step  greedy {g:.4f} (passes {res['spread_greedy'][0]:.4f}-{res['spread_greedy'][1]:.4f})  "
          f"sampled {s:.4f}  beam {b:.4f} (passes {res['spread_beam'][0]:.4f}-{res['spread_beam'][1]:.4f}; +{(b - g) * 1e3:.1f} us, x{b / g:.3f} of greedy)  "
          f"rows moved {res['moved_row_steps']} of {res['row_steps']} (row, step) pairs, {per_step / 1e6:.2f} MB of traffic per step", flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"precision": eng.precision, "max_len": L, "k": K, "best_of": 5, "rows": rows}, f, indent=1)
        f.write("\n")
