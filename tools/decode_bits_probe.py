#!/usr/bin/env python3
"""Developer tool (GPU box): the raw bits of the decode step's logits, for a comparison between two builds of the library
(the GEMV kernels of dec_gemv.hip against the parent commit's).

    python tools/decode_bits_probe.py --out FILE.npz
    python tools/decode_bits_probe.py --compare A.npz B.npz

One side per process: MELLOW_HIP_LIB=path selects the library of a run.  It runs lm_prefill(reserve=6) and 4 teacher-forced
lm_decode_step calls at B = 3 and at B = 40 (two row blocks, the second with 8 rows: the BLK instantiations) on the engines below,
which together reach every GEMV kernel of a decode layer in every weight mode, in the fused and in the five-launch layer, and stores
each logits tensor as uint32 words.  The inputs are a seeded synthetic prefix and seeded tokens, the same on both sides.
Those contexts stop near 393 keys, inside the first chunk of the decode attention (448 keys per split); so each engine and batch also
runs a seeded 1000-position prefix -- beyond one chunk per split in every split count -- and, the fp8 engines,
reserve=400 on the short prefix, which puts two 32-key tiles per wave into split 0; each again followed by the teacher-forced steps.
The fp8 engines' lm_prefill logits are also what covers the MXFP8 output form of the prefill attention.
`--compare` reports per engine, batch and step whether the two files are bit-equal, otherwise how many words differ and whether they
differ in more than the sign of a zero; its exit status is 0 only if nothing but signs of zeros differs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ENGINES = [  # (name, precision, options)
    ("f32", "f32", {}),
    ("f32 decode_fuse=0", "f32", {"decode_fuse": 0}),
    ("f32x3", "f32x3", {}),
    ("fp8", "fp8", {}),
    ("fp8 fp8_prefill=0 fp8_decode_act=0 fp8_kv16=0 decode_fuse=0", "fp8", {"fp8_prefill": 0, "fp8_decode_act": 0, "fp8_kv16": 0, "decode_fuse": 0}),
    ("fp8 decode_fuse=0", "fp8", {"decode_fuse": 0}),
]
BATCHES, STEPS, RESERVE = (3, 40), 4, 6
LONG_T, RESERVE_2TILES = 1000, 400


def run(out):
    from mellow_amd import spec, synth
    from mellow_amd.engine import Engine
    rng = np.random.default_rng(11)
    prefix = (0.25 * rng.standard_normal((max(BATCHES), spec.PREFIX_LEN, spec.D_PROJ))).astype(np.float32)
    long_prefix = (0.25 * np.random.default_rng(12).standard_normal((max(BATCHES), LONG_T, spec.D_PROJ))).astype(np.float32)
    res = {}
    sd = synth.make_state_dict(0)
    for name, precision, options in ENGINES:
        eng = Engine(device=0, precision=precision, options=options)
        eng.load_state_dict(sd)
        toks = rng.integers(1, eng.lm.vocab_size, size=(max(BATCHES), STEPS)).astype(np.int32)
        runs = [("", prefix, RESERVE), (f"|T={LONG_T}", long_prefix, RESERVE)]
        if precision == "fp8":
            runs.append((f"|reserve={RESERVE_2TILES}", prefix, RESERVE_2TILES))
        for B in BATCHES:
            for tag, pre, reserve in runs:
                logits = [eng.lm_prefill(pre[:B], reserve=reserve).cpu().numpy()]
                for i in range(STEPS):
                    logits.append(eng.lm_decode_step(toks[:B, i]).cpu().numpy())
                for i, l in enumerate(logits):
                    res[f"{name}|B={B}{tag}|step={i}"] = np.ascontiguousarray(l).view(np.uint32)
                print(f"{name + tag:72s} B={B:2d}: {len(logits)} logits tensors {logits[-1].shape}, finite {all(np.isfinite(l).all() for l in logits)}", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, library=np.array(os.environ.get("MELLOW_HIP_LIB", "default")), **res)
    print(f"wrote {out}: {len(res)} tensors, {sum(v.size for v in res.values())} words", flush=True)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    print(f"A = {pa} (library {a['library']})\nB = {pb} (library {b['library']})")
    keys = [k for k in a.files if k != "library"]
    if sorted(keys) != sorted(k for k in b.files if k != "library"):
        print("the two files hold different runs")
        return 1
    bad = zeros = 0
    for k in keys:
        x, y = a[k], b[k]
        d = x != y
        n = int(d.sum())
        if n == 0:
            print(f"{k:80s} bit-equal ({x.size} words)")
            continue
        only_zero_signs = bool((((x[d] | y[d]) & 0x7fffffff) == 0).all())      # both words are a zero: they differ in its sign
        zeros += n if only_zero_signs else 0
        bad += 0 if only_zero_signs else 1
        print(f"{k:80s} {n} of {x.size} words differ: " + ("signs of exact zeros only" if only_zero_signs else "MORE than the sign of a zero"))
    print(f"{len(keys)} tensors: {bad} differ in more than signs of zeros; {zeros} words differ in the sign of a zero")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE", help="run this side and write its logits bits here")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files written by --out")
    args = ap.parse_args()
    if bool(args.out) == bool(args.compare):
        ap.error("give --out FILE or --compare A B")
    sys.exit(compare(*args.compare) if args.compare else run(args.out))
