#!/usr/bin/env python3
"""Developer tool (GPU box): the launch plan and the raw result bits of the two dense forward chains -- the HTSAT encoder and the LM
prefill -- for a comparison between two builds of the library (the host code of engine_encoder.cpp and
engine_lm.cpp against the parent commit's).

    python tools/chain_bits_probe.py --out FILE.npz
    python tools/chain_bits_probe.py --compare A.npz B.npz

One side per process: MELLOW_HIP_LIB=path selects the library of a run.  On the synthetic checkpoint at B = 3 it stores
  - the launch plan: with the profiler on (which runs the prefill as one chain), one prefix() + lm_prefill(reserve=1), then every record
    of mellow_dev_prof_dump but its time -- family, M, N, K, epi code, flops -- as int64 rows, for the configurations of PLANS;
  - result bits as raw uint32 words, for "f32", "f32x3" and "fp8": every encoder tap, encode, prefix, the lm_prefill logits and
    lm_forward_logits over all positions (the all_layers span); for "f32" and "f32x3": tokens and log-probs of
    greedy generate(max_len=4, return_logprobs=True), of num_return_sequences=2 (the to_prefix span and the fan-out; n > 1 needs a
    sampled call: do_sample=True, seed 7, top_p 0.9, temperature 0.7) and of the greedy call with two questions per example (the
    pos0 > 0 span); for "f32x3" with prefill_split = 1, 2 and 4 (one chain; parts of 2 + 1
    examples; three parts of one example): prefill logits and greedy tokens; and encode of one 11 s clip (more than 1024 frames: the
    crop path of the encoder tail, two crops).
`--compare` is tools/gemm_bits_probe.py's after a check that both files hold records of the same counts: exit status 0 only if every
word is equal -- nothing here may change a launch, so not even the sign of a zero may differ."""
import argparse
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

B = 3
TAPS = ("power", "logmel_bn", "patch", "stage0", "stage1", "stage2", "stage3", "fpx", "emb33", "proj33")
PLANS = [("f32", {}), ("f32x3", {}), ("fp8", {}), ("f32x3", {"x3_apb": 0}), ("f32x3", {"prefill_fuse_norm": 0}), ("f32x3", {"x3_attn": 0}),
         ("f32x3", {"enc_apb": 0}), ("f32x3", {"splitk": 0}), ("fp8", {"prefill_fuse_norm": 0})]
LONG_SAMPLES = 352000                # 11 s at 32 kHz: 1101 frames


def words(x):
    a = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return a.view(np.uint32).ravel()


def launch_plan(eng, a1, a2, ids):
    """every profile record of one prefix() + lm_prefill(reserve=1) but its time, one int64 row each"""
    fn = eng.lib.mellow_dev_prof_dump
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_char_p]
    eng.prof_enable(True)
    eng.prof_reset()
    eng.lm_prefill(eng.prefix(a1, a2, ids), reserve=1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "prof.csv")
        assert fn(eng.h, path.encode()) == 0
        lines = open(path).read().split("\n")[1:]
    eng.prof_enable(False)
    rows = []
    for line in lines:
        if line:
            fam, M, N, K, epi, _ms, fl = line.split(",")
            rows.append([int(fam), int(M), int(N), int(K), int(epi), int(fl)])
    return np.array(rows, dtype=np.int64)


def run(out):
    from mellow_amd import synth
    from mellow_amd.engine import Engine
    res = {}
    sd = synth.make_state_dict(0)
    a1, a2, ids = synth.make_batch(B)
    ids_q = np.stack([ids, (ids.astype(np.int64) + 1009) % 49152], axis=1).astype(ids.dtype)       # two questions per example
    long_clip = synth.make_clip(900, LONG_SAMPLES)[None]
    sampled = dict(max_len=4, stop_id=-1, return_logprobs=True, do_sample=True, seed=7, top_p=0.9, temperature=0.7)
    for precision, options in PLANS:
        tag = " ".join([precision] + [f"{k}={v}" for k, v in options.items()])
        eng = Engine(device=0, precision=precision, options=options)
        eng.load_state_dict(sd)
        if not options:
            eng.enable_taps(True)
            res[f"{tag}|encode"] = words(eng.encode(a1))
            for name in TAPS:
                res[f"{tag}|tap {name}"] = words(eng.tap(name))
            eng.enable_taps(False)
            prefix = eng.prefix(a1, a2, ids)
            res[f"{tag}|prefix"] = words(prefix)
            res[f"{tag}|lm_prefill"] = words(eng.lm_prefill(prefix, reserve=1))
            res[f"{tag}|lm_forward_logits"] = words(eng.lm_forward_logits(prefix))
            res[f"{tag}|encode long clip"] = words(eng.encode(long_clip))
            if precision != "fp8":
                greedy = dict(max_len=4, stop_id=-1, return_logprobs=True)
                calls = (("generate", (a1, a2, ids), greedy),
                         ("generate n=2", (a1, a2, ids), dict(num_return_sequences=2, **sampled)),       # (n > 1 needs a sampled call)
                         ("generate two questions", (a1, a2, ids_q), greedy))
                for name, args, kw in calls:
                    r = eng.generate(*args, **kw)
                    res[f"{tag}|{name} tokens"] = words(r[0])
                    res[f"{tag}|{name} logprobs"] = words(r[4])
        res[f"{tag}|launch plan"] = words(launch_plan(eng, a1, a2, ids))
        print(f"{tag}: {len(res)} tensors so far; launch plan of {res[f'{tag}|launch plan'].size // 12} records", flush=True)
        eng.close()
    for parts in (1, 2, 4):
        eng = Engine(device=0, precision="f32x3", options={"prefill_split": parts})
        eng.load_state_dict(sd)
        res[f"f32x3 prefill_split={parts}|lm_prefill"] = words(eng.lm_prefill(eng.prefix(a1, a2, ids), reserve=1))
        res[f"f32x3 prefill_split={parts}|generate tokens"] = words(eng.generate(a1, a2, ids, max_len=4, stop_id=-1)[0])
        print(f"f32x3 prefill_split={parts}: the prefill ran as {eng.prefill_parts()} part(s) at most", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, library=np.array(os.environ.get("MELLOW_HIP_LIB", "default")), **res)
    print(f"wrote {out}: {len(res)} tensors, {sum(v.size for v in res.values())} words", flush=True)


def compare(pa, pb):
    from gemm_bits_probe import compare as bits
    a, b = np.load(pa), np.load(pb)
    sizes = [k for k in a.files if k in b.files and a[k].shape != b[k].shape]
    for k in sizes:
        print(f"{k}: {a[k].size} words against {b[k].size}" + (" (12 words per launch record)" if k.endswith("launch plan") else ""))
    if sizes:
        return 1
    plans = [k for k in a.files if k.endswith("launch plan")]
    print(f"{len(plans)} launch plans, {sum(a[k].size // 12 for k in plans)} records: " +
          ("the same record list in every configuration" if all(np.array_equal(a[k], b[k]) for k in plans if k in b.files) else "DIFFERENT"))
    return bits(pa, pb)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE", help="run this side and write its launch plans and bits here")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files written by --out")
    args = ap.parse_args()
    if bool(args.out) == bool(args.compare):
        ap.error("give --out FILE or --compare A B")
    sys.exit(compare(*args.compare) if args.compare else run(args.out))
