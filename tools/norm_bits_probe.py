#!/usr/bin/env python3
"""Developer tool (GPU box): the raw bits of the norm kernels and of the model paths that run them, for a comparison between two
builds of the library (norm.hip against the parent commit's encoder.hip).

    python tools/norm_bits_probe.py --out FILE.npz
    python tools/norm_bits_probe.py --compare A.npz B.npz

One side per process: MELLOW_HIP_LIB=path selects the library of a run.  It stores as raw uint32 / uint8 words
  - every output of debug_norm (the whole device buffer, which held 0xFF bytes before the launch) on the cases of tests/norm_ref.py
    (imported, not copied): "layernorm" over LN_C x (LN_M and LN_MAPPED) in forms 0, 1, 2 and at C = 576 in form 0; "merge" over
    MERGE_CASES in form 0; "rmsnorm" over RMS_C x RMS_M with eps 1e-5 and eps 0 in forms 0, 1, 2; "none" (the two stand-alone
    producers) over PLAIN_CASES in forms 1 and 2 (the tap has no form 0 of it: nothing would be launched);
  - the encoder output and the lm_prefill logits of an f32x3 engine and of an fp8 engine on the synthetic state dict, each with
    prefill_fuse_norm = 0 (the *_apb kernels run inside the LM) and with the default.
`--compare` is tools/gemm_bits_probe.py's: exit status 0 only if every word is equal -- nothing in these kernels may change a sum,
so not even the sign of a zero may differ."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

MODEL_B = 2


def run(out):
    import gemm_ref as G
    import norm_ref as N
    from mellow_amd import synth
    from mellow_amd.engine import Engine
    res = {}

    def keep(name, o):
        for k, t in (o.items() if isinstance(o, dict) else [("out", o)]):
            a = np.ascontiguousarray(t.cpu().numpy())
            res[f"{name}|{k}"] = a.view(np.uint8 if a.dtype == np.uint8 else np.uint32).ravel()

    def forms(name, x, fs, **kw):
        for form in fs:
            keep(f"{name} form {form}", eng.debug_norm(x, form=form, **kw))

    eng = Engine(device=0)
    for C in N.LN_C + (576,):
        for M, mapped in [(M, None) for M in N.LN_M] + [(m[2], m[:2]) for m in N.LN_MAPPED]:
            x, w, b = N.rows(M, C)
            rm = None if mapped is None else G.window_map(*mapped)[0]
            forms(f"layernorm C={C} M={M} map={mapped}", x, (0,) if C == 576 else (0, 1, 2), op="layernorm", w=w, b=b, row_map=rm)
    for n, R, Cin in N.MERGE_CASES:
        x, w, b = N.merge_tokens(n, R, Cin)
        forms(f"merge ({n}, {R}, {Cin})", x, (0,), op="merge", w=w, b=b, n=n, R=R)
    for eps in (1e-5, 0.0):
        for C in N.RMS_C:
            for M in N.RMS_M:
                x, w, _ = N.rows(M, C, zero_row=eps != 0.0)
                forms(f"rmsnorm C={C} M={M} eps={eps}", x, (0, 1, 2), op="rmsnorm", w=w, eps=eps)
    for M, C in N.PLAIN_CASES:
        forms(f"none ({M}, {C})", N.plain_rows(M, C), (1, 2), op="none")          # (form 0 of "none" would launch nothing: the tap refuses it)
    eng.close()
    print(f"debug_norm: {len(res)} tensors", flush=True)
    sd = synth.make_state_dict(0)
    a1, a2, ids = synth.make_batch(MODEL_B)
    for precision in ("f32x3", "fp8"):
        for options in ({"prefill_fuse_norm": 0}, {}):
            eng = Engine(device=0, precision=precision, options=options)
            eng.load_state_dict(sd)
            tag = f"{precision} {'prefill_fuse_norm=0' if options else 'default'}"
            keep(f"encode {tag}", eng.encode(a1))
            keep(f"lm_prefill {tag}", eng.lm_prefill(eng.prefix(a1, a2, ids)))
            print(f"{tag}: encoder output and prefill logits kept", flush=True)
            eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, library=np.array(os.environ.get("MELLOW_HIP_LIB", "default")), **res)
    print(f"wrote {out}: {len(res)} tensors, {sum(v.size for v in res.values())} words", flush=True)


if __name__ == "__main__":
    from gemm_bits_probe import compare
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE", help="run this side and write its bits here")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files written by --out")
    args = ap.parse_args()
    if bool(args.out) == bool(args.compare):
        ap.error("give --out FILE or --compare A B")
    sys.exit(compare(*args.compare) if args.compare else run(args.out))
