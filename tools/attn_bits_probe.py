#!/usr/bin/env python3
"""Developer tool (GPU box): the raw bits of the prefill and window attention kernels, for a comparison between two builds of the
library (prefill_attn.hip and the window attention of encoder.hip against the parent commit's).

    python tools/attn_bits_probe.py --out FILE.npz
    python tools/attn_bits_probe.py --compare A.npz B.npz

One side per process: MELLOW_HIP_LIB=path selects the library of a run.  It stores as uint32 words every output of
debug_prefill_attn and debug_window_attn (the whole device buffer, which held 0xFF bytes before the launch) on the cases of
tests/attn_ref.py (imported, not copied):
  - PREFILL_SHAPES in variants 0 .. 3 (2 and 3 on the bf16-rounded inputs), plain form, and the APB form where the tap has it
    (variants 0 and 1);
  - PAST_CASES (B = 2) in variants 0 and 1, both forms: the launches for the queries from qpos0 on;
  - WINDOW_SHAPES with fp32 input in both forms and with bf16 input in the plain form (the tap has no other).
  - the decode attention and its o_proj merge (debug_dec_attn) on the cases of tests/dec_attn_ref.py with both producers (fused 0 / 1):
    partials, att_ml, the appended position of the pages, x_new, xmidF, xmidF16, ssq; and the F3 images on one case per
    row-block count.  A library that predates the tap is reported and its side holds the other tensors only.
The MXFP8 form of the prefill attention has no tap: the lm_prefill logits of the fp8 engines in tools/decode_bits_probe.py cover it.
`--compare` is tools/gemm_bits_probe.py's: exit status 0 only if every word is equal."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402


def run(out):
    import attn_ref as R
    from mellow_amd.engine import Engine
    res = {}

    def keep(name, t):
        res[name] = np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).ravel()

    eng = Engine(device=0)
    for B, T, Tmax in R.PREFILL_SHAPES:
        for variant in (0, 1, 2, 3):
            q, k, v = R.prefill_inputs(B, T, Tmax, variant >= 2)
            for form in ((0, 1) if variant < 2 else (0,)):
                keep(f"prefill ({B}, {T}, {Tmax}) variant {variant} form {form}", eng.debug_prefill_attn(q, k, v, T, variant=variant, out_form=form))
    print(f"prefill shapes: {len(res)} tensors so far", flush=True)
    for T, qpos0 in R.PAST_CASES:
        q, k, v = R.prefill_inputs(2, T, T + 7)      # (the pages of the test module)
        for variant in (0, 1):
            for form in (0, 1):
                keep(f"past (T, qpos0) = ({T}, {qpos0}) variant {variant} form {form}",
                     eng.debug_prefill_attn(q[:, qpos0:], k, v, T, variant=variant, qpos0=qpos0, out_form=form))
    print(f"past cases: {len(res)} tensors so far", flush=True)
    for windows, nH, nW in R.WINDOW_SHAPES:
        for in16 in (False, True):
            c = R.window_case(windows, nH, nW, in16)
            for form in ((0,) if in16 else (0, 1)):      # (the tap has no APB form of the bf16-input kernel: the engine never launches it)
                keep(f"window ({windows}, {nH}, {nW}) in16 {int(in16)} form {form}", eng.debug_window_attn(c["qkv"], c["bias"], c["mask"], in16=in16, out_form=form))
    if hasattr(eng.lib, "mellow_debug_dec_attn"):
        import dec_attn_ref as D
        for cid in D.CASE_IDS:
            c = D.case(cid)
            for fused in (False, True):
                i = D.inputs(cid, fused)
                for x3 in ((False, True) if cid in ("b-B1-T512-pos224-end449-ts2-fp32", "d-B64-T512-pos447-end512-ts1-fp32") else (False,)):
                    o = eng.debug_dec_attn(i["slabs"], i["x_mid"] if fused else i["x_new"], i["K"], i["V"], pos=c.pos, ctx_end=c.ctx_end, ts=c.ts,
                                           fused=fused, kv16=c.kv16, ssq1=None if fused else i["ssq1"], down=i["down"] if fused else None,
                                           rope_cur=i["rope_cur"], eps=i["eps"], Wo=i["Wo"], want_x3=x3)
                    for name in ("att", "ml", "k", "v", "xnew", "xmid", "x16", "ssq"):      # (of the pages: position pos, the append)
                        keep(f"decode {cid} fused {int(fused)} x3 {int(x3)} {name}", o[name][:, :, c.pos].contiguous() if name in ("k", "v") else o[name])
        print(f"decode attention cases: {len(res)} tensors so far", flush=True)
    else:
        print("this library predates mellow_debug_dec_attn: no decode attention tensors on this side", flush=True)
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
