#!/usr/bin/env python3
"""Developer tool (GPU box): the raw bits of the f32x3 tile GEMMs and of the prefill logits, for a comparison between two builds of
the library (gemm_bf16x3.hip and gemm_fp8.hip against the parent commit's).

    python tools/gemm_bits_probe.py --out FILE.npz
    python tools/gemm_bits_probe.py --compare A.npz B.npz

One side per process: MELLOW_HIP_LIB=path selects the library of a run.  It stores as uint32 words
  - every output of debug_gemm_epi (C, the APB image, ssq, q and the K / V pages; each is filled with 0xFF bytes before the launch)
    for kernels 16 and 17 on the cases of tests/test_gpu_gemm.py: the linear shapes and variants with the hand-over outputs, SwiGLU
    (Nw = 3072: the XCD-ownership tile order), QKV-RoPE, the x3w kernel with the tile kernel beside it, and split-K;
  - the lm_prefill logits of an f32x3 engine and of an fp8 engine (gemm_mx8_kernel) on the synthetic state dict.
The cases are the test module's own (imported, not copied).  `--compare` is tools/decode_bits_probe.py's report; here its exit status
is 0 only if every word is equal -- nothing in these kernels may change a sum, so not even the sign of a zero may differ."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

X3W_CASES = [(8192, 288), (8229, 384)]
SPLITK_CASES = [(33, 128, 1024, "plain"), (130, 544, 4608, "bias_sigmoid_wide"), (64, 768, 3072, "resid_in_place")]
SWIGLU_CASES = [(33, 128, 64), (129, 128, 192), (130, 3072, 64), (129, 3072, 576)]
PREFILL_B = 3


def run(out):
    import test_gpu_gemm as T
    from mellow_amd import spec, synth
    from mellow_amd.engine import Engine
    res = {}

    def keep(name, o):
        tensors = o if isinstance(o, dict) else dict(zip("qkv", o))
        for k, t in tensors.items():
            res[f"{name}|{k}"] = np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).ravel()

    eng = Engine(device=0)
    for kernel in (16, 17):
        for M, Nw, K in T.SHAPES:
            if kernel not in T.kernels_for(K):
                continue
            for variant in T.VARIANTS:
                c = T.linear_case(M, Nw, K, variant)
                hand_over = c["N"] % 64 == 0            # the APB image and ssq: whole 64-column groups only
                keep(f"linear {variant} ({M}, {Nw}, {K}) kernel {kernel}", T.run_linear(eng, c, kernel, want_c3=hand_over, want_ssq=hand_over))
        for M, Nw, K in SWIGLU_CASES:
            for rs in (False, True):
                c = T.swiglu_case(M, Nw, K, rs)
                kw = {} if c["rs"] is None else dict(rs_ssq=c["rs"][0], rs_dim=c["rs"][1], rs_eps=c["rs"][2])
                for want_c3 in (False, True):
                    keep(f"swiglu ({M}, {Nw}, {K}) rs {int(rs)} c3 {int(want_c3)} kernel {kernel}",
                         eng.debug_gemm_epi(c["A"], c["W"], kernel=kernel, epi="swiglu", want_c=not want_c3, want_c3=want_c3, **kw))
        for B, Tq, Tmax, pos0 in T.QKV_CASES:
            for K in (64, 576):
                for rs in (False, True):
                    c = T.qkv_case(B, Tq, Tmax, pos0, K, rs)
                    keep(f"qkv-rope ({B}, {Tq}, {Tmax}, {pos0}) K {K} rs {int(rs)} kernel {kernel}", T.run_qkv(eng, c, kernel, B, Tq, Tmax, pos0))
        for M, Nw, K, variant in SPLITK_CASES:
            keep(f"split-K {variant} ({M}, {Nw}, {K}) kernel {kernel}", T.run_linear(eng, T.linear_case(M, Nw, K, variant), kernel, splitk_max=8))
        print(f"kernel {kernel}: {len(res)} tensors so far", flush=True)
    for M, Nw in X3W_CASES:
        for variant in ("plain", "bias", "bias_gelu"):
            c = T.linear_case(M, Nw, 96, variant)
            keep(f"x3w {variant} ({M}, {Nw})", T.run_linear(eng, c, 17))
            keep(f"x3w {variant} ({M}, {Nw}) no_x3w", T.run_linear(eng, c, 17, no_x3w=True))
    eng.close()
    rng = np.random.default_rng(11)
    prefix = (0.25 * rng.standard_normal((PREFILL_B, spec.PREFIX_LEN, spec.D_PROJ))).astype(np.float32)
    sd = synth.make_state_dict(0)
    for precision in ("f32x3", "fp8"):
        eng = Engine(device=0, precision=precision)
        eng.load_state_dict(sd)
        logits = eng.lm_prefill(prefix).cpu().numpy()
        res[f"lm_prefill {precision} B={PREFILL_B}"] = np.ascontiguousarray(logits).view(np.uint32).ravel()
        print(f"lm_prefill {precision}: logits {logits.shape}, finite {bool(np.isfinite(logits).all())}", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, library=np.array(os.environ.get("MELLOW_HIP_LIB", "default")), **res)
    print(f"wrote {out}: {len(res)} tensors, {sum(v.size for v in res.values())} words", flush=True)


def compare(pa, pb):
    from decode_bits_probe import compare as report
    status = report(pa, pb)
    a, b = np.load(pa), np.load(pb)
    unequal = [k for k in a.files if k != "library" and not np.array_equal(a[k], b[k])]
    print(f"{len(unequal)} tensors are not bit-equal" + (": " + "; ".join(unequal[:8]) if unequal else ""))
    return 1 if status or unequal else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE", help="run this side and write its bits here")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files written by --out")
    args = ap.parse_args()
    if bool(args.out) == bool(args.compare):
        ap.error("give --out FILE or --compare A B")
    sys.exit(compare(*args.compare) if args.compare else run(args.out))
