#!/usr/bin/env python3
"""Build libmellow_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python mellow_amd/csrc/build.py [--force] [--verbose] [--out PATH] [--objdir DIR]

Objects are cached under mellow_amd/csrc/build/ (git-ignored) keyed on source mtimes; the shared
library lands in mellow_amd/lib/ (git-ignored).  A variant for a same-box A/B
(tools/ab_build.sh, tools/ab_decode.sh) is this build with MELLOW_EXTRA_FLAGS="-D..." and a library path and an object
directory of its own (--out, --objdir), so that the source list and the per-file flags exist once."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LIBDIR = os.path.join(PKG, "lib")
OBJDIR = os.path.join(HERE, "build")
LIB = os.path.join(LIBDIR, "libmellow_hip.so")
SOURCES = ["gemm_f32.hip", "gemm_fp8.hip", "gemm_bf16x3.hip", "dec_attn.hip", "dec_gemv.hip", "dec_tail.hip", "dec_weights.hip", "prefill_attn.hip", "encoder.hip", "norm.hip", "stft_fft.hip", "sample.hip", "score.hip", "beam.hip", "logit_rules.hip", "constrain.hip", "stop_strings.hip", "guidance.hip", "top_logprobs.hip", "engine.cpp", "engine_weights.cpp", "engine_encoder.cpp", "engine_lm.cpp", "engine_generate.cpp", "engine_dev.cpp", "engine_taps.cpp"]
HEADERS = ["common.h", "kernels.h", "dec_common.h", "step_tail.h", "gemm_epilogue.h", "gemm_tile.h", "engine_internal.h", os.path.join("..", "..", "include", "mellow_hip.h")]
ARCH = "gfx950"
FLAGS = (["-DMELLOW_KDEBUG"] if os.environ.get("MELLOW_KDEBUG") else []) + os.environ.get("MELLOW_EXTRA_FLAGS", "").split() + ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-x", "hip"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


# Per-file flags.  VGPR-form MFMA: keep accumulators in architectural VGPRs (gfx950's register file is unified).  Without it
# the compiler parks the accumulators of the bf16 / fp8 kernels in AGPRs and copies all 64 of them in and out of VGPRs every
# loop iteration (v_accvgpr_read/write: as many VALU issue slots as the MFMAs themselves), and every `O *= alpha` of the
# flash attention is a read-modify-write through copies.
VGPR_FORM = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
FILE_FLAGS = {name: VGPR_FORM for name in os.environ.get("MELLOW_VGPR_FORM_FILES", "gemm_bf16x3.hip gemm_fp8.hip prefill_attn.hip encoder.hip").split()}
# Kernel-argument preload (gfx950): the command processor writes the first dwords of a kernel's argument block into SGPRs while it
# sets the dispatch up, so the first address computations of a launch do not wait for a scalar load from the argument buffer.
# The decode kernels take their hot pointers as leading scalar arguments for this (dec_*.hip); measured on one kernel of the
# step (gate/up, 30 of 124 launches): 48.2-48.5 -> 47.65 ms of decode per 63 steps, 0.3 us per launch.  MELLOW_KERNARG_PRELOAD=0: off.
KERNARG_PRELOAD = [] if os.environ.get("MELLOW_KERNARG_PRELOAD", "14") == "0" else ["-mllvm", "-amdgpu-kernarg-preload-count=" + os.environ.get("MELLOW_KERNARG_PRELOAD", "14")]
# every file cut from the former decode.hip, the load-time dec_weights.hip too: its kernels stay the instruction streams they were
DECODE_FILES = ["dec_attn.hip", "dec_gemv.hip", "dec_tail.hip", "dec_weights.hip"]
for _name in DECODE_FILES:
    FILE_FLAGS[_name] = FILE_FLAGS.get(_name, []) + KERNARG_PRELOAD


def build(force=False, verbose=False, out=None, objdir=None):
    lib = os.path.abspath(out) if out else LIB
    objdir = os.path.abspath(objdir) if objdir else OBJDIR
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    hdrs = [os.path.join(HERE, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    objs = []
    for src in SOURCES:
        sp = os.path.join(HERE, src)
        op = os.path.join(objdir, src + ".o")
        objs.append(op)
        if force or _stale(op, [sp] + hdrs):
            jobs.append((sp, op))

    def cc(job):
        sp, op = job
        cmd = [hipcc] + FLAGS + FILE_FLAGS.get(os.path.basename(sp), []) + ["-c", sp, "-o", op]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        return sp, r

    with cf.ThreadPoolExecutor(max_workers=max(1, min(len(jobs), int(os.environ.get("MAX_JOBS", 16))))) as ex:
        for sp, r in ex.map(cc, jobs):
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise RuntimeError(f"hipcc failed on {sp}")
            if verbose and r.stderr.strip():
                sys.stderr.write(r.stderr)
    if force or jobs or _stale(lib, objs):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError("link failed")
    return lib


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--out", metavar="PATH", help="write the library here instead of mellow_amd/lib/libmellow_hip.so")
    ap.add_argument("--objdir", metavar="DIR", help="object cache of this build instead of mellow_amd/csrc/build/")
    a = ap.parse_args()
    print(build(a.force, a.verbose, a.out, a.objdir))
