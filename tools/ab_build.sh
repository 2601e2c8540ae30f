#!/bin/bash
# Developer tool: build a second copy of libmellow_hip.so with extra -D flags for same-box A/B runs.
#   tools/ab_build.sh variantB "-DMELLOW_LM_WAVES=4"   ->  mellow_amd/lib/ab/libmellow_hip_variantB.so
# Use it with MELLOW_HIP_LIB=mellow_amd/lib/ab/libmellow_hip_variantB.so python tools/decode_probe.py
# (sources, flags and per-file flags are those of mellow_amd/csrc/build.py: this is that build with an object directory of its own)
set -e
cd "$(dirname "$0")/.."
name=$1; flags=$2
tmp=$(mktemp -d)
MELLOW_EXTRA_FLAGS="$flags" python mellow_amd/csrc/build.py --objdir "$tmp" --out "mellow_amd/lib/ab/libmellow_hip_$name.so"
rm -rf "$tmp"
