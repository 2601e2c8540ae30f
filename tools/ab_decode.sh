#!/bin/bash
# Developer tool: a variant of libmellow_hip.so in which ONLY the decode files are rebuilt with extra -D flags (the other objects
# come from the release build's cache, mellow_amd/csrc/build/): seconds instead of minutes per variant.
#   tools/ab_decode.sh down6 "-DMELLOW_DOWN_WAVES=6"                ->  mellow_amd/lib/ab/libmellow_hip_down6.so (all dec_*.hip rebuilt)
#   tools/ab_decode.sh down6 "-DMELLOW_DOWN_WAVES=6" dec_gemv.hip   ->  the same, only dec_gemv.hip rebuilt (the file that reads the knob)
# Run `python mellow_amd/csrc/build.py` first.  Use with MELLOW_HIP_LIB=... python tools/decode_probe.py, or tools/ab_run.sh.
# (build.py on a copy of its object cache without those objects: the copies keep their times, so nothing else is stale)
set -e
cd "$(dirname "$0")/.."
name=$1; flags=$2; file=${3:-dec_*.hip}
tmp=$(mktemp -d)
cp -p mellow_amd/csrc/build/*.o "$tmp/"
rm -f "$tmp"/$file.o
MELLOW_EXTRA_FLAGS="$flags" python mellow_amd/csrc/build.py --objdir "$tmp" --out "mellow_amd/lib/ab/libmellow_hip_$name.so"
rm -rf "$tmp"
