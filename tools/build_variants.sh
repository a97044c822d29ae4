#!/bin/sh
# Builds experimental variants of libsail_hip.so (same sources, different -D flags) into sail_amd/lib/variants/.
# Usage: tools/build_variants.sh name1 "-DFLAG=1" name2 "-DFLAG=2" ...
# A flags string may start with "src=<file under csrc/>" to build that source in place of sail_trace_sets.hip (the
# precompiled plugin sets and sail_launch_trace).
set -e
cd "$(dirname "$0")/../sail_amd"
mkdir -p lib/variants build/variants
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function --offload-arch=gfx950"
# the host code: every csrc/*.cpp, and the generated sources (in build/variants/, so compiled once)
python3 gen_jit_src.py build/variants/sail_jit_src.cpp csrc
HOST=""
for s in csrc/*.cpp build/variants/sail_jit_src.cpp; do
  o=build/variants/$(basename $s .cpp).o
  $HIPCC $COMMON -c $s -o $o
  HOST="$HOST $o"
done
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  # the device code is one translation unit, like the product: sail_kernels.hip, or a copy of that list with the
  # stand-in's name in the place of sail_trace_sets.hip
  dev=csrc/sail_kernels.hip
  case "$flags" in src=*)
    src=${flags%% *}; src=${src#src=}; flags=${flags#src=$src}
    dev=build/variants/kernels_$name.hip
    sed "s/\"sail_trace_sets.hip\"/\"$src\"/" csrc/sail_kernels.hip > $dev;;
  esac
  $HIPCC $COMMON $flags -Icsrc -c $dev -o build/variants/trace_$name.o
  $HIPCC -shared -fPIC --offload-arch=gfx950 build/variants/trace_$name.o $HOST -o lib/variants/libsail_hip_$name.so -ldl
  echo "built $name ($flags)"
done
