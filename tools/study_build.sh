#!/bin/sh
# Study builds: a copy of sail_amd/csrc patched by tools/study.py <name> (string replacements catalogued in tools/studies.json), built
# like the product into sail_amd/lib/variants/libsail_hip_<name>.so. The product sources are never edited; results of
# a study are measured by tools/variant_bench.py and recorded in profiles/.
# Usage: tools/study_build.sh name [name ...]
set -e
cd "$(dirname "$0")/.."
ROOT=$(pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function --offload-arch=gfx950"
mkdir -p sail_amd/lib/variants
for name in "$@"; do
  d=sail_amd/build/study/$name/csrc   # two levels below the root, like sail_amd/csrc: "../../include" resolves
  rm -rf sail_amd/build/study/$name && mkdir -p $d && cp sail_amd/csrc/* $d/ && ln -sfn ../../../include sail_amd/build/study/include
  python3 tools/study.py $name $d
  # the device code as one translation unit, like the product (sail_kernels.hip lists every kernel file)
  $HIPCC $COMMON -c $d/sail_kernels.hip -o $d/sail_trace.o &
  # the host code: every *.cpp of the copy, the generated sail_jit_src.cpp among them (written first, compiled once)
  python3 sail_amd/gen_jit_src.py $d/sail_jit_src.cpp $d
  OBJS=$d/sail_trace.o
  for s in $d/*.cpp; do
    $HIPCC $COMMON -c $s -o ${s%.cpp}.o &
    OBJS="$OBJS ${s%.cpp}.o"
  done
  wait
  for o in $OBJS; do [ -s $o ] || { echo "study $name: $o failed"; exit 1; }; done
  $HIPCC -shared -fPIC --offload-arch=gfx950 $OBJS -o sail_amd/lib/variants/libsail_hip_$name.so -ldl
  echo "built $name"
done
