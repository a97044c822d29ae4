#!/bin/sh
# Builds sail_amd/csrc as of git revision REV into sail_amd/lib/variants/libsail_hip_NAME.so (with its own embedded
# run-time kernel sources), the control for an A/B variant run of the working tree (tools/variant_bench.py).
# Usage: tools/rev_build.sh REV NAME
set -e
cd "$(dirname "$0")/.."
ROOT=$(pwd)
REV=$1; NAME=$2
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function --offload-arch=gfx950"
d=sail_amd/build/study/$NAME/csrc
rm -rf sail_amd/build/study/$NAME && mkdir -p $d sail_amd/lib/variants && ln -sfn ../../../include sail_amd/build/study/include
for f in $(git ls-tree --name-only $REV sail_amd/csrc/); do git show $REV:$f > $d/$(basename $f); done
git show $REV:sail_amd/gen_jit_src.py > $d/gen_jit_src.py
python3 $d/gen_jit_src.py $d/sail_jit_src.cpp $d
PIDS=""
# the device code is one translation unit (sail_kernels.hip, whatever files the revision lists in it); revisions before
# the noise estimate have sail_trace.hip alone
DEV=sail_trace.hip; [ -f $d/sail_kernels.hip ] && DEV=sail_kernels.hip
# the host code: every *.cpp the revision has, the generated sail_jit_src.cpp among them (written above, compiled once)
OBJS=""
for s in $d/$DEV $d/*.cpp; do
  $HIPCC $COMMON -c $s -o ${s%.*}.o & PIDS="$PIDS $!"
  OBJS="$OBJS ${s%.*}.o"
done
for p in $PIDS; do wait $p; done
$HIPCC -shared -fPIC --offload-arch=gfx950 $OBJS \
  -o sail_amd/lib/variants/libsail_hip_$NAME.so -ldl -lpthread
echo "built $NAME from $REV"
