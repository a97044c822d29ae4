#!/bin/sh
# Builds libsail_hip.so for gfx950 in-tree (sail_amd/lib/). Contraction is off everywhere: the
# kernels follow the reference's f32 expression order and the bit-defined math spec (sail_math.h).
# Also builds libsail_hip_phase.so, the same library with per-phase wave timers (-DSAIL_PHASE_TIMING=1,
# tools/phase_profile.py); tests/test_gpu_parity.py checks that it renders the same bits.
set -e
cd "$(dirname "$0")"
mkdir -p lib build
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${SAIL_ARCH:-gfx950}
COMMON="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function"
rm -f build/*.o  # a failed compile must not leave an older object to link
# the per-plugin-set kernels compiled at run time (sail_jit.cpp) carry the kernel sources in the library
python3 gen_jit_src.py build/sail_jit_src.cpp csrc
PIDS=""
# the device code: csrc/sail_kernels.hip lists every kernel file; one translation unit (one code object)
$HIPCC $COMMON --offload-arch=$ARCH -c csrc/sail_kernels.hip -o build/sail_trace.o ${SAIL_EXTRA:-} & PIDS="$PIDS $!"
$HIPCC $COMMON --offload-arch=$ARCH -DSAIL_PHASE_TIMING=1 -c csrc/sail_kernels.hip -o build/sail_trace_phase.o & PIDS="$PIDS $!"
# the host code: every csrc/*.cpp, and the generated sources (in build/, so compiled once)
HOST=""
for s in csrc/*.cpp build/sail_jit_src.cpp; do
  o=build/$(basename $s .cpp).o
  $HIPCC $COMMON --offload-arch=$ARCH -c $s -o $o & PIDS="$PIDS $!"
  HOST="$HOST $o"
done
FAIL=0
for p in $PIDS; do wait $p || FAIL=1; done
[ $FAIL -eq 0 ] || { echo "build.sh: a compile failed"; exit 1; }
for o in build/sail_trace.o build/sail_trace_phase.o $HOST; do [ -s $o ] || { echo "missing $o"; exit 1; }; done
$HIPCC -shared -fPIC --offload-arch=$ARCH build/sail_trace.o $HOST -o lib/libsail_hip.so -ldl -lpthread
$HIPCC -shared -fPIC --offload-arch=$ARCH build/sail_trace_phase.o $HOST -o lib/libsail_hip_phase.so -ldl -lpthread
