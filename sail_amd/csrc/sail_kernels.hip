// sail_kernels.hip — the library's precompiled device code as ONE translation unit, so libsail_hip.so carries one
// gfx950 code object (tests/test_jit_compile.py disassembles "the" code object of the library). Each kernel file stays
// its own source and compiles on its own too (the study and variant builds under tools/ do that); sail_trace.hip is not
// touched by what is added here: its text is embedded in the library and hashed into every run-time kernel's cache key.
// sail_post.h (what the post-processing kernels share), sail_noise.hip, sail_denoise.hip and sail_tfilter.hip come first:
// they define no macro (sail_post.h includes sail_math.h, which sail_trace.hip includes itself), so the trace kernels
// compile exactly as they do alone. sail_temporal.hip comes last: its G-buffer pass calls sail_trace.hip's mkRay, primT and
// constRow, and nothing it declares is seen by the trace kernels. sail_albedo.hip follows it for the same reason: its
// kernel calls mkRay, primT, constRow and hitRecordU.
#include "sail_post.h"
#include "sail_noise.hip"
#include "sail_denoise.hip"
#include "sail_tfilter.hip"
#include "sail_trace.hip"
#include "sail_temporal.hip"
#include "sail_albedo.hip"
