// sail_kernels.hip — the library's precompiled device code as ONE translation unit, so libsail_hip.so carries one
// gfx950 code object; each file includes what it uses, and the order below is only the order of the kernels in it.
#include "sail_noise.hip"
#include "sail_denoise.hip"
#include "sail_tfilter.hip"
#include "sail_trace_sets.hip"
#include "sail_wavefront.hip"
#include "sail_frame.hip"
#include "sail_temporal.hip"
#include "sail_albedo.hip"
#include "sail_guides.hip"
