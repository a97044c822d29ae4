// sail_trace_sets.hip — the precompiled trace kernels: sail_trace.hip's path loop instantiated for the four plugin sets
// (every plugin, the Cornell box, the rooms, the pre-cull kernel), each as a plain, a _grouped and their _masked
// instances, and sail_launch_trace, which picks among them. No part of a run-time kernel's text: an edit here leaves
// the run-time kernels' cache keys alone.
#include <hip/hip_runtime.h>
#include "sail_trace.hip"

// the precompiled pair and its _masked pair
#define SAIL_TRACE_KERNELS(name, waves, cull, ks, km, kt, kl, nt, gnt, fam)              \
  SAIL_TRACE_KERNELS_NS(name, waves, cull, ks, km, kt, kl, nt, gnt, fam, 1, false)       \
  SAIL_TRACE_KERNELS_NS(name##_masked, waves, cull, ks, km, kt, kl, nt, gnt, fam, 1, true)
// every plugin (any scene of fewer than 8 primitives outside the two sets below)
#define SAIL_GENERIC_WAVES 6
SAIL_TRACE_KERNELS(sail_trace_kernel, SAIL_GENERIC_WAVES, false, ~0u, ~0u, ~0u, ~0u, 256, 256, false)
// the README Cornell box plugin set (C1/C2/C5): Cube + Sphere + Cornellbox, Matte + Mirror, uniform colours
#define SAIL_CORNELL_WAVES 8
#define SAIL_CORNELL_NT 256
#define SAIL_CORNELL_GROUP_NT 256
SAIL_TRACE_KERNELS(sail_trace_kernel_cornell, SAIL_CORNELL_WAVES, false, SAIL_KSET_CORNELL_SHAPES, SAIL_KSET_CORNELL_MATS,
                   SAIL_KSET_CORNELL_TEX, SAIL_KSET_CORNELL_LIGHTS, SAIL_CORNELL_NT, SAIL_CORNELL_GROUP_NT, false)
// rooms of boxes, spheres and rectangle lights (C3 materials demo, UI demo); occupancy measured 5/6/7/8 waves
#define SAIL_ROOM_WAVES 7
#define SAIL_ROOM_NT 256
#define SAIL_ROOM_GROUP_NT 256
SAIL_TRACE_KERNELS(sail_trace_kernel_room, SAIL_ROOM_WAVES, false, SAIL_KSET_ROOM_SHAPES, SAIL_KSET_ROOM_MATS,
                   SAIL_KSET_ROOM_TEX, SAIL_KSET_ROOM_LIGHTS, SAIL_ROOM_NT, SAIL_ROOM_GROUP_NT, true)
// the pre-cull kernel serves scenes with many primitives (C4); 1,024-thread workgroups (16 x 64 strips)
#define SAIL_CULL_WAVES 8
#define SAIL_CULL_NT 1024
#define SAIL_CULL_GROUP_NT 1024
SAIL_TRACE_KERNELS(sail_trace_kernel_cull, SAIL_CULL_WAVES, true, ~0u, ~0u, ~0u, ~0u, SAIL_CULL_NT, SAIL_CULL_GROUP_NT, false)

// ---- host launch wrapper (called by sail_capi.cpp) -----------------------------------------------------------------
hipError_t sail_launch_trace(const SailTraceArgs& A, int blocks, hipStream_t s) {
  const bool g = A.sampleGroups > 1, m = A.tileMap != nullptr;
#define SAIL_LAUNCH(k) \
  hipLaunchKernelGGL(m ? (g ? k##_masked##_grouped : k##_masked) : (g ? k##_grouped : k), dim3(blocks), dim3(256), 0, s, A)
  // ungrouped launches of an NT-thread kernel: blocks = ownedTiles * 16 of 256 threads -> ownedTiles * 4096 / NT
#define SAIL_LAUNCH_NT(k, nt, gnt)                                                              \
  do {                                                                                          \
    if (g) hipLaunchKernelGGL(m ? k##_masked##_grouped : k##_grouped, dim3(blocks * 256 / (gnt)), dim3(gnt), 0, s, A); \
    else hipLaunchKernelGGL(m ? k##_masked : k, dim3(blocks * 256 / (nt)), dim3(nt), 0, s, A);                     \
  } while (0)
  if (A.kernelSet == SAIL_KSET_CORNELL) SAIL_LAUNCH_NT(sail_trace_kernel_cornell, SAIL_CORNELL_NT, SAIL_CORNELL_GROUP_NT);
  else if (A.kernelSet == SAIL_KSET_ROOM) SAIL_LAUNCH_NT(sail_trace_kernel_room, SAIL_ROOM_NT, SAIL_ROOM_GROUP_NT);
  else if (A.cullPrims) SAIL_LAUNCH_NT(sail_trace_kernel_cull, SAIL_CULL_NT, SAIL_CULL_GROUP_NT);
  else SAIL_LAUNCH(sail_trace_kernel);
#undef SAIL_LAUNCH
#undef SAIL_LAUNCH_NT
  return hipGetLastError();
}
