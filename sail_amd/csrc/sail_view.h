// sail_view.h — what the passes that shoot a ray per pixel or per caller's ray share: sail_pick_kernel (sail_frame.hip),
// sail_gbuffer_kernel (sail_temporal.hip), sail_albedo_kernel (sail_albedo.hip) and sail_guides_kernel (sail_guides.hip).
// Which row a pixel shows is decided here once, so the four maps agree on it by construction (tests/test_gpu_guides.py,
// test_view_passes_agree): the flat context, the pixel's ray of a sample without jitter, and the first-hit sweep. The
// f32 operation order of the ray is part of the C ABI (include/sail_hip.h, sail_gbuffer) and is checked bit for bit.
// Only those four files include this one. sail_trace.hip and what it reaches do not: their text is embedded in the
// library and hashed into every run-time kernel's cache key (sail_amd/gen_jit_src.py), so the trace kernel keeps its own
// copy of the corner interpolation, over each sample's own corners. Defines no macro.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_geom.h"
#include "sail_temporal.h"

namespace sv {

// A flat kernel's context with every member set: every shape and texture compiled in, of the materials kMats; no light
// table (nothing of the lights is reachable with ln = 0), no row or texParams copies, no pre-cull. The scene's own masks
// decide what a row shows, as in a render; a pass that only sweeps (pick, G-buffer) passes null tables and zero masks.
__device__ __forceinline__ Ctx flatCtx(const SailPrim* prims, int n, const float* texparams, int tn, uint32_t matMask,
                                       uint32_t texMask, uint32_t kMats) {
  Ctx c;
  c.tp = texparams; c.lt = nullptr; c.lightObjRow = nullptr; c.typeMasks = nullptr;
  c.prims = prims; c.cprims = prims; c.tpl = texparams;
  c.rowCopy = false; c.tpCopy = false;
  c.n = n; c.tn = tn; c.ln = 0;
  c.matMask = matMask; c.texMask = texMask; c.lightMask = 0u;
  c.fcx = 0.0f; c.fcy = 0.0f;
  c.shadowAnyHit = 0;
  c.cullPrims = 0; c.cullFma = 0; c.cullPrimary = 0;
  c.kShapes = ~0u; c.kMats = kMats; c.kTex = ~0u; c.kLights = 0u;
  return c;
}

__device__ __forceinline__ V3 eye(const SailViewArgs& A) { return v3(A.eye[0], A.eye[1], A.eye[2]); }

// The direction through (s, t) of the view's unit square: the trace kernels' corner interpolation for a sample of zero
// jitter (sail_trace_kernel). A pixel centre is s = (x + 0.5) / W, t = (y + 0.5) / H.
__device__ __forceinline__ V3 pixelDir(const SailViewArgs& A, float s, float t) {
  const bool tri0 = s + t <= 1.0f;
  const V3 d0 = v3(A.d[0][0], A.d[0][1], A.d[0][2]), d1 = v3(A.d[1][0], A.d[1][1], A.d[1][2]);
  const V3 d2 = v3(A.d[2][0], A.d[2][1], A.d[2][2]), d3 = v3(A.d[3][0], A.d[3][1], A.d[3][2]);
  return tri0 ? (d0 + (d2 - d0) * s + (d1 - d0) * t) : (d3 + (d1 - d3) * (1.0f - s) + (d2 - d3) * (1.0f - t));
}

// The trace kernels' own primitive sweep for one ray: every row in ascending order, the first row with the smallest
// distance (a hit on a strict `<`). The row index is wave-uniform, so the rows arrive through the scalar cache
// (constRow). A miss gives best = kMaxDistance and bi = -1; the local hit point stays 0 (hitRecord<true> recomputes it).
__device__ __forceinline__ Sweep firstHit(const Ctx& c, const SailPrim* prims, int n, const Ray& r) {
  Sweep sw;
  sw.best = kMaxDistance; sw.bi = -1; sw.bhl = v3s(0.0f);
  for (int k = 0; k < n; k++) {
    const float tk = primT(c, constRow<SailPrim>(prims, k), r, nullptr);
    if (tk < sw.best) { sw.best = tk; sw.bi = k; }
  }
  return sw;
}

}  // namespace sv
