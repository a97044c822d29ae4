// sail_albedo.hip — the albedo map of a view on the MI355X (gfx950): sail_albedo_kernel.
//
// No reference counterpart (the reference has no denoiser that could use one). This is the input of SVGF's albedo
// demodulation (Schied et al. 2017): the surface colour of each pixel's first hit, which sail_denoise_albedo and
// sail_temporal_filter_albedo divide out of the picture before the a-trous passes and multiply back afterwards, so that a
// procedural texture on one plane (one normal, one depth: nothing for the edge stops to see) is not averaged away. A
// pixel's value is the MEAN surface colour over a g x g grid of sub-pixel rays covering the pixel square the frozen
// schedule's jitter covers: the checkerboard's outline is thinner than a pixel, and a pixel-centre value alone would be the
// wrong divisor in a large share of pixels. The formula and its f32 operation order are part of the C ABI
// (include/sail_hip.h, sail_albedo); the surface colour is the trace kernels' own hit record's (hitRecord<true>, Hit::sc,
// with the scene's texture mask), so the map equals the CPU oracle's first hit bit for bit (tests/albedo_ref.py,
// tests/test_gpu_albedo.py).
//
// MI355X design ("sail_albedo_kernel"):
//  * one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip (the post kernels' shape); the
//    g * g sub-rays run in a loop in the lane, j outer and i inner: the summation order of the header;
//  * a sub-ray is the G-buffer pass's ray at (s, t): the same corner interpolation and mkRay; the sweep is
//    sail_pick_kernel's: primT over all rows in order, a hit on a strict `<`; the row index is wave-uniform, so the rows
//    arrive through the scalar cache (constRow);
//  * the hit record is the generic one of all nine shapes (hitRecordU: the winner's row through scalar loads where the
//    wave agrees on it); it diverges by shape only where a wave straddles objects. Emission and the material constants
//    are not read;
//  * one float4 store per pixel; the two counts are wave ballots behind one barrier (sp::tileCounts), summed per tile on
//    the host;
//  * lanes outside ragged tiles load nothing and store nothing;
//  * plain vector stores only, no atomics: equal data give equal bits.
// mkRay, primT, constRow and hitRecordU are sail_geom.h's. No part of a run-time kernel's text
// (sail_amd/gen_jit_src.py). Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_geom.h"
#include "sail_post.h"
#include "sail_albedo.h"

extern "C" __global__ void __launch_bounds__(256) sail_albedo_kernel(SailAlbedoArgs A) {
  __shared__ uint32_t sCnt[2][4];
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hit = false, partial = false;
  if (x < A.W && y < A.H) {
    // a flat kernel's context with every plugin compiled in: the shape's own hit record, the scene's texture mask
    Ctx c;
    c.tp = A.texparams; c.lt = nullptr; c.lightObjRow = nullptr; c.typeMasks = nullptr;
    c.prims = A.prims; c.cprims = A.prims; c.tpl = A.texparams;
    c.rowCopy = false; c.tpCopy = false;
    c.n = A.n; c.tn = A.tn; c.ln = 0;
    c.matMask = ~0u; c.texMask = A.texMask; c.lightMask = 0u;
    c.fcx = 0.0f; c.fcy = 0.0f;
    c.shadowAnyHit = 0;
    c.cullPrims = 0; c.cullFma = 0; c.cullPrimary = 0;
    c.kShapes = ~0u; c.kMats = ~0u; c.kTex = ~0u; c.kLights = ~0u;
    const V3 eye = v3(A.eye[0], A.eye[1], A.eye[2]);
    const V3 d0 = v3(A.d[0][0], A.d[0][1], A.d[0][2]), d1 = v3(A.d[1][0], A.d[1][1], A.d[1][2]);
    const V3 d2 = v3(A.d[2][0], A.d[2][1], A.d[2][2]), d3 = v3(A.d[3][0], A.d[3][1], A.d[3][2]);
    const int g = A.grid;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    int cnt = 0;
#pragma unroll 1
    for (int j = 0; j < g; j++) {
      const float t = ((float)y + ((float)j + 0.5f) / (float)g) / (float)A.H;
#pragma unroll 1
      for (int i = 0; i < g; i++) {
        const float s = ((float)x + ((float)i + 0.5f) / (float)g) / (float)A.W;
        const bool tri0 = s + t <= 1.0f;
        const Ray r = mkRay(eye, tri0 ? (d0 + (d2 - d0) * s + (d1 - d0) * t) : (d3 + (d1 - d3) * (1.0f - s) + (d2 - d3) * (1.0f - t)));
        // sail_pick_kernel's sweep: every row in order, the first row with the smallest distance
        Sweep sw;
        sw.best = kMaxDistance; sw.bi = -1; sw.bhl = v3s(0.0f);  // the local hit point is recomputed (hitRecord<true>)
        for (int k = 0; k < A.n; k++) {
          const float tk = primT(c, constRow<SailPrim>(A.prims, k), r, nullptr);
          if (tk < sw.best) { sw.best = tk; sw.bi = k; }
        }
        if (sw.bi >= 0) {
          const Hit h = hitRecordU<true>(c, r, sw);
          sr += h.sc.x; sg += h.sc.y; sb += h.sc.z;
          cnt += 1;
        }
      }
    }
    float4 a = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if (cnt > 0) {
      const float cf = (float)cnt;
      a = make_float4(sr / cf, sg / cf, sb / cf, cf);
    }
    A.A[(size_t)y * A.W + x] = a;
    hit = cnt > 0;
    partial = cnt > 0 && cnt < g * g;
  }
  sp::tileCounts<2>({sp::waveCount(hit), sp::waveCount(partial)}, sCnt, {A.tileHit, A.tilePartial});
}

hipError_t sail_launch_albedo(const SailAlbedoArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_albedo_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
