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
//  * a sub-ray is the view passes' ray at (s, t) and its sweep their first-hit sweep (sail_view.h): with g = 1 the
//    G-buffer pass's ray;
//  * the hit record is the generic one of all nine shapes (hitRecordU: the winner's row through scalar loads where the
//    wave agrees on it); it diverges by shape only where a wave straddles objects. Emission and the material constants
//    are not read;
//  * one float4 store per pixel; the two counts are wave ballots behind one barrier (sp::tileCounts), summed per tile on
//    the host;
//  * lanes outside ragged tiles load nothing and store nothing;
//  * plain vector stores only, no atomics: equal data give equal bits.
// mkRay and hitRecordU are sail_geom.h's. No part of a run-time kernel's text
// (sail_amd/gen_jit_src.py). Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_view.h"
#include "sail_post.h"
#include "sail_albedo.h"

extern "C" __global__ void __launch_bounds__(256) sail_albedo_kernel(SailAlbedoArgs A) {
  __shared__ uint32_t sCnt[2][4];
  const SailViewArgs& V = A.V;
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hit = false, partial = false;
  if (x < V.W && y < V.H) {
    // every material compiled in and allowed: the shape's own hit record, the scene's texture mask
    const Ctx c = sv::flatCtx(V.prims, V.n, A.texparams, A.tn, ~0u, A.texMask, ~0u);
    const V3 eye = sv::eye(V);
    const int g = A.grid;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    int cnt = 0;
#pragma unroll 1
    for (int j = 0; j < g; j++) {
      const float t = ((float)y + ((float)j + 0.5f) / (float)g) / (float)V.H;
#pragma unroll 1
      for (int i = 0; i < g; i++) {
        const float s = ((float)x + ((float)i + 0.5f) / (float)g) / (float)V.W;
        const Ray r = mkRay(eye, sv::pixelDir(V, s, t));
        const Sweep sw = sv::firstHit(c, V.prims, V.n, r);
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
    A.A[(size_t)y * V.W + x] = a;
    hit = cnt > 0;
    partial = cnt > 0 && cnt < g * g;
  }
  sp::tileCounts<2>({sp::waveCount(hit), sp::waveCount(partial)}, sCnt, {A.tileHit, A.tilePartial});
}

hipError_t sail_launch_albedo(const SailAlbedoArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_albedo_kernel, dim3((A.V.W + 15) / 16, (A.V.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
