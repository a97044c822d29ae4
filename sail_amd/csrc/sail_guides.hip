// sail_guides.hip — the denoiser's guide maps of a view on the MI355X (gfx950): sail_guides_kernel.
//
// No reference counterpart (the reference has no denoiser). The a-trous filters stop at normals and positions, and the
// AOVs give them a specular surface's own: on a mirror or a pane of smooth glass the picture is whatever the surface
// shows, so a sphere's smoothly turning normals stop nothing at the reflected room's edges. This kernel walks each
// pixel-centre ray through mirror and smooth glass, with the random pair of the material sample fixed at (0.5, 0.5), to
// the first surface that scatters, and stores that surface's normal and position in the AOVs' encoding. The walk and its
// f32 operation order are part of the C ABI (include/sail_hip.h, sail_guides): the trace kernels' own sweep, hit record,
// shading frame and material sample, so the maps equal the CPU oracle's walk bit for bit (tests/guides_ref.py,
// tests/test_gpu_guides.py).
//
// MI355X design ("sail_guides_kernel"):
//  * one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip (the post kernels' shape);
//  * the first ray is the G-buffer pass's and every sweep the view passes' first-hit sweep (sail_view.h);
//  * the hit record is the generic one of all nine shapes (hitRecordU), the frame is shadeBounce's, the direction is
//    material()'s with only the mirror and glass plugins compiled in: radiance, throughput and the hash are never made;
//  * lanes leave the walk at different depths. The loop runs while any lane of the wave is alive, finished lanes masked:
//    the sweep's row loads stay scalar, and nothing is compacted (only the specular pixels go round again);
//  * what is live across the loop's back edge: the segment (6), the recorded normal and position (6), the row, the depth
//    and two flags;
//  * two float4 stores per pixel; the three counts are wave ballots behind one barrier (sp::tileCounts), summed per tile
//    on the host;
//  * lanes outside ragged tiles load nothing and store nothing;
//  * plain vector stores only, no atomics: equal data give equal bits.
// mkRay and hitRecordU are sail_geom.h's, material() is sail_shade.h's. No part of a run-time kernel's
// text (sail_amd/gen_jit_src.py). Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_view.h"
#include "sail_shade.h"
#include "sail_post.h"
#include "sail_guides.h"

extern "C" __global__ void __launch_bounds__(256) sail_guides_kernel(SailGuidesArgs A) {
  __shared__ uint32_t sCnt[3][4];
  const SailViewArgs& V = A.V;
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  const bool inside = x < V.W && y < V.H;
  // of the materials the two that are followed are compiled in
  const Ctx c = sv::flatCtx(V.prims, V.n, A.texparams, A.tn, A.matMask, A.texMask, (1u << SAIL_MIRROR) | (1u << SAIL_GLASS));
  Seg ray;
  ray.o = sv::eye(V);
  ray.d = v3s(0.0f);
  // the G-buffer pass's ray (sail_gbuffer_kernel)
  if (inside) ray.d = sv::pixelDir(V, ((float)x + 0.5f) / (float)V.W, ((float)y + 0.5f) / (float)V.H);
  V3 gn = v3s(0.0f), gp = v3s(0.0f);
  int id = -1, depth = 0;
  bool alive = inside, truncated = false;
#pragma unroll 1
  while (__any(alive)) {
    if (alive) {
      const Ray r = mkRay(ray.o, ray.d);
      const Sweep sw = sv::firstHit(c, V.prims, V.n, r);
      alive = false;  // a miss keeps the surface recorded last
      if (sw.bi >= 0) {
        const Hit ins = hitRecordU<true>(c, r, sw);
        gn = ins.normal; gp = ins.hit; id = sw.bi;
        const int cat = ins.matCategory;
        bool follow = false;
        if (cat >= 0 && cat < 32 && ((A.matMask >> cat) & 1u)) {
          if (cat == SAIL_MIRROR) follow = true;
          else if (cat == SAIL_GLASS) follow = TP(c, ins.matRow, 4) < kEps && TP(c, ins.matRow, 5) < kEps;
        }
        if (follow && depth == A.depth) truncated = true;
        if (follow && depth < A.depth) {
          // shadeBounce's frame (sail_shade.h): a unit dpdu is its own normalisation, and the local z of -d is known
          // from the hit record's into test
          const V3 nd3 = -r.d;
          const float dd = dot(ins.dpdu, ins.dpdu);
          const V3 ss = (dd == 1.0f) ? ins.dpdu : ins.dpdu / sqrtf_(dd);
          const V3 ts = cross(ins.normal, ss);
          const V3 wo = v3(dot(nd3, ss), dot(nd3, ts), ins.into ? -ins.nd : ins.nd);
          V3 wiL, f;
          (void)material(c, ins, v2(0.5f, 0.5f), wo, wiL, f);
          const V3 wi = localToWorld(wiL, ins.normal, ss, ts);
          const float outdot = dot(ins.normal, wi);
          ray.o = ins.hit + ins.normal * (outdot > kEps ? 0.0001f : -0.0001f);
          ray.d = wi;
          depth += 1;
          alive = true;
        }
      }
    }
  }
  const bool hit = id >= 0;
  if (inside) {
    const size_t pix = (size_t)y * V.W + x;
    float4 ng = make_float4(0.5f, 0.5f, 0.5f, 0.0f);
    float4 xg = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), -1.0f);
    if (hit) {  // the AOVs' encoding (sail_trace_kernel)
      const V3 qn = gn / 2.0f + 0.5f, qp = normalize(gp);
      ng = make_float4(qn.x, qn.y, qn.z, (float)depth);
      xg = make_float4(qp.x, qp.y, qp.z, (float)id);
    }
    A.Ng[pix] = ng;
    A.Xg[pix] = xg;
  }
  sp::tileCounts<3>({sp::waveCount(hit), sp::waveCount(hit && depth > 0), sp::waveCount(truncated)}, sCnt,
                    {A.tileHit, A.tileFollowed, A.tileTruncated});
}

hipError_t sail_launch_guides(const SailGuidesArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_guides_kernel, dim3((A.V.W + 15) / 16, (A.V.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
