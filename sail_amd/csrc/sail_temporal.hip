// sail_temporal.hip — camera-motion reprojection on the MI355X (gfx950): sail_gbuffer_kernel, sail_reproject_kernel,
// sail_reproject_moved_kernel and sail_temporal_resolve_kernel.
//
// No reference counterpart (the reference throws the picture away on every camera move, src/core/renderer.js:57-60).
// This is the temporal part of SVGF (Schied et al. 2017): a G-buffer pass gives every pixel of a view the world position
// and the object row of its first hit, the reproject pass looks each pixel's position up in the previous view's colour
// history, and the resolve pass blends that history, counted as at most `cap` samples, with the mean of the samples
// rendered since. The formulas and their f32 operation order are part of the C ABI (include/sail_hip.h,
// sail_temporal_begin / sail_temporal_resolve); every operation is an IEEE one, so a numpy float32 restatement gives the
// same bits (tests/temporal_ref.py, tests/test_gpu_temporal.py). The gather, the shown mean, the display transform and
// the per-tile counts are sail_post.h's, shared with the moment kernels (sail_tfilter.hip) and the denoiser.
//
// MI355X design ("sail_gbuffer_kernel, sail_reproject_kernel, sail_temporal_resolve_kernel"):
//  * all four: one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip (the filter and
//    noise kernels' shape): float4 loads and stores in 256-byte runs per row;
//  * G-buffer: the pixel-centre ray and the first-hit sweep of the view passes (sail_view.h). One float4 store per pixel;
//  * reproject: the tap of sp::gather reads Hist and accepts a texel with a count and a finite colour; up to four float4
//    pairs (G_prev, Hist) per pixel, 16-byte loads, straight from L2 / HBM: neighbouring pixels of the new view land on
//    neighbouring texels of the old one, so a wave's taps share cache lines. No LDS staging;
//  * reproject with an object motion pending (sail_move_objects; sail_reproject_moved_kernel, DESIGN.md §5,
//    "sail_reproject_moved_kernel"): the same body as a second instance, MOVED, which looks up X - D[id] and caps the count
//    that crosses the move. An entry point of its own, not a run-time switch: the plain kernel pays no table load;
//  * resolve: pointwise, one float4 of S and of R in, one float4 and one RGBA8 word out;
//  * the counts are wave ballots, one barrier each (sp::tileCounts), summed per tile on the host;
//  * lanes outside ragged tiles load nothing and store nothing;
//  * plain vector stores only, no atomics: equal data give equal bits.
// mkRay is sail_geom.h's. No part of a run-time kernel's text (sail_amd/gen_jit_src.py). Built
// with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_view.h"
#include "sail_post.h"

extern "C" __global__ void __launch_bounds__(256) sail_gbuffer_kernel(SailGbufferArgs A) {
  const SailViewArgs& V = A.V;
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= V.W || y >= V.H) return;
  const Ray r = mkRay(sv::eye(V), sv::pixelDir(V, ((float)x + 0.5f) / (float)V.W, ((float)y + 0.5f) / (float)V.H));
  const Sweep sw = sv::firstHit(sv::flatCtx(V.prims, V.n, nullptr, 0, 0u, 0u, 0u), V.prims, V.n, r);
  const size_t pix = (size_t)y * V.W + x;
  float4 g = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if (sw.bi >= 0) {
    const V3 X = r.o + r.d * sw.best;  // a product and a sum per component, no fma
    g = make_float4(X.x, X.y, X.z, (float)sw.bi);
  }
  A.G[pix] = g;
  if (A.rays) {
    float* q = A.rays + 6 * pix;
    q[0] = r.o.x; q[1] = r.o.y; q[2] = r.o.z; q[3] = r.d.x; q[4] = r.d.y; q[5] = r.d.z;
  }
  if (A.t) A.t[pix] = sw.best;
}

// The reproject pass over the colour history: sp::gather's taps that hold a count and a finite colour. MOVED = false is
// sail_reproject_kernel (motion, n and mc are not read); MOVED = true is the pass after sail_move_objects, where the count
// that crosses the move is at most mc.
template <bool MOVED>
__device__ __forceinline__ void tpReproject(const SailReprojectArgs& A) {
  __shared__ uint32_t sHit[1][4], sHist[1][4];
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hit = false, found = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 g = A.Gcur[pix];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    hit = !(g.w < 0.0f);
    if (hit && A.haveHist) {
      float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f, m = __builtin_inff();
      sp::gather<MOVED>(
          A, g,
          [&](float w, size_t q) {
            const float4 h = A.hist[q];  // one 16-byte load
            if (!(h.w > 0.0f) || !(sp::finite(h.x) && sp::finite(h.y) && sp::finite(h.z))) return;
            ar += w * h.x; ag += w * h.y; ab += w * h.z;
            wsum += w;
            m = sp::min_(m, h.w);
          },
          [&] {
            if (wsum > 0.0f) { out = make_float4(ar / wsum, ag / wsum, ab / wsum, MOVED ? sp::min_(m, A.mc) : m); found = true; }
          });
    }
    A.out[pix] = out;
  }
  sp::tileCounts<1>({sp::waveCount(hit)}, sHit, {A.tileHit});
  sp::tileCounts<1>({sp::waveCount(found)}, sHist, {A.tileHist});
}

extern "C" __global__ void __launch_bounds__(256) sail_reproject_kernel(SailReprojectArgs A) { tpReproject<false>(A); }

extern "C" __global__ void __launch_bounds__(256) sail_reproject_moved_kernel(SailReprojectArgs A) { tpReproject<true>(A); }

extern "C" __global__ void __launch_bounds__(256) sail_temporal_resolve_kernel(SailResolveArgs A) {
  __shared__ uint32_t sHist[1][4], sBad[1][4];
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hist = false, bad = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 s = A.S[pix], r = A.R[pix];
    const float n = sp::shownCount(s, A.mix, A.kf);
    const sp::Rgb c = sp::shownMean(s, A.mix, n);
    const bool fin = sp::finite(c.r) && sp::finite(c.g) && sp::finite(c.b);
    bad = !fin;
    const float m = r.w;
    hist = m > 0.0f;
    const bool cur = n > 0.0f && fin;
    float4 o;
    if (hist && cur) {
      const float ws = m + n;
      o = make_float4(((m * r.x) + (n * c.r)) / ws, ((m * r.y) + (n * c.g)) / ws, ((m * r.z) + (n * c.b)) / ws, sp::min_(ws, A.cap));
    } else if (hist) {
      o = make_float4(r.x, r.y, r.z, m);
    } else {
      o = make_float4(c.r, c.g, c.b, sp::min_(n, A.cap));
    }
    A.Out[pix] = o;
    if (A.out8) A.out8[pix] = sp::rgba8(o.x, o.y, o.z, A.display, A.gammaC);
  }
  sp::tileCounts<1>({sp::waveCount(hist)}, sHist, {A.tileHist});
  sp::tileCounts<1>({sp::waveCount(bad)}, sBad, {A.tileBad});
}

hipError_t sail_launch_gbuffer(const SailGbufferArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_gbuffer_kernel, dim3((A.V.W + 15) / 16, (A.V.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_reproject(const SailReprojectArgs& A, bool moved, hipStream_t s) {
  hipLaunchKernelGGL(moved ? sail_reproject_moved_kernel : sail_reproject_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256),
                     0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_temporal_resolve(const SailResolveArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_temporal_resolve_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

