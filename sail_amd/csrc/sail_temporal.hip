// sail_temporal.hip — camera-motion reprojection on the MI355X (gfx950): sail_gbuffer_kernel, sail_reproject_kernel and
// sail_temporal_resolve_kernel.
//
// No reference counterpart (the reference throws the picture away on every camera move, src/core/renderer.js:57-60).
// This is the temporal part of SVGF (Schied et al. 2017) for a still scene seen from a moving camera: a G-buffer pass
// gives every pixel of a view the world position and the object row of its first hit, the reproject pass looks each
// pixel's position up in the previous view's history with a bilinear gather that only accepts taps of the same object
// at the same place, and the resolve pass blends that history, counted as at most `cap` samples, with the mean of the
// samples rendered since. The formulas and their f32 operation order are part of the C ABI (include/sail_hip.h,
// sail_temporal_begin / sail_temporal_resolve); every operation is an IEEE one, so a numpy float32 restatement gives the
// same bits (tests/test_gpu_temporal.py).
//
// MI355X design ("sail_gbuffer_kernel, sail_reproject_kernel, sail_temporal_resolve_kernel"):
//  * all three: one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip (the filter and
//    noise kernels' shape): float4 loads and stores in 256-byte runs per row;
//  * G-buffer: the pixel's ray is the trace kernels' for a sample of zero jitter (same corner interpolation, mkRay),
//    the sweep is sail_pick_kernel's: primT over all rows in order, a hit on a strict `<`; the row index is
//    wave-uniform, so the rows arrive through the scalar cache (constRow). One float4 store per pixel;
//  * reproject: a data-dependent gather of up to four float4 pairs (G_prev, Hist) per pixel, 16-byte loads, straight
//    from L2 / HBM: neighbouring pixels of the new view land on neighbouring texels of the old one, so a wave's taps
//    share cache lines. Taps outside the frame are never loaded. No LDS staging;
//  * reproject with an object motion pending (sail_move_objects; sail_reproject_moved_kernel, DESIGN.md §5,
//    "sail_reproject_moved_kernel"): the same body, which first takes the pixel's row translation from a table of n float4
//    (one more 16-byte load by the id of G_cur; the table stays in L1/L2) and looks up X - d instead of X;
//  * resolve: pointwise, one float4 of S and of R in, one float4 and one RGBA8 word out;
//  * the counts are wave ballots, summed across the four waves through LDS in a fixed order and per tile on the host;
//  * lanes outside ragged tiles load nothing and store nothing;
//  * plain vector stores only, no atomics: equal data give equal bits.
// Included from sail_kernels.hip AFTER sail_trace.hip (it calls that file's mkRay, primT and constRow) and defines no
// macro: the text of sail_trace.hip is embedded in the library and hashed into every run-time kernel's cache key. Built
// with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_math.h"
#include "sail_temporal.h"

namespace {

__device__ __forceinline__ bool tpFinite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }
__device__ __forceinline__ float tpMin(float a, float b) { return a < b ? a : b; }

// the filter kernel's pointwise display transforms (sail_filter_kernel kinds 0..2) and its quantisation
__device__ __forceinline__ float tpDisplay(float c, int kind, float gammaC) {
  if (kind == 0) return c;
  if (kind == 1) return sm::powf_(c, sm::rcp_rn(gammaC));
  const float xx = sm::fmax_(0.0f, c - 0.004f);
  return sm::fdiv(xx * (6.2f * xx + 0.5f), xx * (6.2f * xx + 1.7f) + 0.06f);
}
__device__ __forceinline__ uint32_t tpQuant(float o) { return (uint32_t)(uint8_t)(int)(sm::clamp_(o, 0.0f, 1.0f) * 255.0f + 0.5f); }

// a tile's count from its four waves' ballots, in a fixed order; every thread of the workgroup calls it
__device__ __forceinline__ void tpTileCount(bool flag, uint32_t* slots, uint32_t* out) {
  const uint32_t cnt = (uint32_t)__popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (slots[0] + slots[1]) + (slots[2] + slots[3]);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) sail_gbuffer_kernel(SailGbufferArgs A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= A.W || y >= A.H) return;
  // the trace kernels' primary ray for a sample without jitter (sail_trace_kernel)
  const float s = ((float)x + 0.5f) / (float)A.W, t = ((float)y + 0.5f) / (float)A.H;
  const bool tri0 = s + t <= 1.0f;
  const V3 eye = v3(A.eye[0], A.eye[1], A.eye[2]);
  const V3 d0 = v3(A.d[0][0], A.d[0][1], A.d[0][2]), d1 = v3(A.d[1][0], A.d[1][1], A.d[1][2]);
  const V3 d2 = v3(A.d[2][0], A.d[2][1], A.d[2][2]), d3 = v3(A.d[3][0], A.d[3][1], A.d[3][2]);
  const Ray r = mkRay(eye, tri0 ? (d0 + (d2 - d0) * s + (d1 - d0) * t) : (d3 + (d1 - d3) * (1.0f - s) + (d2 - d3) * (1.0f - t)));
  // sail_pick_kernel's sweep: every row in order, the first row with the smallest distance
  Ctx c;
  c.kShapes = ~0u;
  float best = kMaxDistance;
  int bi = -1;
  for (int k = 0; k < A.n; k++) {
    const float tk = primT(c, constRow<SailPrim>(A.prims, k), r, nullptr);
    if (tk < best) { best = tk; bi = k; }
  }
  const size_t pix = (size_t)y * A.W + x;
  float4 g = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if (bi >= 0) {
    const V3 X = r.o + r.d * best;  // a product and a sum per component, no fma
    g = make_float4(X.x, X.y, X.z, (float)bi);
  }
  A.G[pix] = g;
  if (A.rays) {
    float* q = A.rays + 6 * pix;
    q[0] = r.o.x; q[1] = r.o.y; q[2] = r.o.z; q[3] = r.d.x; q[4] = r.d.y; q[5] = r.d.z;
  }
  if (A.t) A.t[pix] = best;
}

// The reproject pass. MOVED = false is sail_reproject_kernel as it always was: motion, n and mc are not read. MOVED = true is the
// pass after sail_move_objects: the point the pixel shows sat at Xp = X - D[id] in the previous frame, and the count that
// crosses the move is at most mc.
template <bool MOVED>
__device__ __forceinline__ void tpReproject(const SailReprojectArgs& A, const float4* motion, int n, float mc) {
  __shared__ uint32_t sHit[4], sHist[4];
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hit = false, found = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 g = A.Gcur[pix];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    hit = !(g.w < 0.0f);
    if (hit && A.haveHist) {
      float px = g.x, py = g.y, pz = g.z;
      if (MOVED) {
        const int id = (int)g.w;
        if ((uint32_t)id < (uint32_t)n) {  // G_cur comes from the rows the table was sized for; a row beyond it is never loaded
          const float4 d = motion[id];
          px = g.x - d.x; py = g.y - d.y; pz = g.z - d.z;
        }
      }
      const float c0 = ((A.Mp[0][0] * px + A.Mp[0][1] * py) + A.Mp[0][2] * pz) + A.Mp[0][3];
      const float c1 = ((A.Mp[1][0] * px + A.Mp[1][1] * py) + A.Mp[1][2] * pz) + A.Mp[1][3];
      const float c3 = ((A.Mp[2][0] * px + A.Mp[2][1] * py) + A.Mp[2][2] * pz) + A.Mp[2][3];
      if (c3 > 0.0f) {
        const float u = ((c0 / c3) * 0.5f + 0.5f) * (float)A.W - 0.5f;
        const float v = ((c1 / c3) * 0.5f + 0.5f) * (float)A.H - 0.5f;
        if (tpFinite(u) && tpFinite(v)) {
          const float iu = __builtin_floorf(u), iv = __builtin_floorf(v);
          const float fu = u - iu, fv = v - iv;
          const float rx = px - A.eyePrev[0], ry = py - A.eyePrev[1], rz = pz - A.eyePrev[2];
          const float r2 = (rx * rx + ry * ry) + rz * rz;
          const float lim = A.tol2 * r2;
          float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f, m = __builtin_inff();
#pragma unroll
          for (int b = 0; b < 2; b++) {
#pragma unroll
            for (int a = 0; a < 2; a++) {
              // in floats: u and v may lie far outside the int range
              const float qxf = iu + (float)a, qyf = iv + (float)b;
              if (!(qxf >= 0.0f && qxf <= (float)(A.W - 1) && qyf >= 0.0f && qyf <= (float)(A.H - 1))) continue;
              const float w = (a ? fu : 1.0f - fu) * (b ? fv : 1.0f - fv);
              if (!(w > 0.0f)) continue;
              const size_t q = (size_t)(int)qyf * A.W + (int)qxf;
              const float4 gq = A.Gprev[q];
              if (!(gq.w == g.w)) continue;
              const float ex = px - gq.x, ey = py - gq.y, ez = pz - gq.z;
              if (!((ex * ex + ey * ey) + ez * ez <= lim)) continue;
              const float4 h = A.Hist[q];
              if (!(h.w > 0.0f) || !(tpFinite(h.x) && tpFinite(h.y) && tpFinite(h.z))) continue;
              ar += w * h.x; ag += w * h.y; ab += w * h.z;
              wsum += w;
              m = tpMin(m, h.w);
            }
          }
          if (wsum > 0.0f) { out = make_float4(ar / wsum, ag / wsum, ab / wsum, MOVED ? tpMin(m, mc) : m); found = true; }
        }
      }
    }
    A.R[pix] = out;
  }
  tpTileCount(hit, sHit, A.tileHit);
  tpTileCount(found, sHist, A.tileHist);
}

extern "C" __global__ void __launch_bounds__(256) sail_reproject_kernel(SailReprojectArgs A) {
  tpReproject<false>(A, nullptr, 0, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) sail_reproject_moved_kernel(SailReprojectMovedArgs A) {
  tpReproject<true>(A.base, A.motion, A.n, A.mc);
}

extern "C" __global__ void __launch_bounds__(256) sail_temporal_resolve_kernel(SailResolveArgs A) {
  __shared__ uint32_t sHist[4], sBad[4];
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  bool hist = false, bad = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 s = A.S[pix], r = A.R[pix];
    const float n = A.mix ? A.kf : s.w;
    float cr, cg, cb;
    if (A.mix) { cr = s.x; cg = s.y; cb = s.z; }
    else if (n > 0.0f) { cr = s.x / n; cg = s.y / n; cb = s.z / n; }
    else { cr = 0.0f; cg = 0.0f; cb = 0.0f; }
    const bool fin = tpFinite(cr) && tpFinite(cg) && tpFinite(cb);
    bad = !fin;
    const float m = r.w;
    hist = m > 0.0f;
    const bool cur = n > 0.0f && fin;
    float4 o;
    if (hist && cur) {
      const float ws = m + n;
      o = make_float4(((m * r.x) + (n * cr)) / ws, ((m * r.y) + (n * cg)) / ws, ((m * r.z) + (n * cb)) / ws, tpMin(ws, A.cap));
    } else if (hist) {
      o = make_float4(r.x, r.y, r.z, m);
    } else {
      o = make_float4(cr, cg, cb, tpMin(n, A.cap));
    }
    A.Out[pix] = o;
    if (A.out8)
      A.out8[pix] = tpQuant(tpDisplay(o.x, A.display, A.gammaC)) | (tpQuant(tpDisplay(o.y, A.display, A.gammaC)) << 8) |
                    (tpQuant(tpDisplay(o.z, A.display, A.gammaC)) << 16) | 0xff000000u;
  }
  tpTileCount(hist, sHist, A.tileHist);
  tpTileCount(bad, sBad, A.tileBad);
}

hipError_t sail_launch_gbuffer(const SailGbufferArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_gbuffer_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_reproject(const SailReprojectArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_reproject_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_reproject_moved(const SailReprojectMovedArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_reproject_moved_kernel, dim3((A.base.W + 15) / 16, (A.base.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_temporal_resolve(const SailResolveArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_temporal_resolve_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
