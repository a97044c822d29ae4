// sail_post.h — what the post-processing kernels share (sail_noise.hip, sail_denoise.hip, sail_tfilter.hip,
// sail_temporal.hip): the small f32 helpers, the per-tile counts, the 3x3 variance prefilter and the reprojection gather.
// The formulas and their f32 operation order are part of the C ABI (include/sail_hip.h) and are checked bit for bit, so
// each lives here once. A piece is here only where its sites perform the same operations: a-trous's normal stop
// (sm::fmax_) and the spatial estimate's (a ternary) agree in value, differ in instructions, and stay where they are.
// Defines no macro and is no part of a run-time kernel's text (sail_amd/gen_jit_src.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_math.h"
#include "sail_temporal.h"

namespace sp {

__device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }
__device__ __forceinline__ float lum(float r, float g, float b) { return ((r + g) + b) / 3.0f; }
// the header's min and max: a NaN in either place gives b
__device__ __forceinline__ float min_(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float max_(float a, float b) { return a > b ? a : b; }

// the filter kernel's pointwise display transforms (sail_filter_kernel kinds 0..2) and its quantisation
__device__ __forceinline__ float display(float c, int kind, float gammaC) {
  if (kind == 0) return c;
  if (kind == 1) return sm::powf_(c, sm::rcp_rn(gammaC));
  const float xx = sm::fmax_(0.0f, c - 0.004f);
  return sm::fdiv(xx * (6.2f * xx + 0.5f), xx * (6.2f * xx + 1.7f) + 0.06f);
}
__device__ __forceinline__ uint32_t quant(float o) { return (uint32_t)(uint8_t)(int)(sm::clamp_(o, 0.0f, 1.0f) * 255.0f + 0.5f); }
__device__ __forceinline__ uint32_t rgba8(float r, float g, float b, int kind, float gammaC) {
  return quant(display(r, kind, gammaC)) | (quant(display(g, kind, gammaC)) << 8) | (quant(display(b, kind, gammaC)) << 16) |
         0xff000000u;
}

// the sample count and the mean colour of a texel of the accumulator the context shows: S holds running means over kf
// samples (mix, SAIL_ACCUM_MIX) or sums with the count in .w; no samples give 0. Two functions: a caller that does not
// need n (the denoiser) passes s.w
struct Rgb { float r, g, b; };
__device__ __forceinline__ float shownCount(const float4 s, int mix, float kf) { return mix ? kf : s.w; }
__device__ __forceinline__ Rgb shownMean(const float4 s, int mix, float n) {
  if (mix) return {s.x, s.y, s.z};
  if (n > 0.0f) return {s.x / n, s.y / n, s.z / n};
  return {0.0f, 0.0f, 0.0f};
}

// the albedo factor of a texel of the albedo map (include/sail_hip.h, sail_denoise_albedo): a channel that is finite and
// above amin, else 1. The demodulated instances of the prepare passes divide by it, the remodulating a-trous pass
// multiplies by it; with a map of ones every x / 1 and x * 1 is exact
__device__ __forceinline__ float albedoChannel(float a, float amin) { return (finite(a) && a > amin) ? a : 1.0f; }
__device__ __forceinline__ Rgb albedoFactor(const float4 a, float amin) {
  return {albedoChannel(a.x, amin), albedoChannel(a.y, amin), albedoChannel(a.z, amin)};
}

// Per-tile counts of a 256-thread workgroup: each wave's count (waveCount of a flag, or a sum of them) goes through LDS
// and thread 0 stores (w0 + w1) + (w2 + w3) at the tile's index of out[i]. N counts share ONE barrier; every thread of
// the workgroup calls it.
__device__ __forceinline__ uint32_t waveCount(bool flag) { return (uint32_t)__popcll(__ballot(flag)); }
template <int N>
__device__ __forceinline__ void tileCounts(const uint32_t (&cnt)[N], uint32_t (&slots)[N][4], uint32_t* const (&out)[N]) {
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < N; i++) slots[i][threadIdx.x >> 6] = cnt[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int i = 0; i < N; i++) out[i][tile] = (slots[i][0] + slots[i][1]) + (slots[i][2] + slots[i][3]);
  }
}

// the 3x3 prefilter of the raw variance at pixel (lx, ly) of a 16x16 tile, from the tile and its one-texel halo in LDS
// (18x18, rows packed); texels that are not finite (outside the frame: NaN) are skipped
constexpr int kVarT = 18;
__device__ __forceinline__ float prefilter(const float* sV, int lx, int ly) {
  float acc = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int m = (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
      const float g = m == 0 ? 0.25f : (m == 1 ? 0.125f : 0.0625f);
      const float vq = sV[(ly + 1 + dy) * kVarT + (lx + 1 + dx)];
      if (finite(vq)) { acc += g * vq; wsum += g; }
    }
  }
  return wsum > 0.0f ? acc / wsum : 0.0f;
}

// The reprojection gather of a pixel that hit the scene (g = G_cur's texel, g.w >= 0; A.haveHist is set). The point sat
// at Xp = X in the previous frame, or with MOVED (an object motion is pending, sail_move_objects) at X - D[id]: one more
// 16-byte load, which the plain kernels do not pay. Xp is projected with rows 0, 1 and 3 of the previous P*MV; of its up
// to four bilinear taps, b then a, those inside the frame that show the same object at the same place are handed to
// tap(w, q), q the texel's index in the previous view's maps. Taps outside the frame are never loaded. done() follows
// the last tap of a point that projects into the previous view: sums that only tap and done touch stay out of registers
// until then.
template <bool MOVED, class Tap, class Done>
__device__ __forceinline__ void gather(const SailReprojectArgs& A, const float4 g, Tap tap, Done done) {
  float px = g.x, py = g.y, pz = g.z;
  if (MOVED) {
    const int id = (int)g.w;
    if ((uint32_t)id < (uint32_t)A.n) {  // G_cur comes from the rows the table was sized for; a row beyond it is never loaded
      const float4 d = A.motion[id];
      px = g.x - d.x; py = g.y - d.y; pz = g.z - d.z;
    }
  }
  const float c0 = ((A.Mp[0][0] * px + A.Mp[0][1] * py) + A.Mp[0][2] * pz) + A.Mp[0][3];
  const float c1 = ((A.Mp[1][0] * px + A.Mp[1][1] * py) + A.Mp[1][2] * pz) + A.Mp[1][3];
  const float c3 = ((A.Mp[2][0] * px + A.Mp[2][1] * py) + A.Mp[2][2] * pz) + A.Mp[2][3];
  if (!(c3 > 0.0f)) return;
  const float u = ((c0 / c3) * 0.5f + 0.5f) * (float)A.W - 0.5f;
  const float v = ((c1 / c3) * 0.5f + 0.5f) * (float)A.H - 0.5f;
  if (!(finite(u) && finite(v))) return;
  const float iu = __builtin_floorf(u), iv = __builtin_floorf(v);
  const float fu = u - iu, fv = v - iv;
  const float rx = px - A.eyePrev[0], ry = py - A.eyePrev[1], rz = pz - A.eyePrev[2];
  const float r2 = (rx * rx + ry * ry) + rz * rz;
  const float lim = A.tol2 * r2;
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
      tap(w, q);
    }
  }
  done();
}

}  // namespace sp
