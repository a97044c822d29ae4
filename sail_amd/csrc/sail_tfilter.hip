// sail_tfilter.hip — the filter of a reprojected frame on the MI355X (gfx950): sail_moment_reproject_kernel,
// sail_moment_resolve_kernel and sail_tfilter_prepare_kernel.
//
// No reference counterpart (the reference throws the picture away on every camera move). This is the piece SVGF (Schied et
// al. 2017) has between its temporal accumulation and its a-trous filter: the first two moments of each pixel's luminance
// are reprojected and blended exactly like the colour (sail_temporal.hip), and give a per-pixel variance that survives a
// camera move; where the moments are young or disoccluded a 7x7 spatial estimate over the resolved picture stands in. The
// prepare pass writes exactly the (cv, g0, g1) maps sail_denoise_atrous_kernel reads, so the a-trous passes run unchanged
// over the resolved picture `Out`. The formulas and their f32 operation order are part of the C ABI (include/sail_hip.h,
// sail_temporal_moments / sail_temporal_filter); every operation is an IEEE one, so a numpy float32 restatement gives the
// same bits (tests/temporal_filter_ref.py, tests/test_gpu_temporal_filter.py).
//
// MI355X design ("sail_tfilter_prepare_kernel"):
//  * all three: one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip; float4 loads and stores;
//  * moment reproject: sail_reproject_kernel's gather with Mhist in the place of Hist (Hist is not read), no counts;
//    sail_moment_reproject_moved_kernel is the same body after sail_move_objects, as sail_reproject_moved_kernel;
//  * moment resolve: pointwise, one float4 of S and of MR in, one float4 out;
//  * prepare, three phases with a barrier between them:
//      1. the tile and a four-texel halo (24x24) are staged in LDS as two float4 per texel: (decoded normal, luminance)
//         and (position, usable), usable = inside the frame and colour finite: 18,432 B;
//      2. v0 of the tile and a one-texel halo (18x18, the 3x3 prefilter's reach) goes to LDS: 324 texels over the 256
//         lanes in two rounds. A lane takes the variance of the moments where they are old enough; the 49-tap spatial loop
//         runs only in waves where some lane needs it (a ballot), all of its taps from LDS. Texels outside the frame hold
//         NaN, which the prefilter skips like any non-finite tap;
//      3. every lane prefilters its own pixel and stores (c, v), g0 and g1: the guides come from the stage, only the
//         colour is loaded again (16 B, the line is in L2 from phase 1);
//  * LDS 19,760 B per workgroup: eight workgroups per CU fit, the 32-wave cap binds first. Rows are packed (24 float4 =
//    96 dwords); phase 2 walks the 18x18 grid row-major, so the 16 lanes of a ds_read_b128 group read consecutive texels
//    except where a row ends;
//  * texels outside the frame are never loaded; lanes outside ragged tiles store nothing;
//  * the counts are wave ballots, summed across the four waves through LDS in a fixed order and per tile on the host;
//  * plain vector stores only, no atomics: equal data give equal bits.
// Lives in its own file and defines no macro: the text of sail_trace.hip is embedded in the library and hashed into every
// run-time kernel's cache key. Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_math.h"
#include "sail_tfilter.h"

namespace {

constexpr int kTfS = 24;  // stage: 16 + 2 * (1 prefilter + 3 window) texels, rows packed
constexpr int kTfV = 18;  // v0: 16 + 2 * 1

__device__ __forceinline__ bool tfFinite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }
__device__ __forceinline__ float tfMin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float tfMax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float tfLum(float r, float g, float b) { return ((r + g) + b) / 3.0f; }

// the 7x7 spatial variance of the luminance round stage texel (cx, cy), 3 <= cx, cy <= 20 (include/sail_hip.h)
__device__ __forceinline__ float tfSpatial(const float4* sA, const float4* sB, int cx, int cy, float sx0) {
  const float4 pa = sA[cy * kTfS + cx], pb = sB[cy * kTfS + cx];
  float a1 = 0.0f, a2 = 0.0f, ws = 0.0f;
  for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
    for (int dx = -3; dx <= 3; dx++) {
      const int q = (cy + dy) * kTfS + (cx + dx);
      const float4 qb = sB[q];
      if (!(qb.w > 0.0f)) continue;  // outside the frame, or a colour that is not finite
      const float4 qa = sA[q];
      float w = 1.0f;
      if (dy != 0 || dx != 0) {
        float d = tfMax((pa.x * qa.x + pa.y * qa.y) + pa.z * qa.z, 0.0f);
        d = d * d; d = d * d; d = d * d; d = d * d; d = d * d; d = d * d;
        const float tx = pb.x - qb.x, ty = pb.y - qb.y, tz = pb.z - qb.z;
        const float dx2 = (tx * tx + ty * ty) + tz * tz;
        const float wx = sm::rcp_rn(1.0f + dx2 / sx0);
        w = d * wx;
      }
      if (w > 0.0f) {
        a1 += w * qa.w;
        a2 += w * (qa.w * qa.w);
        ws += w;
      }
    }
  }
  if (!(ws > 0.0f)) return 0.0f;
  const float m1 = a1 / ws;
  return tfMax(a2 / ws - m1 * m1, 0.0f);
}

}  // namespace

// The moment reproject pass. MOVED = false is sail_moment_reproject_kernel as it always was: motion, n and mc are not read.
// MOVED = true follows sail_reproject_moved_kernel: the same Xp = X - D[id], and MR.z = min(m, mc).
template <bool MOVED>
__device__ __forceinline__ void tfMomentReproject(const SailMomentReprojectArgs& A, const float4* motion, int n, float mc) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= A.W || y >= A.H) return;
  const size_t pix = (size_t)y * A.W + x;
  const float4 g = A.Gcur[pix];
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (!(g.w < 0.0f) && A.haveHist) {
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
      if (tfFinite(u) && tfFinite(v)) {
        const float iu = __builtin_floorf(u), iv = __builtin_floorf(v);
        const float fu = u - iu, fv = v - iv;
        const float rx = px - A.eyePrev[0], ry = py - A.eyePrev[1], rz = pz - A.eyePrev[2];
        const float r2 = (rx * rx + ry * ry) + rz * rz;
        const float lim = A.tol2 * r2;
        float a1 = 0.0f, a2 = 0.0f, wsum = 0.0f, m = __builtin_inff();
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
            const float4 h = A.Mhist[q];
            if (!(h.z > 0.0f) || !(tfFinite(h.x) && tfFinite(h.y))) continue;
            a1 += w * h.x; a2 += w * h.y;
            wsum += w;
            m = tfMin(m, h.z);
          }
        }
        if (wsum > 0.0f) out = make_float4(a1 / wsum, a2 / wsum, MOVED ? tfMin(m, mc) : m, 0.0f);
      }
    }
  }
  A.MR[pix] = out;
}

extern "C" __global__ void __launch_bounds__(256) sail_moment_reproject_kernel(SailMomentReprojectArgs A) {
  tfMomentReproject<false>(A, nullptr, 0, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) sail_moment_reproject_moved_kernel(SailMomentReprojectMovedArgs A) {
  tfMomentReproject<true>(A.base, A.motion, A.n, A.mc);
}

extern "C" __global__ void __launch_bounds__(256) sail_moment_resolve_kernel(SailMomentResolveArgs A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= A.W || y >= A.H) return;
  const size_t pix = (size_t)y * A.W + x;
  const float4 s = A.S[pix], r = A.MR[pix];
  const float n = A.mix ? A.kf : s.w;
  float cr, cg, cb;
  if (A.mix) { cr = s.x; cg = s.y; cb = s.z; }
  else if (n > 0.0f) { cr = s.x / n; cg = s.y / n; cb = s.z / n; }
  else { cr = 0.0f; cg = 0.0f; cb = 0.0f; }
  const float l = tfLum(cr, cg, cb);
  const bool cur = n > 0.0f && tfFinite(cr) && tfFinite(cg) && tfFinite(cb);
  const float mh = r.z;
  const bool hist = mh > 0.0f;
  float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (hist && cur) {
    const float ws = mh + n;
    o = make_float4(((mh * r.x) + (n * l)) / ws, ((mh * r.y) + (n * (l * l))) / ws, tfMin(ws, A.cap), 0.0f);
  } else if (hist) {
    o = r;
  } else if (cur) {
    o = make_float4(l, l * l, tfMin(n, A.cap), 0.0f);
  }
  A.Mout[pix] = o;
}

extern "C" __global__ void __launch_bounds__(256) sail_tfilter_prepare_kernel(SailTfilterPrepareArgs A) {
  __shared__ float4 sA[kTfS * kTfS];  // (decoded normal, luminance)
  __shared__ float4 sB[kTfS * kTfS];  // (position, usable)
  __shared__ float sV[kTfV * kTfV];
  __shared__ uint32_t sBad[4], sTmp[4];
  const int tx0 = (int)blockIdx.x * 16, ty0 = (int)blockIdx.y * 16;
  // 1. the stage
  for (int t = threadIdx.x; t < kTfS * kTfS; t += 256) {
    const int sy = t / kTfS, sx = t - sy * kTfS;
    const int qx = tx0 - 4 + sx, qy = ty0 - 4 + sy;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (qx >= 0 && qx < A.W && qy >= 0 && qy < A.H) {
      const size_t q = (size_t)qy * A.W + qx;
      const float4 o = A.Out[q], nn = A.N[q], xp = A.X[q];
      const bool fin = tfFinite(o.x) && tfFinite(o.y) && tfFinite(o.z);
      a = make_float4(2.0f * nn.x - 1.0f, 2.0f * nn.y - 1.0f, 2.0f * nn.z - 1.0f, tfLum(o.x, o.y, o.z));
      b = make_float4(xp.x, xp.y, xp.z, fin ? 1.0f : 0.0f);
    }
    sA[t] = a;
    sB[t] = b;
  }
  __syncthreads();
  // 2. v0 of the tile and its one-texel halo
  uint32_t nTemporal = 0;
#pragma unroll 1
  for (int r = 0; r < 2; r++) {
    const int t = (int)threadIdx.x + r * 256;
    const int vy = t / kTfV, vx = t - vy * kTfV;
    const int qx = tx0 - 1 + vx, qy = ty0 - 1 + vy;
    const bool inside = t < kTfV * kTfV && qx >= 0 && qx < A.W && qy >= 0 && qy < A.H;
    float v0 = __builtin_nanf("");  // outside the frame: skipped by the prefilter
    bool temporal = false;
    if (inside) {
      const size_t q = (size_t)qy * A.W + qx;
      const float4 m = A.Mout[q];
      const float n = A.mix ? A.kf : A.S[q].w;
      const float nn = n > 0.0f ? n : 1.0f;
      const float vt = (tfMax(m.y - m.x * m.x, 0.0f) * nn) / m.z;
      temporal = m.z >= A.minHist && tfFinite(vt);
      if (temporal) v0 = vt;
    }
    const bool need = inside && !temporal;
    if (__ballot(need) != 0ull) {  // wave-uniform: a wave whose lanes all have old moments skips the 49 taps
      if (need) v0 = tfSpatial(sA, sB, vx + 3, vy + 3, A.sx0);
    }
    if (t < kTfV * kTfV) sV[t] = v0;
    // the tile's own pixels, not its halo
    const bool own = temporal && vx >= 1 && vx <= 16 && vy >= 1 && vy <= 16;
    nTemporal += (uint32_t)__popcll(__ballot(own));
  }
  __syncthreads();
  // 3. the prefilter and the a-trous passes' inputs
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  bool bad = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 o = A.Out[pix];
    const float4 ga = sA[(ly + 4) * kTfS + (lx + 4)], gb = sB[(ly + 4) * kTfS + (lx + 4)];
    bad = !(gb.w > 0.0f);
    float acc = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const int m = (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
        const float g = m == 0 ? 0.25f : (m == 1 ? 0.125f : 0.0625f);
        const float vq = sV[(ly + 1 + dy) * kTfV + (lx + 1 + dx)];
        if (tfFinite(vq)) { acc += g * vq; wsum += g; }
      }
    }
    const float v = wsum > 0.0f ? acc / wsum : 0.0f;
    A.cv[pix] = make_float4(o.x, o.y, o.z, v);
    A.g0[pix] = make_float4(ga.x, ga.y, ga.z, gb.x);
    A.g1[pix] = make_float2(gb.y, gb.z);
  }
  const uint32_t nBad = (uint32_t)__popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0) { sBad[threadIdx.x >> 6] = nBad; sTmp[threadIdx.x >> 6] = nTemporal; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    A.tileBad[tile] = (sBad[0] + sBad[1]) + (sBad[2] + sBad[3]);
    A.tileTemporal[tile] = (sTmp[0] + sTmp[1]) + (sTmp[2] + sTmp[3]);
  }
}

hipError_t sail_launch_moment_reproject(const SailMomentReprojectArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_moment_reproject_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_moment_reproject_moved(const SailMomentReprojectMovedArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_moment_reproject_moved_kernel, dim3((A.base.W + 15) / 16, (A.base.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_moment_resolve(const SailMomentResolveArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_moment_resolve_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_tfilter_prepare(const SailTfilterPrepareArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_tfilter_prepare_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
