// sail_tfilter.hip — the filter of a reprojected frame on the MI355X (gfx950): sail_moment_reproject_kernel,
// sail_moment_resolve_kernel and sail_tfilter_prepare_kernel, and the latter's albedo-demodulated instance
// sail_tfilter_prepare_demod_kernel (sail_temporal_filter_albedo).
//
// No reference counterpart (the reference throws the picture away on every camera move). This is the piece SVGF (Schied et
// al. 2017) has between its temporal accumulation and its a-trous filter: the first two moments of each pixel's luminance
// are reprojected and blended exactly like the colour (sail_temporal.hip), and give a per-pixel variance that survives a
// camera move; where the moments are young or disoccluded a 7x7 spatial estimate over the resolved picture stands in. The
// prepare pass writes exactly the (cv, g0, g1) maps sail_denoise_atrous_kernel reads, so the a-trous passes run unchanged
// over the resolved picture `Out`. The formulas and their f32 operation order are part of the C ABI (include/sail_hip.h,
// sail_temporal_moments / sail_temporal_filter); every operation is an IEEE one, so a numpy float32 restatement gives the
// same bits (tests/temporal_filter_ref.py, tests/test_gpu_temporal_filter.py). The gather, the shown mean, the 3x3
// prefilter and the per-tile counts are sail_post.h's, shared with sail_temporal.hip and sail_denoise.hip.
//
// MI355X design ("sail_tfilter_prepare_kernel"):
//  * all three: one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip; float4 loads and stores;
//  * moment reproject: the tap of sp::gather reads Mhist and accepts a texel with a count (.z) and finite moments; no
//    per-tile counts. sail_moment_reproject_moved_kernel is the MOVED instance, as sail_reproject_moved_kernel;
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
//  * the prepare pass's two counts are wave ballots behind one barrier (sp::tileCounts), summed per tile on the host;
//  * plain vector stores only, no atomics: equal data give equal bits.
// Lives in its own file, no part of the text embedded in the library and hashed into every run-time kernel's cache key
// (sail_amd/gen_jit_src.py), and defines no macro. Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_post.h"
#include "sail_tfilter.h"
#include "sail_albedo.h"

namespace {

constexpr int kTfS = 24;        // stage: 16 + 2 * (1 prefilter + 3 window) texels, rows packed
constexpr int kTfV = sp::kVarT;  // v0: 16 + 2 * 1, the tile sp::prefilter reads

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
        float d = sp::max_((pa.x * qa.x + pa.y * qa.y) + pa.z * qa.z, 0.0f);
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
  return sp::max_(a2 / ws - m1 * m1, 0.0f);
}

}  // namespace

// The moment reproject pass: sail_temporal.hip's tpReproject over Mhist, with .z as the count, and no per-tile counts.
// MOVED as there.
template <bool MOVED>
__device__ __forceinline__ void tfMomentReproject(const SailReprojectArgs& A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= A.W || y >= A.H) return;
  const size_t pix = (size_t)y * A.W + x;
  const float4 g = A.Gcur[pix];
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (!(g.w < 0.0f) && A.haveHist) {
    float a1 = 0.0f, a2 = 0.0f, wsum = 0.0f, m = __builtin_inff();
    sp::gather<MOVED>(
        A, g,
        [&](float w, size_t q) {
          const float4& h = A.hist[q];  // a reference: .z, .x and .y are loaded one by one, each where it is first tested
          if (!(h.z > 0.0f) || !(sp::finite(h.x) && sp::finite(h.y))) return;
          a1 += w * h.x; a2 += w * h.y;
          wsum += w;
          m = sp::min_(m, h.z);
        },
        [&] {
          if (wsum > 0.0f) out = make_float4(a1 / wsum, a2 / wsum, MOVED ? sp::min_(m, A.mc) : m, 0.0f);
        });
  }
  A.out[pix] = out;
}

extern "C" __global__ void __launch_bounds__(256) sail_moment_reproject_kernel(SailReprojectArgs A) { tfMomentReproject<false>(A); }

extern "C" __global__ void __launch_bounds__(256) sail_moment_reproject_moved_kernel(SailReprojectArgs A) { tfMomentReproject<true>(A); }

extern "C" __global__ void __launch_bounds__(256) sail_moment_resolve_kernel(SailMomentResolveArgs A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= A.W || y >= A.H) return;
  const size_t pix = (size_t)y * A.W + x;
  const float4 s = A.S[pix], r = A.MR[pix];
  const float n = sp::shownCount(s, A.mix, A.kf);
  const sp::Rgb c = sp::shownMean(s, A.mix, n);
  const float l = sp::lum(c.r, c.g, c.b);
  const bool cur = n > 0.0f && sp::finite(c.r) && sp::finite(c.g) && sp::finite(c.b);
  const float mh = r.z;
  const bool hist = mh > 0.0f;
  float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (hist && cur) {
    const float ws = mh + n;
    o = make_float4(((mh * r.x) + (n * l)) / ws, ((mh * r.y) + (n * (l * l))) / ws, sp::min_(ws, A.cap), 0.0f);
  } else if (hist) {
    o = r;
  } else if (cur) {
    o = make_float4(l, l * l, sp::min_(n, A.cap), 0.0f);
  }
  A.Mout[pix] = o;
}

// The prepare pass. DEMOD = false is sail_tfilter_prepare_kernel (alb and amin are not read). DEMOD = true is
// sail_temporal_filter_albedo's (include/sail_hip.h): wherever the text reads c it is Out.rgb divided by the albedo factor
// f channel by channel, so the stage holds the demodulated luminance and its finiteness, vt is divided by lf * lf, and
// the a-trous input is the demodulated colour: one more float4 load per texel of the stage, of the v0 tile and per pixel.
template <bool DEMOD>
__device__ __forceinline__ void tfPrepare(const SailTfilterPrepareArgs& A, const float4* alb, float amin) {
  __shared__ float4 sA[kTfS * kTfS];  // (decoded normal, luminance)
  __shared__ float4 sB[kTfS * kTfS];  // (position, usable)
  __shared__ float sV[kTfV * kTfV];
  __shared__ uint32_t sCnt[2][4];
  const int tx0 = (int)blockIdx.x * 16, ty0 = (int)blockIdx.y * 16;
  // 1. the stage
  for (int t = threadIdx.x; t < kTfS * kTfS; t += 256) {
    const int sy = t / kTfS, sx = t - sy * kTfS;
    const int qx = tx0 - 4 + sx, qy = ty0 - 4 + sy;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (qx >= 0 && qx < A.W && qy >= 0 && qy < A.H) {
      const size_t q = (size_t)qy * A.W + qx;
      float4 o = A.Out[q];
      const float4 nn = A.N[q], xp = A.X[q];
      if (DEMOD) {
        const sp::Rgb f = sp::albedoFactor(alb[q], amin);
        o = make_float4(o.x / f.r, o.y / f.g, o.z / f.b, o.w);
      }
      const bool fin = sp::finite(o.x) && sp::finite(o.y) && sp::finite(o.z);
      a = make_float4(2.0f * nn.x - 1.0f, 2.0f * nn.y - 1.0f, 2.0f * nn.z - 1.0f, sp::lum(o.x, o.y, o.z));
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
      float vt = (sp::max_(m.y - m.x * m.x, 0.0f) * nn) / m.z;
      if (DEMOD) {
        const sp::Rgb f = sp::albedoFactor(alb[q], amin);
        const float lf = sp::lum(f.r, f.g, f.b);
        vt = vt / (lf * lf);
      }
      temporal = m.z >= A.minHist && sp::finite(vt);
      if (temporal) v0 = vt;
    }
    const bool need = inside && !temporal;
    if (__ballot(need) != 0ull) {  // wave-uniform: a wave whose lanes all have old moments skips the 49 taps
      if (need) v0 = tfSpatial(sA, sB, vx + 3, vy + 3, A.sx0);
    }
    if (t < kTfV * kTfV) sV[t] = v0;
    // the tile's own pixels, not its halo
    const bool own = temporal && vx >= 1 && vx <= 16 && vy >= 1 && vy <= 16;
    nTemporal += sp::waveCount(own);
  }
  __syncthreads();
  // 3. the prefilter and the a-trous passes' inputs
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  bool bad = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    float4 o = A.Out[pix];
    if (DEMOD) {
      const sp::Rgb f = sp::albedoFactor(alb[pix], amin);
      o = make_float4(o.x / f.r, o.y / f.g, o.z / f.b, o.w);
    }
    const float4 ga = sA[(ly + 4) * kTfS + (lx + 4)], gb = sB[(ly + 4) * kTfS + (lx + 4)];
    bad = !(gb.w > 0.0f);
    const float v = sp::prefilter(sV, lx, ly);
    A.cv[pix] = make_float4(o.x, o.y, o.z, v);
    A.g0[pix] = make_float4(ga.x, ga.y, ga.z, gb.x);
    A.g1[pix] = make_float2(gb.y, gb.z);
  }
  sp::tileCounts<2>({sp::waveCount(bad), nTemporal}, sCnt, {A.tileBad, A.tileTemporal});
}

extern "C" __global__ void __launch_bounds__(256) sail_tfilter_prepare_kernel(SailTfilterPrepareArgs A) {
  tfPrepare<false>(A, nullptr, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) sail_tfilter_prepare_demod_kernel(SailTfilterPrepareDemodArgs A) {
  tfPrepare<true>(A.P, A.alb, A.amin);
}

hipError_t sail_launch_moment_reproject(const SailReprojectArgs& A, bool moved, hipStream_t s) {
  hipLaunchKernelGGL(moved ? sail_moment_reproject_moved_kernel : sail_moment_reproject_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16),
                     dim3(256), 0, s, A);
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

hipError_t sail_launch_tfilter_prepare_demod(const SailTfilterPrepareDemodArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_tfilter_prepare_demod_kernel, dim3((A.P.W + 15) / 16, (A.P.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
