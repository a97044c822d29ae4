// sail_denoise.hip — the variance-guided a-trous denoiser of a progressive frame on the MI355X (gfx950):
// sail_denoise_prepare_kernel and sail_denoise_atrous_kernel, and their albedo-demodulated instances
// sail_denoise_prepare_demod_kernel and sail_denoise_atrous_remod_kernel (sail_denoise_albedo; the remodulating pass also
// ends sail_temporal_filter_albedo).
//
// No reference counterpart (the reference's only denoiser is the `wavelet` display filter, sail_filter_kernel kind 4,
// whose edge stops are constants and which never reads the normal map). This one is the edge-avoiding a-trous wavelet of
// SVGF (Schied et al. 2017; Dammertz et al. 2010) without the temporal part: the variance of the mean's luminance comes
// from the two half buffers the noise estimate already keeps (S, the accumulator shown, and P, the mark), and steers the
// luminance edge stop per pixel; the normal and position AOVs stop the other edges. The formula and its f32 operation
// order are part of the C ABI (include/sail_hip.h, sail_denoise). Weights are rational, not exp(): every operation is an
// IEEE one, so a numpy float32 restatement gives the same bits (tests/atrous_ref.py, tests/test_gpu_denoise.py). The
// shown mean, the 3x3 prefilter, the display transform and the per-tile count are sail_post.h's, shared with the temporal
// kernels (sail_temporal.hip, sail_tfilter.hip).
//
// MI355X design:
//  * prepare: one 256-thread workgroup per 16x16 tile, one lane per pixel; the raw variance of the tile and a one-texel
//    halo (18x18) is staged in LDS for the 3x3 prefilter; texels outside the frame hold NaN there, which the prefilter
//    skips like any non-finite tap. It writes (c, v) as one float4 and the guides as a float4 (decoded normal,
//    position.x) and a float2 (position.yz): 40 B per texel for every later pass;
//  * a-trous, one launch per pass: for step s a workgroup owns ONE residue class (x mod s, y mod s) and a 16x16 block
//    of that class's decimated grid, so its LDS tile is 20x20 texels whatever the step and all 25 taps of every pixel
//    come from LDS. The strided global loads of one class are completed by the neighbouring classes' workgroups
//    (adjacent blockIdx.x) out of L2 / the last-level cache;
//  * LDS layout: three arrays of 20x20 texels with packed rows, two of float4 and one of float2, 16,000 B per workgroup.
//    A wave is a 16x4 strip, so a ds_read_b128 lane group (16 lanes over two rows 80 dwords apart) meets some banks
//    twice. A conflict-free layout (row strides of 32 and 48 texels, 28 KB) measured the same: the pass is bound by its
//    VALU work, above all the formula's IEEE divides, not by LDS;
//  * the formula's two reciprocals 1 / (1 + q) are sm::rcp_rn, which equals the IEEE 1.0f / b for every f32 b
//    (sail_math.h); the two quotients stay IEEE divides;
//  * texels outside the frame are never loaded (their LDS slots hold zeros and their taps are skipped by coordinates);
//    lanes outside ragged tiles load nothing and store nothing;
//  * the last pass stores the RGBA output, the variance and the display transform as RGBA8 in one 32-bit store;
//  * plain vector stores only, no atomics: equal data give equal bits;
//  * the demodulated instances ("sail_albedo_kernel and the albedo-demodulated filters") are second
//    instances of the same bodies, entry points of their own, not run-time switches: the plain kernels pay no map load.
// Lives in its own file, no part of the text embedded in the library and hashed into every run-time kernel's cache key
// (sail_amd/gen_jit_src.py), and defines no macro. Built with the library's flags (no contraction, no fast math: `/` is the IEEE divide).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_post.h"
#include "sail_denoise.h"
#include "sail_albedo.h"

namespace {

constexpr int kDnT = 20;  // a-trous LDS tile: 16 + 2 * 2 taps, rows packed

// variance of the mean's luminance from the two halves (include/sail_hip.h): every operation rounds to f32, in this order
__device__ __forceinline__ float dnRawVariance(const float4 s, const float4 p, int mix, float kf, float hf) {
  const float n = mix ? kf : s.w, h = mix ? hf : p.w;
  if (!(h > 0.0f) || !(n > h)) return 0.0f;
  const float dn = n - h;
  float ar, ag, ab, br, bg, bb;
  if (mix) {
    ar = p.x; ag = p.y; ab = p.z;
    br = ((n * s.x) - (h * ar)) / dn; bg = ((n * s.y) - (h * ag)) / dn; bb = ((n * s.z) - (h * ab)) / dn;
  } else {
    ar = p.x / h; ag = p.y / h; ab = p.z / h;
    br = (s.x - p.x) / dn; bg = (s.y - p.y) / dn; bb = (s.z - p.z) / dn;
  }
  const float dl = sp::lum(ar, ag, ab) - sp::lum(br, bg, bb);
  return (dl * dl) * ((h * dn) / (n * n));
}

}  // namespace

// The prepare pass. DEMOD = false is sail_denoise_prepare_kernel (alb and amin are not read). DEMOD = true is
// sail_denoise_albedo's (include/sail_hip.h): S and P are divided by the albedo factor f channel by channel, an IEEE divide
// each, before anything else reads them: two more float4 loads per texel of the variance stage's halo (the map at q) and
// one per pixel, which the plain kernel does not pay.
template <bool DEMOD>
__device__ __forceinline__ void dnPrepare(const SailDenoisePrepareArgs& A, const float4* alb, float amin) {
  __shared__ float sV[sp::kVarT * sp::kVarT];
  __shared__ uint32_t sBad[1][4];
  const int x0 = (int)blockIdx.x * 16 - 1, y0 = (int)blockIdx.y * 16 - 1;
  for (int t = threadIdx.x; t < sp::kVarT * sp::kVarT; t += 256) {
    const int ly = t / sp::kVarT, lx = t - ly * sp::kVarT;
    const int qx = x0 + lx, qy = y0 + ly;
    float v = __builtin_nanf("");  // outside the frame: skipped by the prefilter
    if (qx >= 0 && qx < A.W && qy >= 0 && qy < A.H) {
      const size_t q = (size_t)qy * A.W + qx;
      float4 sq = A.S[q], pq = A.P[q];
      if (DEMOD) {
        const sp::Rgb f = sp::albedoFactor(alb[q], amin);
        sq = make_float4(sq.x / f.r, sq.y / f.g, sq.z / f.b, sq.w);
        pq = make_float4(pq.x / f.r, pq.y / f.g, pq.z / f.b, pq.w);
      }
      v = dnRawVariance(sq, pq, A.mix, A.kf, A.hf);
    }
    sV[t] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x = (int)blockIdx.x * 16 + lx, y = (int)blockIdx.y * 16 + ly;
  bool bad = false;
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    float4 s = A.S[pix];
    if (DEMOD) {
      const sp::Rgb f = sp::albedoFactor(alb[pix], amin);
      s = make_float4(s.x / f.r, s.y / f.g, s.z / f.b, s.w);
    }
    const sp::Rgb c = sp::shownMean(s, A.mix, s.w);
    bad = !(sp::finite(c.r) && sp::finite(c.g) && sp::finite(c.b));
    const float v = sp::prefilter(sV, lx, ly);
    const float4 nn = A.N[pix], xp = A.X[pix];
    A.cv[pix] = make_float4(c.r, c.g, c.b, v);
    A.g0[pix] = make_float4(2.0f * nn.x - 1.0f, 2.0f * nn.y - 1.0f, 2.0f * nn.z - 1.0f, xp.x);
    A.g1[pix] = make_float2(xp.y, xp.z);
  }
  sp::tileCounts<1>({sp::waveCount(bad)}, sBad, {A.tileBad});
}

extern "C" __global__ void __launch_bounds__(256) sail_denoise_prepare_kernel(SailDenoisePrepareArgs A) {
  dnPrepare<false>(A, nullptr, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) sail_denoise_prepare_demod_kernel(SailDenoisePrepareDemodArgs A) {
  dnPrepare<true>(A.P, A.alb, A.amin);
}

// One a-trous pass. REMOD = false is sail_denoise_atrous_kernel (alb and amin are not read). REMOD = true is the last pass
// of the demodulated filters: the outputs are multiplied by the albedo factor again (colour by f, variance by lf * lf): one
// more float4 load per pixel. With a step above 1 a wave's pixels lie `step` texels apart, so that load, like the pass's
// stores, uses 16 bytes of every cache line it touches: loading the texel ahead of the taps measured the same.
template <bool REMOD>
__device__ __forceinline__ void dnAtrous(const SailDenoiseAtrousArgs& A, const float4* alb, float amin) {
  __shared__ float4 sCV[kDnT * kDnT];
  __shared__ float4 sG0[kDnT * kDnT];
  __shared__ float2 sG1[kDnT * kDnT];
  const int s = A.step;
  const int classesX = s < A.W ? s : A.W, classesY = s < A.H ? s : A.H;  // residue classes that hold a pixel
  const int rx = (int)blockIdx.x % classesX, bx = (int)blockIdx.x / classesX;
  const int ry = (int)blockIdx.y % classesY, by = (int)blockIdx.y / classesY;
  for (int t = threadIdx.x; t < kDnT * kDnT; t += 256) {
    const int tj = t / kDnT, ti = t - tj * kDnT;
    const int qx = rx + s * (bx * 16 - 2 + ti), qy = ry + s * (by * 16 - 2 + tj);
    float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = cv;
    float2 g1 = make_float2(0.0f, 0.0f);
    if (qx >= 0 && qx < A.W && qy >= 0 && qy < A.H) {
      const size_t q = (size_t)qy * A.W + qx;
      cv = A.src[q]; g0 = A.g0[q]; g1 = A.g1[q];
    }
    sCV[tj * kDnT + ti] = cv;
    sG0[tj * kDnT + ti] = g0;
    sG1[tj * kDnT + ti] = g1;
  }
  __syncthreads();
  const int li = threadIdx.x & 15, lj = threadIdx.x >> 4;
  const int x = rx + s * (bx * 16 + li), y = ry + s * (by * 16 + lj);
  if (x >= A.W || y >= A.H) return;
  const float4 cp = sCV[(lj + 2) * kDnT + (li + 2)];
  const float4 gp = sG0[(lj + 2) * kDnT + (li + 2)];
  const float2 hp = sG1[(lj + 2) * kDnT + (li + 2)];
  const float den = A.sl2 * cp.w + 1e-8f;
  const float lp = sp::lum(cp.x, cp.y, cp.z);
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, vacc = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + s * dy;
    if (qy < 0 || qy >= A.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + s * dx;
      if (qx < 0 || qx >= A.W) continue;
      const int ady = dy < 0 ? -dy : dy, adx = dx < 0 ? -dx : dx;
      const float ky = ady == 0 ? 0.375f : (ady == 1 ? 0.25f : 0.0625f);
      const float kx = adx == 0 ? 0.375f : (adx == 1 ? 0.25f : 0.0625f);
      const float kw = ky * kx;
      const float4 cq = sCV[(lj + 2 + dy) * kDnT + (li + 2 + dx)];
      float w = kw;
      if (dy != 0 || dx != 0) {
        const float4 gq = sG0[(lj + 2 + dy) * kDnT + (li + 2 + dx)];
        const float2 hq = sG1[(lj + 2 + dy) * kDnT + (li + 2 + dx)];
        float d = sm::fmax_((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.0f);
        d = d * d; d = d * d; d = d * d; d = d * d; d = d * d; d = d * d;
        const float tx = gp.w - gq.w, ty = hp.x - hq.x, tz = hp.y - hq.y;
        const float dx2 = (tx * tx + ty * ty) + tz * tz;
        const float wx = sm::rcp_rn(1.0f + dx2 / A.sxs);
        const float dq = lp - sp::lum(cq.x, cq.y, cq.z);
        const float wl = sm::rcp_rn(1.0f + (dq * dq) / den);
        w = ((kw * d) * wx) * wl;
      }
      if (w > 0.0f && sp::finite(cq.x) && sp::finite(cq.y) && sp::finite(cq.z) && sp::finite(cq.w)) {
        ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
        vacc += (w * w) * cq.w;
        wsum += w;
      }
    }
  }
  float4 o = cp;
  if (wsum > 0.0f) o = make_float4(ar / wsum, ag / wsum, ab / wsum, vacc / (wsum * wsum));
  const size_t pix = (size_t)y * A.W + x;
  if (!A.last) { A.dst[pix] = o; return; }
  if (REMOD) {
    const sp::Rgb f = sp::albedoFactor(alb[pix], amin);
    const float lf = sp::lum(f.r, f.g, f.b);
    o = make_float4(o.x * f.r, o.y * f.g, o.z * f.b, o.w * (lf * lf));
  }
  if (A.dst) A.dst[pix] = make_float4(o.x, o.y, o.z, 1.0f);
  if (A.outVar) A.outVar[pix] = o.w;
  if (A.out8) A.out8[pix] = sp::rgba8(o.x, o.y, o.z, A.display, A.gammaC);
}

extern "C" __global__ void __launch_bounds__(256) sail_denoise_atrous_kernel(SailDenoiseAtrousArgs A) {
  dnAtrous<false>(A, nullptr, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) sail_denoise_atrous_remod_kernel(SailDenoiseAtrousRemodArgs A) {
  dnAtrous<true>(A.P, A.alb, A.amin);
}

hipError_t sail_launch_denoise_prepare(const SailDenoisePrepareArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_denoise_prepare_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_denoise_prepare_demod(const SailDenoisePrepareDemodArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_denoise_prepare_demod_kernel, dim3((A.P.W + 15) / 16, (A.P.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_denoise_atrous(const SailDenoiseAtrousArgs& A, hipStream_t s) {
  // per axis: the residue classes that hold a pixel, times the 16-wide blocks of the largest class (class 0)
  const int cx = A.step < A.W ? A.step : A.W, cy = A.step < A.H ? A.step : A.H;
  const int nx = ((A.W + A.step - 1) / A.step + 15) / 16, ny = ((A.H + A.step - 1) / A.step + 15) / 16;
  hipLaunchKernelGGL(sail_denoise_atrous_kernel, dim3(cx * nx, cy * ny), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_denoise_atrous_remod(const SailDenoiseAtrousRemodArgs& R, hipStream_t s) {
  const SailDenoiseAtrousArgs& A = R.P;
  const int cx = A.step < A.W ? A.step : A.W, cy = A.step < A.H ? A.step : A.H;
  const int nx = ((A.W + A.step - 1) / A.step + 15) / 16, ny = ((A.H + A.step - 1) / A.step + 15) / 16;
  hipLaunchKernelGGL(sail_denoise_atrous_remod_kernel, dim3(cx * nx, cy * ny), dim3(256), 0, s, R);
  return hipGetLastError();
}
