// sail_noise.hip — the noise estimate of a progressive frame on the MI355X (gfx950): sail_noise_kernel.
//
// No reference counterpart (the reference accumulates until the user stops looking). The estimate is the half-buffer
// one of progressive tracers (Cycles, pbrt-v4): S is the accumulator the context shows, P a snapshot of it taken
// earlier (the mark), and each pixel compares the mean of the samples before the mark with the mean of those since.
// The formula and its f32 operation order are part of the C ABI (include/sail_hip.h, sail_noise_estimate).
//
// MI355X design (DESIGN.md §Noise estimate):
//  * one 256-thread workgroup per 16x16 tile, one lane per pixel, each wave a 16x4 strip (sail_filter_kernel's shape):
//    one float4 load of S and one of P per lane, 256-byte runs per row;
//  * the tile's sum is reduced within the wave by a butterfly of cross-lane adds, then across the four waves through
//    LDS as (w0 + w1) + (w2 + w3): a fixed tree of depth 8 and no atomics, so equal data give equal bits;
//  * lanes outside the frame (ragged tiles) load nothing and add +0;
//  * with remark each lane stores the float4 of S it just read into P: a doubling schedule costs one pass per look;
//  * with a tile mask (active64) the workgroup tests its 64x64 tile's byte, uniformly, and the remark store (and
//    sail_noise_copy_kernel, the masked sail_noise_mark) leaves the P of a frozen tile alone; the estimate reads no mask;
//  * plain vector stores only.
// The finite test and the wave count are sail_post.h's; the reduction stays here, since the sum and the count share its
// one barrier. Lives in its own file, no part of the text embedded in the library and hashed into every run-time
// kernel's cache key (sail_amd/gen_jit_src.py). Built with the library's flags (no contraction, no fast math: `/` and sqrt are the IEEE ones, as
// sail_math_probe functions 7 and 8 show on the device).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_post.h"
#include "sail_noise.h"

namespace {

// the per-pixel error (include/sail_hip.h): every operation rounds to f32, in this order
__device__ __forceinline__ float noiseError(const float4 s, const float4 p, int mix, float kf, float hf) {
  const float n = mix ? kf : s.w, h = mix ? hf : p.w;
  if (!(h > 0.0f) || !(n > h)) return 0.0f;  // no samples, or none since the mark
  float ar, ag, ab, br, bg, bb, mr, mg, mb;
  if (mix) {  // running means: a = P, m = S, b = (n m - h a) / (n - h)
    ar = p.x; ag = p.y; ab = p.z;
    mr = s.x; mg = s.y; mb = s.z;
    const float dn = n - h;
    br = ((n * mr) - (h * ar)) / dn; bg = ((n * mg) - (h * ag)) / dn; bb = ((n * mb) - (h * ab)) / dn;
  } else {    // sums and counts
    ar = p.x / h; ag = p.y / h; ab = p.z / h;
    const float dn = n - h;
    br = (s.x - p.x) / dn; bg = (s.y - p.y) / dn; bb = (s.z - p.z) / dn;
    mr = s.x / n; mg = s.y / n; mb = s.z / n;
  }
  const float d = (__builtin_fabsf(ar - br) + __builtin_fabsf(ag - bg)) + __builtin_fabsf(ab - bb);
  const float l = (mr + mg) + mb;
  return (0.5f * d) / (1e-4f + __builtin_sqrtf(__builtin_fmaxf(l, 0.0f) / 3.0f));
}

// whether the workgroup's 16x16 tile may write P: no mask, or its 64x64 tile (4 x 4 of these) is active
__device__ __forceinline__ bool tileWritesMark(const SailNoiseArgs& A) {
  return !A.active64 || A.active64[(size_t)(blockIdx.y >> 2) * A.tiles64X + (blockIdx.x >> 2)] != 0;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) sail_noise_kernel(SailNoiseArgs A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  float e = 0.0f;
  bool bad = false;
  const bool remark = A.remark && tileWritesMark(A);
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    const float4 s = A.S[pix], p = A.P[pix];
    e = noiseError(s, p, A.mix, A.kf, A.hf);
    if (!sp::finite(e)) { bad = true; e = 0.0f; }  // NaN or Inf: counted, adds nothing
    if (A.pixErr) A.pixErr[pix] = e;
    if (remark) A.P[pix] = s;
  }
  // within the wave: a butterfly, every lane ends with the same sum; the count is a ballot
  float v = e;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const uint32_t cnt = sp::waveCount(bad);
  // across the four waves through LDS, in a fixed order
  __shared__ float sSum[4];
  __shared__ uint32_t sBad[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sSum[wave] = v; sBad[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    A.tileSum[tile] = (sSum[0] + sSum[1]) + (sSum[2] + sSum[3]);
    A.tileBad[tile] = (sBad[0] + sBad[1]) + (sBad[2] + sBad[3]);
  }
}

// sail_noise_mark under a tile mask: P = S in the 16x16 tiles of active 64x64 tiles, the others keep their P
extern "C" __global__ void __launch_bounds__(256) sail_noise_copy_kernel(SailNoiseArgs A) {
  if (!tileWritesMark(A)) return;  // uniform over the workgroup
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x < A.W && y < A.H) {
    const size_t pix = (size_t)y * A.W + x;
    A.P[pix] = A.S[pix];
  }
}

hipError_t sail_launch_noise_copy(const SailNoiseArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_noise_copy_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t sail_launch_noise(const SailNoiseArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_noise_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
