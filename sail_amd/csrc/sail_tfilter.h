// sail_tfilter.h — arguments of the temporal filter's kernels (sail_tfilter.hip), shared with the host library. Kept out of
// sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <stdint.h>

struct SailMomentResolveArgs {
  const float4* S;        // the accumulator the context shows
  const float4* MR;
  float4* Mout;           // out: (mu1, mu2, mm, 0) of the current view
  int W, H;
  int mix;                // 1: S holds running means over kf samples (SAIL_ACCUM_MIX); 0: sums with counts in .w
  float kf;
  float cap;
};

struct SailTfilterPrepareArgs {
  const float4* Out;      // the resolved picture of the current view (o, mo)
  const float4* Mout;     // its moments
  const float4* S;        // the accumulator the context shows: only .w is read, and only when mix == 0
  const float4* N;        // normal AOV as stored (0.5 n + 0.5)
  const float4* X;        // position AOV as stored
  float4* cv;             // out: (Out.rgb, prefiltered variance): sail_denoise_atrous_kernel's input
  float4* g0;             // out: (decoded normal, position.x)
  float2* g1;             // out: (position.y, position.z)
  uint32_t* tileBad;      // out, per 16x16 tile: pixels whose colour is not finite
  uint32_t* tileTemporal; // out, per tile: pixels whose variance came from the moments
  int W, H;
  int mix;
  float kf;
  float minHist;
  float sx0;              // (sigma_x * 2) * (sigma_x * 2)
};
