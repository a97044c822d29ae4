// sail_denoise.h — arguments of the denoiser's kernels (sail_denoise.hip), shared with the host library. Kept out of
// sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <stdint.h>

struct SailDenoisePrepareArgs {
  const float4* S;     // the accumulator the context shows
  const float4* P;     // the noise estimate's mark
  const float4* N;     // normal AOV as stored (0.5 n + 0.5)
  const float4* X;     // position AOV as stored
  float4* cv;          // out: (mean colour, prefiltered variance of the mean's luminance)
  float4* g0;          // out: (decoded normal, position.x)
  float2* g1;          // out: (position.y, position.z)
  uint32_t* tileBad;   // out, per 16x16 tile: pixels whose mean colour is not finite
  int W, H;
  int mix;             // 1: S and P hold running means over kf and hf samples (SAIL_ACCUM_MIX); 0: sums with counts in .w
  float kf, hf;        // the context's sample index now and at the mark (MIX)
};

struct SailDenoiseAtrousArgs {
  const float4* src;   // (c, v) of the pass before
  float4* dst;         // (c, v) of this pass; the last pass stores (c, 1), the RGBA output (may be NULL then)
  const float4* g0;
  const float2* g1;
  float* outVar;       // last pass: the filtered variance (may be NULL)
  uint32_t* out8;      // last pass: the display transform of c as RGBA8, one word per pixel (may be NULL)
  int W, H;
  int step;            // 1 << pass
  int last;
  float sl2;           // sigma_l * sigma_l
  float sxs;           // (sigma_x * step) * (sigma_x * step)
  int display;         // 0 colour, 1 gamma, 2 tonemapping
  float gammaC;
};
