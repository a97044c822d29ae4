// sail_albedo.h — arguments of the albedo map's kernel (sail_albedo.hip) and of the albedo-demodulated instances of the
// denoiser's and the temporal filter's kernels (sail_denoise.hip, sail_tfilter.hip), shared with the host library. Kept out
// of sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <stdint.h>
#include "sail_denoise.h"
#include "sail_tfilter.h"
#include "sail_temporal.h"

struct SailAlbedoArgs {
  SailViewArgs V;           // the rows and the view
  const float* texparams;   // the scene's texParams table
  int tn;
  uint32_t texMask;         // the scene's own texture plugins: a texture outside it gives 0, as in a render
  int grid;                // g: g * g sub-pixel rays per pixel, 1..4
  float4* A;                // out: (mean surface colour, rays that hit); no hit stores (1, 1, 1, 0)
  uint32_t* tileHit;        // out, per 16x16 tile: pixels with a hit (A.w > 0)
  uint32_t* tilePartial;    // out, per tile: pixels where some but not all rays hit (0 < A.w < g * g)
};

// The demodulated instances take the plain kernel's arguments and the map: f = A.rgb where finite and > amin, else 1
struct SailDenoisePrepareDemodArgs {
  SailDenoisePrepareArgs P;
  const float4* alb;
  float amin;
};

struct SailTfilterPrepareDemodArgs {
  SailTfilterPrepareArgs P;
  const float4* alb;
  float amin;
};

struct SailDenoiseAtrousRemodArgs {
  SailDenoiseAtrousArgs P;  // P.last is set: the remodulating instance is the last pass
  const float4* alb;
  float amin;
};
