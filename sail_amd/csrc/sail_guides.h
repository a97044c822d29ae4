// sail_guides.h — arguments of the guide maps' kernel (sail_guides.hip), shared with the host library. Kept out of
// sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sail_temporal.h"

struct SailGuidesArgs {
  SailViewArgs V;           // the rows and the view
  const float* texparams;   // the scene's texParams table: the material rows of the walk
  int tn;
  uint32_t matMask;         // the scene's own material plugins: a category outside it is not followed, as in a render
  uint32_t texMask;         // the scene's own texture plugins (the hit record's surface colour)
  int depth;               // D: mirror and smooth glass are followed at most this many times, 0..8
  float4* Ng;               // out: (0.5 n + 0.5, depth walked); a miss stores (0.5, 0.5, 0.5, 0)
  float4* Xg;               // out: (normalize(p), row); a miss stores (NaN, NaN, NaN, -1)
  uint32_t* tileHit;        // out, per 16x16 tile: pixels whose first ray hit (Xg.w >= 0)
  uint32_t* tileFollowed;   // out, per tile: pixels that left their first surface (Ng.w > 0)
  uint32_t* tileTruncated;  // out, per tile: pixels stopped by D on a surface that could be followed
};
