// sail_noise.h — arguments of the noise-estimate kernel (sail_noise.hip), shared with the host library. Kept out of
// sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <stdint.h>

struct SailNoiseArgs {
  const float4* S;     // the accumulator the context shows
  float4* P;           // the mark: a snapshot of it taken earlier (rewritten with S when remark is set)
  float* tileSum;      // per 16x16 tile: the sum of its pixels' finite errors
  uint32_t* tileBad;   // per tile: how many of its pixels' errors are not finite
  float* pixErr;       // optional W x H per-pixel error map (0 where not finite)
  int W, H;
  int mix;             // 1: S and P hold running means over kf and hf samples (SAIL_ACCUM_MIX); 0: sums with counts in .w
  float kf, hf;        // the context's sample index now and at the mark (MIX)
  int remark;          // 1: P = S in the same pass
  // optional tile mask (sail_set_active_tiles): one byte per 64x64 tile, tiles64X a row; with it the remark and
  // sail_noise_copy_kernel write P only in 16x16 tiles whose 64x64 tile is active
  const uint8_t* active64;
  int tiles64X;
};
