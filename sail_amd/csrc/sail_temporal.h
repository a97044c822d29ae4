// sail_temporal.h — arguments of the camera-motion reprojection kernels (sail_temporal.hip), shared with the host library.
// Kept out of sail_device.h: that file's text is embedded in the library and hashed into every run-time kernel's cache key.
#pragma once
#include <stdint.h>

struct SailPrim;

// A view of the scene as the passes that shoot a ray per pixel take it (sail_view.h): a member of the G-buffer, albedo
// and guide kernels' arguments, filled by the host's viewArgs
struct SailViewArgs {
  const SailPrim* prims;  // the scene's rows, swept in order
  int n;
  float d[4][3];          // corner directions of the zero-jitter inverse (the host's cornerDirs)
  float eye[3];
  int W, H;
};

struct SailGbufferArgs {
  SailViewArgs V;
  float4* G;          // out: (X.xyz, (float)id); a miss stores (0, 0, 0, -1)
  float* rays;            // out, may be NULL: 6 floats per pixel, origin then direction
  float* t;               // out, may be NULL: the hit distance, 1e5 on a miss
};

// The four reproject kernels: sail_reproject_kernel and sail_reproject_moved_kernel over the colour history (hist = Hist,
// out = R), sail_moment_reproject_kernel and sail_moment_reproject_moved_kernel over the moments (hist = Mhist, out = MR,
// no counts). The gather itself is sail_post.h's.
struct SailReprojectArgs {
  const float4* Gcur;
  const float4* Gprev;
  const float4* hist;     // the previous view's (rgb mean, effective sample count), or its (mu1, mu2, mm, 0)
  float4* out;            // out: hist seen from the new view, or 0
  uint32_t* tileHit;      // out, per 16x16 tile: pixels of the new view that hit the scene (NULL for the moments)
  uint32_t* tileHist;     // out, per tile: pixels that found a history (NULL for the moments)
  float Mp[3][4];         // rows 0, 1 and 3 of the previous view's P*MV in f32
  float eyePrev[3];
  float tol2;             // pos_tol * pos_tol
  int W, H;
  int haveHist;           // 0: no committed history, out = 0 everywhere (Gprev and hist are not read)
  // the moved kernels only, after sail_move_objects; the plain ones read none of these
  const float4* motion;   // n rows of (d.xyz, 0): each row's translation since G_prev, read per lane by G_cur's id
  int n;
  float mc;               // the count of a history that crosses the move is at most this (+inf: no cap)
};

struct SailResolveArgs {
  const float4* S;        // the accumulator the context shows
  const float4* R;
  float4* Out;            // out: (o, mo)
  uint32_t* out8;         // out, may be NULL: the display transform of o as RGBA8, one word per pixel
  uint32_t* tileHist;     // out, per tile: pixels with a history (R.w > 0)
  uint32_t* tileBad;      // out, per tile: pixels whose current mean is not finite
  int W, H;
  int mix;                // 1: S holds running means over kf samples (SAIL_ACCUM_MIX); 0: sums with counts in .w
  float kf;
  float cap;
  int display;            // 0 colour, 1 gamma, 2 tonemapping
  float gammaC;
};
