/* sail_hip.h — C ABI of libsail_hip.so, the MI355X drop-in for Sail's per-frame GPU work.
 *
 * Sail drives its hot path through WebGL: Renderer.update(scene) -> Tracer.update uploads the scene
 * rows as R32F textures and links a generated trace program (src/core/tracer.js:42-90,
 * src/core/shader.js:58-76); Renderer.render(scene) -> Tracer.render sets the per-frame uniforms and
 * calls gl.drawArrays (src/core/tracer.js:92-101, src/core/webgl.js:51-93), then RenderShader.render
 * runs the display filter (src/core/renderer.js:54-72). Each entry point below names the reference
 * interface it replaces. Plain C types only; the caller owns every host pointer (valid for the call);
 * the library owns all device memory; no global state; a context is used from one thread.
 * Every function returns SAIL_OK (0) or a negative SAIL_E_* code; sail_last_error() gives text.
 * The JS host binds these through the N-API addon in sail_amd/js/native.
 */
#ifndef SAIL_HIP_H
#define SAIL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAIL_ABI_VERSION 4

enum sail_status {
  SAIL_OK = 0,
  SAIL_E_INVALID = -1,   /* bad argument / shape mismatch */
  SAIL_E_HIP = -2,       /* HIP runtime error */
  SAIL_E_OOM = -3,       /* device allocation failed */
  SAIL_E_STATE = -4,     /* call out of order (e.g. render before set_scene) */
  SAIL_E_RCCL = -5,      /* collective failed or RCCL unavailable */
  SAIL_E_NODEVICE = -6   /* no HIP device */
};

/* sail_create flags */
enum sail_flags {
  SAIL_FLAG_AOV = 1u << 0,          /* keep the normal/position outputs (fstrace.glsl:15-16) */
  SAIL_FLAG_SEGMENT_COUNT = 1u << 1 /* exact in-kernel segment counter (sail_stats.segments) */
};
/* accumulation modes (sail_set_accum_mode) */
enum sail_accum_mode {
  SAIL_ACCUM_SUM = 0,    /* float4 sum + count; mean = sum / count (default, order-independent) */
  SAIL_ACCUM_MIX = 1,    /* the reference's running mean mix(e, prev, k/(k+1)) (fstrace.glsl:14) */
  SAIL_ACCUM_COMPAT8 = 2 /* MIX with the per-frame UNORM8 store of a WebGL2 RGB8 frame texture */
};
/* multi-GPU partition of one frame (sail_set_partition) */
enum sail_partition { SAIL_PART_TILES = 0, SAIL_PART_SAMPLES = 1 };
/* display filters (Scene.filter, src/shader/filter/shader.filter.js:18-30) */
enum sail_filter_kind {
  SAIL_FILTER_COLOR = 0, SAIL_FILTER_GAMMA = 1, SAIL_FILTER_TONEMAPPING = 2, SAIL_FILTER_WINDOW = 3,
  SAIL_FILTER_WAVELET = 4,  /* wavelet.glsl: a-trous over colour + position AOV (needs SAIL_FLAG_AOV) */
  SAIL_FILTER_NORMAL = 5,   /* normal.glsl: the normal AOV (needs SAIL_FLAG_AOV) */
  SAIL_FILTER_POSITION = 6  /* position.glsl: the position AOV (needs SAIL_FLAG_AOV) */
};

/* compiled plugin set (Scene.tracerConfig(), src/scene/scene.js:70-112), as bit masks over category ids:
 * shape bit = shape id (define.glsl:18-26), material bit = material id (:32-35), texture bit = texture id
 * (:38-44; UniformColor is always available), light bit = light id (:28-30). */
typedef struct sail_plugins {
  uint32_t shape_mask, material_mask, texture_mask, light_mask;
} sail_plugins;

typedef struct sail_stats {
  uint64_t samples;          /* samples accumulated since the last reset (this rank) */
  uint64_t segments;         /* exact segments traced (needs SAIL_FLAG_SEGMENT_COUNT) */
  uint64_t nominal_segments; /* pixels * samples * max_bounces of the launches since reset */
  double kernel_ms;          /* sum of trace-kernel durations (HIP events) since reset */
  double last_launch_ms;     /* duration of the most recent trace launch */
  uint32_t launches;         /* trace launches since reset */
} sail_stats;

typedef struct sail_ctx sail_ctx;

/* new Sail.Renderer(canvas) (src/core/renderer.js:9-39): one device, a W x H float accumulator.
 * device < 0 uses the current device. */
int sail_create(sail_ctx** out, int width, int height, int device, uint32_t flags);
/* new Sail.Renderer({devices: N}): ONE context over n_devices GPUs of this process (devices = NULL: 0..n-1).
 * The reference renders on one WebGL context (src/core/renderer.js:9-39, tracer.js:92-101); here the frame's
 * 64x64 tiles (or, after sail_set_partition(ctx, 0, 1, SAIL_PART_SAMPLES), its samples) are dealt across the
 * devices, each renders its share on its own stream, and readback / read_accum / filter first sum the devices'
 * accumulators into device 0 with one grouped RCCL reduce over a ncclCommInitAll communicator (progressive:
 * the sum is recomputed from the cumulative accumulators whenever something was rendered since). Every other
 * entry point fans out. Devices must be all distinct (RCCL over xGMI) or all the same one (the partition runs on
 * one GPU and a kernel sums it: the emulation the parity tests use). sail_comm_init is refused on it. */
int sail_create_multi(sail_ctx** out, int width, int height, const int* devices, int n_devices, uint32_t flags);
void sail_destroy(sail_ctx* ctx);
const char* sail_last_error(const sail_ctx* ctx); /* ctx may be NULL: last creation error */
int sail_device_count(int* count);
/* Device facts for reports (bench.py's roofline): compute units and peak engine clock in kHz. No reference
 * counterpart (WebGL exposes neither). */
int sail_device_info(int device, int* compute_units, int* clock_khz);

/* Tracer.update(scene) (src/core/tracer.js:42-90): the objects / texParams / lights rows exactly as
 * gen() serialises them (18 / 16 / 18 floats per row, Appendix A of SURVEY.md). Copied. */
int sail_set_scene(sail_ctx* ctx, const float* objects, int n, const float* texparams, int tn,
                   const float* lights, int ln, const sail_plugins* plugins);
/* Tracer.updateObjects(scene) (src/core/tracer.js:25-40): new object rows, same n; resets accumulation */
int sail_update_objects(sail_ctx* ctx, const float* objects, int n);

/* Both restart the accumulation (see sail_reset), also when they set what is already set. A running mean cannot be split by
 * samples: SAIL_ACCUM_MIX or SAIL_ACCUM_COMPAT8 under a sample partition over more than one rank (the devices of a
 * multi-device context are its ranks), and such a partition under those modes, are refused with SAIL_E_INVALID and nothing
 * changes. A multi-device context takes sail_set_partition(ctx, 0, 1, mode) only. */
int sail_set_accum_mode(sail_ctx* ctx, int mode);
int sail_set_partition(sail_ctx* ctx, int rank, int world, int mode);
int sail_set_launch_samples(sail_ctx* ctx, int spp_per_launch); /* samples per kernel launch; 0 (default) = by kernel form: 1024 for the Cornell form with 16 samples in flight, else 64 */
/* Test / study switches (no reference counterpart; none changes a result, which the parity suite checks).
 * The product's defaults are the values in brackets. */
enum sail_debug_option {
  SAIL_DEBUG_CULL_MIN_PRIMS = 1, /* scenes with >= value primitives use the padded-box pre-cull kernel [8] */
  SAIL_DEBUG_FORCE_GENERIC = 2,  /* 1: always launch the all-plugin kernel [0] */
  SAIL_DEBUG_CULL_FMA = 3,       /* 0: the plain pre-cull slab form instead of the fused one [1] */
  SAIL_DEBUG_SAMPLE_GROUPS = 4,  /* > 0: fixed sample-group count per 16x16 block [0 = sized by occupancy] */
  /* multi-device contexts of distinct devices only: 1 builds the ncclCommInitAll communicator now even for ONE
   * device, so the grouped RCCL reduce (the path of N distinct GPUs) runs on a one-GPU machine [0: a one-device
   * context needs no reduce]. Refused (SAIL_E_INVALID) on a context whose devices are all the same GPU. */
  SAIL_DEBUG_FORCE_RCCL = 5,
  /* 1: scenes on the pre-cull path are traced by the wavefront split (one sample at a time, path state in HBM, sweep /
   * shade / shadow kernels per bounce) instead of the megakernel; same results [0] */
  SAIL_DEBUG_WAVEFRONT = 6,
  /* > 0: residency rounds of workgroups queued per launch when sizing the sample groups, flat kernels [36] and the
   * pre-cull kernel [64] (SAIL_DEBUG_SAMPLE_GROUPS overrides both) */
  SAIL_DEBUG_GROUP_ROUNDS = 7,
  SAIL_DEBUG_CULL_GROUP_ROUNDS = 8,
  /* which scenes run a kernel compiled by hipRTC for exactly their plugin set at sail_set_scene (the reference's
   * per-scene program, src/scene/scene.js:70-112), a sum of bits: 1 flat-path scenes (fewer than
   * SAIL_DEBUG_CULL_MIN_PRIMS primitives) that the precompiled Cornell and room kernels do not cover, 8 those as a
   * room-family kernel (SAIL_JIT_MODE_ROOM) instead of a plain one, 4 scenes of the room kernel's set, 2 pre-cull-path
   * scenes, 16 every flat-path scene of at most 8 primitives compiled for its rows too (their count and shape types).
   * 32 the value kernel (SAIL_DEBUG_JIT_VALUES_AFTER) of a scene of at most 3 rows in the row-shading form: a wave whose
   * paths all hit one quiet row (no emission, a light term of exactly +0) shades in that row's branch, on the row's
   * material constants and without touching the radiance (profiles/rowshade.jsonl).
   * 64, inverted (a study switch: the default leaves it clear): the value kernel WITHOUT its deferred Sphere row. A value
   * kernel otherwise leaves the root solve of the scene's first Sphere row undone in the sweep of every bounce that sorts
   * its paths and is not the last, sorts the rays that may hit it under the sphere's key, and finishes the solve in the
   * sphere's waves after the sort (profiles/spheredefer.jsonl).
   * 0: the precompiled kernels only. Same results [59 = 1 + 2 + 8 + 16 + 32; measured in profiles/r04_jit_*.jsonl] */
  SAIL_DEBUG_JIT = 9,
  /* how long (ms) a launch waits for the scene's run-time kernel while it is still being built in the background; -1:
   * until it is built. Meanwhile the precompiled kernel of the scene's set renders, with the same results [0: never
   * wait, so Renderer.update / render stay interactive; the Python binding used by the tests and bench.py sets -1] */
  SAIL_DEBUG_JIT_WAIT = 10,
  /* samples of each pixel in flight per workgroup of the run-time kernels: 1, 4 or 16 (the workgroup's lanes hold
   * 256 / value pixels, 1,024 / value in the pre-cull form, each with `value` samples); 0 = the form's default */
  SAIL_DEBUG_JIT_NS = 11,
  /* threads per workgroup of the run-time kernels: 128, 256, 512 or 1024 (the path sort's pool); 0 = the form's own
   * [0: 256 flat, 1,024 pre-cull] */
  SAIL_DEBUG_JIT_NT = 12,
  /* the value kernel, a second tier on top of the scene's run-time kernel: a flat-form kernel compiled for the rows'
   * values (the decoded rows and the texParams table as constants), asked for once the context has rendered `value`
   * samples since its rows last changed (sail_set_scene, sail_update_objects, a switch or partition that changes the
   * run-time kernel; not sail_reset or the camera). 0: asked for at once; < 0: never. A launch uses it when it is loaded
   * and never waits for it; a change of the rows returns to the kernel above at the next launch. Same results [256: a
   * policy value that keeps scenes in motion and few-sample renders from compiling, not a tuned one] */
  SAIL_DEBUG_JIT_VALUES_AFTER = 13
};
int sail_set_debug(sail_ctx* ctx, int option, int value);

/* Tracer.render(mvp, eye, k) (src/core/tracer.js:92-101) = one progressive sample with the caller's
 * jittered inverse matrix (16 f32, column-major as uniformMatrix4fv uploads it, webgl.js:103) and seed.
 * One-sample frames are queued and launched together (up to sail_set_launch_samples of them per launch) when
 * nothing observes the frame in between: every entry point that reads, filters, reduces, counts or changes the
 * context launches the queue first, and a change of eye or bounce count launches it before the new sample is
 * queued. The frame is bit-identical to one launch per call (samples are accumulated in the same order); a
 * launch error of a queued sample is reported by the call that launches it. A sample's record (its corner directions, seed,
 * running-mean weight and sample index) is taken when the call is made, and sail_stats.samples and the sample index of
 * sail_save_accum count it from then on; the tile mask and the kernel are those of the launch.
 * The calls that restart the accumulation (sail_reset) and sail_load_accum do not launch the queue, they drop it: its
 * samples belong to the accumulation that goes. A refused call may leave the queue as it is. Calls that only read host state
 * launch nothing: sail_get_active_tiles, sail_kernel_name, sail_get_kernel_info, sail_kernel_ready, sail_accum_parts.
 * On a multi-device context every device has its own queue. The calls that show the reduced frame (sail_readback,
 * sail_read_accum, sail_filter, sail_reduce, the noise, denoise and temporal calls) and the calls that fan out (sail_sync,
 * sail_get_stats, the setters, sail_render_schedule) launch every device's; a call that works on one device's sub-context
 * launches that device's only (sail_pick, sail_gbuffer, sail_albedo and sail_guides on device 0, sail_save_accum on its
 * part), which no result shows: the frame is reduced from all of them before it is read. */
int sail_render(sail_ctx* ctx, const float inv_mvp[16], const float eye[3], float time_seed, int max_bounces);
/* spp samples in one call: inv_mvp = spp x 16 floats, seeds = spp floats (a deterministic schedule). */
int sail_render_schedule(sail_ctx* ctx, const float* inv_mvp, const float* seeds, const float eye[3],
                         int spp, int max_bounces);
/* Renderer.render with scene.moving: sampleCount = 0 (src/core/renderer.js:57-60). A restart of the accumulation, as are
 * sail_set_scene, sail_update_objects, sail_move_objects, sail_set_accum_mode and sail_set_partition: the accumulator is
 * zeroed, the sample index and sail_stats return to 0, queued samples are dropped, the tile mask and the noise mark go. The
 * AOV maps restart at +0, and at -0 outside the tiles of a rank of a tile partition over several ranks (the identity of
 * the reduce's sum). */
int sail_reset(sail_ctx* ctx);
int sail_sync(sail_ctx* ctx);

/* mean image (W*H*4 f32, row 0 = bottom, like glReadPixels), optional AOVs (W*H*4 each) */
int sail_readback(sail_ctx* ctx, float* rgba, float* normal, float* position);
/* raw accumulator (SUM: rgb sums + count in .w; MIX: running mean) */
int sail_read_accum(sail_ctx* ctx, float* rgba);
/* RenderShader.render (src/core/renderer.js:63) -> pixelFilter (src/shader/filter/<kind>.glsl):
 * out_rgba = W*H*4 f32 (may be NULL), out_rgba8 = W*H*4 UNORM8 canvas pixels (may be NULL).
 * weights16 = the 16-entry window table (window filters), radius (rx, ry) in pixels, gamma_c for GAMMA. */
/* Pickup.pick (src/core/pickup.js:46-66) on the GPU: for each of `count` rays (origin xyz, direction xyz;
 * f32, 6 per ray) the trace kernel's own primitive sweep returns the first object row with the smallest
 * distance (-1 on a miss) and that distance (1e5 = MAX_DISTANCE on a miss). Replaces the reference's f64 CPU
 * picker (geometry.js intersect(), whose Rectangle test has the wrong plane) with the shader's intersection. */
int sail_pick(sail_ctx* ctx, const float* rays, int count, int32_t* index, float* t);
int sail_filter(sail_ctx* ctx, int kind, const float* weights16, float rx, float ry, float gamma_c,
                float* out_rgba, uint8_t* out_rgba8);
int sail_get_stats(sail_ctx* ctx, sail_stats* out);

/* ---- device-side noise estimate and render-until-converged (no reference counterpart: the reference accumulates until
 * the user stops looking; the half-buffer estimate of progressive tracers such as Cycles and pbrt-v4) ----
 * The context keeps a snapshot P (the "mark") of the accumulator it shows, S (its own, or the reduced frame). An estimate
 * compares the mean a of the samples before the mark with the mean b of those since, per pixel, in f32 and in this order:
 *   n = S.w, h = P.w                       (SAIL_ACCUM_MIX: n, h = the sample index now and at the mark, as f32)
 *   e = 0 unless h > 0 and n > h           (no samples, or none since the mark)
 *   a = P / h, b = (S - P) / (n - h), m = S / n   per channel   (MIX: a = P, m = S, b = (n m - h a) / (n - h))
 *   e = (0.5 ((|a.r-b.r| + |a.g-b.g|) + |a.b-b.b|)) / (1e-4 + sqrt(max((m.r + m.g) + m.b, 0) / 3))
 * With equal halves 0.5 |a - b| is |m - a|, the error of the OLDER half's mean: a conservative estimate for the whole
 * frame, whose mean has twice the samples. A non-finite e (a NaN or Inf in the accumulator) counts in `nonfinite` and
 * adds nothing to any sum: one bad pixel does not keep a frame from converging. One pass over S and P on the device
 * (sail_noise_kernel: a sum per 16x16 tile, no atomics, so equal data give equal bits); the host adds the tiles in double.
 * A tile's sum is an f32 tree, fixed: the tile's rows 4 w .. 4 w + 3 are strip w, its 64 errors v[0..63] in row-major order
 * (+0 outside the frame); for off = 32, 16, 8, 4, 2, 1: v[i] = v[i] + v[i + off] for i < off; the tile is
 * (strip0 + strip1) + (strip2 + strip3). tile_err is that sum divided in double by the tile's in-frame pixels, as f32.
 * sail_reset, sail_set_scene, sail_update_objects, sail_move_objects, sail_set_accum_mode and sail_set_partition drop the mark;
 * sail_load_accum keeps it (a loaded checkpoint continues a render). SAIL_ACCUM_COMPAT8 is refused (SAIL_E_STATE): its
 * 8-bit store makes the halves' difference meaningless. On a multi-device context both calls reduce first and work on
 * device 0's frame, like sail_filter. */
typedef struct sail_noise_info {
  double mean, max_tile;       /* sum of the tiles' sums / (W H); largest tile sum / in-frame pixels of that tile */
  uint64_t k, k_mark;          /* sample index now and at the mark */
  uint64_t nonfinite;          /* pixels whose error is not finite */
  int tiles_x, tiles_y;        /* 16x16 tiles */
  double kernel_ms;            /* device time of the pass (HIP events) */
} sail_noise_info;
/* P = the shown accumulator, k_mark = k */
int sail_noise_mark(sail_ctx* ctx);
/* tile_err (may be NULL): tiles_x * tiles_y mean errors per tile, row 0 = bottom; pixel_err (may be NULL): W * H errors
 * (0 where not finite); remark != 0 also sets the mark to the current accumulator in the same pass. SAIL_E_STATE without
 * a mark or with no sample since it. */
int sail_noise_estimate(sail_ctx* ctx, sail_noise_info* out, float* tile_err, float* pixel_err, int remark);
/* host only: the next look of the doubling schedule. k < min_spp -> min_spp; else min(2k, max_spp); k >= max_spp -> k */
int sail_plan_until(uint64_t k, uint64_t min_spp, uint64_t max_spp, uint64_t* next);
typedef struct sail_until_step { uint64_t k; double mean, max_tile; } sail_until_step;
/* Render the frozen schedule (sail_schedule) from the context's sample index on, looking at sail_plan_until's indices:
 * mark at the first look (its step reports mean = max_tile = +inf: no estimate yet), estimate + remark at each later one,
 * stop when mean <= target (*converged = 1) or k == max_spp (0). The look it stops at does not re-mark: a frame that had a
 * second look keeps the mark of the look before, for sail_denoise. The frame equals sail_render_schedule over the same
 * indices bit for bit. history (may be NULL) receives the first `capacity` looks, *looks (may be NULL) the number of looks
 * made; *out is the last estimate (mean = max_tile = +inf when no look estimated). A context already at or past max_spp
 * renders nothing. No scene, SAIL_ACCUM_COMPAT8 or a half-loaded checkpoint: SAIL_E_STATE before anything is rendered. max_spp is at most 2^31 - 1 (the schedule's index type). */
int sail_render_until(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], int max_bounces, double target,
                      uint64_t min_spp, uint64_t max_spp, sail_noise_info* out, int* converged,
                      sail_until_step* history, int capacity, int* looks);

/* ---- adaptive sampling: a mask over the 64x64 partition tiles, and render-until-every-tile-converged (the use progressive
 * tracers such as Cycles and pbrt-v4 make of the estimate above; no reference counterpart) ----
 * Tiles are sail_partition_tiles': (W+63)/64 x (H+63)/64 of them, index t = ty * tilesX + tx, row 0 = bottom. With a mask
 * set, a launch traces the active tiles of the context's share and nothing else: an inactive tile's accumulator texels
 * (their sample count in .w included) and AOV texels keep what they held. Sample k has one seed and one jitter whatever the
 * mask, so a tile rendered for samples 0..k-1 and then left alone holds the bits of the uniform k-sample frame.
 *   which tiles a device traces: one device, the active tiles; SAIL_PART_TILES, its own tiles that are active;
 *     SAIL_PART_SAMPLES, the active tiles for its samples; sail_comm_init ranks likewise, each with its own intersection.
 *     A launch without an active tile of its own launches nothing; the sample index advances all the same.
 *   sail_set_active_tiles launches queued samples first, then copies `active` (count = the number of tiles; a byte != 0 is
 *     active). (NULL, 0) removes the mask. An all-ones mask is a mask (the table path) and gives the bits of none.
 *   everything that restarts the accumulator removes the mask: sail_reset, sail_set_scene, sail_update_objects,
 *     sail_move_objects, sail_set_accum_mode, sail_set_partition, sail_load_accum (a host resuming a checkpoint sets it
 *     again: checkpoints do not hold it).
 *   refused, nothing changed, (NULL, 0) too: SAIL_E_STATE in SAIL_ACCUM_MIX and SAIL_ACCUM_COMPAT8 (no per-pixel count) and on a
 *     half-loaded checkpoint; SAIL_E_INVALID for a count that is not the number of tiles (or active == NULL with count != 0).
 *     On a multi-device context a device that fails while the mask is set (memory, a HIP error) gives the devices
 *     before it their previous mask back: the devices never trace under different masks.
 *   sail_get_active_tiles: the mask as bytes 0 / 1 (all 1 without one), *n_active (may be NULL) the number of active tiles.
 *   sail_stats.nominal_segments counts a masked launch's active in-frame pixels x samples x bounces (pixels not traced
 *     earn no rate); sail_stats.samples stays the sample index.
 *   AOV maps: an inactive tile keeps its last rendered sample's values (one device, tile partitions). Under a sample
 *     partition the shown maps are those of the rank that rendered the frame's last sample, so an inactive tile shows
 *     that rank's last sample of it.
 *   the mark with a mask: sail_noise_mark and the remark of sail_noise_estimate write P only in the 16x16 tiles of active
 *     64x64 tiles. A frozen tile therefore keeps the pair (P of the look before it froze, S of the look it froze at): its
 *     error reads the same bits at every later look and sail_denoise still finds two halves there. The estimate itself does
 *     not read the mask. A context without a mark yet marks the whole frame. */
int sail_set_active_tiles(sail_ctx* ctx, const uint8_t* active, int count);
int sail_get_active_tiles(sail_ctx* ctx, uint8_t* active, int count, int* n_active);
/* host only: the next mask from sail_noise_estimate's tile_err map (16x16 tiles, row 0 = bottom). Per 64x64 tile t
 *   e64[t] = (sum of (double)tile_err16[i] * px_i) / (sum of px_i)  over its in-frame 16x16 tiles i, rows outer, in index
 *            order, px_i the in-frame pixels of i (the tile's mean pixel error, as max_tile is a 16x16 tile's)
 *   noisy[t] = !(e64[t] <= target)          (a NaN error is noisy)
 *   active[t] = prev_active[t] && (noisy[t] || (dilate && one of t's up to 8 neighbours is noisy))
 * prev_active == NULL: all ones. A frozen tile never returns, so the active set only shrinks and every active tile holds
 * exactly the samples 0..k-1. dilate (0 or 1) keeps a converged tile beside a noisy one rendering, which avoids a visible
 * seam. active may be prev_active; tile_err64 (doubles, one per tile) and n_active may be NULL. SAIL_E_INVALID: a size < 1,
 * a NaN target, a dilate outside 0..1, tile_err16 or active NULL. */
int sail_plan_adaptive(int width, int height, const float* tile_err16, double target, int dilate,
                       const uint8_t* prev_active, uint8_t* active, double* tile_err64, int* n_active);
typedef struct sail_adaptive_params {
  double target;               /* every tile's e64 <= target ends the render */
  uint64_t min_spp, max_spp;   /* as sail_render_until */
  int dilate;                  /* 0 or 1 */
} sail_adaptive_params;
typedef struct sail_adaptive_info {
  sail_noise_info noise;       /* the last estimate (mean = max_tile = +inf when no look estimated) */
  int converged;               /* 1: no tile is active */
  int active_tiles;            /* tiles still active at the end */
  int tiles_x, tiles_y;        /* 64x64 tiles */
  uint64_t pixel_samples;      /* traced by this call: sum over its launches of active in-frame pixels x samples */
  uint64_t frame_pixel_samples;  /* W H x the samples this call advanced the index by: what sail_render_until traces */
  double kernel_ms;            /* trace kernel time of this call (sail_stats.kernel_ms after - before) */
} sail_adaptive_info;
/* target +inf, min_spp 16, max_spp 1024, dilate 1 */
int sail_adaptive_defaults(sail_adaptive_params* p);
/* sail_render_until with a mask: the frozen schedule from the context's sample index on, looks at sail_plan_until's
 * indices. The first look marks. Each later look estimates (no remark in the pass), plans the mask from the estimate's
 * tile_err with the context's mask as prev_active, sets it, and, while a tile is active and k < max_spp, marks (masked)
 * and goes on. It stops when no tile is active (converged = 1) or at k == max_spp (converged = 0 unless nothing is
 * active); the look it stops at does not re-mark. The mask stays set afterwards (sail_get_active_tiles shows it) until the
 * next restart removes it, so a later call on the same context continues under it: frozen tiles stay frozen, and a call
 * that finds no tile active renders nothing. tile_samples (one per tile, may be NULL): the sample index at which the tile
 * was frozen, or k at the end for an active one. Every tile's texels equal the uniform frame's at that index, bit for bit.
 * That holds for masks this call produced: a tile switched off by hand before the call reports the sample index it was
 * switched off at (0 on a fresh accumulator) and keeps what it held, and a tile switched back on by hand reports k
 * although it lacks the samples it sat out; tile_samples means nothing for such tiles.
 * Refusals are sail_render_until's and the mask's (SAIL_ACCUM_MIX too), before anything is rendered; params == NULL: the
 * defaults. */
int sail_render_adaptive(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], int max_bounces,
                         const sail_adaptive_params* params, sail_adaptive_info* out, sail_until_step* history,
                         int capacity, int* looks, uint32_t* tile_samples);

/* ---- variance-guided a-trous denoiser of a progressive frame (no reference counterpart: the reference's only denoiser is
 * the `wavelet` display filter, whose edge stops are constants; the edge-avoiding a-trous wavelet of SVGF, Schied et al.
 * 2017, without its temporal part) ----
 * Works on what the noise estimate keeps: S, the accumulator the context shows, P, the mark, and the normal and position
 * AOVs N and X (SAIL_FLAG_AOV). Every operation is an f32 IEEE operation in the order written:
 *   n, h as in sail_noise_estimate (SUM: S.w, P.w; MIX: f32 of the sample index now / at the mark)
 *   lum(c) = ((c.r + c.g) + c.b) / 3
 *   c0 = n > 0 ? S.rgb / n : 0                  (MIX: c0 = S.rgb)
 *   halves = h > 0 and n > h
 *   a = P.rgb / h; b = (S.rgb - P.rgb) / (n - h)           (MIX: a, b as in the estimate)
 *   dl = lum(a) - lum(b);   v0 = halves ? (dl*dl) * ((h*(n-h)) / (n*n)) : 0      -- variance of the mean
 *   v = 3x3 prefilter of v0: taps dy,dx in -1..1 row-major (dy outer), weight g[|dy|+|dx|], g = {1/4, 1/8, 1/16},
 *       skipping taps outside the frame or not finite; v = acc / wsum, or 0 if wsum is not > 0
 *   nd = 2 * N.xyz - 1   (decoded normal AOV);   x = X.xyz (position AOV as stored)
 *   for it = 0 .. iterations-1, s = 1 << it, from (c, v) of the pass before:
 *     den = (sigma_l*sigma_l) * v_p + 1e-8;   sxs = (sigma_x * (float)s) * (sigma_x * (float)s);   lp = lum(c_p)
 *     for dy = -2..2 (outer), dx = -2..2, q = p + s*(dx, dy), skipped when outside the frame (no wrap, never loaded):
 *       kw = k[|dy|] * k[|dx|],  k = {3/8, 1/4, 1/16}
 *       centre tap: w = kw
 *       else: d = max((nd_p.x*nd_q.x + nd_p.y*nd_q.y) + nd_p.z*nd_q.z, 0); six times d = d*d          (power 64)
 *             t = x_p - x_q;  dx2 = (t.x*t.x + t.y*t.y) + t.z*t.z;  wx = 1 / (1 + dx2 / sxs)
 *             dq = lp - lum(c_q);  wl = 1 / (1 + (dq*dq) / den)
 *             w = ((kw * d) * wx) * wl
 *       the tap counts only if w > 0 and c_q.r, c_q.g, c_q.b and v_q are all finite
 *       acc += w * c_q;   vacc += (w*w) * v_q;   wsum += w
 *     if wsum > 0: c_p = acc / wsum, v_p = vacc / (wsum*wsum);   else c_p, v_p stay
 * The weights are rational instead of exp() on purpose: no math-library question, a float32 restatement gives the same
 * bits. A pixel that misses the scene carries a NaN position, takes no neighbours and stays as it is; a pixel whose mean
 * is not finite stays as it is and feeds nobody. out_rgba8 is the display transform (sail_filter's kinds 0..2, applied to
 * the denoised texel itself) quantised as the filter kernel does: (uint8)(int)(clamp(o, 0, 1) * 255 + 0.5), alpha 255.
 * State rules as sail_noise_estimate: queued samples are launched first; no mark, or no sample since it: SAIL_E_STATE;
 * SAIL_ACCUM_COMPAT8, a context without SAIL_FLAG_AOV and a half-loaded checkpoint are refused (SAIL_E_STATE); a
 * multi-device context reduces first and works on device 0's frame and AOV maps. Nothing a later call can see changes. */
typedef struct sail_denoise_params {
  int iterations;   /* a-trous passes with step 1, 2, 4, ...: 1..6            [4]   */
  float sigma_l;    /* luminance edge stop, in standard deviations of the mean [1.0] */
  float sigma_x;    /* position edge stop per pixel of step                    [0.2] */
  int display;      /* SAIL_FILTER_COLOR | GAMMA | TONEMAPPING, for out_rgba8  [COLOR] */
  float gamma_c;    /*                                                         [2.2] */
} sail_denoise_params;
typedef struct sail_denoise_info {
  uint64_t k, k_mark, nonfinite;   /* nonfinite: pixels whose mean colour is not finite */
  int iterations;
  double kernel_ms, pass_ms[8];    /* HIP events: total; [0] = prepare, [1..] = each a-trous pass */
} sail_denoise_info;
/* host only: the bracketed defaults */
int sail_denoise_defaults(sail_denoise_params* p);
/* p == NULL: the defaults. out_rgba (W H 4 f32: the denoised mean, w = 1, row 0 = bottom), out_var (W H f32: the filtered
 * variance of the mean's luminance), out_rgba8 (W H 4 bytes) and info may each be NULL. SAIL_E_INVALID: iterations outside
 * 1..6, a sigma that is not finite and > 0, a display other than kinds 0..2. */
int sail_denoise(sail_ctx* ctx, const sail_denoise_params* p, float* out_rgba, float* out_var, uint8_t* out_rgba8,
                 sail_denoise_info* info);

/* ---- camera-motion reprojection: a G-buffer pass and a temporal resolve (no reference counterpart: the reference resets
 * its accumulation on every camera move, src/core/renderer.js:57-60; the temporal part of SVGF, Schied et al. 2017, for a
 * still scene under a moving camera) ----
 * The context keeps, beside the accumulator, five W x H float4 maps and two views (P*MV with each double rounded to f32,
 * row-major, and the eye): G_cur and G_prev (world position and object row of each pixel's first hit for the current and
 * the previous view), Hist (rgb mean, w = effective sample count m: the committed output of the previous view), R (Hist
 * seen from the current view) and Out (the resolved picture of the current view). They are allocated by the first call
 * below that needs them. Every operation is an f32 IEEE operation in the order written; min(a, b) is a < b ? a : b.
 *
 * G-buffer of a view (mvp, eye), pixel (x, y), row 0 = bottom:
 *   d0..d3 = the corner directions a sample of zero jitter gets: cornerDirs(sail_jitter_inverse(mvp, 0, 0, W, H), eye), i.e.
 *            for corner c = (-1,-1), (-1,1), (1,-1), (1,1): q = inv * (cx, cy, 0, 1) summed left to right,
 *            w = q.xyz * (1/q.w) - eye, len = sqrt((w.x*w.x + w.y*w.y) + w.z*w.z), d_c = w * (1/len)
 *   s = (x + 0.5) / W;  t = (y + 0.5) / H
 *   d = s + t <= 1 ? (d0 + (d2 - d0)*s) + (d1 - d0)*t : (d3 + (d1 - d3)*(1 - s)) + (d2 - d3)*(1 - t);  o = eye
 *   (id, dist) = sail_pick of the ray (o, d): the first row with the smallest distance, (-1, 1e5) on a miss
 *   G = (o + d * dist, (float)id), each component a product and a sum;  a miss stores (0, 0, 0, -1)
 *
 * Reproject, pixel p of the current view, with Mp = the previous view's matrix, eye_prev its eye:
 *   (X, id) = G_cur[p];  id < 0 -> R[p] = 0
 *   c_i = ((Mp[i][0]*X.x + Mp[i][1]*X.y) + Mp[i][2]*X.z) + Mp[i][3]      i = 0, 1, 3
 *   !(c_3 > 0) -> R[p] = 0
 *   u = ((c_0 / c_3) * 0.5 + 0.5) * W - 0.5;   v likewise with c_1 and H;   u or v not finite -> R[p] = 0
 *   iu = floor(u), fu = u - iu;  iv, fv likewise
 *   r = X - eye_prev;  r2 = (r.x*r.x + r.y*r.y) + r.z*r.z;  lim = (pos_tol*pos_tol) * r2
 *   taps b = 0, 1 (outer), a = 0, 1:  q = (iu + a, iv + b),  w = (a ? fu : 1 - fu) * (b ? fv : 1 - fv)
 *     counted only if q is inside the frame (else never loaded), w > 0, G_prev[q].w == (float)id, Hist[q].w > 0,
 *     Hist[q].rgb all finite, and with e = X - G_prev[q].xyz:  (e.x*e.x + e.y*e.y) + e.z*e.z <= lim
 *     acc += w * Hist[q].rgb;  wsum += w;  m = min(m, Hist[q].w)      (m starts at +inf)
 *   wsum > 0 ? R[p] = (acc / wsum, m) : R[p] = 0
 *
 * Resolve, pointwise, with S the accumulator the context shows and n, c0 as in sail_denoise (SUM: n = S.w,
 * c0 = n > 0 ? S.rgb / n : 0; MIX: n = f32 of the sample index, c0 = S.rgb):
 *   m = R.w;  hist = m > 0;  cur = n > 0 and c0.rgb all finite
 *   hist and cur:  ws = m + n;  o = ((m * R.rgb) + (n * c0)) / ws;  mo = min(ws, cap)
 *   hist only:     o = R.rgb;  mo = m
 *   otherwise:     o = c0;     mo = min(n, cap)
 *   Out[p] = (o, mo)
 * so the history counts as at most `cap` samples: after a move it carries the picture, and as the still frame converges
 * its weight goes to cap / (cap + n) and the output to the plain mean. out_rgba8 is the display transform of o
 * (sail_filter's kinds 0..2) quantised as the filter kernel does, alpha 255.
 *
 * State rules: sail_set_scene and sail_update_objects drop all of it (ids and positions are stale); sail_reset,
 * sail_load_accum, sail_set_accum_mode and sail_set_partition keep it. Queued samples are launched first. SAIL_E_INVALID,
 * before anything else, for a cap that is not finite or < 1, a pos_tol that is not finite or <= 0 and a display outside
 * kinds 0..2; SAIL_E_STATE for a resolve without a begin, no scene, SAIL_ACCUM_COMPAT8 and a half-loaded checkpoint. A
 * multi-device context reduces first and works on device 0's frame and scene, like sail_filter. Nothing any other call can
 * see changes: accumulator, AOVs, noise mark, sample index, stats. */
typedef struct sail_temporal_params {
  float cap;        /* the history counts as at most this many samples: finite, >= 1  [32]    */
  float pos_tol;    /* a tap's position may differ by this share of its distance      [0.05]  */
  int display;      /* SAIL_FILTER_COLOR | GAMMA | TONEMAPPING, for out_rgba8         [COLOR] */
  float gamma_c;    /*                                                                [2.2]   */
} sail_temporal_params;
typedef struct sail_temporal_info {
  uint64_t k;               /* the context's sample index */
  uint64_t hit_pixels;      /* pixels of the current view that hit the scene */
  uint64_t history_pixels;  /* pixels of the current view that found a history (R.w > 0) */
  uint64_t nonfinite;       /* resolve: pixels whose c0 is not finite (begin: 0) */
  double kernel_ms, pass_ms[3];  /* HIP events: the call's passes; [0] G-buffer, [1] reproject, [2] resolve */
} sail_temporal_info;
enum sail_temporal_map { SAIL_TEMPORAL_G_CUR = 0, SAIL_TEMPORAL_G_PREV = 1, SAIL_TEMPORAL_HIST = 2, SAIL_TEMPORAL_R = 3,
                         SAIL_TEMPORAL_OUT = 4 };
/* host only: the bracketed defaults */
int sail_temporal_defaults(sail_temporal_params* p);
/* The G-buffer pass for a view, into a scratch map; a public id and depth pass. Each output may be NULL: rays6 (W H 6 f32:
 * origin, direction), id (W H int32), t (W H f32), xyz (W H 3 f32). Changes no temporal state. */
int sail_gbuffer(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], float* rays6, int32_t* id, float* t,
                 float* xyz);
/* "The camera is now here." Launches the queued samples and synchronises. If a view is already current it is committed:
 * Hist <- Out, G_prev <- G_cur, view_prev <- view_cur (pointer swaps). Then G_cur is computed for the new view, R from the
 * history (R = 0 when there is none) and Out <- R, so a view that is never resolved hands the history through unchanged.
 * p == NULL: the defaults; info may be NULL. A singular mvp: SAIL_E_INVALID, nothing committed. */
int sail_temporal_begin(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], const sail_temporal_params* p,
                        sail_temporal_info* info);
/* Launches the queue, synchronises, resolves the shown accumulator with R into Out and copies back what is asked: out_rgba
 * (W H 4 f32: (o, mo)), out_rgba8 (W H 4 bytes), info; each may be NULL. Calling it again on the same view, after more
 * samples, blends again from the same R. */
int sail_temporal_resolve(sail_ctx* ctx, const sail_temporal_params* p, float* out_rgba, uint8_t* out_rgba8,
                          sail_temporal_info* info);
/* copy one of the five maps (sail_temporal_map) into out (W H 4 f32). G_CUR, R and OUT need a current view, G_PREV and HIST
 * a committed one: SAIL_E_STATE otherwise */
int sail_temporal_read(sail_ctx* ctx, int which, float* out);
/* install hist (W H 4 f32) and g (W H 4 f32) with their view as the committed history; no view is current afterwards, so
 * the next sail_temporal_begin reprojects from exactly this. For tests and for a host that keeps its own history. */
int sail_temporal_load_history(sail_ctx* ctx, const float* hist, const float* g, const double mvp_prev_rowmajor[16],
                               const float eye_prev[3]);

/* ---- filtering the reprojected frame: temporal luminance moments and the a-trous passes over Out (no reference
 * counterpart; the variance estimation of SVGF, Schied et al. 2017, between its temporal accumulation and its filter) ----
 * Opt-in state of the temporal context: three more W x H float4 maps, Mhist (the committed moments of the previous view),
 * MR (Mhist seen from the current view) and Mout (the moments of the current view). A texel is (mu1, mu2, mm, 0): the first
 * and second moment of the luminance and the moments' own effective sample count. sail_temporal_moments(ctx, 1) allocates
 * them zeroed, sail_temporal_moments(ctx, 0) and sail_destroy free them. A context that never switches them on allocates
 * nothing and runs no extra pass: the calls above behave, bit for bit and pass for pass, as without this section; with
 * tracking on their colour outputs are the same bits too. Every operation is an f32 IEEE operation in the order written,
 * no contraction; min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b with the operands in the order written (so a
 * NaN first operand gives the second); lum(c) = ((c.r + c.g) + c.b) / 3.
 *
 * With tracking on, sail_temporal_begin also commits Mhist <- Mout (a pointer swap, with the others) and, after the
 * G-buffer pass, runs the moment reproject and copies Mout <- MR; sail_temporal_resolve also runs the moment resolve;
 * sail_set_scene and sail_update_objects zero the three maps (tracking stays on); the calls that keep the temporal state
 * keep them; sail_temporal_load_history zeroes Mhist.
 *
 * Moment reproject, pixel p of the current view: X, id, c_i, u, v, iu, fu, iv, fv, lim and the early-outs exactly as the
 * colour reproject (the R[p] = 0 cases give MR[p] = 0):
 *   taps b = 0, 1 (outer), a = 0, 1:  q, w as the colour reproject
 *     counted only if q is inside the frame (else never loaded), w > 0, G_prev[q].w == (float)id, with e = X - G_prev[q].xyz:
 *     (e.x*e.x + e.y*e.y) + e.z*e.z <= lim, Mhist[q].z > 0, Mhist[q].x and .y finite          (Hist is not read)
 *     a1 += w * Mhist[q].x;  a2 += w * Mhist[q].y;  wsum += w;  m = min(m, Mhist[q].z)     (m starts at +inf)
 *   MR[p] = wsum > 0 ? (a1 / wsum, a2 / wsum, m, 0) : 0
 * Moment resolve, pointwise, n and c0 as sail_temporal_resolve:
 *   l = lum(c0);  cur = n > 0 and c0.rgb all finite;  mh = MR.z;  hist = mh > 0
 *   hist and cur:  ws = mh + n;  mu1 = ((mh * MR.x) + (n * l)) / ws;  mu2 = ((mh * MR.y) + (n * (l*l))) / ws;
 *                  Mout = (mu1, mu2, min(ws, cap), 0)
 *   hist only:     Mout = MR          cur only:  Mout = (l, l*l, min(n, cap), 0)          neither:  Mout = 0
 *
 * sail_temporal_filter: a variance from the moments, then sail_denoise's a-trous passes over Out. Inputs: Out (o, mo) and
 * Mout of the current view, the AOVs N and X (SAIL_FLAG_AOV), and n of the shown accumulator (SUM: per pixel S.w; MIX: f32
 * of the sample index):
 *   c = Out.rgb;  nd = 2 * N.xyz - 1;  x = X.xyz                          (the guides exactly as sail_denoise)
 *   nn = n > 0 ? n : 1
 *   vt = (max(Mout.y - Mout.x * Mout.x, 0) * nn) / Mout.z                 -- temporal: variance of the mean
 *   spatial, 7x7: dy = -3..3 (outer), dx = -3..3, q = p + (dx, dy) inside the frame (else never loaded);
 *     sx0 = (sigma_x * 2) * (sigma_x * 2)
 *     centre tap: w = 1
 *     else: d = max((nd_p.x*nd_q.x + nd_p.y*nd_q.y) + nd_p.z*nd_q.z, 0); six times d = d*d
 *           t = x_p - x_q;  dx2 = (t.x*t.x + t.y*t.y) + t.z*t.z;  wx = 1 / (1 + dx2 / sx0);  w = d * wx
 *     the tap counts only if w > 0 and c_q.rgb are all finite:  lq = lum(c_q);  a1 += w*lq;  a2 += w*(lq*lq);  ws += w
 *   vs = ws > 0 ? max(a2/ws - (a1/ws)*(a1/ws), 0) : 0
 *   v0 = (Mout.z >= min_hist and vt is finite) ? vt : vs        -- counted in temporal_pixels / spatial_pixels
 *   v = the 3x3 prefilter of v0, then (c, v), nd, x and every a-trous pass: exactly sail_denoise's text above
 * `* nn` makes vt the variance of the mean when every frame of the history carried the same number of samples; with one
 * sample per frame, the interactive case, it is the plain (mu2 - mu1*mu1) / mm. With unequal frame sizes it is only a
 * steering estimate. nonfinite counts the pixels whose c is not finite: they stay as they are and feed nobody, as in
 * sail_denoise. The outputs are sail_denoise's.
 *
 * State rules of sail_temporal_filter: SAIL_E_INVALID, before anything else, for iterations outside 1..6, a sigma that is
 * not finite and > 0, a min_hist that is not finite or < 1 and a display outside kinds 0..2. Then queued samples are
 * launched and the stream synchronised. SAIL_E_STATE: tracking off; no current view, or one not resolved since the
 * accumulator last restarted (sail_reset, sail_load_accum, sail_set_accum_mode and sail_set_partition keep the maps, but
 * Out and Mout then belong to the accumulator before: resolve again first); sample index 0 (the AOVs would belong to
 * another view); no SAIL_FLAG_AOV; SAIL_ACCUM_COMPAT8; a half-loaded checkpoint. A
 * multi-device context reduces first and works on device 0's maps. Nothing any other call can see changes: Out, Hist, the
 * moment maps, accumulator, AOVs, mark, sample index and stats all stay; the unfiltered Out stays the history. */
typedef struct sail_tfilter_params {
  int iterations;   /* a-trous passes with step 1, 2, 4, ...: 1..6                          [4]   */
  float sigma_l;    /* luminance edge stop, in standard deviations of the mean              [4.0] */
  float sigma_x;    /* position edge stop per pixel of step                                 [0.2] */
  float min_hist;   /* moments younger than this many samples use the spatial estimate: finite, >= 1  [4] */
  int display;      /* SAIL_FILTER_COLOR | GAMMA | TONEMAPPING, for out_rgba8               [COLOR] */
  float gamma_c;    /*                                                                      [2.2] */
} sail_tfilter_params;
typedef struct sail_tfilter_info {
  uint64_t k;                 /* the context's sample index */
  uint64_t temporal_pixels;   /* pixels whose v0 is vt */
  uint64_t spatial_pixels;    /* pixels whose v0 is vs; the two add up to W * H */
  uint64_t nonfinite;         /* pixels whose c is not finite */
  int iterations;
  double kernel_ms, pass_ms[8];    /* HIP events: total; [0] = prepare, [1..] = each a-trous pass */
} sail_tfilter_info;
enum sail_temporal_moment_map { SAIL_TEMPORAL_M_HIST = 0, SAIL_TEMPORAL_M_R = 1, SAIL_TEMPORAL_M_OUT = 2 };
/* on = 1: allocate the three moment maps, zeroed (nothing happens if tracking is already on); on = 0: free them. Another
 * value: SAIL_E_INVALID. A multi-device context keeps them on device 0, with the other temporal maps. */
int sail_temporal_moments(sail_ctx* ctx, int on);
/* install mom (W H 4 f32) as Mhist. Valid only when a history is committed and no view is current, i.e. right after
 * sail_temporal_load_history; otherwise, and with tracking off, SAIL_E_STATE. */
int sail_temporal_load_moments(sail_ctx* ctx, const float* mom);
/* copy one of the three moment maps (sail_temporal_moment_map) into out (W H 4 f32). M_R and M_OUT need a current view,
 * M_HIST a committed one, as sail_temporal_read: SAIL_E_STATE otherwise and with tracking off; SAIL_E_INVALID for another
 * `which`. */
int sail_temporal_read_moments(sail_ctx* ctx, int which, float* out);
/* host only: the bracketed defaults */
int sail_temporal_filter_defaults(sail_tfilter_params* p);
/* p == NULL: the defaults. out_rgba (W H 4 f32: the filtered picture, w = 1, row 0 = bottom), out_var (W H f32: the filtered
 * variance), out_rgba8 (W H 4 bytes) and info may each be NULL. */
int sail_temporal_filter(sail_ctx* ctx, const sail_tfilter_params* p, float* out_rgba, float* out_var, uint8_t* out_rgba8,
                         sail_tfilter_info* info);

/* ---- keeping the temporal history across an object drag (no reference counterpart: the reference restarts its
 * accumulation on every drag step, src/scene/scene.js:65-68; every drag there is a pure translation of one object,
 * scene.js:143-261, which the host knows exactly) ----
 * sail_move_objects is sail_update_objects without the loss of the temporal state: it decodes and uploads the rows, runs
 * the last-bounce plan, restarts the settle count and the accumulator (the noise mark goes) exactly as sail_update_objects,
 * but leaves the current view, the committed history and the moment maps alone. If a view is current or a history is
 * committed, the context also keeps, for the next sail_temporal_begin, a pending table D of n rows of 3 floats (+0 at first)
 * and a pending cap mc (+inf at first):
 *   D[r] = D[r] + motion[r]   per component, in f32, in call order (motion == NULL: every component +0)
 *   mc = min(mc, hist_cap)    when hist_cap != 0
 * and pending becomes 1. With no temporal state at all the call is exactly sail_update_objects: nothing is pending and the
 * next begin finds no history. For sail_temporal_filter's "resolved since the accumulator last restarted" rule it is an
 * accumulator restart.
 *
 * sail_temporal_begin with pending == 1 commits as always, computes G_cur from the new rows, then reprojects with motion:
 * a pixel whose first hit is on row id shows a surface point that sat at Xp = X - D[id] in the previous frame, so
 *   (X, id) = G_cur[p];  id < 0 -> R[p] = 0
 *   d = D[(int)id];  Xp = X - d                                            (per component)
 *   c_i, u, v, iu, fu, iv, fv exactly as the reproject above with Xp in the place of X;  r = Xp - eye_prev;  lim as there
 *   taps as there, with e = Xp - G_prev[q].xyz                             (the id test still compares with (float)id)
 *   wsum > 0 ? R[p] = (acc / wsum, min(m, mc)) : R[p] = 0
 * and the moment reproject, with tracking on, uses the same Xp and stores MR.z = min(m, mc). The id and position tests
 * reject what the move uncovered: a pixel whose row did not move but which a moved row used to hide projects onto that
 * row's texels and finds no history. mc is there because a move changes the shading everywhere (shadows, reflections,
 * bounce light): clamping the count of a history that crosses a move lets the new samples take over faster; it applies to
 * every pixel. After a successful begin D is +0, mc is +inf and pending is 0; a begin that fails keeps them.
 * sail_set_scene, sail_update_objects and sail_temporal_load_history clear them; sail_reset, sail_load_accum,
 * sail_set_accum_mode and sail_set_partition keep them. With pending == 0 a begin launches the kernels above with the
 * arguments above: no table, no extra load, the same bits.
 *
 * Validation, before anything changes (a refused call leaves rows, accumulator and temporal state as they were):
 * SAIL_E_STATE without a scene; SAIL_E_INVALID for an n that is not the scene's or objects == NULL, as sail_update_objects,
 * for a motion component that is not finite and for a hist_cap that is neither 0 nor finite and >= 1. A multi-device
 * context fans the rows out as sail_update_objects does; the pending state lives with the temporal maps on device 0. */
/* sail_update_objects that keeps the temporal state. motion: n x 3 f32, the translation of each row since the rows the
 * context holds now (NULL: all +0). hist_cap: 0 = none, else finite and >= 1. */
int sail_move_objects(sail_ctx* ctx, const float* objects, int n, const float* motion, float hist_cap);
/* what is pending for the next sail_temporal_begin: motion (n x 3, may be NULL), *hist_cap (+inf when none), *pending (1
 * after a sail_move_objects that found temporal state, until the next successful begin); each may be NULL */
int sail_temporal_pending_motion(sail_ctx* ctx, float* motion, float* hist_cap, int* pending);

/* ---- albedo map of a view, and the albedo-demodulated denoiser and temporal filter (no reference counterpart; the
 * demodulation stage of SVGF, Schied et al. 2017) ----
 * Both a-trous filters stop at normals, positions and a luminance stop scaled by the variance. A procedural texture on one
 * plane has one normal and one depth, and at low sample counts the variance is large, so nothing stops them from averaging
 * across the texture. The demodulated calls divide the picture by the first hit's surface colour before filtering and
 * multiply it back afterwards. The surface colour of a hit is the texture value the trace kernels shade with (the shader's
 * getSurfaceColor): it enters every material's throughput linearly; emission and the material constants (kd, kr, kt) are
 * not part of the map.
 *
 * The map A of a view (mvp, eye) with grid g in 1..4; pixel (x, y), row 0 = bottom; every operation an f32 IEEE one, in
 * this order:
 *   d0..d3 = the corner directions of the G-buffer pass above
 *   sum = (+0, +0, +0);  cnt = 0
 *   for j = 0..g-1 (outer), i = 0..g-1:
 *     s = ((float)x + ((float)i + 0.5f) / (float)g) / (float)W
 *     t = ((float)y + ((float)j + 0.5f) / (float)g) / (float)H
 *     d = the G-buffer pass's interpolation of d0..d3 at (s, t);  o = eye
 *     the sweep of the G-buffer pass: every row in order, the first row with the smallest distance
 *     on a hit: sc = the trace kernels' hit record's surface colour for that row and distance, with the scene's own texture
 *               plugins (a texture the scene does not compile gives 0, as in a render)
 *               sum = sum + sc  (per channel);  cnt = cnt + 1
 *   A[p] = cnt > 0 ? (sum / (float)cnt, (float)cnt) : (1, 1, 1, 0)
 * The g x g grid covers exactly the pixel square the frozen schedule's jitter covers (+-1/W in NDC). For g = 1 the ray is
 * the G-buffer pass's ray bit for bit, so A.w > 0 exactly where its id is >= 0. hit_pixels counts A.w > 0, partial_pixels
 * 0 < A.w < g*g (a silhouette runs through the pixel).
 *
 * State. The albedo call follows the G-buffer call's rules: it launches queued samples, needs a scene (SAIL_E_STATE), and
 * refuses a singular mvp and, before anything else, a grid outside 1..4 (SAIL_E_INVALID); a multi-device context works on
 * device 0's scene. It keeps the map as the context's albedo map together with its view, stored as the temporal views are
 * (each double of P*MV rounded to f32, and the eye); the map is allocated on first use (device 0 of a multi-device
 * context). The load call installs a caller's map (W H 4 f32) for the view the caller passes. A new scene, updated rows and
 * moved rows invalidate the map; a reset, a loaded checkpoint, the accumulation mode, the partition and the temporal
 * calls keep it. Without a valid map the read call and both demodulated filters return SAIL_E_STATE. A context that never
 * calls these functions allocates nothing, launches nothing new and produces the same bits as before.
 *
 * Demodulation, for both filters (amin finite and > 0, else SAIL_E_INVALID before anything else):
 *   f_c(p) = (A_c(p) is finite and A_c(p) > amin) ? A_c(p) : 1          c in r, g, b
 *   lf(p) = ((f.r + f.g) + f.b) / 3
 * The demodulated denoiser: S'(p) = (S.rgb / f, S.w) and P'(p) = (P.rgb / f, P.w), an IEEE divide per channel; the
 * denoiser's text above is applied to S', P', N and X unchanged and gives (o, ov); out.rgb = o.rgb * f, out.w = 1,
 * out_var = ov * (lf*lf), out_rgba8 = the display transform of out.rgb. nonfinite counts the pixels whose demodulated c0
 * is not finite. Parameters and state rules are otherwise the denoiser's.
 * The demodulated temporal filter: the temporal filter's text with c(q) = Out(q).rgb / f(q) wherever it reads c (the
 * centre, the 49 spatial taps, the a-trous input) and vt' = vt / (lf_p*lf_p) in vt's place, its finiteness test included;
 * the outputs are remodulated as above. The history stays un-demodulated: Out, Hist and the moment maps do not change.
 * It also returns SAIL_E_STATE unless the map's stored view equals the current temporal view bit for bit.
 * With A = (1, 1, 1, .) everywhere f = 1 and lf = 1 exactly, every x/1, x*1 and x/(1*1) is exact, and both calls return
 * the plain calls' bits. */
typedef struct sail_albedo_info {
  uint64_t hit_pixels;      /* pixels where some sub-ray hit the scene */
  uint64_t partial_pixels;  /* pixels where some but not all did */
  int grid;
  double kernel_ms;         /* HIP events */
} sail_albedo_info;
#define SAIL_ALBEDO_AMIN_DEFAULT 0.01f   /* a guard, not a tuned value */
/* compute the map of a view and keep it; out_rgba (W H 4 f32) and info may each be NULL */
int sail_albedo(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], int grid, float* out_rgba,
                sail_albedo_info* info);
/* install map (W H 4 f32) as the context's albedo map of the view (mvp, eye) */
int sail_albedo_load(sail_ctx* ctx, const float* map, const double mvp_rowmajor[16], const float eye[3]);
/* copy the context's albedo map into out (W H 4 f32) */
int sail_albedo_read(sail_ctx* ctx, float* out);
/* the denoiser over the demodulated frame; arguments as the plain call's */
int sail_denoise_albedo(sail_ctx* ctx, const sail_denoise_params* p, float amin, float* out_rgba, float* out_var,
                        uint8_t* out_rgba8, sail_denoise_info* info);
/* the temporal filter over the demodulated picture; arguments as the plain call's */
int sail_temporal_filter_albedo(sail_ctx* ctx, const sail_tfilter_params* p, float amin, float* out_rgba, float* out_var,
                                uint8_t* out_rgba8, sail_tfilter_info* info);

/* ---- guide maps of a view: the denoiser's normals and positions followed through mirror and glass (no reference
 * counterpart) ----
 * Both a-trous filters read the normal and position AOVs, which show a specular surface's own normal and position, while the
 * picture on such a pixel is whatever the mirror or the glass shows: a sphere's normals turn smoothly, so nothing stops
 * the filter at the reflected room's edges, and its normal stop cuts the footprint on the reflected flat walls. The guide
 * maps hold, per pixel, the normal and the position of the first surface that scatters, reached by walking the pixel-centre
 * ray through mirror and smooth glass with the material's random pair fixed.
 *
 * The maps Ng, Xg of a view (mvp, eye) with follow depth D in 0..8; pixel (x, y), row 0 = bottom; every operation an f32
 * IEEE one, in the trace kernels' order:
 *   ray = the G-buffer pass's ray at s = (x + 0.5) / W, t = (y + 0.5) / H            (bit for bit sail_gbuffer's)
 *   depth = 0
 *   loop:
 *     ins = the trace kernels' intersection of ray with every row (the sweep of sail_pick: the first row with the smallest
 *           d) and its full hit record (normal, hit, dpdu, into, material row and category, surface colour with the
 *           scene's own texture plugins)
 *     a miss: depth == 0 -> the pixel is a miss; else the surface recorded last stays. stop.
 *     record n = ins.normal, p = ins.hit, id = ins.index
 *     followable = the category is MIRROR, or GLASS whose row gives ur < 1e-5 and vr < 1e-5 (the smooth branch), and the
 *                  scene's material plugins hold the category
 *     not followable -> stop;   depth == D -> the pixel is truncated, stop
 *     ss = normalize(ins.dpdu);  ts = cross(ins.normal, ss);  wo = worldToLocal(-ray.dir, ins.normal, ss, ts)
 *     wi = the material's sampled direction with u = (0.5, 0.5) in the place of the hash pair
 *          (mirror: (-wo.x, -wo.y, wo.z); smooth glass: Fd = frDielectric(wo.z, 1, eta); 0.5 < Fd reflects like the
 *          mirror, else refract(-wo, (0, 0, 1), into ? 1 / eta : eta / 1))
 *     wi = localToWorld(wi, ins.normal, ss, ts)
 *     ray.origin = ins.hit + ins.normal * (dot(ins.normal, wi) > 1e-5 ? 1e-4 : -1e-4);  ray.dir = wi;  depth = depth + 1
 *   Ng[p] = (n / 2 + 0.5, (float)depth)           -- the normal AOV's encoding
 *   Xg[p] = (normalize(p), (float)id)             -- the position AOV's encoding
 *   a miss: Ng = (0.5, 0.5, 0.5, 0), Xg = (NaN, NaN, NaN, -1): a non-finite position gives every tap with it weight 0
 * This is the path loop with the random pair fixed: it carries no radiance and stops at the first surface that scatters. A
 * pane of smooth glass follows one branch of its reflect/refract mix. With D = 0 the xyz of both maps equal the AOVs of a
 * one-sample render without jitter wherever that sample hits. hit_pixels counts Xg.w >= 0, followed_pixels Ng.w > 0,
 * truncated_pixels the pixels that stopped at depth D on a followable surface.
 *
 * State. sail_guides follows the albedo call's rules: a depth outside 0..8 is SAIL_E_INVALID before anything else; it
 * needs a scene (SAIL_E_STATE), refuses a singular mvp (SAIL_E_INVALID) and launches queued samples first; a multi-device
 * context works on device 0's scene. It keeps both maps as the context's guide maps together with their view, stored as
 * the temporal views are (each double of P*MV rounded to f32, and the eye); the maps are allocated on first use (device 0
 * of a multi-device context). sail_guides_load installs a caller's maps (W H 4 f32 each) for the view the caller passes. A
 * new scene, updated rows and moved rows invalidate the maps; a reset, a loaded checkpoint, the accumulation mode, the
 * partition and the temporal calls keep them. Without valid maps sail_guides_read returns SAIL_E_STATE.
 *
 * sail_use_guides(ctx, 1): sail_denoise, sail_denoise_albedo, sail_temporal_filter and sail_temporal_filter_albedo read
 * Ng and Xg wherever their text reads N and X; nothing else of their text changes. They then return SAIL_E_STATE without
 * valid maps, the two temporal filters also unless the maps' stored view equals the current temporal view bit for bit, and
 * none of them needs SAIL_FLAG_AOV: guide maps belong to a view, not to a launch, so a context that filters with them
 * spares the two AOV stores per pixel of every launch. on = 0, the default, restores today's calls exactly; another value
 * is SAIL_E_INVALID. The switch survives everything but sail_destroy. Reprojection (sail_temporal_begin) keeps using the
 * first hit, and the albedo map stays a first-hit map: the mirror's tint and the Fresnel mix are not part of a followed
 * surface colour, and dividing by it measured worse. A context that never calls these functions allocates nothing,
 * launches nothing new and produces the same bits as before. */
typedef struct sail_guides_info {
  uint64_t hit_pixels;        /* pixels whose first ray hit the scene */
  uint64_t followed_pixels;   /* pixels that left their first surface (depth > 0) */
  uint64_t truncated_pixels;  /* pixels stopped by `depth` on a surface that could be followed */
  int depth;                  /* D of the call */
  int max_depth;              /* the largest depth any pixel walked */
  double kernel_ms;           /* HIP events */
} sail_guides_info;
enum sail_guide_map { SAIL_GUIDE_N = 0, SAIL_GUIDE_X = 1 };
/* compute the maps of a view and keep them; out_n, out_x (W H 4 f32 each) and info may each be NULL */
int sail_guides(sail_ctx* ctx, const double mvp_rowmajor[16], const float eye[3], int depth, float* out_n, float* out_x,
                sail_guides_info* info);
/* install n_map and x_map (W H 4 f32 each) as the context's guide maps of the view (mvp, eye) */
int sail_guides_load(sail_ctx* ctx, const float* n_map, const float* x_map, const double mvp_rowmajor[16],
                     const float eye[3]);
/* copy one of the context's guide maps (sail_guide_map) into out (W H 4 f32); another `which`: SAIL_E_INVALID */
int sail_guides_read(sail_ctx* ctx, int which, float* out);
/* on = 1: the four filters read the guide maps in the AOVs' place; on = 0 (the default): the AOVs */
int sail_use_guides(sail_ctx* ctx, int on);

/* ---- checkpoint / resume of a progressive render (no reference counterpart: the reference restarts its
 * accumulation on every camera or object change, src/core/renderer.js:57-60, src/scene/scene.js:65-68) ----
 * A context's accumulation is `parts` raw accumulators (1 for sail_create, one per device for sail_create_multi),
 * each W*H*4 f32 in sail_read_accum's layout, plus the global sample index k of the next sample. Saving every part
 * and loading them into a fresh context with the same size, scene, partition and accumulation mode continues the
 * render bit for bit: render k -> save -> new context -> load -> render k more == the 2k-sample frame.
 * sail_save_accum launches the part's queued samples first, so the sums hold every sample below the k it returns.
 * sail_load_accum drops queued samples and the tile mask and keeps the noise mark (a new context has none);
 * sail_stats.samples becomes sail_plan_reduce's `samples` for the loaded k and the context's partition. */
int sail_accum_parts(sail_ctx* ctx, int* parts);
/* copy accumulator `part` (this rank's own, never the reduced frame) and the sample index k */
int sail_save_accum(sail_ctx* ctx, int part, float* sums, uint64_t* k);
/* replace accumulator `part` by `sums` and set the sample index to k (every part of the context). part = -1 loads a
 * whole-frame accumulator (sail_read_accum of a reduced frame): on a multi-device context each device keeps its own
 * tiles of it (tile partition) or device 0 takes all of it (sample partition: equal to the uninterrupted render to
 * summation order only; load the parts for bit-exactness). The AOVs restart with the next sample. On a multi-device
 * context a part-wise load must be followed by every other part with the same k: until then rendering, reading,
 * filtering, saving and reducing fail with SAIL_E_STATE (sail_reset abandons the half-loaded checkpoint), and a part
 * with a different k fails with SAIL_E_INVALID. The caller checks the sums' size: W*H*4 floats. */
int sail_load_accum(sail_ctx* ctx, int part, const float* sums, uint64_t k);

/* ---- run-time compiled plugin-set kernels (Scene.tracerConfig -> Generator.generate, src/scene/scene.js:70-112,
 * src/shader/generator.js:107-123: the reference builds one program per scene plugin set) ----
 * Host only, no device needed: compile (hipRTC, gfx950) the trace kernel pair for exactly this plugin set in one of the
 * kernel forms below, from the kernel sources embedded in the library, with the product's floating-point flags.
 * *bytes = the code object's size; with code != NULL and *bytes large enough on entry it is copied there. The
 * contexts do the same at sail_set_scene (SAIL_DEBUG_JIT) and load the result on their device. */
enum sail_jit_mode {
  SAIL_JIT_MODE_FLAT = 0, /* flat path, the all-plugin kernel's form (6 waves per SIMD, three-barrier sort) */
  SAIL_JIT_MODE_CULL = 1, /* pre-cull path (1,024-thread workgroups) */
  SAIL_JIT_MODE_ROOM = 2  /* flat path, the room kernel's form (7 waves, two-barrier sort, first sample group at home) */
};
/* rows > 0 (at most 8, flat forms only): compile for a scene of exactly these rows, row_types[i] = the shape id of row i
 * (SAIL_CUBE ..., each in plugins->shape_mask): the primitive sweeps become straight-line code over the rows */
int sail_jit_compile(const sail_plugins* plugins, int mode, const int32_t* row_types, int rows, void* code,
                     size_t* bytes);
/* The reference links a scene's program inside Renderer.update in milliseconds (src/core/renderer.js:45-52 ->
 * tracer.js:42-90 -> webgl.js:165-192); a hipRTC compile takes seconds, so sail_set_scene / sail_update_objects only
 * START the build of the scene's run-time kernel, on a background thread, and return; launches use the precompiled
 * kernel of the scene's plugin set until the module is loaded (bit-identical frames). Code objects are cached on disk,
 * keyed by (arch, spec, kernel-source hash, compile flags, compiler version): a read-only cache beside the library
 * (<lib dir>/jit, filled by sail_jit_prebuild at build time) and the user's cache. A code object produced by another
 * compiler than the one that built the library is refused (the precompiled kernels serve). */
enum sail_kernel_jit_state {
  SAIL_KERNEL_JIT_NONE = 0,     /* the scene gets no run-time kernel (switches, or a precompiled kernel is exact) */
  SAIL_KERNEL_JIT_PENDING = 1,  /* being built in the background */
  SAIL_KERNEL_JIT_READY = 2,    /* loaded: launches use it */
  SAIL_KERNEL_JIT_FAILED = 3    /* could not be built or loaded (jit_error): the precompiled kernel serves */
};
typedef struct sail_kernel_info {
  char name[64];          /* the kernel the last launch ran (sail_kernel_name) */
  uint64_t build_id;      /* its build identity: FNV-1a 64 of the code object with the compiler's source-derived
                           * compilation-unit id masked (run-time kernels), or of the library image and the kernel's name
                           * (precompiled): profiles are matched to kernels by it */
  /* the jit_* fields describe the best tier that is loaded -- the value kernel once it is (SAIL_DEBUG_JIT_VALUES_AFTER),
   * else the scene's run-time kernel -- that is, what the next launch runs; name and build_id are the last launch's */
  int jit_state;          /* sail_kernel_jit_state of the scene's run-time kernel */
  int jit_from_cache;     /* its code object came from 0: hipRTC in this process, 1: the user's disk cache, 2: the
                           * cache shipped beside the library */
  double jit_compile_ms;  /* hipRTC time of that code object (0 from a cache) */
  uint64_t jit_build_id;  /* the run-time kernel's build identity once READY */
  char jit_error[256];    /* why it FAILED */
} sail_kernel_info;
int sail_get_kernel_info(sail_ctx* ctx, sail_kernel_info* out);
/* *ready = 1 when the scene's run-time kernel is loaded (the next launch uses it), after waiting up to timeout_ms for
 * its build (-1: until done); 0 while it is still building, when none applies, or when it failed */
int sail_kernel_ready(sail_ctx* ctx, int timeout_ms, int* ready);
/* process-wide user cache directory of run-time code objects: NULL = default ($XDG_CACHE_HOME or $HOME/.cache, then
 * sail_amd/jit), "" = no user cache. The directory holds the run-time kernels' objects; the value kernels' objects
 * (SAIL_DEBUG_JIT_VALUES_AFTER) are written to a directory beside it, the same path with "-values" appended (dir
 * "/x/jit": "/x/jit-values"), which is created on demand and holds at most 32 objects, the oldest deleted first. The
 * same rule names the value directory of sail_jit_prebuild's `dir` and of the cache shipped beside the library. */
int sail_set_jit_cache(const char* dir);
/* Host only (no device): build the run-time kernel a context with the default switches derives for this scene (the rows
 * of sail_set_scene) for `arch`, into the cache directory `dir` (the shipped cache when dir is <lib dir>/jit). *built
 * (may be NULL) = 1 when the scene gets a run-time kernel, 0 when it does not. */
int sail_jit_prebuild(const float* objects, int n, const float* texparams, int tn, const float* lights, int ln,
                      const sail_plugins* plugins, const char* arch, const char* dir, int* built);
/* The value kernel (SAIL_DEBUG_JIT_VALUES_AFTER): sail_jit_prebuild builds it too for every scene whose run-time kernel is
 * the flat form compiled for rows with at most 32 texParams rows. Host only, nothing is compiled: *key = the disk caches'
 * key of the value kernel a context with the default switches derives for this scene once it has settled (its object is
 * <dir>-values/<key as 16 hex digits>.co, beside the cache directory <dir> of the types kernels; 0 when the scene gets none), and the source prefix it is compiled with -- the rows and
 * the texParams table as 32-bit words, so that two scenes differing in one bit (+0 / -0, a NaN payload) are two kernels.
 * *defs_len (may be NULL) = the prefix's size with its terminator; copied into defs when *defs_len on entry is enough. */
int sail_jit_value_key(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                       const char* arch, uint64_t* key, char* defs, size_t* defs_len);
/* The same for a context with SAIL_DEBUG_JIT = jit (< 0: the default switches): the key and source prefix of its value
 * kernel (value != 0) or of the run-time kernel under it (value == 0; the types kernel). */
int sail_jit_spec_key(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                      const char* arch, int jit, int value, uint64_t* key, char* defs, size_t* defs_len);
/* 1 when a context that rendered `settled` samples since its rows last changed asks for its value kernel under
 * SAIL_DEBUG_JIT_VALUES_AFTER = after (0: at once, < 0: never), else 0 */
int sail_plan_settle(uint64_t settled, int after);
/* Host only (no device): the shape of one trace launch, as a context with these facts derives it -- which precompiled
 * kernel set the scene falls in, which run-time kernel runs, how the launch's samples are split into staged sample groups,
 * and the grid. Frames are bit-identical whatever the split, so this is where that policy is stated and tested
 * (tests/test_launch_plan.py). The entry derives the run-time kernel's spec itself from the scene, the switches and the
 * share; `tier` only says which tier a context has loaded. Returns -1 with a message (sail_last_error(NULL)) for bad
 * facts, among them a tier the scene does not get under these switches. */
enum sail_launch_tier {
  SAIL_LAUNCH_TIER_NONE = 0,  /* no run-time kernel is loaded: the precompiled kernel of the scene's set runs */
  SAIL_LAUNCH_TIER_TYPES = 1, /* the scene's run-time kernel */
  SAIL_LAUNCH_TIER_VALUE = 2  /* the value kernel on top of it (SAIL_DEBUG_JIT_VALUES_AFTER) */
};
typedef struct sail_launch_facts {
  /* the scene, as sail_set_scene takes it (ln light rows; the rows themselves are not read) */
  const float* objects;
  const float* texparams;
  const sail_plugins* plugins;
  int n, tn, ln;
  /* the switches: bit o of debug_set says sail_set_debug(ctx, o, debug[o]) was called, every other option is at its
   * default. Only the options that decide a kernel or a launch shape are taken (not SAIL_DEBUG_CULL_FMA, FORCE_RCCL,
   * JIT_WAIT). launch_spp: sail_set_launch_samples (0: by form). */
  uint32_t debug_set;
  int debug[16];
  int launch_spp;
  /* the share of the frame and the device (sail_set_partition; compute_units as sail_device_info reports them) */
  int width, height, rank, world, part_mode, compute_units;
  /* the launch: its samples; the tiles a tile mask leaves active of this rank's share, or -1 without a mask; whether the
   * fused pre-cull form is safe and whether primary rays may use the pre-cull for this eye (both decided from the eye
   * and the scene's extent by the context); the tier that is loaded */
  int nspp, active_tiles, cull_fma_ok, eye_near_scene, tier;
} sail_launch_facts;
typedef struct sail_launch_plan {
  int kernel_set;     /* 0 every plugin, 1 the Cornell box's set, 2 the rooms' */
  int cull_prims;     /* 0 flat path, 1 the plain pre-cull form, 2 the fused one */
  int cull_primary;   /* primary rays use the pre-cull */
  int wavefront;      /* the launch goes by the wavefront split (SAIL_DEBUG_WAVEFRONT on a pre-cull scene) */
  int jit_mode;       /* sail_jit_mode of the run-time kernel that runs, -1: a precompiled kernel or the wavefront split */
  int ns;             /* samples of each pixel in flight per workgroup */
  int sample_groups;  /* workgroups per block that share the launch's samples */
  int group_spp;      /* samples per group (the last group takes the rest) */
  int group_home;     /* 1: group 0 adds its samples to the accumulator itself */
  int staged;         /* 1: the groups' samples go through the stage, and sail_accum_kernel follows */
  /* a run-time kernel: grid workgroups of `threads`; a precompiled kernel: grid counts 256-thread blocks, launched as
   * grid * 256 / threads workgroups of `threads`; the wavefront split: every one of its passes */
  uint32_t grid, threads;
  int kernel_lights;  /* the kernel has a light plugin compiled in (sail_plan_last_bounce's kernel_lights) */
  int launch_samples; /* the samples a context with these switches puts into one launch while it holds the scene's
                       * run-time kernel (built or still building): nspp never exceeds it */
} sail_launch_plan;
int sail_plan_launch(const sail_launch_facts* facts, sail_launch_plan* plan);
/* What the process keeps of value kernels: *code_objects in host memory, *modules loaded on devices. A value kernel is
 * one per pose of a scene at rest, so both are released when the last context that holds one drops it (a change of its
 * rows, another scene, sail_destroy): they are bounded by the live contexts, not by the poses seen. The objects stay in
 * the disk caches. */
int sail_jit_resident(int* code_objects, int* modules);

/* ---- host math of the reference, so every host language gets identical uniforms ---- */
/* Camera(eye, center, up) + makePerspective(fovy, aspect, near, far) (src/scene/camera.js:6-57):
 * P*MV (scene.mat, src/scene/scene.js:40-42) as 16 doubles, row-major */
int sail_camera(const double eye[3], const double center[3], const double up[3], double fovy, double aspect,
                double znear, double zfar, double mvp_rowmajor[16]);
/* inverse(Translation(jx/W, jy/H, 0) * mvp) flattened column-major in f32 (tracer.js:94-96, matrix.js:501-527) */
int sail_jitter_inverse(const double mvp_rowmajor[16], double jx, double jy, int width, int height, float inv_colmajor[16]);
/* The frozen deterministic schedule: sample k uses time_seed = 0.001*round(1000*(k+1)/60)
 * and jitter from xorshift32(0x5A11 + k). Fills spp x 16 matrices and spp seeds for k = k0 .. k0+spp-1. */
int sail_schedule(const double mvp_rowmajor[16], int width, int height, int k0, int spp, float* inv_colmajor, float* seeds);

/* Object3D.boundbox() (src/scene/geometry.js; the picker's pre-test, pickup.js:55-56), answered by the bounds the
 * trace kernels' pre-cull tests: for each of the n object rows (18 floats, Appendix A wire format; tn = the
 * texParams row count the rows index), 6 floats min.xyz, max.xyz of the padded box, +-inf where a primitive has no
 * finite bound; a row whose category is not a shape gets an empty box (+inf, -inf). Host-only (no device). */
int sail_prim_bounds(const float* objects, int n, int tn, float* out_minmax);
/* Host only (no device): what the last bounce of the flat kernels' Cornell and all-plugin forms does with a hit on each
 * row of a scene of at most 32 rows (sail_set_scene's arguments; the room form runs its last bounce like the others). A path's last bounce only adds radiance. Bit r of *quiet_rows: a hit on row r adds
 * exactly (+0, +0, +0) x throughput whatever its hit record holds -- the row's emission words are +0.0f bit for bit
 * and it is not a matte, or it is a Lambertian matte (sigma < EPSILON) of a constant colour (a Cornellbox's walls, a
 * uniform texture) with kd x colour / pi finite, in a kernel without a light plugin -- so no record is built for it.
 * *skip_sort = 1 when, besides, every other row that a ray can hit emits and its last bounce needs no BSDF sample:
 * the last bounce's path sort is skipped as well. kernel_lights: nonzero when the kernel that runs has a light plugin
 * compiled in (every kernel but the Cornell set's and a run-time kernel of a scene whose light mask is 0). Larger
 * scenes get 0 and 0. */
int sail_plan_last_bounce(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                          int kernel_lights, uint32_t* quiet_rows, int* skip_sort);

/* ---- multi-GPU (one process per GPU): image tiles / sample split + RCCL sum-reduce of the accumulators ---- */
int sail_comm_unique_id(char id[128]);
/* a second call replaces the communicator */
int sail_comm_init(sail_ctx* ctx, const char id[128], int nranks, int rank);
/* Sum of every rank's float4 accumulator (and, with SAIL_FLAG_AOV on a tile partition, of the AOV maps) into a
 * separate frame on `root`; collective: every rank calls it, all created with the same flags. The ranks'
 * accumulators are left as they are, so render -> reduce -> render -> reduce is progressive: each reduce sums
 * the cumulative accumulators afresh. On root, readback / read_accum / filter show that frame until the next
 * sail_render* or sail_reset (then this rank's own accumulator again). With a sample partition the AOVs shown are
 * those of the rank that rendered the frame's last sample, as on one GPU. Asynchronous RCCL errors are reported
 * here and by sail_sync (ncclCommGetAsyncError). On a multi-device context it reduces into device 0 (root 0). */
int sail_reduce(sail_ctx* ctx, int root);
/* this rank's own accumulator (device 0's on a multi-device context), never the reduced frame: since ABI v2 the
 * reduce is out of place, so after sail_reduce the pointer still holds rank-local sums */
int sail_accum_device_ptr(sail_ctx* ctx, void** ptr, size_t* bytes);
/* the 64x64 tiles rank `rank` of `world` owns in a W x H frame (tile t -> rank t % world), as
 * (x0, y0, w, h) quadruples; returns the tile count (or a negative error); out may be NULL to count */
int sail_partition_tiles(int width, int height, int rank, int world, int* out_xywh, int capacity);
/* Host only (no device): the bookkeeping both reduces follow -- sail_reduce (one process per GPU) and a multi-device
 * context's grouped reduce -- for rank `rank` of `world` under partition `mode` once k samples (global indices
 * 0 .. k-1) are rendered, the frame reduced into `root`. Both derive their choices from this function, so a host
 * language, or a test over gloo (tests/test_partition_gloo.py), plans the same exchange without a device. */
typedef struct sail_reduce_plan {
  int receives;       /* 1: this rank is `root`, where the reduced frame lands */
  int tiles;          /* 64x64 tiles this rank renders: tiles t = rank (mod world), or every tile (sample partition) */
  int aov_owner;      /* the rank whose AOV maps the frame shows: the one that rendered sample k-1 (sample partition; 0
                       * before any sample), or -1 for a tile partition (every rank owns its own tiles' maps) */
  int send_own_aovs;  /* 1: this rank reduces its own AOV maps; 0: it sends -0 maps, the additive identity that keeps
                       * every bit of the owner's maps (x + -0 == x for +-0 and NaN too) */
  uint64_t samples;   /* how many of the samples 0 .. k-1 this rank rendered: k for a tile partition, those with index
                       * = rank (mod world) for a sample partition */
} sail_reduce_plan;
int sail_plan_reduce(int width, int height, int rank, int world, int mode, uint64_t k, int root, sail_reduce_plan* out);
/* Host only: what rank `rank` keeps of a whole-frame accumulator when it resumes from it (sail_load_accum part -1):
 * its own tiles and zeros elsewhere, or for a sample partition all of it on rank 0 and zeros on the others. sums and
 * out hold W*H*4 floats (they may be the same buffer). */
int sail_plan_keep(int width, int height, int rank, int world, int mode, const float* sums, float* out);
/* Host only: one step of a part-wise checkpoint load over `parts` parts (sail_load_accum on a multi-device context).
 * *missing = bit mask of the parts still to load (0: no load in progress), *k = the checkpoint's sample index. Loading
 * part `part` saved at index k_part: the first part of a checkpoint sets *missing to every part and *k = k_part, then
 * clears its own bit; a later part with another index fails with SAIL_E_INVALID and leaves the state unchanged; part -1
 * (a whole frame) clears *missing. A frame is usable again once *missing is 0. */
int sail_plan_load_part(uint64_t* missing, uint64_t* k, int parts, int part, uint64_t k_part);

/* ---- diagnostics ---- */
/* evaluate the build's f32 math spec on the device (fn: 0 sin 1 cos 2 tan 3 atan2(y,x) 4 acos 5 pow(x,y)
 * 6 atan 7 sqrt 8 x/y); for the CPU/GPU bit-parity test */
int sail_math_probe(int fn, const float* x, const float* y, float* out, int count);
int sail_abi_version(void);
/* the trace kernel the context's current scene launches (a plugin-set specialisation, like the reference's
 * per-scene generated program): writes its name (e.g. "sail_trace_kernel_cornell") into name[len]; after a launch
 * that split its samples into groups, the "_grouped" form it ran (followed by sail_accum_kernel) */
int sail_kernel_name(sail_ctx* ctx, char* name, int len);
/* device time of the last sail_filter pass (HIP events around the kernel), for the stencil's roofline */
int sail_filter_ms(sail_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* SAIL_HIP_H */
