// sail_capi.cpp — libsail_hip.so: context, scene decode, launches, readback, filter, RCCL reduce.
// The C ABI is declared (with the reference interface each entry replaces) in include/sail_hip.h.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/sail_hip.h"
#include "sail_device.h"

// launch wrappers defined next to the kernels (sail_trace.hip)
hipError_t sail_launch_trace(const SailTraceArgs& A, int blocks, hipStream_t s);
// sail_jit.cpp: the trace kernel pair compiled at run time for exactly one plugin set (on the current device)
#include "sail_jit.h"
hipError_t sail_launch_filter(const SailFilterArgs& A, hipStream_t s);
hipError_t sail_launch_accum(const SailTraceArgs& A, int blocks, hipStream_t s);
hipError_t sail_launch_math(int fn, const float* x, const float* y, float* out, int count);
hipError_t sail_launch_sum(const SailSumArgs& A, hipStream_t s);
hipError_t sail_launch_negzero_unowned(float4* a, float4* b, int W, int H, int rank, int world, hipStream_t s);
hipError_t sail_launch_wavefront(const SailTraceArgs& A, const SailWfState& S, hipStream_t s);
hipError_t sail_launch_pick(const SailPrim* prims, int n, const float* rays, int count, int32_t* index, float* t,
                            hipStream_t s);
// sail_noise.hip: the noise estimate's per-tile pass
#include "sail_noise.h"
hipError_t sail_launch_noise(const SailNoiseArgs& A, hipStream_t s);
hipError_t sail_launch_noise_copy(const SailNoiseArgs& A, hipStream_t s);
// sail_denoise.hip: the denoiser's prepare pass and one a-trous pass
#include "sail_denoise.h"
hipError_t sail_launch_denoise_prepare(const SailDenoisePrepareArgs& A, hipStream_t s);
hipError_t sail_launch_denoise_atrous(const SailDenoiseAtrousArgs& A, hipStream_t s);
// sail_temporal.hip: the G-buffer, reproject and temporal resolve passes
#include "sail_temporal.h"
hipError_t sail_launch_gbuffer(const SailGbufferArgs& A, hipStream_t s);
hipError_t sail_launch_reproject(const SailReprojectArgs& A, bool moved, hipStream_t s);
hipError_t sail_launch_temporal_resolve(const SailResolveArgs& A, hipStream_t s);
// sail_tfilter.hip: the moment reproject and resolve passes and the temporal filter's prepare pass
#include "sail_tfilter.h"
hipError_t sail_launch_moment_reproject(const SailReprojectArgs& A, bool moved, hipStream_t s);
hipError_t sail_launch_moment_resolve(const SailMomentResolveArgs& A, hipStream_t s);
hipError_t sail_launch_tfilter_prepare(const SailTfilterPrepareArgs& A, hipStream_t s);
// sail_albedo.hip: the albedo map of a view; the albedo-demodulated instances live beside the plain kernels
#include "sail_albedo.h"
hipError_t sail_launch_albedo(const SailAlbedoArgs& A, hipStream_t s);
hipError_t sail_launch_denoise_prepare_demod(const SailDenoisePrepareDemodArgs& A, hipStream_t s);
hipError_t sail_launch_denoise_atrous_remod(const SailDenoiseAtrousRemodArgs& A, hipStream_t s);
hipError_t sail_launch_tfilter_prepare_demod(const SailTfilterPrepareDemodArgs& A, hipStream_t s);

namespace {

thread_local std::string g_create_error;

// ---- RCCL, bound at run time (the process may already hold torch's copy under the same soname) ----
typedef struct { char internal[128]; } nccl_uid_t;
typedef void* nccl_comm_t;
struct Rccl {
  bool tried = false, ok = false;
  int (*getUniqueId)(nccl_uid_t*) = nullptr;
  int (*commInitRank)(nccl_comm_t*, int, nccl_uid_t, int) = nullptr;
  int (*reduce)(const void*, void*, size_t, int, int, int, nccl_comm_t, hipStream_t) = nullptr;
  int (*commDestroy)(nccl_comm_t) = nullptr;
  int (*commInitAll)(nccl_comm_t*, int, const int*) = nullptr;   // single-process multi-device communicator
  int (*groupStart)() = nullptr;
  int (*groupEnd)() = nullptr;
  int (*commGetAsyncError)(nccl_comm_t, int*) = nullptr;
  const char* (*errStr)(int) = nullptr;
  bool load() {
    if (tried) return ok;
    tried = true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return false;
    getUniqueId = (int (*)(nccl_uid_t*))dlsym(h, "ncclGetUniqueId");
    commInitRank = (int (*)(nccl_comm_t*, int, nccl_uid_t, int))dlsym(h, "ncclCommInitRank");
    reduce = (int (*)(const void*, void*, size_t, int, int, int, nccl_comm_t, hipStream_t))dlsym(h, "ncclReduce");
    commDestroy = (int (*)(nccl_comm_t))dlsym(h, "ncclCommDestroy");
    errStr = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    commInitAll = (int (*)(nccl_comm_t*, int, const int*))dlsym(h, "ncclCommInitAll");
    groupStart = (int (*)())dlsym(h, "ncclGroupStart");
    groupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
    commGetAsyncError = (int (*)(nccl_comm_t, int*))dlsym(h, "ncclCommGetAsyncError");
    ok = getUniqueId && commInitRank && reduce && commDestroy && commInitAll && groupStart && groupEnd &&
         commGetAsyncError;
    return ok;
  }
};
Rccl g_rccl;
constexpr int kNcclFloat32 = 7, kNcclSum = 0;

// GLSL division on the host, for the shader expressions evaluated here once per scene or per sample: the math
// spec's a * RN(1/b) (sail_math.h fdiv, oracle/ref_math.h div_s); host f32 arithmetic is IEEE (no contraction)
float gdiv(float a, float b) { return a * (1.0f / b); }

// ---- the reference's texture addressing (texhelper.glsl, NEAREST + CLAMP_TO_EDGE) ----------------------
int texel(float c, int size) {
  if (c != c) return 0;  // NaN row coordinate (n = 1 / ln = 1: 0/0) addresses texel 0
  const float s = floorf(c * (float)size);
  if (!(s >= 0.0f)) return 0;
  if (s >= (float)(size - 1)) return size - 1;
  return (int)s;
}
int to_int(float x) {
  if (x != x) return 0;
  if (x >= 2147483647.0f) return 2147483647;
  if (x <= -2147483648.0f) return (-2147483647 - 1);
  return (int)x;
}
struct TexView {
  const float* d; int w, h;
  float at(float cx, float cy) const {
    if (h <= 0) return 0.0f;
    return d[texel(cy, h) * w + texel(cx, w)];
  }
  float readFloat(float x, float y, float width) const { return at(gdiv(x, width), y); }
  void readVec3(float x, float y, float width, float* out) const {
    float px = gdiv(x, width);
    out[0] = at(px, y); px += gdiv(1.0f, width);
    out[1] = at(px, y); px += gdiv(1.0f, width);
    out[2] = at(px, y);
  }
};

}  // namespace

// union of the primitives' finite bounds and its diagonal (sceneBox)
struct SceneBox { double lo[3], hi[3]; double diag; };

// One run-time kernel of a context: the spec it holds (sail_jit_hold), whether its code object is still being built, is
// loaded or failed, the loaded pair, and why a build failed. The hold is what keeps the build worker from skipping the
// spec's queued build and, for a value spec, what keeps its module loaded: it is taken, polled and released here only.
struct JitSlot {
  bool have = false;
  SailJitSpec spec;
  int state = SAIL_KERNEL_JIT_NONE;
  SailJitKernel k;
  std::string error;

  // The loaded pair, waiting up to wait_ms for its build (-1: until it is done); false while nothing is held, while the
  // build is still running, and once it has failed (the caller's next tier then runs, with the same results)
  bool poll(int device, int wait_ms, SailJitKernel* out = nullptr) {
    if (!have || state == SAIL_KERNEL_JIT_FAILED) return false;
    if (state != SAIL_KERNEL_JIT_READY) {
      std::string err;
      const int r = sail_jit_kernels(device, spec, wait_ms, &k, &err);
      if (r == 1) return false;
      if (r < 0) { state = SAIL_KERNEL_JIT_FAILED; error = err; return false; }
      state = SAIL_KERNEL_JIT_READY;
    }
    if (out) *out = k;
    return true;
  }
  // Release the hold and clear the slot. The last hold on a value spec unloads the module (sail_jit_hold): no launch of
  // a loaded kernel may still be running on the context's stream.
  void drop(int device, hipStream_t stream) {
    if (have) {
      if (state == SAIL_KERNEL_JIT_READY && stream) {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
      }
      sail_jit_hold(device, spec, -1);
    }
    *this = JitSlot{};
  }
  // Hold `s` (not a reference into this slot) and ask for it once without waiting: the build starts in the background,
  // or the object loads here when a disk cache has it. A spec held before goes as in drop, but only after the new one is
  // held: a build both share is never skipped in between.
  void adopt(int device, hipStream_t stream, const SailJitSpec& s) {
    sail_jit_hold(device, s, +1);
    drop(device, stream);
    have = true;
    spec = s;
    state = SAIL_KERNEL_JIT_PENDING;
    (void)poll(device, 0);
  }
};

struct sail_ctx {
  int device = 0, W = 0, H = 0;
  uint32_t flags = 0;
  hipStream_t stream = nullptr;
  float4* accum = nullptr;
  float4* aovN = nullptr;
  float4* aovP = nullptr;
  float4* filterOut = nullptr;    // display-filter outputs, allocated on first use
  uint8_t* filterOut8 = nullptr;
  unsigned long long* segCounter = nullptr;
  SailPrim* prims = nullptr;
  float* tp = nullptr;
  float* lt = nullptr;
  int32_t* lightObjRow = nullptr;
  SailSample* samples = nullptr;
  int samplesCap = 0;
  int samplesPos = 0;  // ring position: each launch sequence reads its own slice of the sample buffer
  SailSample* samplesPinned = nullptr;  // pinned host mirror of the ring (asynchronous uploads)
  std::vector<SailSample> hostSamples;
  std::vector<float> objectsRows;
  std::vector<float> tpRows;  // host copy of texParams (category words of updated objects)
  int n = 0, tn = 0, ln = 0;
  sail_plugins plugins{};
  bool haveScene = false;
  int shadowAnyHit = 0;
  // the rows' last-bounce classes (lastBounceRows) for a kernel without ([0]) and with ([1]) a light plugin compiled in,
  // re-derived whenever the rows are decoded (sail_set_scene, sail_update_objects: texParams and plugin masks change
  // only with the former); launchTrace passes the pair of the kernel it launches
  uint32_t lastQuietRows[2] = {0u, 0u};
  int lastSkipSort[2] = {0, 0};
  std::vector<unsigned long long> typeMasksHost;  // staging for the per-chunk type masks (async copy source)
  int cullMinPrims = 8;  // scenes with at least this many primitives use the padded-box pre-cull
  int lastGroups = 1;         // the last trace launch: sample groups (sail_kernel_name)
  bool lastWavefront = false;
  int flatGroupRounds = 36;  // sample groups: residency rounds queued per launch (flat kernels, SAIL_DEBUG_GROUP_ROUNDS)
  int cullGroupRounds = 64;  // the same for the pre-cull kernel's 1,024-thread workgroups
  int cullFma = 1;       // SAIL_CULL_FMA=0: always the plain pre-cull form (tests)
  double primExtent = INFINITY;  // largest |padded bound| coordinate (inf: some primitive is unbounded)
  SceneBox scene{};              // union of the primitives' finite bounds (padPrimBounds)
  int forceGeneric = 0;  // SAIL_FORCE_GENERIC=1: always launch the all-plugin kernel (tests)
  int forceGroups = 0;   // SAIL_SAMPLE_GROUPS=g: fixed sample-group count (tests); 0 = by occupancy
  int wavefront = 0;     // SAIL_DEBUG_WAVEFRONT: the pre-cull path by the wavefront split (study)
  int jit = 59;  // SAIL_DEBUG_JIT bits: which scenes get a run-time kernel (jitSpecFor; instrumented in the phase build)
  // The scene's run-time kernel (refreshJit), compiled for its plugin set and its rows' types. Until it is loaded the
  // precompiled kernel of the scene's set serves (same results); a launch waits up to jitWait ms for it
  // (SAIL_DEBUG_JIT_WAIT; -1 until it is built). Its error is the one sail_get_kernel_info reports.
  JitSlot typesSlot;
  int jitWait = 0;
  int jitNt = 0;  // SAIL_DEBUG_JIT_NT: threads per workgroup of the run-time kernels (0: the form's own)
  int jitNs = 0;  // SAIL_DEBUG_JIT_NS: samples in flight of the run-time kernels (0: the form's default, jitNsFor)
  // The value kernel, a second tier on top of the scene's run-time kernel (refreshValues): the same spec with the rows'
  // and the texParams table's words compiled in, asked for once `settled` samples were rendered since the rows last
  // changed (sail_set_scene, sail_update_objects, a new types spec; not sail_reset or the camera). A launch uses it when
  // it is loaded and never waits for it. jitValuesAfter (SAIL_DEBUG_JIT_VALUES_AFTER): 0 at once, < 0 never; 256 is a
  // policy value, not tuned -- it only has to keep scenes in motion and few-sample renders from compiling.
  int jitValuesAfter = 256;
  uint64_t settled = 0;
  std::vector<uint32_t> rowWords;  // the decoded rows as uploaded (uploadPrims), 32 words each
  JitSlot valueSlot;
  bool lastMasked = false;  // the last trace launch ran a _masked instance (a tile mask was set)
  // The MASKED instances of the scene's run-time kernels (SailJitSpec.masked), asked for at the first launch under a tile
  // mask (maskedTwin): one follows the types spec, one the value spec, and each goes before the slot it follows. Built in
  // the background like their unmasked twins; until one is loaded a masked launch runs the precompiled _masked kernel of
  // the scene's set, with the same results.
  JitSlot typesTwin, valueTwin;
  bool lastJit = false;  // the last trace launch ran a run-time compiled kernel (sail_kernel_name)
  int lastJitMode = 0;
  uint64_t lastBuildId = 0;  // the run-time kernel's build identity (sail_get_kernel_info)
  std::vector<int> primTypes;  // decoded shape id of each row (run-time kernels compiled for the scene's rows)
  float4* wf = nullptr;  // its path state: 11 float4 arrays of wfSlots
  size_t wfSlots = 0;
  int numCUs = 256;
  float* stage = nullptr;    // sample-group staging, allocated on first use
  size_t stageBytes = 0;
  int accumMode = SAIL_ACCUM_SUM;
  int rank = 0, world = 1, partMode = SAIL_PART_TILES;
  // samples per launch (sail_set_launch_samples); 0 = by form (launchSamples): 64 measured C2 +0.7 %, C3 +0.5 %, C4/C5
  // +-0.2 % over 32 (profiles/r04_launch_spp*)
  int launchSpp = 0;
  uint64_t k = 0;  // global sample index of the next sample (the reference's sampleCount)
  uint64_t samplesThisRank = 0;
  uint64_t nominalSegments = 0;
  std::vector<hipEvent_t> evPool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double kernelMs = 0.0, lastLaunchMs = 0.0;
  double lastFilterMs = 0.0;  // device time of the last display-filter pass
  uint32_t launches = 0;
  // Noise estimate (sail_noise_mark / sail_noise_estimate): the mark, a snapshot of the shown accumulator at sample index
  // noiseK, allocated on first mark; resetAccum drops it (sail_load_accum keeps it). On a multi-device context device
  // 0's sub-context holds it (the reduced frame lives there). noiseOut: per tile a float sum then a uint32 count.
  float4* noiseMark = nullptr;
  bool noiseHave = false;
  uint64_t noiseK = 0;
  float* noiseOut = nullptr;
  float* noisePix = nullptr;  // the optional per-pixel map, allocated on first use
  // Tile mask (sail_set_active_tiles), on every context that traces or holds the mark (each sub-context of a multi-device
  // one keeps the whole mask: device 0's masks the mark, every device intersects it with its share). maskSet: a launch
  // walks tileMap, the ascending table of this rank's active tiles (maskTiles of them, maskPixels in-frame pixels);
  // maskBytes is the whole mask, a byte per 64x64 tile, for the noise kernels. Both device arrays hold one entry per tile
  // of the frame, allocated on first use and rewritten only with the stream idle. frozenAt[t]: the sample index at
  // which the inactive tile t was switched off. resetAccum removes the mask.
  bool maskSet = false;
  std::vector<uint8_t> mask;
  std::vector<uint32_t> frozenAt;
  int32_t* tileMap = nullptr;
  uint8_t* maskBytes = nullptr;
  int maskTiles = 0;
  long long maskPixels = 0;
  // Denoiser (sail_denoise): one block of work buffers, allocated on first use: two (c, v) float4 maps, the guides as a
  // float4 and a float2 map, the variance map, the RGBA8 map and the per-tile non-finite counts
  void* denoiseWork = nullptr;
  // Camera-motion reprojection (sail_temporal_*): one block, allocated on first use, holding the five float4 maps, the
  // RGBA8 map and three counts per 16x16 tile; the map pointers are swapped when a view is committed. tpHaveCur: a view
  // is current (G_cur, R and Out are its); tpHavePrev: a history is committed (G_prev, Hist and tpPrev are its).
  // sail_set_scene and sail_update_objects drop both (sail_move_objects keeps them). On a multi-device context device
  // 0's sub-context holds it.
  void* tpWork = nullptr;
  float4 *tpGcur = nullptr, *tpGprev = nullptr, *tpHist = nullptr, *tpR = nullptr, *tpOut = nullptr;
  bool tpHaveCur = false, tpHavePrev = false;
  struct TpView { float m[16]; float eye[3]; } tpCur{}, tpPrev{};
  uint64_t tpHitPixels = 0;
  // Moment tracking (sail_temporal_moments): one block of three float4 maps (mu1, mu2, mm, 0) and a count per tile,
  // allocated when tracking is switched on and freed when it is switched off; the pointers are swapped with the colour
  // maps'. tpResolved: the current view has been resolved (sail_temporal_filter needs its Out and Mout).
  void* tpMom = nullptr;
  float4 *tpMhist = nullptr, *tpMR = nullptr, *tpMout = nullptr;
  bool tpResolved = false;
  // Object motion pending for the next sail_temporal_begin (sail_move_objects): tpMotion is the table D, n rows of
  // (d.xyz, 0), the sum of the moves since the last begin; tpMotionCap is mc (+inf: none). tpMotionDev is D's device copy,
  // allocated on first use and uploaded by the begin that consumes it. sail_set_scene, sail_update_objects and
  // sail_temporal_load_history clear the pending state; on a multi-device context device 0's sub-context holds it.
  bool tpMotionPending = false;
  std::vector<float> tpMotion;
  float tpMotionCap = INFINITY;
  float4* tpMotionDev = nullptr;
  int tpMotionDevRows = 0;
  // Albedo map (sail_albedo / sail_albedo_load): one float4 map and two counts per 16x16 tile, allocated on first use,
  // with the view it belongs to, kept as the temporal views are. sail_set_scene, sail_update_objects and sail_move_objects
  // invalidate it (the rows it shows are gone); on a multi-device context device 0's sub-context holds it.
  float4* albMap = nullptr;
  bool albHave = false;
  TpView albView{};
  nccl_comm_t comm = nullptr;
  int commRanks = 0, commRank = 0;
  // Reduced frame (root of sail_reduce / device 0 of a multi-device context): the sum of every rank's
  // cumulative accumulator, recomputed from scratch by each reduce, so render -> reduce -> render -> reduce
  // never counts a sample twice. While `reduced` is set, readback / read_accum / filter show this frame.
  float4* frame = nullptr;
  float4* frameN = nullptr;  // reduced AOVs (SAIL_FLAG_AOV)
  float4* frameP = nullptr;
  bool reduced = false;
  // Multi-device context (sail_create_multi): one sub-context per device, each rendering its share of the
  // partition on its own stream; `dirty` = rendered since the last reduce. Devices are all distinct (grouped
  // RCCL reduce over a ncclCommInitAll communicator) or all the same one (`groupLocal`: summed by a kernel).
  std::vector<sail_ctx*> subs;
  // A checkpoint loaded part by part (sail_load_accum part >= 0): the parts still missing (bit i = device i) and the
  // checkpoint's k. Until every part is in, the frame mixes old and loaded accumulators, so rendering, reading, saving
  // and reducing are refused.
  uint64_t loadMissing = 0;
  uint64_t loadK = 0;
  std::vector<nccl_comm_t> groupComms;
  bool groupLocal = false;
  bool dirty = false;
  // One-sample frames of sail_render waiting to be launched together (sail_render / flushQueued): their records
  // (global sample index already counted in k), the bounce count and eye they were queued with
  std::vector<SailSample> queued;
  int queuedBounces = 0;
  float eyeCache[3] = {0.0f, 0.0f, 0.0f};
  std::string err;
};

namespace {

int fail(sail_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}
// a multi-device context's call failed in one of its sub-contexts: carry that context's message up
int relay(sail_ctx* c, int rc, const sail_ctx* sub) {
  if (rc != SAIL_OK && sub && c != sub) c->err = sub->err;
  return rc;
}
// a part-wise checkpoint load still missing parts (sail_load_accum): refuse whatever would see the half-loaded frame
int loadIncomplete(sail_ctx* c, const char* what) {
  if (!c->loadMissing) return SAIL_OK;
  return fail(c, SAIL_E_STATE, "%s: checkpoint parts not loaded yet (mask 0x%llx of %d devices); load every part or reset",
              what, (unsigned long long)c->loadMissing, (int)c->subs.size());
}
#define HIPCHK(ctx, call)                                                                       \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return fail((ctx), SAIL_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// A device buffer allocated on first use and kept for the context's life (sail_destroy frees it)
template <class T>
int allocOnce(sail_ctx* c, T** p, size_t bytes, const char* what) {
  if (*p) return SAIL_OK;
  if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; return fail(c, SAIL_E_OOM, "%s", what); }
  return SAIL_OK;
}
// A grow-only device buffer of *size units: a request for more waits for the stream (launches in flight read the old
// one), frees it and allocates `bytes` anew
template <class T, class N>
int growBuffer(sail_ctx* c, T** p, N* size, N need, size_t bytes, const char* what) {
  if (need <= *size) return SAIL_OK;
  if (*p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(*p)); *p = nullptr; }
  *size = 0;
  if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; return fail(c, SAIL_E_OOM, "%s", what); }
  *size = need;
  return SAIL_OK;
}

// the smallest precompiled plugin-set kernel that covers the scene (sail_device.h SAIL_KSET_*)
int kernelSetFor(const sail_ctx* c) {
  if (c->forceGeneric || c->n >= c->cullMinPrims) return SAIL_KSET_GENERIC;
  const sail_plugins& p = c->plugins;
  const bool lightsOk = c->ln == 0 || (p.light_mask & ~SAIL_KSET_CORNELL_LIGHTS) == 0;
  if ((p.shape_mask & ~SAIL_KSET_CORNELL_SHAPES) == 0 && (p.material_mask & ~SAIL_KSET_CORNELL_MATS) == 0 &&
      (p.texture_mask & ~SAIL_KSET_CORNELL_TEX) == 0 && lightsOk && SAIL_KSET_CORNELL_LIGHTS == 0 && c->ln == 0)
    return SAIL_KSET_CORNELL;
  if ((p.shape_mask & ~SAIL_KSET_ROOM_SHAPES) == 0) return SAIL_KSET_ROOM;
  return SAIL_KSET_GENERIC;
}

// the sample-group stage's cap (12 B per owned pixel per staged sample): 8 GiB
constexpr size_t kStageCapBytes = (size_t)8 << 30;
// Launch bounds of a run-time kernel by form and by the precompiled family its plugin set falls in: the precompiled
// kernels' own (6 waves all-plugin, 8 Cornell, 7 room, 8 pre-cull), except that a flat scene outside the Cornell and room
// sets compiled in the room form runs at 8 waves (its smaller kernel spills less: ALL +3.6 %, AREA +3.8 % over 7,
// profiles/r04_jit_occupancy.jsonl).
int jitWaves(int mode, int kernelSet) {
  if (mode == SAIL_JIT_MODE_CULL) return 8;
  if (mode == SAIL_JIT_MODE_ROOM) return kernelSet == SAIL_KSET_ROOM ? 7 : 8;
  return kernelSet == SAIL_KSET_CORNELL ? 8 : 6;
}
// the tiles of this rank's share of the partition
int partitionTiles(const sail_ctx* c, int* tilesX, int* tilesY) {
  const int tx = (c->W + 63) / 64, ty = (c->H + 63) / 64;
  *tilesX = tx; *tilesY = ty;
  if (c->partMode == SAIL_PART_SAMPLES) return tx * ty;
  const int total = tx * ty;
  return c->rank < total ? (total - c->rank + c->world - 1) / c->world : 0;
}
// Workgroup shape of a run-time kernel by form (profiles/r05_ns_*.jsonl, r05_nt*_C1.jsonl; 1080p / 4K, 64-sample
// launches, bit-identical): the Cornell form at 512 threads holding 16 samples of 32 pixels (C1 98.6 Gseg/s against 97.5-98.1
// at 256 threads x 1 sample with 8 staged sample groups: no stage and no sail_accum_kernel at full frame; 512 x 1 sample,
// staged, 98.8-99.0); the room and pre-cull forms at their 256 / 1,024 threads holding 4 samples (C3 +1.2 %, C4 +0.8 %;
// 16 samples C3 -0.4 %, C4 -1.3 %; C3 at 128 / 512 threads -9 % / -4 %, C4 at 512 -62 %: its LDS tables then
// leave room for too few workgroups).
// The Cornell form's 16 samples in flight pay while the context's share of the frame queues enough workgroups: with a
// small share (a rank of 8 or more, one eighth of 1080p) it holds 1 sample and the launch is split into staged sample
// groups instead (C2 per GPU at N = 8: 95.4 Gseg/s against 92.1 with 16 samples and no groups, 91.4 with both; at
// N = 4 95.2 against 94.9; profiles/r05_scale_ns_c2.jsonl, tools/scale_groups.sh).
// (the share is the partition's, whatever tile mask is set: a mask must not swap the scene's kernel for another build)
bool cornellShareLarge(const sail_ctx* c) {
  int tx, ty;
  const int owned = partitionTiles(c, &tx, &ty);
  // residency rounds of 512-thread workgroups at 8 waves per SIMD (4,096 / 32 pixels = 128 workgroups per tile)
  const double rounds = (double)owned * 128.0 / ((double)c->numCUs * 4.0);
  return rounds >= 12.0;
}
int jitNsFor(const sail_ctx* c, int mode, int kernelSet) {
  if (mode == SAIL_JIT_MODE_FLAT && kernelSet == SAIL_KSET_CORNELL) return cornellShareLarge(c) ? 16 : 1;
  if (mode == SAIL_JIT_MODE_ROOM || mode == SAIL_JIT_MODE_CULL) return 4;
  return 1;
}
int jitNtFor(int mode, int kernelSet) {
  return (mode == SAIL_JIT_MODE_FLAT && kernelSet == SAIL_KSET_CORNELL) ? 512 : 0;
}
// The run-time kernel spec of the context's scene under its switches, or false when none applies.
// SAIL_DEBUG_JIT bits (include/sail_hip.h): 1 flat scenes outside the Cornell and room sets, 2 pre-cull scenes, 4 room-set
// scenes, 8 the flat scenes of bit 1 in the room form, 16 flat scenes compiled for their rows as well (any flat scene),
// 32 the row-shading form of the value kernel (valueSpecFor).
bool jitSpecFor(const sail_ctx* c, SailJitSpec* out, int* mode) {
  if (!c->jit || !c->haveScene || c->forceGeneric) return false;
  const int set = kernelSetFor(c);
  const bool rows = (c->jit & 16) && c->n >= 1 && c->n <= kSailJitMaxRows && c->n < c->cullMinPrims &&
                    (int)c->primTypes.size() == c->n;
  int m;
  if (set == SAIL_KSET_GENERIC && c->n >= c->cullMinPrims) {
    if (!(c->jit & 2)) return false;
    m = SAIL_JIT_MODE_CULL;
  } else if (set == SAIL_KSET_GENERIC) {
    if (!(c->jit & 1) && !rows) return false;
    m = (c->jit & 8) ? SAIL_JIT_MODE_ROOM : SAIL_JIT_MODE_FLAT;
  } else if (set == SAIL_KSET_ROOM) {
    if (!(c->jit & 4) && !rows) return false;
    m = SAIL_JIT_MODE_ROOM;
  } else {
    if (!rows) return false;  // the Cornell kernel's set is the Cornell box's own
    m = SAIL_JIT_MODE_FLAT;
  }
  const sail_plugins& p = c->plugins;
  SailJitSpec spec;
  spec.ks = p.shape_mask; spec.km = p.material_mask; spec.kt = p.texture_mask; spec.kl = p.light_mask;
  spec.mode = m;
  spec.waves = jitWaves(m, set);
  spec.ldsFit = (m == SAIL_JIT_MODE_CULL && c->n <= SAIL_CULL_LDS_ROWS && c->tn <= SAIL_CULL_LDS_TP) ? 1 : 0;
  spec.ns = c->jitNs ? c->jitNs : jitNsFor(c, m, set);
  spec.nt = c->jitNt ? c->jitNt : jitNtFor(m, set);
  if (sailJitThreads(spec) / spec.ns < 16) spec.ns = 4;  // at least 16 pixels per workgroup
  if (rows && m != SAIL_JIT_MODE_CULL) {
    spec.rows = c->n;
    for (int i = 0; i < c->n; i++) spec.types[i] = c->primTypes[i];
    for (int i = 0; i < c->n; i++)
      if (spec.types[i] < 1 || !((spec.ks >> spec.types[i]) & 1u)) spec.rows = 0;  // a row no compiled shape hits
    if (!spec.rows) for (int& t : spec.types) t = 0;
    // the room form copies both tables into LDS (C3 +2.8 %, UI +2.2 %; the Cornell form measured -0.5 %)
    if (spec.rows && m == SAIL_JIT_MODE_ROOM && c->tn >= 1 && c->tn <= kSailJitMaxFlatTp) spec.tn = c->tn;
  }
  *out = spec;
  *mode = m;
  return true;
}
// The rows changed, or the spec their value kernel was derived from: the hold on the value spec goes (a queued build of it
// is skipped, a finished one stays in the caches for a scene that returns to this pose), its masked twin's first, launches
// run the types kernel again, and the settle count restarts.
void dropValues(sail_ctx* c) {
  c->valueTwin.drop(c->device, c->stream);
  c->valueSlot.drop(c->device, c->stream);
  c->settled = 0;
}
// Whether the value kernel of a scene that rendered `settled` samples since its rows changed is asked for now
// (sail_plan_settle; after: SAIL_DEBUG_JIT_VALUES_AFTER)
bool settledFor(uint64_t settled, int after) { return after >= 0 && settled >= (uint64_t)after; }
// What a path's last bounce can add at a hit on each row (SailTraceArgs.lastQuietRows / lastSkipSort), decided with
// the kernel's own tests and f32 operations on the values it reads (sail_trace.hip shadeLast: emission, matCat,
// matRow -> kd, sigma, the Cornellbox wall constants or the uniform texture's colour). `lights`: the kernel that will
// run has a light plugin compiled in (shadeLast then declines every lit matte hit).
//   quiet: the emission words are +0.0f bit for bit (the facing test can only zero them again), and the row is not a
//     matte, or it is one whose light term is fma(f, 0, 0) with f = (kd * sc) * (1 / pi) finite for every colour sc the
//     record can give it: +0. Its update is e + (+0) * throughput whatever the record says.
//   record-only: shadeLast accepts every hit on the row, but the value depends on the record (an emitter's facing test,
//     a non-finite f).
//   full: shadeLast can decline (a light plugin, Oren-Nayar), or the matte's colour is not a per-scene constant.
// Rows of more than 32-row scenes are not classified (the pre-cull kernels take none of this); a row no ray can hit
// (type 0) has no class. skipSort: no full row, and every record-only row emits (a black one is a matte whose light
// term is not +0: those keep the sort). Anything this cannot decide is full.
void lastBounceRows(const std::vector<SailPrim>& prims, const float* tp, int tn, uint32_t matMask, bool lights,
                    uint32_t* quietRows, int* skipSort) {
  *quietRows = 0;
  *skipSort = 0;
  const int n = (int)prims.size();
  if (n < 1 || n > 32 || tn < 1 || !tp) return;
  constexpr float kEps = 1e-5f, kInvPI = 0.3183098861837907f;  // sail_trace.hip
  bool skip = true, any = false;
  for (int i = 0; i < n; i++) {
    const SailPrim& p = prims[(size_t)i];
    if (p.type == 0) continue;
    any = true;
    uint32_t eb[3];
    memcpy(eb, p.em, sizeof eb);
    const bool emPosZero = (eb[0] | eb[1] | eb[2]) == 0u;
    const bool emBlack = p.em[0] == 0.0f && p.em[1] == 0.0f && p.em[2] == 0.0f;  // isBlack: -0 too, never NaN
    const bool matte = (int)(short)(p.cats & 0xffff) == SAIL_MATTE;
    bool matteOk = true;  // a lit matte hit on the row adds exactly +0
    if (matte) {
      const bool rowsOk = p.matRow >= 0 && p.matRow < tn && p.texRow >= 0 && p.texRow < tn;
      if (lights || !rowsOk) {
        matteOk = false;
      } else if ((matMask >> SAIL_MATTE) & 1u) {  // material()'s matte branch; without the plugin f stays +0
        const float kd = tp[(size_t)p.matRow * 16 + 1], sigma = tp[(size_t)p.matRow * 16 + 2];
        float sc[4][3] = {{0.25f, 0.75f, 0.25f}, {0.25f, 0.25f, 0.75f}, {1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f}};
        int ncol = 0;
        if (p.type == SAIL_CORNELLBOX) {
          ncol = 4;
        } else if ((p.cats >> 16) == SAIL_TEX_UNIFORM) {
          for (int k = 0; k < 3; k++) sc[0][k] = tp[(size_t)p.texRow * 16 + 1 + k];
          ncol = 1;
        }
        matteOk = sigma < kEps && ncol > 0;
        for (int q = 0; q < ncol; q++)
          for (int k = 0; k < 3; k++) {
            volatile float f = kd * sc[q][k];  // two roundings, as the kernel's (kd * sc) * kInvPI
            f = f * kInvPI;
            if (!std::isfinite((float)f)) matteOk = false;
          }
      }
    }
    if (emPosZero && matteOk) *quietRows |= 1u << i;
    else if (!(matteOk && !emBlack)) skip = false;
  }
  *skipSort = (any && skip) ? 1 : 0;
}
// The value spec of a types spec: the flat form compiled for rows, with a texParams table small enough to compile in.
// Scenes of the Cornell plugin set only (cubes, spheres, the box; matte and mirror; no textures, no lights): the form
// that was measured and that the parity tests run with constant rows. A flat-form kernel of a wider set (SAIL_DEBUG_JIT
// without bit 8) would read its light sampler's geometry rows, textures and a full texParams table through the constant
// tables too, which no test covers: it keeps its types kernel.
// jit: the SAIL_DEBUG_JIT switches; bit 32 gives scenes of at most kSailJitRowRecordMax rows the row-shading form
// (SAIL_JIT_ROWSHADE in sail_trace.hip).
bool valueSpecFor(const SailJitSpec& types, const std::vector<uint32_t>& rowWords, const float* tp, int tn, int jit, SailJitSpec* out) {
  const bool cornellSet = (types.ks & ~SAIL_KSET_CORNELL_SHAPES) == 0 && (types.km & ~SAIL_KSET_CORNELL_MATS) == 0 &&
                          (types.kt & ~SAIL_KSET_CORNELL_TEX) == 0 && types.kl == 0;
  if (!cornellSet || types.mode != SAIL_JIT_MODE_FLAT || types.rows <= 0 || types.tn != 0 || tn < 0 || tn > kSailJitMaxFlatTp ||
      rowWords.size() != (size_t)types.rows * 32 || (tn > 0 && !tp))
    return false;
  *out = types;
  out->rowWords = rowWords;
  out->tpWords.resize((size_t)tn * 16);
  if (tn > 0) memcpy(out->tpWords.data(), tp, sizeof(float) * 16 * (size_t)tn);
  out->rowForm = out->rowShade = out->rowQuiet = 0;
  if ((jit & 32) && types.rows <= kSailJitRowRecordMax) {
    out->rowForm = 1;
    // The rows that get a shading copy of their own: the quiet ones (lastBounceRows, for a kernel without a light plugin:
    // cornellSet), whose copies also leave the radiance alone. Measured on C2: a copy
    // for every row lost 4.8 % (VGPR spills 22 -> 50), copies for the quiet rows gained 4.5 %, and 6.7 % without the
    // radiance round trip; a copy for the emitting row on top of those gained less (3.9 %).
    std::vector<SailPrim> prims((size_t)types.rows);
    memcpy(prims.data(), rowWords.data(), sizeof(SailPrim) * prims.size());
    uint32_t quiet = 0;
    int skip = 0;
    lastBounceRows(prims, tp, tn, types.km, false, &quiet, &skip);
    out->rowShade = (int)(quiet & ((1u << types.rows) - 1u));
    out->rowQuiet = out->rowShade;
  }
  return true;
}
// Ask for the scene's value kernel once it has settled (after every refreshJit, and between and after launches): the build
// starts in the background, or the object loads here when a disk cache has it, as refreshJit does for the types kernel.
// When it fails the types kernel serves.
void refreshValues(sail_ctx* c) {
  if (!c->subs.empty() || c->valueSlot.have || !c->typesSlot.have || !settledFor(c->settled, c->jitValuesAfter)) return;
  SailJitSpec spec;
  if (!valueSpecFor(c->typesSlot.spec, c->rowWords, c->tpRows.data(), c->tn, c->jit, &spec)) return;
  c->valueSlot.adopt(c->device, c->stream, spec);
}
// Re-derive the scene's run-time kernel after anything it depends on changed (scene, rows, switches). A new spec starts
// its background build now (Tracer.update links the scene's program, tracer.js:42-90), so the caller never waits for it.
void refreshJit(sail_ctx* c) {
  // a multi-device context renders through its sub-contexts, which derive their own kernels (its own plugins and rows
  // are not kept: a spec derived here would be a useless build)
  if (!c->subs.empty()) return;
  SailJitSpec spec;
  int mode = 0;
  const bool have = jitSpecFor(c, &spec, &mode);
  if (have == c->typesSlot.have && (!have || sailJitSpecEqual(spec, c->typesSlot.spec))) return;
  dropValues(c);  // the value kernel is the old spec's
  c->typesTwin.drop(c->device, c->stream);  // and so is the types kernel's masked twin
  if (have) c->typesSlot.adopt(c->device, c->stream, spec);
  else c->typesSlot.drop(c->device, c->stream);
}
// The masked twin of the loaded kernel in `base`, held in `twin`: asked for at the first launch under a tile mask, and
// anew when the base's spec changed. Launches wait up to jitWait for it, as for the types kernel; null while it is being
// built or when it failed.
JitSlot* maskedTwin(sail_ctx* c, JitSlot& twin, const JitSlot& base) {
  SailJitSpec want = base.spec;
  want.masked = 1;
  if (!twin.have || !sailJitSpecEqual(twin.spec, want)) twin.adopt(c->device, c->stream, want);
  return twin.poll(c->device, c->jitWait) ? &twin : nullptr;
}
// The slot whose kernel a launch runs, or null: the precompiled kernel of the scene's set then runs (its _masked instance
// under a tile mask), with the same results. The value kernel when it is loaded, else the types kernel, waited for up to
// jitWait; under a tile mask the masked twin of the first of the two that is loaded and whose twin is. No launch waits
// for the value kernel itself: it is a bonus of a scene at rest, and its build may take longer than the render. None
// under the wavefront switch.
JitSlot* runningSlot(sail_ctx* c, bool masked, bool wavefront) {
  if (wavefront) return nullptr;
  if (c->valueSlot.poll(c->device, 0)) {
    JitSlot* s = masked ? maskedTwin(c, c->valueTwin, c->valueSlot) : &c->valueSlot;
    if (s) return s;
  }
  if (c->typesSlot.poll(c->device, c->jitWait)) return masked ? maskedTwin(c, c->typesTwin, c->typesSlot) : &c->typesSlot;
  return nullptr;
}
// Samples per launch when the host has not fixed them: the Cornell form holding 16 samples in flight runs a whole
// 1,024-sample frame in one launch (its waves live 16 times longer, so their per-wave start -- the spill stores of the
// loop-invariant registers among it -- is paid 16 times less often: C1 Gseg/s at 64 / 128 / 256 / 1,024 samples per
// launch 97.26 / 97.73 / 97.99 / 98.36, profiles/r05_launch_*.jsonl); everything else 64 (sample groups stage a launch's
// samples, which a larger launch would push past the stage's cap).
int launchSamples(const sail_ctx* c) {
  if (c->launchSpp > 0) return c->launchSpp;
  const JitSlot& t = c->typesSlot;
  return (t.have && t.state != SAIL_KERNEL_JIT_FAILED && t.spec.ns >= 16) ? 1024 : 64;
}
// the tiles a launch traces, and their in-frame pixels: the share, or with a tile mask its active tiles (tileMap)
int ownedTiles(const sail_ctx* c, int* tilesX, int* tilesY) {
  const int part = partitionTiles(c, tilesX, tilesY);
  return c->maskSet ? c->maskTiles : part;
}
long long ownedPixels(const sail_ctx* c) {
  if (c->maskSet) return c->maskPixels;
  int tx, ty;
  const int owned = partitionTiles(c, &tx, &ty);
  long long px = 0;
  const int w = (c->partMode == SAIL_PART_SAMPLES) ? 1 : c->world, r = (c->partMode == SAIL_PART_SAMPLES) ? 0 : c->rank;
  for (int j = 0; j < owned; j++) {
    const int t = r + j * w;
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    const int cw = (c->W - x0) < 64 ? (c->W - x0) : 64, ch = (c->H - y0) < 64 ? (c->H - y0) : 64;
    px += (long long)cw * ch;
  }
  return px;
}

int collectEvents(sail_ctx* c) {
  for (auto& pr : c->pending) {
    HIPCHK(c, hipEventSynchronize(pr.second));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, pr.first, pr.second));
    c->kernelMs += ms;
    c->lastLaunchMs = ms;
    c->evPool.push_back(pr.first);
    c->evPool.push_back(pr.second);
  }
  c->pending.clear();
  return SAIL_OK;
}
int getEvent(sail_ctx* c, hipEvent_t* ev) {
  if (!c->evPool.empty()) { *ev = c->evPool.back(); c->evPool.pop_back(); return SAIL_OK; }
  HIPCHK(c, hipEventCreate(ev));
  return SAIL_OK;
}
// up to 8 events of the pool for the length of a scope: rc is getEvent's failure, and the ones taken go back at the end
struct PooledEvents {
  sail_ctx* c;
  hipEvent_t ev[8] = {};
  int n = 0, rc = SAIL_OK;
  PooledEvents(sail_ctx* ctx, int want) : c(ctx) {
    while (n < want && !(rc = getEvent(c, &ev[n]))) n++;
  }
  ~PooledEvents() {
    for (int i = 0; i < n; i++) c->evPool.push_back(ev[i]);
  }
  PooledEvents(const PooledEvents&) = delete;
  PooledEvents& operator=(const PooledEvents&) = delete;
  hipEvent_t operator[](int i) const { return ev[i]; }
};

// corner directions of vstrace.glsl:4-6 for one jittered inverse matrix (column-major, f32)
void cornerDirs(const float* M, const float* eye, float out[4][3]) {
  static const float cx[4] = {-1.0f, -1.0f, 1.0f, 1.0f}, cy[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
  for (int c = 0; c < 4; c++) {
    float q[4];
    for (int r = 0; r < 4; r++) q[r] = M[0 * 4 + r] * cx[c] + M[1 * 4 + r] * cy[c] + M[2 * 4 + r] * 0.0f + M[3 * 4 + r] * 1.0f;
    const float w[3] = {gdiv(q[0], q[3]) - eye[0], gdiv(q[1], q[3]) - eye[1], gdiv(q[2], q[3]) - eye[2]};
    const float len = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    out[c][0] = gdiv(w[0], len); out[c][1] = gdiv(w[1], len); out[c][2] = gdiv(w[2], len);
  }
}

int resetAccum(sail_ctx* c) {
  c->reduced = false;
  c->queued.clear();  // queued one-sample frames belong to the accumulation being discarded
  c->noiseHave = false;  // so does the noise estimate's mark (sail_load_accum puts it back: it continues a render)
  c->maskSet = false;    // and the tile mask: every tile of the new accumulation starts at sample 0
  c->mask.clear();
  c->frozenAt.clear();
  c->tpResolved = false;  // Out no longer belongs to this accumulator: sail_temporal_filter wants a resolve of the new one
  const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
  HIPCHK(c, hipMemsetAsync(c->accum, 0, bytes, c->stream));
  if (c->aovN) HIPCHK(c, hipMemsetAsync(c->aovN, 0, bytes, c->stream));
  if (c->aovP) HIPCHK(c, hipMemsetAsync(c->aovP, 0, bytes, c->stream));
  if ((c->aovN || c->aovP) && c->partMode == SAIL_PART_TILES && c->world > 1)
    HIPCHK(c, sail_launch_negzero_unowned(c->aovN, c->aovP, c->W, c->H, c->rank, c->world, c->stream));
  if (c->segCounter) HIPCHK(c, hipMemsetAsync(c->segCounter, 0, SAIL_SEG_SLOTS * sizeof(unsigned long long), c->stream));
  int rc = collectEvents(c);
  if (rc) return rc;
  c->k = 0;
  c->samplesThisRank = 0;
  c->nominalSegments = 0;
  c->kernelMs = 0.0;
  c->lastLaunchMs = 0.0;
  c->launches = 0;
  return SAIL_OK;
}

// Decode the objects rows into SailPrim records with the reference's addressing rules
// (shader.shape.js:34 row = float(i)/float(n-1); parseX readFloat/readVec3 columns; matIndex/texIndex as
// readFloat(...)/float(tn-1) normalised rows; cornellbox.glsl:17 material from slot 7).
// Rectangle frame (rectangle.glsl:32-44), the same f32 operations in the same order as the per-ray GLSL,
// evaluated once per scene: a[6..8] normal, a[9..11] ss, a[12..14] ts, a[15] maxX, a[16] maxY and
// a[17] the area-light pdf 1/(|x||y|) of sampleGeometry (shader.shape.js:53-67). Host f32 arithmetic is
// IEEE (SSE, no contraction), so the values are bit-identical to the kernel's own evaluation.
struct F3 { float x, y, z; };
F3 f3cross(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float f3dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
F3 f3div(F3 a, float s) { return {gdiv(a.x, s), gdiv(a.y, s), gdiv(a.z, s)}; }
void rectFrameHost(SailPrim& p) {
  const F3 dpdu{p.a[3] - p.a[0], 0.0f, 0.0f}, dpdv{0.0f, p.a[4] - p.a[1], p.a[5] - p.a[2]};
  const F3 cr = f3cross(dpdu, dpdv);
  const F3 normal = f3div(cr, sqrtf(f3dot(cr, cr)));
  const float maxX = sqrtf(f3dot(dpdu, dpdu)), maxY = sqrtf(f3dot(dpdv, dpdv));
  const F3 ss = f3div(dpdu, maxX);
  const F3 ts = f3cross(normal, ss);
  const float f[12] = {normal.x, normal.y, normal.z, ss.x, ss.y, ss.z, ts.x, ts.y, ts.z, maxX, maxY,
                       gdiv(1.0f, maxX * maxY)};
  memcpy(&p.a[6], f, sizeof f);
}

// GLSL min/max as v_min_f32/v_max_f32 evaluate them (a NaN operand yields the other; -0 < +0)
float hwmin(float a, float b) { if (a != a) return b; if (b != b) return a; if (a < b) return a; if (b < a) return b; return signbit(a) ? a : b; }
float hwmax(float a, float b) { if (a != a) return b; if (b != b) return a; if (a > b) return a; if (b > a) return b; return signbit(a) ? b : a; }
// Per-scene quadric constants, each the exact f32 expression the GLSL evaluates per ray:
//   cone (cone.glsl:58-59)            a[5] = (rad / h)^2
//   hyperboloid (hyperboloid.glsl:13-24)  a[11] = max(r1, r2), a[12] = min(p1.z, p2.z), a[13] = max(p1.z, p2.z)
//   paraboloid (paraboloid.glsl:60)   a[6] = zMax / (rad * rad)
void quadricHost(SailPrim& p) {
  if (p.type == SAIL_CONE) { float k = gdiv(p.a[4], p.a[3]); p.a[5] = k * k; }
  if (p.type == SAIL_HYPERBOLOID) {
    const float r1 = sqrtf(p.a[3] * p.a[3] + p.a[4] * p.a[4]), r2 = sqrtf(p.a[6] * p.a[6] + p.a[7] * p.a[7]);
    p.a[11] = hwmax(r1, r2); p.a[12] = hwmin(p.a[5], p.a[8]); p.a[13] = hwmax(p.a[5], p.a[8]);
  }
  if (p.type == SAIL_PARABOLOID) p.a[6] = gdiv(hwmax(p.a[3], p.a[4]), p.a[5] * p.a[5]);
}

// Conservative world-space bounds of what each primitive's intersection can return, padded, in a[18..23]
// (min xyz, max xyz; +-inf when the shape has no finite bound). The trace kernel uses them for a cheap f32
// pre-cull before the exact per-primitive test: a primitive whose padded box the ray misses, or enters
// beyond the closest distance so far, cannot change the sweep's result (n = 67).
// Local frames: OBJECT_SPACE maps world (x, y, z) -> local (-z, x, y), so the local z axis is world y.
struct PrimBox { double lo[3], hi[3]; };
PrimBox primBoundsRaw(const SailPrim& p) {
  const double inf = INFINITY;
  PrimBox b{{-inf, -inf, -inf}, {inf, inf, inf}};
  double* lo = b.lo;
  double* hi = b.hi;
  const float* a = p.a;
  auto box = [&](double x0, double y0, double z0, double x1, double y1, double z1) {
    lo[0] = fmin(x0, x1); lo[1] = fmin(y0, y1); lo[2] = fmin(z0, z1);
    hi[0] = fmax(x0, x1); hi[1] = fmax(y0, y1); hi[2] = fmax(z0, z1);
  };
  switch (p.type) {
    case SAIL_CUBE: case SAIL_CORNELLBOX: box(a[0], a[1], a[2], a[3], a[4], a[5]); break;
    case SAIL_RECTANGLE: {  // corners mn + {0, maxX} ss + {0, maxY} ts (rectangle.glsl:32-63)
      const double ss[3] = {a[9], a[10], a[11]}, ts[3] = {a[12], a[13], a[14]}, mx = a[15], my = a[16];
      for (int k = 0; k < 3; k++) {
        const double c0 = a[k], c1 = a[k] + mx * ss[k], c2 = a[k] + my * ts[k], c3 = a[k] + mx * ss[k] + my * ts[k];
        lo[k] = fmin(fmin(c0, c1), fmin(c2, c3));
        hi[k] = fmax(fmax(c0, c1), fmax(c2, c3));
      }
      break;
    }
    case SAIL_SPHERE: { const double r = fabs(a[3]); box(a[0] - r, a[1] - r, a[2] - r, a[0] + r, a[1] + r, a[2] + r); break; }
    case SAIL_CONE: case SAIL_CYLINDER: {  // radius <= rad for local z in [-EPS, h]
      const double r = fabs(a[4]);
      box(a[0] - r, a[1], a[2] - r, a[0] + r, a[1] + a[3], a[2] + r);
      break;
    }
    case SAIL_DISK: { const double r = fabs(a[3]); box(a[0] - r, a[1], a[2] - r, a[0] + r, a[1], a[2] + r); break; }
    case SAIL_HYPERBOLOID: {  // ah (x^2 + y^2) - ch z^2 = 1 for z in [zMin, zMax] (a[12], a[13])
      const double ah = a[9], ch = a[10], z0 = a[12], z1 = a[13];
      double r2 = -1.0;
      if (ah > 0.0 && z0 <= z1) {
        const double zs[3] = {z0, z1, (z0 < 0.0 && z1 > 0.0) ? 0.0 : z0};
        for (double z : zs) r2 = fmax(r2, (1.0 + ch * z * z) / ah);
      }
      if (r2 >= 0.0 && std::isfinite(r2)) {
        const double r = sqrt(r2);
        box(a[0] - r, a[1] + z0, a[2] - r, a[0] + r, a[1] + z1, a[2] + r);
      }
      break;
    }
    case SAIL_PARABOLOID: {  // k (x^2 + y^2) = z, k = zMax / rad^2 (a[6]); z in [min(z0,z1), max(z0,z1)]
      const double k = a[6], z0 = fmin(a[3], a[4]), z1 = fmax(a[3], a[4]);
      if (k > 0.0 && std::isfinite(k) && z1 >= 0.0) {
        const double r = sqrt(z1 / k);
        box(a[0] - r, a[1] + z0, a[2] - r, a[0] + r, a[1] + z1, a[2] + r);
      }
      break;
    }
    default: break;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) { lo[k] = -inf; hi[k] = inf; }
  return b;
}

// Union of the primitives' finite bounds: every hit point, hence every bounce / shadow ray origin, lies in it.
SceneBox sceneBox(const std::vector<PrimBox>& raw) {
  SceneBox s{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0.0};
  bool any = false;
  for (const PrimBox& b : raw) {
    if (!std::isfinite(b.lo[0]) || !std::isfinite(b.lo[1]) || !std::isfinite(b.lo[2])) continue;
    any = true;
    for (int k = 0; k < 3; k++) { s.lo[k] = fmin(s.lo[k], b.lo[k]); s.hi[k] = fmax(s.hi[k], b.hi[k]); }
  }
  if (!any) { for (int k = 0; k < 3; k++) s.lo[k] = s.hi[k] = 0.0; }
  s.diag = sqrt((s.hi[0] - s.lo[0]) * (s.hi[0] - s.lo[0]) + (s.hi[1] - s.lo[1]) * (s.hi[1] - s.lo[1]) +
                (s.hi[2] - s.lo[2]) * (s.hi[2] - s.lo[2]));
  return s;
}

// Padding of each primitive's bounds into a[18..23]. The exact f32 tests (the reference's GLSL) can report a hit
// slightly outside the true surface, the more so the farther the ray origin: a slab / plane distance is off by
// about L 2^-23 at range L, and a quadric's discriminant b^2 - 4ac loses about 20 L^2 2^-24 to cancellation,
// which moves its hit band by that over the local radius (and by its square root near a cone apex or where the
// radius is unknown). Origins here are hit points inside the scene box, or the eye when it lies within one
// scene diagonal D of the box (sail_launch: cullPrimary), so L = 2D bounds every origin-to-primitive distance.
// Padding = 1e-3 + 1e-4 |bound| + 2^-20 L, plus 1.2e-6 L^2 / r for quadrics (+ 1.1e-3 L for cones,
// hyperboloids and paraboloids). Measured by the far-origin tests (tests/test_gpu_fullsize.py).
void padPrimBounds(std::vector<SailPrim>& prims, const std::vector<PrimBox>& raw, const SceneBox& sb) {
  const double L = 2.0 * sb.diag, kQ = 20.0 / 16777216.0;
  for (size_t i = 0; i < prims.size(); i++) {
    SailPrim& p = prims[i];
    const PrimBox& b = raw[i];
    double extra = L / 1048576.0;
    double r = -1.0;  // local radius of a quadric (its smallest), -1: not a quadric
    bool apex = false;
    switch (p.type) {
      case SAIL_SPHERE: r = fabs(p.a[3]); break;
      case SAIL_CYLINDER: r = fabs(p.a[4]); break;
      case SAIL_CONE: r = fabs(p.a[4]); apex = true; break;
      case SAIL_HYPERBOLOID: case SAIL_PARABOLOID:
        r = 0.5 * fmin(b.hi[0] - b.lo[0], b.hi[2] - b.lo[2]); apex = true; break;
      default: break;
    }
    if (r >= 0.0) {
      extra += (r > 0.0 && std::isfinite(r)) ? kQ * L * L / r : INFINITY;
      if (apex) extra += sqrt(kQ) * L;
    }
    for (int k = 0; k < 3; k++) {
      double lo = b.lo[k], hi = b.hi[k];
      if (std::isfinite(lo) && std::isfinite(hi) && std::isfinite(extra)) {
        const double pad = 1e-3 + 1e-4 * fmax(fabs(lo), fabs(hi)) + extra;
        lo -= pad; hi += pad;
      } else {
        lo = -INFINITY; hi = INFINITY;
      }
      p.a[18 + k] = (float)lo; p.a[21 + k] = (float)hi;
    }
  }
}

// Largest padded-bound coordinate of the scene, inf when a primitive has no finite bound. Every ray origin
// is the eye or a hit point inside some padded box, so |origin| <= max(extent, |eye|) (see cullFmaOk).
double primExtent(const std::vector<SailPrim>& prims) {
  double m = 0.0;
  for (const SailPrim& p : prims)
    for (int k = 18; k < 24; k++) m = fmax(m, std::isfinite(p.a[k]) ? fabs((double)p.a[k]) : INFINITY);
  return m;
}

// The fused pre-cull form (sail_trace.hip padHitF) tests each slab plane as fma(a, R, -RN(o R)): the plane
// lands within |o| 2^-24 of where the plain (a - o) R puts it, so the test stays conservative while that is
// far inside the 1e-3 padding. |o| < 4096 keeps it under 2.5e-4; it also keeps o R finite with R <= 1e30.
bool cullFmaOk(const sail_ctx* c) {
  const double e = fmax(fmax(fabs(c->eyeCache[0]), fabs(c->eyeCache[1])), fabs(c->eyeCache[2]));
  return c->cullFma && fmax(c->primExtent, e) < 4096.0;
}

// Primary rays may use the pre-cull only when the eye lies within one scene diagonal of the scene box: the
// padding (padPrimBounds) covers origin-to-primitive distances up to two diagonals.
int eyeNearScene(const sail_ctx* c) {
  double d2 = 0.0;
  for (int k = 0; k < 3; k++) {
    const double e = c->eyeCache[k];
    const double g = e < c->scene.lo[k] ? c->scene.lo[k] - e : (e > c->scene.hi[k] ? e - c->scene.hi[k] : 0.0);
    d2 += g * g;
  }
  return d2 == d2 && sqrt(d2) <= c->scene.diag;
}

// the category words the kernel tests (material.glsl / texture dispatch: int(readFloat(row, 0))), clamped to
// [-1, 32] (every test is == c, < 0 or >= 32 against categories in [0, 31]) and packed in SailPrim.cats
void fillCats(std::vector<SailPrim>& prims, const float* texparams, int tn) {
  auto cat = [&](int row) {
    const int v = (tn > 0 && row >= 0 && row < tn) ? to_int(texparams[(size_t)row * 16]) : 0;
    return v < -1 ? -1 : (v > 32 ? 32 : v);
  };
  for (SailPrim& p : prims)
    p.cats = (int32_t)(((uint32_t)(uint16_t)(int16_t)cat(p.matRow)) | ((uint32_t)(uint16_t)(int16_t)cat(p.texRow) << 16));
}

void decodePrims(const float* objects, int n, int tn, uint32_t shapeMask, std::vector<SailPrim>& out, int* anyHitOk,
                 SceneBox* sbOut) {
  std::vector<PrimBox> raw((size_t)n);
  TexView o{objects, 18, n};
  const float L = 17.0f;
  out.assign((size_t)n, SailPrim{});
  *anyHitOk = 1;
  auto row = [&](float v) { return texel(gdiv(v, (float)(tn - 1)), tn); };
  for (int i = 0; i < n; i++) {
    const float rc = gdiv((float)i, (float)(n - 1));
    SailPrim& p = out[i];
    memset(&p, 0, sizeof p);
    const int cat = to_int(o.at(0.0f, rc));
    if (cat < 1 || cat > 9 || !((shapeMask >> cat) & 1u)) { p.type = 0; continue; }
    p.type = cat;
    float v3[3];
    switch (cat) {
      case SAIL_CUBE: case SAIL_RECTANGLE:
        o.readVec3(1.0f, rc, L, &p.a[0]); o.readVec3(4.0f, rc, L, &p.a[3]);
        p.rev = to_int(o.readFloat(7.0f, rc, L)) == 1;
        p.matRow = row(o.readFloat(8.0f, rc, L)); p.texRow = row(o.readFloat(9.0f, rc, L));
        o.readVec3(10.0f, rc, L, v3);
        if (cat == SAIL_RECTANGLE) rectFrameHost(p);
        break;
      case SAIL_SPHERE:
        o.readVec3(1.0f, rc, L, &p.a[0]); p.a[3] = o.readFloat(4.0f, rc, L);
        p.rev = to_int(o.readFloat(5.0f, rc, L)) == 1;
        p.matRow = row(o.readFloat(6.0f, rc, L)); p.texRow = row(o.readFloat(7.0f, rc, L));
        o.readVec3(8.0f, rc, L, v3);
        break;
      case SAIL_CONE: case SAIL_CYLINDER: case SAIL_DISK:  // p3, (h r) or (r innerR)
        o.readVec3(1.0f, rc, L, &p.a[0]); p.a[3] = o.readFloat(4.0f, rc, L); p.a[4] = o.readFloat(5.0f, rc, L);
        p.rev = to_int(o.readFloat(6.0f, rc, L)) == 1;
        p.matRow = row(o.readFloat(7.0f, rc, L)); p.texRow = row(o.readFloat(8.0f, rc, L));
        o.readVec3(9.0f, rc, L, v3);
        break;
      case SAIL_HYPERBOLOID:
        o.readVec3(1.0f, rc, L, &p.a[0]); o.readVec3(4.0f, rc, L, &p.a[3]); o.readVec3(7.0f, rc, L, &p.a[6]);
        p.a[9] = o.readFloat(10.0f, rc, L); p.a[10] = o.readFloat(11.0f, rc, L);
        p.rev = to_int(o.readFloat(12.0f, rc, L)) == 1;
        p.matRow = row(o.readFloat(13.0f, rc, L)); p.texRow = row(o.readFloat(14.0f, rc, L));
        o.readVec3(15.0f, rc, L, v3);
        break;
      case SAIL_PARABOLOID:
        o.readVec3(1.0f, rc, L, &p.a[0]);
        p.a[3] = o.readFloat(4.0f, rc, L); p.a[4] = o.readFloat(5.0f, rc, L); p.a[5] = o.readFloat(6.0f, rc, L);
        p.rev = to_int(o.readFloat(7.0f, rc, L)) == 1;
        p.matRow = row(o.readFloat(8.0f, rc, L)); p.texRow = row(o.readFloat(9.0f, rc, L));
        o.readVec3(10.0f, rc, L, v3);
        break;
      case SAIL_CORNELLBOX:
        o.readVec3(1.0f, rc, L, &p.a[0]); o.readVec3(4.0f, rc, L, &p.a[3]);
        p.rev = 0;
        p.matRow = row(o.readFloat(7.0f, rc, L));  // slot 7 = reverseNormal (cornellbox.glsl:17)
        p.texRow = 0;
        v3[0] = v3[1] = v3[2] = 0.0f;
        break;
      default: break;
    }
    p.em[0] = v3[0]; p.em[1] = v3[1]; p.em[2] = v3[2];
    quadricHost(p);
    raw[i] = primBoundsRaw(p);
    // only slabs return t > EPSILON strictly; anything else may tie or undercut EPSILON, so shadow
    // rays must then find the true closest distance (shader.light.js:24-31)
    if (cat != SAIL_CUBE && cat != SAIL_CORNELLBOX) *anyHitOk = 0;
  }
  const SceneBox sb = sceneBox(raw);
  padPrimBounds(out, raw, sb);
  if (sbOut) *sbOut = sb;
}

int ensureSamples(sail_ctx* c, int count) {
  if (count <= c->samplesCap) return SAIL_OK;
  c->samplesPos = 0;
  int cap = 4096;  // 256 KB: thousands of one-sample frames before the ring wraps
  while (cap < count) cap *= 2;
  if (int rc = growBuffer(c, &c->samples, &c->samplesCap, cap, sizeof(SailSample) * cap, "sample buffer")) return rc;
  if (c->samplesPinned) { (void)hipHostFree(c->samplesPinned); c->samplesPinned = nullptr; }
  if (hipHostMalloc(&c->samplesPinned, sizeof(SailSample) * cap) != hipSuccess) c->samplesPinned = nullptr;
  return SAIL_OK;
}

int launchTrace(sail_ctx* c, const SailSample* hs, int count, int maxBounces) {
  int tx, ty;
  const int owned = ownedTiles(c, &tx, &ty);
  if (count <= 0 || owned <= 0) return SAIL_OK;
  int rc = ensureSamples(c, count);
  if (rc) return rc;
  // The upload is ordered with its launches on the context stream. Each call takes the next slice of a ring
  // of sample records, so the host never waits for launches still reading earlier slices (one-sample frames
  // from Renderer.render() queue back to back); only a wrap of the ring waits for the stream.
  if (c->samplesPos + count > c->samplesCap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->samplesPos = 0;
  }
  SailSample* dev = c->samples + c->samplesPos;
  const SailSample* src = hs;
  if (c->samplesPinned) {  // staged in the pinned mirror: the copy is a true async DMA (pageable ones wait)
    memcpy(c->samplesPinned + c->samplesPos, hs, sizeof(SailSample) * count);
    src = c->samplesPinned + c->samplesPos;
  }
  c->samplesPos += count;
  HIPCHK(c, hipMemcpyAsync(dev, src, sizeof(SailSample) * count, hipMemcpyHostToDevice, c->stream));
  const long long px = ownedPixels(c);
  // The stage holds 12 B per owned pixel per staged sample. It is capped (kStageCapBytes): a launch that would need
  // more runs one workgroup per block (no stage).
  const long long stageStride = (long long)owned * 4096;
  const int stageSpp = (int)std::max<long long>(1, (long long)(kStageCapBytes / ((size_t)stageStride * 12)));
  const int L = launchSamples(c);
  for (int s0 = 0; s0 < count; s0 += L) {
    const int nspp = (count - s0) < L ? (count - s0) : L;
    SailTraceArgs A;
    memset(&A, 0, sizeof A);
    A.prims = c->prims; A.typeMasks = reinterpret_cast<const unsigned long long*>(c->prims + c->n);
    A.texparams = c->tp; A.lights = c->lt; A.lightObjRow = c->lightObjRow;
    A.samples = dev + s0;
    A.accum = c->accum; A.aovN = c->aovN; A.aovP = c->aovP; A.segCounter = c->segCounter;
    A.W = c->W; A.H = c->H; A.n = c->n; A.tn = c->tn; A.ln = c->ln;
    A.matMask = c->plugins.material_mask; A.texMask = c->plugins.texture_mask; A.lightMask = c->plugins.light_mask;
    A.maxBounces = maxBounces; A.spp = nspp; A.accumMode = c->accumMode;
    A.tilesX = tx; A.tilesY = ty;
    A.world = (c->partMode == SAIL_PART_SAMPLES) ? 1 : c->world;
    A.rank = (c->partMode == SAIL_PART_SAMPLES) ? 0 : c->rank;
    A.ownedTiles = owned;
    A.tileMap = c->maskSet ? c->tileMap : nullptr;
    A.shadowAnyHit = c->shadowAnyHit;
    A.cullPrims = c->n >= c->cullMinPrims ? (cullFmaOk(c) ? 2 : 1) : 0;
    A.cullPrimary = eyeNearScene(c);
    A.kernelSet = kernelSetFor(c);
    memcpy(A.eye, c->eyeCache, sizeof A.eye);
    // Sample groups: a rank's share of a small frame is too few workgroups to fill the device (1/8 of 1080p
    // = 1,016 workgroups = 4 waves per SIMD); split the launch's samples over G workgroups per block so
    // that about 4 rounds of 7-wave-per-SIMD residency are queued, and add the staged samples in order.
    const bool wavefront = c->wavefront && A.kernelSet == SAIL_KSET_GENERIC && A.cullPrims;
    refreshValues(c);  // the settle count may have crossed its threshold with the launch before
    const JitSlot* run = runningSlot(c, A.tileMap != nullptr, wavefront);
    // samples of each pixel in flight per workgroup (the run-time kernels' spec; the precompiled kernels hold one):
    // NS times the workgroups of one sample in flight, each NS times shorter
    const int ns = run ? run->spec.ns : 1;
    {  // the last bounce's row classes for the light plugins compiled into the kernel that runs (shadeLast's kLights)
      const bool kl = run ? run->spec.kl != 0u : A.kernelSet != SAIL_KSET_CORNELL;
      A.lastQuietRows = A.cullPrims ? 0u : c->lastQuietRows[kl];
      A.lastSkipSort = A.cullPrims ? 0 : c->lastSkipSort[kl];
    }
    int G = 1;
    if (c->forceGroups > 0) {
      G = c->forceGroups;
    } else if (A.kernelSet == SAIL_KSET_GENERIC && A.cullPrims) {
      // The pre-cull kernel's workgroups are 1,024 threads, two per CU at 8 waves per SIMD. Its per-workgroup cost
      // varies with the primitives a 16x64 strip sees, so a grid of few rounds ends in a long tail (1/8 of C4: 1,020
      // workgroups = 2 rounds, 0.92 of the one-GPU rate per GPU): below 6 rounds, split the samples so that about 8
      // rounds are queued (the grouped kernel is 1,024 threads too; measured 0.95 at N = 8 with 4 groups).
      // Round 3: more groups pay at any frame size (a shorter tail per launch); C4 at N = 1: G = 1 / 2 / 4 9.96 / 10.06
      // / 10.12 Gseg/s (gpurun_out/r03o), so about SAIL_CULL_GROUP_ROUNDS rounds are queued.
      const double rounds = (double)owned * 4.0 * ns / (double)(c->numCUs * 2);
      if (rounds < (double)c->cullGroupRounds) G = (int)ceil((double)c->cullGroupRounds / rounds);
    } else {
      // Round 3: splitting pays at full frame size too (shorter launch tails): C2 at N = 1 with G = 1 / 2 / 4 / 8 / 16
      // 89.3 / 89.7 / 90.9 / 91.6 / 91.4 Gseg/s, C5 87.0 / 89.3 / 90.9 / 91.6 / 91.9, C3 29.2 / 28.6 / 29.2 / 29.5 / 29.4;
      // at N = 8 (C2) G = 8 / 16 / 32 85 / 87 / 88 (gpurun_out/r03o). About 36 rounds of 7-wave residency are queued.
      const long long waves = (long long)owned * 16 * 4 * ns;
      const long long target = (long long)c->numCUs * 4 * 7 * c->flatGroupRounds;
      G = (int)((target + waves - 1) / waves);
      // the Cornell form holds 16 samples in flight only while its share queues enough workgroups (jitNsFor), and then
      // runs unsplit: staged groups lost 2-3 % per GPU at N = 4 and 8 (profiles/r05_scale_groups_c2.jsonl)
      // (under a tile mask that leaves too few active tiles for that, the kernel still holds its 16 samples, so the launch
      // is split after all: rate_by_active_tiles against rate_by_active_tiles_unsplit in profiles/adaptive_1080p.json)
      const bool fewActive = c->maskSet && (double)owned * 128.0 / ((double)c->numCUs * 4.0) < 12.0;
      if (ns >= 16 && !fewActive) G = 1;
    }
    if (G > nspp) G = nspp;
    if (G < 1) G = 1;
    if (nspp > stageSpp) G = 1;  // the stage would pass its cap
    A.groupSpp = (nspp + G - 1) / G;
    // whole steps of the workgroup's samples in flight: a group of 11 samples at 4 in flight would idle a quarter of
    // the lanes in its last step (C4 per GPU at N = 2 and 4: 12.6 Gseg/s against 13.4, profiles/r05_scale_groups_c4.jsonl)
    if (ns > 1 && A.groupSpp < nspp && c->forceGroups <= 0) A.groupSpp = ((A.groupSpp + ns - 1) / ns) * ns;
    A.sampleGroups = (nspp + A.groupSpp - 1) / A.groupSpp;
    A.groupHome = (run ? run->spec.mode == SAIL_JIT_MODE_ROOM : SAIL_GROUP_HOME_FOR(A.kernelSet)) ? 1 : 0;
    A.stageStride = stageStride;
    const bool staged = A.sampleGroups > 1;
    if (staged) {  // sized for this launch's samples (it grows to the largest launch seen)
      const size_t need = (size_t)A.stageStride * (size_t)nspp * 3 * sizeof(float);
      if ((rc = growBuffer(c, &c->stage, &c->stageBytes, need, need, "sample-group stage"))) return rc;
      A.stage = c->stage;
    }
    SailWfState WS;
    memset(&WS, 0, sizeof WS);
    if (wavefront) {
      A.sampleGroups = 1; A.groupSpp = nspp; A.stage = nullptr;
      const size_t slots = (size_t)owned * 4096;
      if ((rc = growBuffer(c, &c->wf, &c->wfSlots, slots, slots * 11 * sizeof(float4), "wavefront state"))) return rc;
      float4* b = c->wf;
      WS.o = b; WS.d = b + c->wfSlots; WS.f = b + 2 * c->wfSlots; WS.e = b + 3 * c->wfSlots; WS.s = b + 4 * c->wfSlots;
      for (int i = 0; i < 6; i++) WS.sp[i] = b + (5 + i) * c->wfSlots;
    }
    hipEvent_t e0, e1;
    if ((rc = getEvent(c, &e0)) || (rc = getEvent(c, &e1))) return rc;
    HIPCHK(c, hipEventRecord(e0, c->stream));
    if (wavefront) {
      HIPCHK(c, sail_launch_wavefront(A, WS, c->stream));
    } else {
      if (run) {
        void* args[] = {&A};
        const unsigned nt = (unsigned)sailJitThreads(run->spec);
        const unsigned px = nt / (unsigned)ns;                            // pixels per workgroup
        HIPCHK(c, hipModuleLaunchKernel(A.sampleGroups > 1 ? run->k.grouped : run->k.plain,
                                        (unsigned)owned * (4096u / px) * (unsigned)A.sampleGroups, 1, 1, nt, 1, 1, 0,
                                        c->stream, args, nullptr));
        c->lastJit = true;
        c->lastJitMode = run->spec.mode;
        c->lastBuildId = run->k.buildId;
      } else {
        HIPCHK(c, sail_launch_trace(A, owned * 16 * A.sampleGroups, c->stream));
        c->lastJit = false;
      }
      if (staged) HIPCHK(c, sail_launch_accum(A, owned * 16, c->stream));
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    c->pending.emplace_back(e0, e1);
    c->lastGroups = A.sampleGroups;
    c->lastMasked = A.tileMap != nullptr;
    c->lastWavefront = wavefront;
    c->launches++;
    c->nominalSegments += (uint64_t)px * (uint64_t)nspp * (uint64_t)maxBounces;
    c->settled += (uint64_t)nspp;
  }
  refreshValues(c);
  return SAIL_OK;
}

// Launch the queued one-sample frames of sail_render as one launch sequence (launchTrace splits it into launches of
// launchSpp samples). Their sample index and counts were taken when they were queued.
int flushQueued(sail_ctx* c) {
  if (c->queued.empty()) return SAIL_OK;
  std::vector<SailSample> q;
  q.swap(c->queued);
  HIPCHK(c, hipSetDevice(c->device));
  return launchTrace(c, q.data(), (int)q.size(), c->queuedBounces);
}

// ---- reduced frame (sail_reduce, multi-device contexts) -----------------------------------------------------------
int ensureFrame(sail_ctx* c) {
  const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
  float4** bufs[3] = {&c->frame, c->aovN ? &c->frameN : nullptr, c->aovP ? &c->frameP : nullptr};
  for (float4** b : bufs) {
    if (!b) continue;
    if (int rc = allocOnce(c, b, bytes, "reduced frame")) return rc;
  }
  return SAIL_OK;
}
// the buffers readback / filter show: the last reduced frame while it is current, else this rank's own
const float4* shownAccum(const sail_ctx* c) { return c->reduced ? c->frame : c->accum; }
const float4* shownAovN(const sail_ctx* c) { return c->reduced && c->frameN ? c->frameN : c->aovN; }
const float4* shownAovP(const sail_ctx* c) { return c->reduced && c->frameP ? c->frameP : c->aovP; }

// the a-trous passes' work buffers (sail_denoise and sail_temporal_filter share them), allocated on first use:
// cvA | cvB | g0 (16 B each) | g1 (8 B) | var (4 B) | rgba8 (4 B) per pixel, then a count per 16x16 tile
int ensureDenoiseWork(sail_ctx* c) {
  const size_t nt = (size_t)((c->W + 15) / 16) * (size_t)((c->H + 15) / 16), np = (size_t)c->W * c->H;
  return allocOnce(c, &c->denoiseWork, np * 64 + nt * 4, "denoise work buffers");
}

struct DenoiseWork {
  float4* cv[2];
  float4* g0;
  float2* g1;
  float* var;
  uint32_t* u8;
  uint32_t* bad;
};
DenoiseWork denoiseWork(const sail_ctx* c) {
  const size_t np = (size_t)c->W * c->H;
  char* base = (char*)c->denoiseWork;
  return {{(float4*)base, (float4*)(base + np * 16)}, (float4*)(base + np * 32), (float2*)(base + np * 48),
          (float*)(base + np * 56), (uint32_t*)(base + np * 60), (uint32_t*)(base + np * 64)};
}

// What sail_denoise and sail_temporal_filter share: `prepare` launches the pass that fills (cv[0], g0, g1) and the
// per-tile counts, then the a-trous passes run with steps 1, 2, 4, ..., an event round every pass (ms[0] = prepare,
// ms[1..] = the passes); the stream is synchronised and the outputs that are asked for are copied back.
// With a map `alb` (the demodulated calls) the last pass is the remodulating instance.
template <class Prepare>
hipError_t runAtrous(sail_ctx* c, const DenoiseWork& w, Prepare prepare, int iterations, float sigma_l, float sigma_x,
                     int display, float gamma_c, float* out_rgba, float* out_var, uint8_t* out_rgba8, float ms[8],
                     float* total, int* rc, const float4* alb = nullptr, float amin = 0.0f) {
  const size_t np = (size_t)c->W * c->H;
  const int nev = iterations + 2;  // before the prepare pass, then after every pass
  PooledEvents ev(c, nev);
  if ((*rc = ev.rc)) return hipSuccess;
  hipError_t e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = prepare();
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  int cur = 0;
  for (int it = 0; it < iterations && e == hipSuccess; it++) {
    const bool last = it == iterations - 1;
    SailDenoiseAtrousArgs B;
    memset(&B, 0, sizeof B);
    B.src = w.cv[cur];
    B.dst = (last && !out_rgba) ? nullptr : w.cv[cur ^ 1];
    B.g0 = w.g0; B.g1 = w.g1;
    B.outVar = (last && out_var) ? w.var : nullptr;
    B.out8 = (last && out_rgba8) ? w.u8 : nullptr;
    B.W = c->W; B.H = c->H;
    B.step = 1 << it;
    B.last = last;
    B.sl2 = sigma_l * sigma_l;
    const float sx = sigma_x * (float)B.step;
    B.sxs = sx * sx;
    B.display = display; B.gammaC = gamma_c;
    if (last && alb) {
      SailDenoiseAtrousRemodArgs R;
      memset(&R, 0, sizeof R);
      R.P = B; R.alb = alb; R.amin = amin;
      e = sail_launch_denoise_atrous_remod(R, c->stream);
    } else {
      e = sail_launch_denoise_atrous(B, c->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(ev[it + 2], c->stream);
    cur ^= 1;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  for (int i = 0; i + 1 < nev && e == hipSuccess; i++) e = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  if (e == hipSuccess) e = hipEventElapsedTime(total, ev[0], ev[nev - 1]);
  if (e == hipSuccess && out_rgba) e = hipMemcpy(out_rgba, w.cv[cur], np * 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_var) e = hipMemcpy(out_var, w.var, np * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_rgba8) e = hipMemcpy(out_rgba8, w.u8, np * 4, hipMemcpyDeviceToHost);
  return e;
}

// the three moment maps of a context that tracks them (sail_temporal_moments), zeroed on its stream
hipError_t zeroMoments(sail_ctx* c) {
  if (!c->tpMom) return hipSuccess;
  return hipMemsetAsync(c->tpMom, 0, (size_t)c->W * c->H * 48, c->stream);
}

// nothing is pending for the next sail_temporal_begin any more (sail_move_objects)
void clearMotion(sail_ctx* c) {
  c->tpMotionPending = false;
  c->tpMotion.clear();
  c->tpMotionCap = INFINITY;
}

// asynchronous RCCL errors (ncclCommGetAsyncError): a failed collective surfaces here, not at enqueue time
int commCheck(sail_ctx* c, nccl_comm_t comm) {
  if (!comm || !g_rccl.commGetAsyncError) return SAIL_OK;
  int ae = 0;
  const int r = g_rccl.commGetAsyncError(comm, &ae);
  constexpr int kNcclInProgress = 7;  // non-blocking communicators only; this library creates blocking ones
  if (r != 0 || (ae != 0 && ae != kNcclInProgress)) {
    const int code = r ? r : ae;
    return fail(c, SAIL_E_RCCL, "RCCL communicator error %d: %s", code, g_rccl.errStr ? g_rccl.errStr(code) : "?");
  }
  return SAIL_OK;
}
int groupCommCheck(sail_ctx* g) {
  for (nccl_comm_t cm : g->groupComms) if (int rc = commCheck(g, cm)) return rc;
  return SAIL_OK;
}

// The reduce plan of rank `rank` of `world` (sail_plan_reduce): the one place sail_reduce and groupReduce take their
// choices from. A sample partition shows the AOVs of the rank (device) that rendered the frame's last sample, as on one
// GPU (sample k is rendered by rank k % world; k = the context's sample count); every other rank sends -0 maps.
sail_reduce_plan planReduce(int W, int H, int rank, int world, int mode, uint64_t k, int root) {
  sail_reduce_plan p;
  memset(&p, 0, sizeof p);
  const bool tiles = mode == SAIL_PART_TILES;
  const int tx = (W + 63) / 64, ty = (H + 63) / 64, total = tx * ty;
  p.receives = rank == root;
  p.tiles = tiles ? (rank < total ? (total - rank + world - 1) / world : 0) : total;
  p.aov_owner = tiles ? -1 : (k > 0 ? (int)((k - 1) % (uint64_t)world) : 0);
  p.send_own_aovs = tiles || rank == p.aov_owner;
  if (tiles || world <= 1) p.samples = k;
  else p.samples = k > (uint64_t)rank ? (k - 1 - (uint64_t)rank) / (uint64_t)world + 1 : 0;
  return p;
}
// one step of a part-wise checkpoint load (sail_plan_load_part): SAIL_OK or SAIL_E_INVALID, state unchanged on error
int planLoadPart(uint64_t* missing, uint64_t* k, int parts, int part, uint64_t kPart) {
  if (parts < 1 || parts > 64 || part < -1 || part >= parts) return SAIL_E_INVALID;
  if (part == -1) { *missing = 0; *k = kPart; return SAIL_OK; }
  const uint64_t all = parts >= 64 ? ~0ull : (1ull << parts) - 1ull;
  uint64_t m = *missing, kk = *k;
  if (!m) { m = all; kk = kPart; }
  else if (kPart != kk) return SAIL_E_INVALID;
  *missing = m & ~(1ull << part);
  *k = kk;
  return SAIL_OK;
}
// -0 in every component: the additive identity that keeps each AOV bit (x + -0 == x for +-0 and NaN too)
hipError_t fillNegZero(float4* p, size_t np, hipStream_t s) {
  return hipMemsetD32Async((hipDeviceptr_t)p, (int)0x80000000u, np * 4, s);
}

// Multi-device context: device 0's frame = the sum of every device's cumulative accumulator (and, for tile
// partitions, of the AOV maps: -0 outside each device's tiles, so the sum is exact). Recomputed from scratch
// whenever something was rendered since the last one, so progressive frames never count a sample twice.
// Sample partitions show the AOVs of the device that rendered the last sample: in the RCCL reduce every other
// device contributes a -0 map, so the reduced maps are that device's bits (the tile reduce's rule).
int groupReduce(sail_ctx* g) {
  const int nd = (int)g->subs.size();
  sail_ctx* r = g->subs[0];
  for (sail_ctx* s : g->subs) if (int rc = flushQueued(s)) return relay(g, rc, s);
  if ((nd == 1 && g->groupComms.empty()) || !g->dirty) return SAIL_OK;
  HIPCHK(g, hipSetDevice(r->device));
  if (int rc = ensureFrame(r)) return relay(g, rc, r);
  const bool tiles = g->partMode == SAIL_PART_TILES;
  const size_t np = (size_t)g->W * g->H, bytes = np * sizeof(float4);
  // every device's share of the exchange (sail_plan_reduce: device i = rank i of nd, root 0)
  std::vector<sail_reduce_plan> plan((size_t)nd);
  for (int i = 0; i < nd; i++) plan[i] = planReduce(g->W, g->H, i, nd, g->partMode, r->k, 0);
  const int owner = tiles ? 0 : plan[0].aov_owner;
  if (g->groupLocal) {  // every "device" is the same GPU: wait for the others' streams, sum in rank order
    for (sail_ctx* s : g->subs) HIPCHK(g, hipStreamSynchronize(s->stream));
    auto sum = [&](float4* dst, float4* sail_ctx::*src) -> hipError_t {
      SailSumArgs A;
      memset(&A, 0, sizeof A);
      A.dst = dst; A.n = (long long)np; A.nsrc = nd;
      for (int i = 0; i < nd; i++) A.src[i] = g->subs[i]->*src;
      return sail_launch_sum(A, r->stream);
    };
    const sail_ctx* o = g->subs[owner];
    HIPCHK(g, sum(r->frame, &sail_ctx::accum));
    if (r->aovN) HIPCHK(g, tiles ? sum(r->frameN, &sail_ctx::aovN) : hipMemcpyAsync(r->frameN, o->aovN, bytes, hipMemcpyDeviceToDevice, r->stream));
    if (r->aovP) HIPCHK(g, tiles ? sum(r->frameP, &sail_ctx::aovP) : hipMemcpyAsync(r->frameP, o->aovP, bytes, hipMemcpyDeviceToDevice, r->stream));
    HIPCHK(g, hipStreamSynchronize(r->stream));  // the other devices' next renders may overwrite their inputs
  } else {  // one grouped RCCL reduce into device 0 over the ncclCommInitAll communicator
    const bool aov = r->aovN || r->aovP;
    if (!tiles && aov) {  // every device but the owner sends a -0 map (its frameN / frameP, device 0's in place)
      for (int i = 0; i < nd; i++) {
        sail_ctx* s = g->subs[i];
        HIPCHK(g, hipSetDevice(s->device));
        if (int rc = ensureFrame(s)) return relay(g, rc, s);
        if (!plan[i].send_own_aovs) {
          if (s->frameN) HIPCHK(g, fillNegZero(s->frameN, np, s->stream));
          if (s->frameP) HIPCHK(g, fillNegZero(s->frameP, np, s->stream));
        }
      }
    }
    int e = g_rccl.groupStart();
    for (int i = 0; i < nd && e == 0; i++) {
      sail_ctx* s = g->subs[i];
      if (hipSetDevice(s->device) != hipSuccess) { e = -1; break; }
      e = g_rccl.reduce(s->accum, i == 0 ? r->frame : s->accum, np * 4, kNcclFloat32, kNcclSum, 0, g->groupComms[i], s->stream);
      const bool own = plan[i].send_own_aovs != 0;  // the send buffer of this device's AOV maps
      if (e == 0 && s->aovN)
        e = g_rccl.reduce(own ? s->aovN : s->frameN, i == 0 ? r->frameN : (own ? s->aovN : s->frameN), np * 4,
                          kNcclFloat32, kNcclSum, 0, g->groupComms[i], s->stream);
      if (e == 0 && s->aovP)
        e = g_rccl.reduce(own ? s->aovP : s->frameP, i == 0 ? r->frameP : (own ? s->aovP : s->frameP), np * 4,
                          kNcclFloat32, kNcclSum, 0, g->groupComms[i], s->stream);
    }
    const int e2 = g_rccl.groupEnd();
    if (e || e2) return fail(g, SAIL_E_RCCL, "grouped ncclReduce: %s", g_rccl.errStr ? g_rccl.errStr(e ? e : e2) : "?");
    HIPCHK(g, hipSetDevice(r->device));
    if (int rc = groupCommCheck(g)) return rc;
  }
  r->reduced = true;
  g->dirty = false;
  return SAIL_OK;
}

// Host copy of a whole-frame accumulator keeping only what partition (rank, world, mode) holds: its own tiles, or
// (sample partition) everything on rank 0 and nothing elsewhere (sail_load_accum part -1, sail_plan_keep)
void keepPart(int W, int H, int rank, int world, int mode, const float* sums, float* out) {
  const size_t np = (size_t)W * H;
  if (world <= 1 || (mode == SAIL_PART_SAMPLES && rank == 0)) {
    if (out != sums) memmove(out, sums, np * 4 * sizeof(float));
    return;
  }
  if (mode == SAIL_PART_SAMPLES) { memset(out, 0, np * 4 * sizeof(float)); return; }
  const int tx = (W + 63) / 64;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const size_t i = ((size_t)y * W + x) * 4;
      if (((y >> 6) * tx + (x >> 6)) % world != rank) memset(out + i, 0, 4 * sizeof(float));
      else if (out != sums) memcpy(out + i, sums + i, 4 * sizeof(float));
    }
}

}  // namespace

extern "C" {

int sail_abi_version(void) { return SAIL_ABI_VERSION; }

int sail_filter_ms(sail_ctx* c, double* ms) {
  if (!c || !ms) return SAIL_E_INVALID;
  if (!c->subs.empty()) return sail_filter_ms(c->subs[0], ms);
  *ms = c->lastFilterMs;
  return SAIL_OK;
}

int sail_kernel_name(sail_ctx* c, char* name, int len) {
  if (!c || !name || len <= 0) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_kernel_name(c->subs[0], name, len), c->subs[0]);
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_kernel_name: no scene");
  const int set = kernelSetFor(c);
  const char* k = set == SAIL_KSET_CORNELL ? "sail_trace_kernel_cornell"
                  : set == SAIL_KSET_ROOM ? "sail_trace_kernel_room"
                  : (c->n >= c->cullMinPrims ? "sail_trace_kernel_cull" : "sail_trace_kernel");
  // the last launch's form: sample groups run the _grouped kernel followed by sail_accum_kernel
  if (c->lastWavefront) k = "sail_wf_*";
  else if (c->lastJit) k = c->lastJitMode == SAIL_JIT_MODE_CULL ? "sail_trace_kernel_cull_jit" : "sail_trace_kernel_jit";
  snprintf(name, (size_t)len, "%s%s%s", k, (!c->lastWavefront && c->lastMasked) ? "_masked" : "",
           (!c->lastWavefront && c->lastGroups > 1) ? "_grouped" : "");
  return SAIL_OK;
}

int sail_get_kernel_info(sail_ctx* c, sail_kernel_info* out) {
  if (!c || !out) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_get_kernel_info(c->subs[0], out), c->subs[0]);
  memset(out, 0, sizeof *out);
  if (int rc = sail_kernel_name(c, out->name, (int)sizeof out->name)) return rc;
  out->build_id = c->lastJit ? c->lastBuildId : sail_precompiled_build_id(out->name);
  // poll the background builds (a finished one loads its module); once the value kernel is loaded it is the scene's
  // run-time kernel (the next launch uses it)
  (void)c->typesSlot.poll(c->device, 0);
  const JitSlot& s = c->valueSlot.poll(c->device, 0) ? c->valueSlot : c->typesSlot;
  out->jit_state = s.state;
  out->jit_build_id = s.state == SAIL_KERNEL_JIT_READY ? s.k.buildId : 0;
  out->jit_compile_ms = s.k.compileMs;
  out->jit_from_cache = s.k.fromCache;
  snprintf(out->jit_error, sizeof out->jit_error, "%s", c->typesSlot.error.c_str());
  return SAIL_OK;
}

int sail_kernel_ready(sail_ctx* c, int timeout_ms, int* ready) {
  if (!c || !ready || timeout_ms < -1) return SAIL_E_INVALID;
  *ready = 0;
  if (!c->subs.empty()) {
    int all = 1;
    for (sail_ctx* s : c->subs) {
      int r = 0;
      if (int rc = sail_kernel_ready(s, timeout_ms, &r)) return relay(c, rc, s);
      all &= r;
    }
    *ready = all;
    return SAIL_OK;
  }
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_kernel_ready: no scene");
  // the best tier asked for so far: the value kernel once the scene has settled, else the types kernel
  JitSlot& best = (c->valueSlot.have && c->valueSlot.state != SAIL_KERNEL_JIT_FAILED) ? c->valueSlot : c->typesSlot;
  *ready = best.poll(c->device, timeout_ms) ? 1 : 0;
  return SAIL_OK;
}

int sail_set_jit_cache(const char* dir) {
  sail_jit_set_cache_dir(dir);
  return SAIL_OK;
}

int sail_device_count(int* count) {
  if (!count) return SAIL_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return SAIL_OK;
}

int sail_device_info(int device, int* compute_units, int* clock_khz) {
  if (!compute_units || !clock_khz) return SAIL_E_INVALID;
  int cus = 0, khz = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device) != hipSuccess)
    return SAIL_E_HIP;
  *compute_units = cus;
  *clock_khz = khz;
  return SAIL_OK;
}

const char* sail_last_error(const sail_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sail_create(sail_ctx** out, int width, int height, int device, uint32_t flags) {
  if (!out || width <= 0 || height <= 0 || width > 32768 || height > 32768)
    return fail(nullptr, SAIL_E_INVALID, "sail_create: bad arguments %dx%d", width, height);
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SAIL_E_NODEVICE, "no HIP device");
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
  if (device >= ndev) return fail(nullptr, SAIL_E_INVALID, "device %d out of range (%d devices)", device, ndev);
  sail_ctx* c = new sail_ctx();
  c->device = device; c->W = width; c->H = height; c->flags = flags;
  auto bail = [&](int code, const char* what) {
    g_create_error = std::string("sail_create: ") + what;
    sail_destroy(c);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(SAIL_E_HIP, "hipSetDevice");
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->numCUs = cus;
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(SAIL_E_HIP, "stream");
  const size_t bytes = (size_t)width * height * sizeof(float4);
  if (hipMalloc(&c->accum, bytes) != hipSuccess) return bail(SAIL_E_OOM, "accumulator");
  if (flags & SAIL_FLAG_AOV) {
    if (hipMalloc(&c->aovN, bytes) != hipSuccess || hipMalloc(&c->aovP, bytes) != hipSuccess) return bail(SAIL_E_OOM, "aov");
  }
  if (flags & SAIL_FLAG_SEGMENT_COUNT) {
    if (hipMalloc(&c->segCounter, SAIL_SEG_SLOTS * sizeof(unsigned long long)) != hipSuccess) return bail(SAIL_E_OOM, "counter");
  }
  if (resetAccum(c) != SAIL_OK) return bail(SAIL_E_HIP, c->err.c_str());
  if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(SAIL_E_HIP, "sync");
  *out = c;
  return SAIL_OK;
}

void sail_destroy(sail_ctx* c) {
  if (!c) return;
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (s) { (void)hipSetDevice(s->device); (void)hipStreamSynchronize(s->stream); }
    for (nccl_comm_t cm : c->groupComms) if (cm && g_rccl.commDestroy) g_rccl.commDestroy(cm);
    for (sail_ctx* s : c->subs) sail_destroy(s);
    delete c;
    return;
  }
  if (c->device >= 0) (void)hipSetDevice(c->device);
  dropValues(c);
  c->typesTwin.drop(c->device, c->stream);
  c->typesSlot.drop(c->device, c->stream);  // its queued build, if any, is no longer needed
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && g_rccl.commDestroy) g_rccl.commDestroy(c->comm);
  for (auto& pr : c->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (auto e : c->evPool) (void)hipEventDestroy(e);
  void* bufs[] = {c->accum, c->frame, c->frameN, c->frameP, c->aovN, c->aovP, c->filterOut, c->filterOut8, c->stage, c->segCounter, c->prims, c->tp, c->lt, c->lightObjRow, c->samples, c->wf,
                  c->noiseMark, c->noiseOut, c->noisePix, c->denoiseWork, c->tpWork, c->tpMom, c->tpMotionDev, c->albMap,
                  c->tileMap, c->maskBytes};
  for (void* b : bufs) if (b) (void)hipFree(b);
  if (c->samplesPinned) (void)hipHostFree(c->samplesPinned);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int sail_create_multi(sail_ctx** out, int width, int height, const int* devices, int n_devices, uint32_t flags) {
  if (!out || n_devices < 1 || n_devices > 64)
    return fail(nullptr, SAIL_E_INVALID, "sail_create_multi: bad arguments (%d devices)", n_devices);
  *out = nullptr;
  std::vector<int> dev((size_t)n_devices);
  for (int i = 0; i < n_devices; i++) dev[i] = devices ? devices[i] : i;
  for (int i = 0; i < n_devices; i++)  // a negative ordinal is the current device (sail_create's rule), resolved first
    if (dev[i] < 0 && hipGetDevice(&dev[i]) != hipSuccess) return fail(nullptr, SAIL_E_HIP, "sail_create_multi: hipGetDevice");
  bool allSame = true, allDistinct = true;
  for (int i = 0; i < n_devices; i++)
    for (int j = 0; j < n_devices; j++) {
      if (dev[i] != dev[j]) allSame = false;
      if (i != j && dev[i] == dev[j]) allDistinct = false;
    }
  if (!allSame && !allDistinct)
    return fail(nullptr, SAIL_E_INVALID, "sail_create_multi: devices must be all distinct or all the same one");
  sail_ctx* g = new sail_ctx();
  g->W = width; g->H = height; g->flags = flags; g->device = dev[0];
  g->world = n_devices;
  g->groupLocal = n_devices > 1 && allSame;
  for (int i = 0; i < n_devices; i++) {
    sail_ctx* s = nullptr;
    int rc = sail_create(&s, width, height, dev[i], flags);
    if (rc == SAIL_OK) g->subs.push_back(s);
    if (rc == SAIL_OK) rc = sail_set_partition(s, i, n_devices, SAIL_PART_TILES);
    if (rc != SAIL_OK) {
      const std::string msg = s ? s->err : g_create_error;
      sail_destroy(g);
      return fail(nullptr, rc, "sail_create_multi: device %d: %s", dev[i], msg.c_str());
    }
  }
  if (n_devices > 1 && allDistinct) {
    if (!g_rccl.load()) { sail_destroy(g); return fail(nullptr, SAIL_E_RCCL, "sail_create_multi: librccl not loadable"); }
    g->groupComms.assign((size_t)n_devices, nullptr);
    const int r = g_rccl.commInitAll(g->groupComms.data(), n_devices, dev.data());
    if (r) {
      g->groupComms.clear();
      sail_destroy(g);
      return fail(nullptr, SAIL_E_RCCL, "ncclCommInitAll: %s", g_rccl.errStr ? g_rccl.errStr(r) : "?");
    }
  }
  *out = g;
  return SAIL_OK;
}

int sail_set_debug(sail_ctx* c, int option, int value) {
  if (!c) return SAIL_E_INVALID;
  if (option == SAIL_DEBUG_FORCE_RCCL) {  // the multi-device context's own communicator, not its devices'
    if (c->subs.empty() || c->groupLocal)
      return fail(c, SAIL_E_INVALID, "SAIL_DEBUG_FORCE_RCCL needs a multi-device context of distinct devices");
    for (sail_ctx* s : c->subs) if (int rc = flushQueued(s)) return relay(c, rc, s);
    const int nd = (int)c->subs.size();
    if (value && c->groupComms.empty()) {
      if (!g_rccl.load()) return fail(c, SAIL_E_RCCL, "librccl not loadable");
      std::vector<int> dev((size_t)nd);
      for (int i = 0; i < nd; i++) dev[i] = c->subs[i]->device;
      c->groupComms.assign((size_t)nd, nullptr);
      const int r = g_rccl.commInitAll(c->groupComms.data(), nd, dev.data());
      if (r) {
        c->groupComms.clear();
        return fail(c, SAIL_E_RCCL, "ncclCommInitAll: %s", g_rccl.errStr ? g_rccl.errStr(r) : "?");
      }
    } else if (!value && nd == 1 && !c->groupComms.empty()) {
      for (sail_ctx* s : c->subs) { (void)hipSetDevice(s->device); (void)hipStreamSynchronize(s->stream); }
      for (nccl_comm_t cm : c->groupComms) if (cm) g_rccl.commDestroy(cm);
      c->groupComms.clear();
    }
    c->dirty = true;
    return SAIL_OK;
  }
  for (sail_ctx* s : c->subs) if (int rc = sail_set_debug(s, option, value)) return relay(c, rc, s);
  if (int rc = flushQueued(c)) return rc;  // queued samples launch with the settings they were queued under
  switch (option) {
    case SAIL_DEBUG_CULL_MIN_PRIMS: c->cullMinPrims = value; break;
    case SAIL_DEBUG_FORCE_GENERIC: c->forceGeneric = value; break;
    case SAIL_DEBUG_CULL_FMA: c->cullFma = value; break;
    case SAIL_DEBUG_SAMPLE_GROUPS: c->forceGroups = value; break;
    case SAIL_DEBUG_WAVEFRONT: c->wavefront = value; break;
    case SAIL_DEBUG_JIT:
      // the value kernel's other form, derived anew below (refreshValues); the rows did not move: the count stays
      if ((c->jit ^ value) & 32) { const uint64_t s = c->settled; dropValues(c); c->settled = s; }
      c->jit = value;
      break;
    case SAIL_DEBUG_JIT_NT:
      if (value != 0 && value != 128 && value != 256 && value != 512 && value != 1024)
        return fail(c, SAIL_E_INVALID, "sail_set_debug: threads per workgroup must be 0 (default), 128, 256, 512 or 1024");
      c->jitNt = value;
      break;
    case SAIL_DEBUG_JIT_NS:
      if (value != 0 && value != 1 && value != 4 && value != 16)
        return fail(c, SAIL_E_INVALID, "sail_set_debug: samples in flight must be 0 (default), 1, 4 or 16");
      c->jitNs = value;
      break;
    case SAIL_DEBUG_JIT_WAIT:
      if (value < -1) return fail(c, SAIL_E_INVALID, "sail_set_debug: jit wait must be >= -1");
      c->jitWait = value;
      break;
    case SAIL_DEBUG_JIT_VALUES_AFTER:
      c->jitValuesAfter = value;
      if (value < 0) { const uint64_t s = c->settled; dropValues(c); c->settled = s; }  // never: back to the types kernel
      break;
    case SAIL_DEBUG_GROUP_ROUNDS:
      if (value <= 0) return fail(c, SAIL_E_INVALID, "sail_set_debug: group rounds must be > 0");
      c->flatGroupRounds = value;
      break;
    case SAIL_DEBUG_CULL_GROUP_ROUNDS:
      if (value <= 0) return fail(c, SAIL_E_INVALID, "sail_set_debug: group rounds must be > 0");
      c->cullGroupRounds = value;
      break;
    default: return fail(c, SAIL_E_INVALID, "sail_set_debug: unknown option %d", option);
  }
  refreshJit(c);  // the switches decide which run-time kernel (if any) the scene gets
  refreshValues(c);
  return SAIL_OK;
}

// The primitive buffer holds the decoded rows followed by the candidate sweep's per-type masks: for each chunk
// of 64 rows, 16 words whose bit j says row 64*chunk + j has shape type t (SailTraceArgs.typeMasks).
static size_t primBytes(int n) {
  const size_t chunks = (size_t)(n + 63) / 64;
  return sizeof(SailPrim) * (size_t)(n > 0 ? n : 1) + chunks * 16 * sizeof(unsigned long long);
}
static int uploadPrims(sail_ctx* c, const std::vector<SailPrim>& prims) {
  const int n = (int)prims.size();
  if (n <= 0) return SAIL_OK;
  const size_t chunks = (size_t)(n + 63) / 64;
  c->typeMasksHost.assign(chunks * 16, 0ull);
  for (int i = 0; i < n; i++)
    if (prims[i].type >= 0 && prims[i].type < 16) c->typeMasksHost[(size_t)(i / 64) * 16 + prims[i].type] |= 1ull << (i % 64);
  HIPCHK(c, hipMemcpyAsync(c->prims, prims.data(), sizeof(SailPrim) * n, hipMemcpyHostToDevice, c->stream));
  c->rowWords.resize((size_t)n * 32);  // what a value kernel compiles in (refreshValues)
  memcpy(c->rowWords.data(), prims.data(), sizeof(SailPrim) * (size_t)n);
  HIPCHK(c, hipMemcpyAsync(c->prims + n, c->typeMasksHost.data(), chunks * 16 * sizeof(unsigned long long),
                           hipMemcpyHostToDevice, c->stream));
  return SAIL_OK;
}

// Decode the rows for the context's plugin set (c->plugins) and derive what follows them: the category words, the
// last-bounce classes for a kernel without and with a light plugin, and the scene's extent
static void decodeRows(sail_ctx* c, const float* objects, int n, const float* texparams, int tn, std::vector<SailPrim>& prims) {
  decodePrims(objects, n, tn, c->plugins.shape_mask, prims, &c->shadowAnyHit, &c->scene);
  fillCats(prims, texparams, tn);
  for (int l = 0; l < 2; l++)
    lastBounceRows(prims, texparams, tn, c->plugins.material_mask, l != 0, &c->lastQuietRows[l], &c->lastSkipSort[l]);
  c->primExtent = primExtent(prims);
}

int sail_set_scene(sail_ctx* c, const float* objects, int n, const float* texparams, int tn, const float* lights,
                   int ln, const sail_plugins* plugins) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs)
      if (int rc = sail_set_scene(s, objects, n, texparams, tn, lights, ln, plugins)) return relay(c, rc, s);
    c->haveScene = true; c->n = n; c->tn = tn; c->ln = ln; c->dirty = false;
    c->loadMissing = 0;  // every device's accumulation restarted: a half-loaded checkpoint is abandoned
    return SAIL_OK;
  }
  if (n < 0 || tn < 0 || ln < 0 || (n > 0 && !objects) || (tn > 0 && !texparams) || (ln > 0 && !lights) || !plugins)
    return fail(c, SAIL_E_INVALID, "sail_set_scene: bad arguments (n=%d tn=%d ln=%d)", n, tn, ln);
  if (n > 0 && tn < 1) return fail(c, SAIL_E_INVALID, "sail_set_scene: objects need texParams rows");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->plugins = *plugins;
  c->lastGroups = 1;
  c->lastWavefront = false;
  c->lastJit = false;
  std::vector<SailPrim> prims;
  decodeRows(c, objects, n, texparams, tn, prims);
  c->primTypes.clear();
  for (const SailPrim& q : prims) c->primTypes.push_back(q.type);
  // per light row: the geometry row an AreaLight samples (area.glsl:8 + shader.shape.js:56)
  std::vector<int32_t> lrow((size_t)(ln > 0 ? ln : 1), 0);
  TexView lv{lights, 18, ln};
  for (int r = 0; r < ln; r++) {
    const float rc = (ln == 1) ? NAN : gdiv((float)r, (float)(ln - 1));
    const int gi = to_int(lv.readFloat(1.0f, rc, 17.0f));
    lrow[r] = (n > 0) ? texel(gdiv((float)gi, (float)(n - 1)), n) : 0;
  }
  void* old[] = {c->prims, c->tp, c->lt, c->lightObjRow};
  for (void* b : old) if (b) HIPCHK(c, hipFree(b));
  c->prims = nullptr; c->tp = nullptr; c->lt = nullptr; c->lightObjRow = nullptr;
  const size_t pb = primBytes(n), tb = sizeof(float) * 16 * (size_t)(tn > 0 ? tn : 1),
               lb = sizeof(float) * 18 * (size_t)(ln > 0 ? ln : 1), rb = sizeof(int32_t) * lrow.size();
  if (hipMalloc(&c->prims, pb) != hipSuccess || hipMalloc(&c->tp, tb) != hipSuccess || hipMalloc(&c->lt, lb) != hipSuccess ||
      hipMalloc(&c->lightObjRow, rb) != hipSuccess)
    return fail(c, SAIL_E_OOM, "scene buffers");
  HIPCHK(c, hipMemsetAsync(c->tp, 0, tb, c->stream));
  HIPCHK(c, hipMemsetAsync(c->lt, 0, lb, c->stream));
  if (int rc = uploadPrims(c, prims)) return rc;
  if (tn > 0) HIPCHK(c, hipMemcpyAsync(c->tp, texparams, sizeof(float) * 16 * tn, hipMemcpyHostToDevice, c->stream));
  if (ln > 0) HIPCHK(c, hipMemcpyAsync(c->lt, lights, sizeof(float) * 18 * ln, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->lightObjRow, lrow.data(), rb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->objectsRows.assign(objects, objects + (size_t)n * 18);
  c->tpRows.assign(texparams, texparams + (size_t)tn * 16);
  c->n = n; c->tn = tn; c->ln = ln;
  c->haveScene = true;
  c->tpHaveCur = c->tpHavePrev = c->tpResolved = false;  // the temporal maps' ids and positions are stale
  c->albHave = false;                                    // and so are the albedo map's colours
  clearMotion(c);
  HIPCHK(c, zeroMoments(c));
  // Tracer.update links the scene's program (tracer.js:42-90): the plugin set's kernel starts building now, in the
  // background; the precompiled kernel of the set serves until it is loaded
  dropValues(c);
  refreshJit(c);
  refreshValues(c);
  return resetAccum(c);
}

// New rows for a single-device context whose arguments have been checked: sail_update_objects (the temporal state goes,
// its ids and positions are stale) and sail_move_objects (it stays: the caller records how the rows moved)
static int updateRows(sail_ctx* c, const float* objects, int n, bool keepTemporal) {
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<SailPrim> prims;
  decodeRows(c, objects, n, c->tpRows.data(), c->tn, prims);
  c->primTypes.clear();
  for (const SailPrim& q : prims) c->primTypes.push_back(q.type);  // a kernel compiled for the rows follows them
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = uploadPrims(c, prims)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->objectsRows.assign(objects, objects + (size_t)n * 18);
  c->albHave = false;  // the albedo map shows the rows as they were, whoever moved them
  if (!keepTemporal) {
    c->tpHaveCur = c->tpHavePrev = c->tpResolved = false;  // the temporal maps' ids and positions are stale
    clearMotion(c);
    HIPCHK(c, zeroMoments(c));
  }
  dropValues(c);  // the rows' values moved: the value kernel goes, the settle count restarts
  refreshJit(c);  // a drag keeps the types kernel; a changed shape type starts the new rows' kernel building
  refreshValues(c);
  return resetAccum(c);
}

int sail_update_objects(sail_ctx* c, const float* objects, int n) {
  if (c && !c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_update_objects(s, objects, n)) return relay(c, rc, s);
    c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (!c || !c->haveScene) return c ? fail(c, SAIL_E_STATE, "sail_update_objects before sail_set_scene") : SAIL_E_INVALID;
  if (n != c->n || !objects) return fail(c, SAIL_E_INVALID, "sail_update_objects: n must stay %d", c->n);
  return updateRows(c, objects, n, false);
}

int sail_move_objects(sail_ctx* c, const float* objects, int n, const float* motion, float hist_cap) {
  if (!c) return SAIL_E_INVALID;
  // everything is checked before anything changes: a refused call leaves rows, accumulator and temporal state alone
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_move_objects before sail_set_scene");
  if (n != c->n || !objects) return fail(c, SAIL_E_INVALID, "sail_move_objects: n must stay %d", c->n);
  for (size_t i = 0; motion && i < (size_t)n * 3; i++)
    if (!std::isfinite(motion[i]))
      return fail(c, SAIL_E_INVALID, "sail_move_objects: the motion of row %d is not finite", (int)(i / 3));
  if (!(hist_cap == 0.0f || (std::isfinite(hist_cap) && hist_cap >= 1.0f)))
    return fail(c, SAIL_E_INVALID, "sail_move_objects: hist_cap %g must be 0 (none) or finite and >= 1", (double)hist_cap);
  if (!c->subs.empty()) {  // the temporal maps, and with them what is pending, live on device 0
    for (size_t i = 0; i < c->subs.size(); i++) {
      sail_ctx* s = c->subs[i];
      if (int rc = i == 0 ? sail_move_objects(s, objects, n, motion, hist_cap) : sail_update_objects(s, objects, n))
        return relay(c, rc, s);
    }
    c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  const bool temporal = c->tpHaveCur || c->tpHavePrev;
  if (int rc = updateRows(c, objects, n, temporal)) return rc;
  if (!temporal) return SAIL_OK;  // no temporal state: exactly sail_update_objects, nothing is pending
  if (!c->tpMotionPending) {
    c->tpMotion.assign((size_t)n * 4, 0.0f);
    c->tpMotionCap = INFINITY;
    c->tpMotionPending = true;
  }
  for (int r = 0; motion && r < n; r++)
    for (int j = 0; j < 3; j++) c->tpMotion[(size_t)r * 4 + j] = c->tpMotion[(size_t)r * 4 + j] + motion[r * 3 + j];
  if (hist_cap != 0.0f) c->tpMotionCap = hist_cap < c->tpMotionCap ? hist_cap : c->tpMotionCap;
  return SAIL_OK;
}

int sail_temporal_pending_motion(sail_ctx* c, float* motion, float* hist_cap, int* pending) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_temporal_pending_motion(c->subs[0], motion, hist_cap, pending), c->subs[0]);
  for (int r = 0; motion && r < c->n; r++)
    for (int j = 0; j < 3; j++) motion[r * 3 + j] = c->tpMotionPending ? c->tpMotion[(size_t)r * 4 + j] : 0.0f;
  if (hist_cap) *hist_cap = c->tpMotionPending ? c->tpMotionCap : INFINITY;
  if (pending) *pending = c->tpMotionPending ? 1 : 0;
  return SAIL_OK;
}

int sail_set_accum_mode(sail_ctx* c, int mode) {
  if (!c) return SAIL_E_INVALID;
  if (mode < SAIL_ACCUM_SUM || mode > SAIL_ACCUM_COMPAT8) return fail(c, SAIL_E_INVALID, "accum mode %d", mode);
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_set_accum_mode(s, mode)) return relay(c, rc, s);
    c->accumMode = mode; c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (mode != SAIL_ACCUM_SUM && c->partMode == SAIL_PART_SAMPLES && c->world > 1)
    return fail(c, SAIL_E_INVALID, "running-mean accumulation cannot be split by samples");
  HIPCHK(c, hipSetDevice(c->device));
  c->accumMode = mode;
  return resetAccum(c);
}

int sail_set_partition(sail_ctx* c, int rank, int world, int mode) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {  // the devices of one context split the frame among themselves: only the mode is chosen
    if (rank != 0 || world != 1 || (mode != SAIL_PART_TILES && mode != SAIL_PART_SAMPLES))
      return fail(c, SAIL_E_INVALID, "multi-device context: partition must be (0, 1, mode), got (%d, %d, %d)", rank, world, mode);
    const int nd = (int)c->subs.size();
    for (int i = 0; i < nd; i++) if (int rc = sail_set_partition(c->subs[i], i, nd, mode)) return relay(c, rc, c->subs[i]);
    c->partMode = mode; c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (world < 1 || rank < 0 || rank >= world || (mode != SAIL_PART_TILES && mode != SAIL_PART_SAMPLES))
    return fail(c, SAIL_E_INVALID, "partition rank=%d world=%d mode=%d", rank, world, mode);
  if (mode == SAIL_PART_SAMPLES && world > 1 && c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_INVALID, "sample partition needs SAIL_ACCUM_SUM");
  HIPCHK(c, hipSetDevice(c->device));
  c->rank = rank; c->world = world; c->partMode = mode;
  refreshJit(c);  // the Cornell form's samples in flight follow the share of the frame (jitNsFor)
  refreshValues(c);
  return resetAccum(c);
}

int sail_set_launch_samples(sail_ctx* c, int spp) {
  if (!c) return SAIL_E_INVALID;
  if (spp < 0 || spp > 1 << 20) return fail(c, SAIL_E_INVALID, "launch samples %d", spp);  // 0: by form
  for (sail_ctx* s : c->subs) if (int rc = sail_set_launch_samples(s, spp)) return relay(c, rc, s);
  if (int rc = flushQueued(c)) return rc;
  c->launchSpp = spp;
  return SAIL_OK;
}

int sail_render_schedule(sail_ctx* c, const float* inv, const float* seeds, const float eye[3], int spp, int maxBounces) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    // every device queues its share on its own stream; the host does not wait
    if (int rc = loadIncomplete(c, "sail_render_schedule")) return rc;
    for (sail_ctx* s : c->subs)
      if (int rc = sail_render_schedule(s, inv, seeds, eye, spp, maxBounces)) return relay(c, rc, s);
    c->dirty = true;
    return SAIL_OK;
  }
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_render before sail_set_scene");
  if (spp < 0 || (spp > 0 && (!inv || !seeds)) || !eye || maxBounces < 0 || maxBounces > 1024)
    return fail(c, SAIL_E_INVALID, "sail_render_schedule: bad arguments (spp=%d bounces=%d)", spp, maxBounces);
  if (int rc = flushQueued(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  memcpy(c->eyeCache, eye, sizeof(float) * 3);
  c->hostSamples.clear();
  for (int s = 0; s < spp; s++) {
    const uint64_t k = c->k + (uint64_t)s;
    if (c->partMode == SAIL_PART_SAMPLES && c->world > 1 && (int)(k % (uint64_t)c->world) != c->rank) continue;
    SailSample S;
    memset(&S, 0, sizeof S);
    cornerDirs(inv + 16 * s, eye, S.d);
    S.seed = seeds[s];
    S.mixw = (float)((double)k / (double)(k + 1));  // tracer.js:97, f64 then uniform1f
    c->hostSamples.push_back(S);
  }
  const int rc = launchTrace(c, c->hostSamples.data(), (int)c->hostSamples.size(), maxBounces);
  if (rc) return rc;
  c->reduced = false;  // the frame of the last sail_reduce is stale now: reduce again to refresh it
  c->samplesThisRank += c->hostSamples.size();
  c->k += (uint64_t)spp;
  return SAIL_OK;
}

// One progressive sample (Renderer.render): queued, and launched with the samples queued after it once launchSpp of
// them are waiting or anything observes or changes the context (flushQueued). The sample's record is built now,
// from the sample index it is given now, exactly as sail_render_schedule builds it.
int sail_render(sail_ctx* c, const float inv[16], const float eye[3], float seed, int maxBounces) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_render")) return rc;
    for (sail_ctx* s : c->subs) if (int rc = sail_render(s, inv, eye, seed, maxBounces)) return relay(c, rc, s);
    c->dirty = true;
    return SAIL_OK;
  }
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_render before sail_set_scene");
  if (!inv || !eye || maxBounces < 0 || maxBounces > 1024)
    return fail(c, SAIL_E_INVALID, "sail_render: bad arguments (bounces=%d)", maxBounces);
  // a launch has one eye (its pre-cull decisions) and one bounce count
  if (!c->queued.empty() && (maxBounces != c->queuedBounces || memcmp(eye, c->eyeCache, sizeof(float) * 3) != 0))
    if (int rc = flushQueued(c)) return rc;
  memcpy(c->eyeCache, eye, sizeof(float) * 3);
  c->queuedBounces = maxBounces;
  const uint64_t k = c->k;
  if (!(c->partMode == SAIL_PART_SAMPLES && c->world > 1 && (int)(k % (uint64_t)c->world) != c->rank)) {
    SailSample S;
    memset(&S, 0, sizeof S);
    cornerDirs(inv, eye, S.d);
    S.seed = seed;
    S.mixw = (float)((double)k / (double)(k + 1));  // tracer.js:97, f64 then uniform1f
    c->queued.push_back(S);
    c->samplesThisRank++;
  }
  c->k++;
  c->reduced = false;
  // one-sample frames launch 64 at a time unless the host fixed the launch size: the host keeps queueing the next
  // frames while a launch runs (a whole 1,024-frame queue launched at once left the GPU idle meanwhile: the JS host's
  // render() per frame at 85,391 against 91,161 Msamples/s, profiles/r05_bench_js_host*.json)
  if ((int)c->queued.size() >= (c->launchSpp > 0 ? c->launchSpp : 64)) return flushQueued(c);
  return SAIL_OK;
}

int sail_reset(sail_ctx* c) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_reset(s)) return relay(c, rc, s);
    c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return resetAccum(c);
}

int sail_sync(sail_ctx* c) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_sync(s)) return relay(c, rc, s);
    return groupCommCheck(c);
  }
  if (int rc = flushQueued(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = commCheck(c, c->comm)) return rc;
  return collectEvents(c);
}

int sail_read_accum(sail_ctx* c, float* rgba) {
  if (!c || !rgba) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_read_accum")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_read_accum(c->subs[0], rgba), c->subs[0]);
  }
  int rc = sail_sync(c);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(rgba, shownAccum(c), (size_t)c->W * c->H * sizeof(float4), hipMemcpyDeviceToHost));
  return SAIL_OK;
}

int sail_readback(sail_ctx* c, float* rgba, float* normal, float* position) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_readback")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_readback(c->subs[0], rgba, normal, position), c->subs[0]);
  }
  int rc = sail_sync(c);
  if (rc) return rc;
  const size_t np = (size_t)c->W * c->H, bytes = np * sizeof(float4);
  if (rgba) {
    HIPCHK(c, hipMemcpy(rgba, shownAccum(c), bytes, hipMemcpyDeviceToHost));
    if (c->accumMode == SAIL_ACCUM_SUM) {
      for (size_t i = 0; i < np; i++) {
        const float cnt = rgba[4 * i + 3];
        if (cnt > 0.0f) { rgba[4 * i] /= cnt; rgba[4 * i + 1] /= cnt; rgba[4 * i + 2] /= cnt; }
        rgba[4 * i + 3] = 1.0f;
      }
    }
  }
  if (normal) {
    if (!c->aovN) return fail(c, SAIL_E_STATE, "AOVs not enabled (SAIL_FLAG_AOV)");
    HIPCHK(c, hipMemcpy(normal, shownAovN(c), bytes, hipMemcpyDeviceToHost));
  }
  if (position) {
    if (!c->aovP) return fail(c, SAIL_E_STATE, "AOVs not enabled (SAIL_FLAG_AOV)");
    HIPCHK(c, hipMemcpy(position, shownAovP(c), bytes, hipMemcpyDeviceToHost));
  }
  return SAIL_OK;
}

int sail_filter(sail_ctx* c, int kind, const float* weights16, float rx, float ry, float gammaC, float* out, uint8_t* out8) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    // the display pass runs on device 0 over the reduced frame
    if (int rc = loadIncomplete(c, "sail_filter")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_filter(c->subs[0], kind, weights16, rx, ry, gammaC, out, out8), c->subs[0]);
  }
  if (kind < SAIL_FILTER_COLOR || kind > SAIL_FILTER_POSITION || (kind == SAIL_FILTER_WINDOW && !weights16))
    return fail(c, SAIL_E_INVALID, "sail_filter: kind %d", kind);
  if (kind >= SAIL_FILTER_WAVELET && !c->aovN)
    return fail(c, SAIL_E_STATE, "sail_filter: kind %d reads the AOVs (create with SAIL_FLAG_AOV)", kind);
  HIPCHK(c, hipSetDevice(c->device));
  int rc = sail_sync(c);
  if (rc) return rc;
  const size_t np = (size_t)c->W * c->H;
  if (out && (rc = allocOnce(c, &c->filterOut, np * sizeof(float4), "filter output"))) return rc;
  if (out8 && (rc = allocOnce(c, &c->filterOut8, np * 4, "filter output"))) return rc;
  float4* dOut = out ? c->filterOut : nullptr;
  uint8_t* dOut8 = out8 ? c->filterOut8 : nullptr;
  SailFilterArgs A;
  memset(&A, 0, sizeof A);
  A.accum = shownAccum(c); A.aovN = shownAovN(c); A.aovP = shownAovP(c);
  A.out = dOut; A.out8 = dOut8; A.W = c->W; A.H = c->H; A.kind = kind; A.accumMode = c->accumMode;
  if (weights16) memcpy(A.weights, weights16, sizeof A.weights);
  A.rx = rx; A.ry = ry; A.gammaC = gammaC;
  // window taps reach 0.875 r pixels (offsets (j + 0.5) r / 4, j < 4) + the bilinear footprint + rounding
  if (kind == SAIL_FILTER_WINDOW) {
    const float r = fmaxf(fabsf(rx), fabsf(ry));
    const int h = (r == r) ? (int)ceilf(0.875f * r) + 2 : 99;
    A.halo = h <= 8 ? h : 0;
  }
  hipEvent_t f0 = nullptr, f1 = nullptr;
  int rcE = getEvent(c, &f0);
  if (rcE == SAIL_OK) rcE = getEvent(c, &f1);
  if (rcE != SAIL_OK) return rcE;
  hipError_t e = hipEventRecord(f0, c->stream);
  if (e == hipSuccess) e = sail_launch_filter(A, c->stream);
  if (e == hipSuccess) e = hipEventRecord(f1, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) {
    float ms = 0.0f;
    e = hipEventElapsedTime(&ms, f0, f1);
    c->lastFilterMs = ms;
  }
  c->evPool.push_back(f0);
  c->evPool.push_back(f1);
  if (e == hipSuccess && out) e = hipMemcpy(out, dOut, np * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess && out8) e = hipMemcpy(out8, dOut8, np * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_filter: %s", hipGetErrorString(e));
  return SAIL_OK;
}

int sail_pick(sail_ctx* c, const float* rays, int count, int32_t* index, float* t) {
  if (!c || count < 0 || (count > 0 && (!rays || !index || !t))) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_pick(c->subs[0], rays, count, index, t), c->subs[0]);
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_pick: no scene (call sail_set_scene first)");
  if (count == 0) return SAIL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = sail_sync(c);
  if (rc) return rc;
  float* dRays = nullptr;
  void* dOut = nullptr;
  if (hipMalloc(&dRays, (size_t)count * 6 * sizeof(float)) != hipSuccess) return fail(c, SAIL_E_OOM, "pick rays");
  if (hipMalloc(&dOut, (size_t)count * 8) != hipSuccess) { (void)hipFree(dRays); return fail(c, SAIL_E_OOM, "pick out"); }
  int32_t* dIdx = (int32_t*)dOut;
  float* dT = (float*)((char*)dOut + (size_t)count * 4);
  hipError_t e = hipMemcpyAsync(dRays, rays, (size_t)count * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = sail_launch_pick(c->prims, c->n, dRays, count, dIdx, dT, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(index, dIdx, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t, dT, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(dRays);
  (void)hipFree(dOut);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_pick: %s", hipGetErrorString(e));
  return SAIL_OK;
}

int sail_get_stats(sail_ctx* c, sail_stats* s) {
  if (!c || !s) return SAIL_E_INVALID;
  if (!c->subs.empty()) {  // samples per pixel of the frame; work summed; time = the slowest device's
    memset(s, 0, sizeof *s);
    for (sail_ctx* d : c->subs) {
      sail_stats q;
      if (int rc = sail_get_stats(d, &q)) return relay(c, rc, d);
      s->samples = c->partMode == SAIL_PART_SAMPLES ? s->samples + q.samples : q.samples;
      s->segments += q.segments;
      s->nominal_segments += q.nominal_segments;
      s->kernel_ms = fmax(s->kernel_ms, q.kernel_ms);
      s->last_launch_ms = fmax(s->last_launch_ms, q.last_launch_ms);
      s->launches = q.launches > s->launches ? q.launches : s->launches;
    }
    return SAIL_OK;
  }
  int rc = sail_sync(c);
  if (rc) return rc;
  memset(s, 0, sizeof *s);
  s->samples = c->samplesThisRank;
  s->nominal_segments = c->nominalSegments;
  s->kernel_ms = c->kernelMs;
  s->last_launch_ms = c->lastLaunchMs;
  s->launches = c->launches;
  if (c->segCounter) {
    unsigned long long v[SAIL_SEG_SLOTS];
    HIPCHK(c, hipMemcpy(v, c->segCounter, sizeof v, hipMemcpyDeviceToHost));
    s->segments = 0;
    for (int i = 0; i < SAIL_SEG_SLOTS; i++) s->segments += v[i];
  }
  return SAIL_OK;
}

// ---- noise estimate and render-until-converged (include/sail_hip.h; the kernel is sail_noise.hip) -------------------------
int sail_noise_mark(sail_ctx* c) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {  // device 0's reduced frame, like sail_filter
    if (int rc = loadIncomplete(c, "sail_noise_mark")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_noise_mark(c->subs[0]), c->subs[0]);
  }
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "sail_noise_mark: SAIL_ACCUM_COMPAT8 stores 8-bit frames, whose halves cannot be compared");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
  if (int rc = allocOnce(c, &c->noiseMark, bytes, "noise mark")) return rc;
  if (c->maskSet && c->noiseHave) {  // frozen tiles keep the mark they froze with
    SailNoiseArgs A;
    memset(&A, 0, sizeof A);
    A.S = shownAccum(c); A.P = c->noiseMark;
    A.W = c->W; A.H = c->H;
    A.active64 = c->maskBytes; A.tiles64X = (c->W + 63) / 64;
    HIPCHK(c, sail_launch_noise_copy(A, c->stream));
  } else {
    HIPCHK(c, hipMemcpyAsync(c->noiseMark, shownAccum(c), bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->noiseHave = true;
  c->noiseK = c->k;
  return SAIL_OK;
}

int sail_noise_estimate(sail_ctx* c, sail_noise_info* out, float* tile_err, float* pixel_err, int remark) {
  if (!c || !out) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_noise_estimate")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_noise_estimate(c->subs[0], out, tile_err, pixel_err, remark), c->subs[0]);
  }
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "sail_noise_estimate: SAIL_ACCUM_COMPAT8 stores 8-bit frames, whose halves cannot be compared");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (!c->noiseHave || !c->noiseMark)
    return fail(c, SAIL_E_STATE, "sail_noise_estimate: no mark (sail_noise_mark first; a reset or a new scene drops it)");
  if (c->k <= c->noiseK)
    return fail(c, SAIL_E_STATE, "sail_noise_estimate: no sample since the mark (k = %llu, marked at %llu)",
                (unsigned long long)c->k, (unsigned long long)c->noiseK);
  const int tx = (c->W + 15) / 16, ty = (c->H + 15) / 16;
  const size_t nt = (size_t)tx * ty, np = (size_t)c->W * c->H;
  if (int rc = allocOnce(c, &c->noiseOut, nt * 8, "noise tiles")) return rc;
  if (pixel_err)
    if (int rc = allocOnce(c, &c->noisePix, np * sizeof(float), "noise map")) return rc;
  SailNoiseArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.P = c->noiseMark;
  A.tileSum = c->noiseOut; A.tileBad = (uint32_t*)(c->noiseOut + nt);
  A.pixErr = pixel_err ? c->noisePix : nullptr;
  A.W = c->W; A.H = c->H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k; A.hf = (float)c->noiseK;
  A.remark = remark != 0;
  if (c->maskSet) { A.active64 = c->maskBytes; A.tiles64X = (c->W + 63) / 64; }
  std::vector<float> host(nt * 2);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (int rc = getEvent(c, &e0)) return rc;
  if (int rc = getEvent(c, &e1)) { c->evPool.push_back(e0); return rc; }
  float ms = 0.0f;
  hipError_t e = hipEventRecord(e0, c->stream);
  if (e == hipSuccess) e = sail_launch_noise(A, c->stream);
  if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  c->evPool.push_back(e0);
  c->evPool.push_back(e1);
  if (e == hipSuccess) e = hipMemcpy(host.data(), c->noiseOut, nt * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && pixel_err) e = hipMemcpy(pixel_err, c->noisePix, np * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_noise_estimate: %s", hipGetErrorString(e));
  // the tiles in index order, in double
  const uint32_t* bad = (const uint32_t*)(host.data() + nt);
  double sum = 0.0, maxTile = 0.0;
  uint64_t nonfinite = 0;
  for (int j = 0; j < ty; j++)
    for (int i = 0; i < tx; i++) {
      const size_t t = (size_t)j * tx + i;
      const int w = c->W - i * 16 < 16 ? c->W - i * 16 : 16, h = c->H - j * 16 < 16 ? c->H - j * 16 : 16;
      const double tileMean = (double)host[t] / (double)(w * h);
      sum += (double)host[t];
      if (tileMean > maxTile) maxTile = tileMean;
      nonfinite += bad[t];
      if (tile_err) tile_err[t] = (float)tileMean;
    }
  memset(out, 0, sizeof *out);
  out->mean = sum / (double)np;
  out->max_tile = maxTile;
  out->k = c->k;
  out->k_mark = c->noiseK;
  out->nonfinite = nonfinite;
  out->tiles_x = tx; out->tiles_y = ty;
  out->kernel_ms = ms;
  if (remark) c->noiseK = c->k;  // the kernel stored S into the mark
  return SAIL_OK;
}

int sail_plan_until(uint64_t k, uint64_t min_spp, uint64_t max_spp, uint64_t* next) {
  if (!next || min_spp < 1 || max_spp < min_spp)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_until: need 1 <= min_spp <= max_spp (min %llu, max %llu)",
                (unsigned long long)min_spp, (unsigned long long)max_spp);
  if (k < min_spp) *next = min_spp;
  else if (k >= max_spp) *next = k;
  else *next = k > max_spp / 2 ? max_spp : (2 * k < max_spp ? 2 * k : max_spp);
  return SAIL_OK;
}

// Render the frozen schedule's samples *k .. next (sail_render_until, sail_render_adaptive: `who` in the message)
static int renderSamplesTo(sail_ctx* c, const char* who, const double mvp[16], const float eye[3], int maxBounces,
                           uint64_t* k, uint64_t next) {
  constexpr uint64_t kChunk = 4096;  // samples whose matrices are built at a time (launches split anywhere bit for bit)
  std::vector<float> inv, seeds;
  while (*k < next) {
    const int spp = (int)(next - *k < kChunk ? next - *k : kChunk);
    inv.resize((size_t)spp * 16);
    seeds.resize((size_t)spp);
    if (int rc = sail_schedule(mvp, c->W, c->H, (int)*k, spp, inv.data(), seeds.data()))
      return fail(c, rc, "%s: sail_schedule failed (a singular camera matrix?)", who);
    if (int rc = sail_render_schedule(c, inv.data(), seeds.data(), eye, spp, maxBounces)) return rc;
    *k += (uint64_t)spp;
  }
  return SAIL_OK;
}

int sail_render_until(sail_ctx* c, const double mvp[16], const float eye[3], int maxBounces, double target,
                      uint64_t min_spp, uint64_t max_spp, sail_noise_info* out, int* converged, sail_until_step* history,
                      int capacity, int* looks) {
  if (!c) return SAIL_E_INVALID;
  // the frozen schedule indexes samples with an int (sail_schedule)
  if (!mvp || !eye || !out || min_spp < 1 || max_spp < min_spp || max_spp > 2147483647ull || target != target || capacity < 0)
    return fail(c, SAIL_E_INVALID, "sail_render_until: bad arguments (min_spp %llu, max_spp %llu, target %g)",
                (unsigned long long)min_spp, (unsigned long long)max_spp, target);
  // what the looks would refuse is refused before anything is rendered
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "sail_render_until: SAIL_ACCUM_COMPAT8 stores 8-bit frames, whose halves cannot be compared");
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_render_until before sail_set_scene");
  if (int rc = loadIncomplete(c, "sail_render_until")) return rc;
  uint64_t k = c->subs.empty() ? c->k : c->subs[0]->k;
  memset(out, 0, sizeof *out);
  out->mean = out->max_tile = INFINITY;  // until the first estimate
  out->k = out->k_mark = k;
  out->tiles_x = (c->W + 15) / 16; out->tiles_y = (c->H + 15) / 16;
  int nlooks = 0, conv = 0;
  bool marked = false;
  for (;;) {
    uint64_t next = k;
    if (int rc = sail_plan_until(k, min_spp, max_spp, &next)) return fail(c, rc, "sail_render_until: %s", sail_last_error(nullptr));
    if (next == k) break;  // at max_spp
    if (int rc = renderSamplesTo(c, "sail_render_until", mvp, eye, maxBounces, &k, next)) return rc;
    sail_until_step step{k, INFINITY, INFINITY};
    if (!marked) {  // the first look only marks: no estimate yet
      if (int rc = sail_noise_mark(c)) return rc;
      marked = true;
      out->k = out->k_mark = k;
    } else {
      // the last look (converged, or at max_spp) leaves the mark at the look before, so that the frame keeps its two
      // halves for sail_denoise; every other look moves the mark to now
      if (int rc = sail_noise_estimate(c, out, nullptr, nullptr, 0)) return rc;
      step.mean = out->mean; step.max_tile = out->max_tile;
      conv = out->mean <= target;
      if (!conv && k < max_spp)
        if (int rc = sail_noise_mark(c)) return rc;
    }
    if (history && nlooks < capacity) history[nlooks] = step;
    nlooks++;
    if (conv) break;
  }
  if (converged) *converged = conv;
  if (looks) *looks = nlooks;
  return SAIL_OK;
}

// ---- adaptive sampling: the tile mask and render-until-every-tile-converged (include/sail_hip.h) ---------------------------
int sail_set_active_tiles(sail_ctx* c, const uint8_t* active, int count) {
  if (!c) return SAIL_E_INVALID;
  const int tx = (c->W + 63) / 64, ty = (c->H + 63) / 64, tiles = tx * ty;
  const bool clear = !active && count == 0;
  // everything is checked before anything changes
  if (!clear && (!active || count != tiles))
    return fail(c, SAIL_E_INVALID, "sail_set_active_tiles: count %d, the frame has %d x %d = %d tiles (NULL, 0 removes the mask)",
                count, tx, ty, tiles);
  if (c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_STATE, "sail_set_active_tiles: SAIL_ACCUM_MIX and SAIL_ACCUM_COMPAT8 keep no per-pixel sample count");
  if (int rc = loadIncomplete(c, "sail_set_active_tiles")) return rc;
  if (!c->subs.empty()) {
    // a device that fails (memory, a HIP error) must not leave the devices before it under another mask than the rest:
    // they get the mask they had back, with the sample indices their tiles were switched off at
    const bool hadMask = c->subs[0]->maskSet;
    const std::vector<uint8_t> before = c->subs[0]->mask;
    std::vector<std::vector<uint32_t>> frozenBefore;
    for (sail_ctx* s : c->subs) frozenBefore.push_back(s->frozenAt);
    for (size_t i = 0; i < c->subs.size(); i++) {
      const int rc = sail_set_active_tiles(c->subs[i], active, count);
      if (rc == SAIL_OK) continue;
      relay(c, rc, c->subs[i]);
      for (size_t j = 0; j < i; j++) {
        (void)sail_set_active_tiles(c->subs[j], hadMask ? before.data() : nullptr, hadMask ? tiles : 0);
        c->subs[j]->frozenAt = frozenBefore[j];
      }
      return rc;
    }
    return SAIL_OK;
  }
  if (int rc = flushQueued(c)) return rc;  // queued samples were asked for under the mask as it was
  if (clear) {
    c->maskSet = false;
    c->mask.clear();
    c->frozenAt.clear();
    return SAIL_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight read the tables
  if (int rc = allocOnce(c, &c->tileMap, sizeof(int32_t) * (size_t)tiles, "tile table")) return rc;
  if (int rc = allocOnce(c, &c->maskBytes, (size_t)tiles, "tile mask")) return rc;
  std::vector<uint8_t> m((size_t)tiles);
  for (int t = 0; t < tiles; t++) m[(size_t)t] = active[t] ? 1 : 0;
  // this rank's active tiles, ascending, and their in-frame pixels
  const int w = (c->partMode == SAIL_PART_SAMPLES) ? 1 : c->world, r = (c->partMode == SAIL_PART_SAMPLES) ? 0 : c->rank;
  std::vector<int32_t> table;
  long long px = 0;
  for (int t = r; t < tiles; t += w) {
    if (!m[(size_t)t]) continue;
    table.push_back(t);
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    const int cw = (c->W - x0) < 64 ? (c->W - x0) : 64, ch = (c->H - y0) < 64 ? (c->H - y0) : 64;
    px += (long long)cw * ch;
  }
  if (!table.empty())
    HIPCHK(c, hipMemcpy(c->tileMap, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->maskBytes, m.data(), (size_t)tiles, hipMemcpyHostToDevice));
  if (c->frozenAt.size() != (size_t)tiles) c->frozenAt.assign((size_t)tiles, 0u);
  for (int t = 0; t < tiles; t++) {
    const bool was = !c->maskSet || c->mask[(size_t)t];
    if (was && !m[(size_t)t]) c->frozenAt[(size_t)t] = (uint32_t)c->k;
  }
  c->mask.swap(m);
  c->maskSet = true;
  c->maskTiles = (int)table.size();
  c->maskPixels = px;
  return SAIL_OK;
}

int sail_get_active_tiles(sail_ctx* c, uint8_t* active, int count, int* n_active) {
  if (!c) return SAIL_E_INVALID;
  const int tiles = ((c->W + 63) / 64) * ((c->H + 63) / 64);
  if (!active || count != tiles)
    return fail(c, SAIL_E_INVALID, "sail_get_active_tiles: count %d, the frame has %d tiles", count, tiles);
  const sail_ctx* h = c->subs.empty() ? c : c->subs[0];  // every device of a multi-device context holds the whole mask
  int n = 0;
  for (int t = 0; t < tiles; t++) {
    active[t] = (!h->maskSet || h->mask[(size_t)t]) ? 1 : 0;
    n += active[t];
  }
  if (n_active) *n_active = n;
  return SAIL_OK;
}

int sail_plan_adaptive(int width, int height, const float* tile_err16, double target, int dilate, const uint8_t* prev_active,
                       uint8_t* active, double* tile_err64, int* n_active) {
  if (width < 1 || height < 1 || !tile_err16 || !active || target != target || dilate < 0 || dilate > 1)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_adaptive: bad arguments (%d x %d, target %g, dilate %d)", width, height,
                target, dilate);
  const int tx16 = (width + 15) / 16, ty16 = (height + 15) / 16, tx = (width + 63) / 64, ty = (height + 63) / 64;
  std::vector<uint8_t> noisy((size_t)tx * ty);
  for (int j = 0; j < ty; j++)
    for (int i = 0; i < tx; i++) {
      double sum = 0.0, px = 0.0;
      for (int v = j * 4; v < j * 4 + 4 && v < ty16; v++)
        for (int u = i * 4; u < i * 4 + 4 && u < tx16; u++) {
          const int w = width - u * 16 < 16 ? width - u * 16 : 16, h = height - v * 16 < 16 ? height - v * 16 : 16;
          sum += (double)tile_err16[(size_t)v * tx16 + u] * (double)(w * h);
          px += (double)(w * h);
        }
      const double e64 = sum / px;
      const size_t t = (size_t)j * tx + i;
      if (tile_err64) tile_err64[t] = e64;
      noisy[t] = !(e64 <= target);
    }
  int n = 0;
  for (int j = 0; j < ty; j++)
    for (int i = 0; i < tx; i++) {
      const size_t t = (size_t)j * tx + i;
      bool keep = noisy[t] != 0;
      for (int dj = -1; dilate && !keep && dj <= 1; dj++)
        for (int di = -1; !keep && di <= 1; di++) {
          const int a = i + di, b = j + dj;
          if (a >= 0 && a < tx && b >= 0 && b < ty && noisy[(size_t)b * tx + a]) keep = true;
        }
      const bool prev = !prev_active || prev_active[t];
      active[t] = (prev && keep) ? 1 : 0;
      n += active[t];
    }
  if (n_active) *n_active = n;
  return SAIL_OK;
}

int sail_adaptive_defaults(sail_adaptive_params* p) {
  if (!p) return SAIL_E_INVALID;
  p->target = INFINITY;
  p->min_spp = 16;
  p->max_spp = 1024;
  p->dilate = 1;
  return SAIL_OK;
}

int sail_render_adaptive(sail_ctx* c, const double mvp[16], const float eye[3], int maxBounces, const sail_adaptive_params* params,
                         sail_adaptive_info* out, sail_until_step* history, int capacity, int* looks, uint32_t* tile_samples) {
  if (!c) return SAIL_E_INVALID;
  sail_adaptive_params p;
  sail_adaptive_defaults(&p);
  if (params) p = *params;
  if (!mvp || !eye || !out || p.min_spp < 1 || p.max_spp < p.min_spp || p.max_spp > 2147483647ull || p.target != p.target ||
      p.dilate < 0 || p.dilate > 1 || capacity < 0)
    return fail(c, SAIL_E_INVALID, "sail_render_adaptive: bad arguments (min_spp %llu, max_spp %llu, target %g, dilate %d)",
                (unsigned long long)p.min_spp, (unsigned long long)p.max_spp, p.target, p.dilate);
  // what the looks and the mask would refuse is refused before anything is rendered
  if (c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_STATE, "sail_render_adaptive: SAIL_ACCUM_MIX and SAIL_ACCUM_COMPAT8 keep no per-pixel sample count");
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_render_adaptive before sail_set_scene");
  if (int rc = loadIncomplete(c, "sail_render_adaptive")) return rc;
  const sail_ctx* h = c->subs.empty() ? c : c->subs[0];  // holds the sample index, the whole mask and the mark
  const int tx = (c->W + 63) / 64, ty = (c->H + 63) / 64, tiles = tx * ty;
  const int tx16 = (c->W + 15) / 16, ty16 = (c->H + 15) / 16;
  auto tilePixels = [&](int t) {
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    return (uint64_t)((c->W - x0) < 64 ? (c->W - x0) : 64) * (uint64_t)((c->H - y0) < 64 ? (c->H - y0) : 64);
  };
  std::vector<uint8_t> active((size_t)tiles);
  int nActive = 0;
  if (int rc = sail_get_active_tiles(c, active.data(), tiles, &nActive)) return rc;
  auto activePixels = [&]() {
    uint64_t px = 0;
    for (int t = 0; t < tiles; t++) if (active[(size_t)t]) px += tilePixels(t);
    return px;
  };
  sail_stats st0;
  if (int rc = sail_get_stats(c, &st0)) return rc;
  uint64_t k = h->k;
  const uint64_t k0 = k;
  memset(out, 0, sizeof *out);
  out->noise.mean = out->noise.max_tile = INFINITY;  // until the first estimate
  out->noise.k = out->noise.k_mark = k;
  out->noise.tiles_x = tx16; out->noise.tiles_y = ty16;
  out->tiles_x = tx; out->tiles_y = ty;
  int nlooks = 0;
  bool marked = false;
  std::vector<float> err16((size_t)tx16 * ty16);
  while (nActive > 0) {
    uint64_t next = k;
    if (int rc = sail_plan_until(k, p.min_spp, p.max_spp, &next)) return fail(c, rc, "sail_render_adaptive: %s", sail_last_error(nullptr));
    if (next == k) break;  // at max_spp
    out->pixel_samples += activePixels() * (next - k);
    if (int rc = renderSamplesTo(c, "sail_render_adaptive", mvp, eye, maxBounces, &k, next)) return rc;
    sail_until_step step{k, INFINITY, INFINITY};
    if (!marked) {  // the first look only marks: no estimate yet
      if (int rc = sail_noise_mark(c)) return rc;
      marked = true;
      out->noise.k = out->noise.k_mark = k;
    } else {
      if (int rc = sail_noise_estimate(c, &out->noise, err16.data(), nullptr, 0)) return rc;
      step.mean = out->noise.mean; step.max_tile = out->noise.max_tile;
      if (int rc = sail_plan_adaptive(c->W, c->H, err16.data(), p.target, p.dilate, active.data(), active.data(), nullptr, &nActive))
        return fail(c, rc, "sail_render_adaptive: %s", sail_last_error(nullptr));
      if (int rc = sail_set_active_tiles(c, active.data(), tiles)) return rc;
      // the look it stops at leaves the mark at the look before, for sail_denoise; every other look moves the active
      // tiles' mark to now
      if (nActive > 0 && k < p.max_spp)
        if (int rc = sail_noise_mark(c)) return rc;
    }
    if (history && nlooks < capacity) history[nlooks] = step;
    nlooks++;
  }
  sail_stats st1;
  if (int rc = sail_get_stats(c, &st1)) return rc;
  out->converged = nActive == 0;
  out->active_tiles = nActive;
  out->frame_pixel_samples = (uint64_t)c->W * (uint64_t)c->H * (k - k0);
  out->kernel_ms = st1.kernel_ms - st0.kernel_ms;
  if (tile_samples)
    for (int t = 0; t < tiles; t++)
      tile_samples[t] = (!h->maskSet || h->mask[(size_t)t]) ? (uint32_t)k : h->frozenAt[(size_t)t];
  if (looks) *looks = nlooks;
  return SAIL_OK;
}

// ---- variance-guided a-trous denoiser (include/sail_hip.h; the kernels are sail_denoise.hip) --------------------------------
int sail_denoise_defaults(sail_denoise_params* p) {
  if (!p) return SAIL_E_INVALID;
  p->iterations = 4;
  p->sigma_l = 1.0f;
  p->sigma_x = 0.2f;
  p->display = SAIL_FILTER_COLOR;
  p->gamma_c = 2.2f;
  return SAIL_OK;
}

}  // extern "C"

namespace {

bool aminOk(float amin) { return std::isfinite(amin) && amin > 0.0f; }

// sail_denoise (demod = false: amin is not read, no map is needed) and sail_denoise_albedo
int denoiseCall(sail_ctx* c, const char* who, bool demod, const sail_denoise_params* params, float amin, float* out_rgba,
                float* out_var, uint8_t* out_rgba8, sail_denoise_info* info) {
  if (!c) return SAIL_E_INVALID;
  sail_denoise_params p;
  sail_denoise_defaults(&p);
  if (params) p = *params;
  if (p.iterations < 1 || p.iterations > 6 || !(p.sigma_l > 0.0f) || !std::isfinite(p.sigma_l) || !(p.sigma_x > 0.0f) ||
      !std::isfinite(p.sigma_x) || p.display < SAIL_FILTER_COLOR || p.display > SAIL_FILTER_TONEMAPPING)
    return fail(c, SAIL_E_INVALID, "%s: bad parameters (iterations %d of 1..6, sigma_l %g and sigma_x %g finite and > 0, display %d of 0..2)",
                who, p.iterations, (double)p.sigma_l, (double)p.sigma_x, p.display);
  if (demod && !aminOk(amin)) return fail(c, SAIL_E_INVALID, "%s: amin %g must be finite and > 0", who, (double)amin);
  if (!c->subs.empty()) {  // device 0's reduced frame and AOV maps, like sail_filter
    if (int rc = loadIncomplete(c, who)) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, denoiseCall(c->subs[0], who, demod, &p, amin, out_rgba, out_var, out_rgba8, info), c->subs[0]);
  }
  if (!c->aovN || !c->aovP)
    return fail(c, SAIL_E_STATE, "%s: reads the normal and position AOVs (create with SAIL_FLAG_AOV)", who);
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "%s: SAIL_ACCUM_COMPAT8 stores 8-bit frames, whose halves cannot be compared", who);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (!c->noiseHave || !c->noiseMark)
    return fail(c, SAIL_E_STATE, "%s: no mark (sail_noise_mark first; a reset or a new scene drops it)", who);
  if (c->k <= c->noiseK)
    return fail(c, SAIL_E_STATE, "%s: no sample since the mark (k = %llu, marked at %llu)", who,
                (unsigned long long)c->k, (unsigned long long)c->noiseK);
  if (demod && (!c->albHave || !c->albMap))
    return fail(c, SAIL_E_STATE, "%s: no albedo map (sail_albedo or sail_albedo_load first; new rows drop it)", who);
  const size_t nt = (size_t)((c->W + 15) / 16) * (size_t)((c->H + 15) / 16);
  if (int rc = ensureDenoiseWork(c)) return rc;
  const DenoiseWork w = denoiseWork(c);
  SailDenoisePrepareArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.P = c->noiseMark; A.N = shownAovN(c); A.X = shownAovP(c);
  A.cv = w.cv[0]; A.g0 = w.g0; A.g1 = w.g1; A.tileBad = w.bad;
  A.W = c->W; A.H = c->H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k; A.hf = (float)c->noiseK;
  float ms[8] = {}, total = 0.0f;
  int rc = SAIL_OK;
  SailDenoisePrepareDemodArgs D;
  memset(&D, 0, sizeof D);
  D.P = A; D.alb = c->albMap; D.amin = amin;
  hipError_t e = runAtrous(c, w, [&] { return demod ? sail_launch_denoise_prepare_demod(D, c->stream)
                                                      : sail_launch_denoise_prepare(A, c->stream); },
                           p.iterations, p.sigma_l, p.sigma_x, p.display, p.gamma_c, out_rgba, out_var, out_rgba8, ms, &total,
                           &rc, demod ? c->albMap : nullptr, amin);
  if (rc) return rc;
  std::vector<uint32_t> bad(nt);
  if (e == hipSuccess) e = hipMemcpy(bad.data(), w.bad, nt * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "%s: %s", who, hipGetErrorString(e));
  if (info) {
    memset(info, 0, sizeof *info);
    info->k = c->k;
    info->k_mark = c->noiseK;
    for (uint32_t b : bad) info->nonfinite += b;
    info->iterations = p.iterations;
    info->kernel_ms = total;
    for (int i = 0; i <= p.iterations; i++) info->pass_ms[i] = ms[i];
  }
  return SAIL_OK;
}

}  // namespace

extern "C" {

int sail_denoise(sail_ctx* c, const sail_denoise_params* params, float* out_rgba, float* out_var, uint8_t* out_rgba8,
                 sail_denoise_info* info) {
  return denoiseCall(c, "sail_denoise", false, params, 0.0f, out_rgba, out_var, out_rgba8, info);
}

int sail_denoise_albedo(sail_ctx* c, const sail_denoise_params* params, float amin, float* out_rgba, float* out_var,
                        uint8_t* out_rgba8, sail_denoise_info* info) {
  return denoiseCall(c, "sail_denoise_albedo", true, params, amin, out_rgba, out_var, out_rgba8, info);
}

// ---- camera-motion reprojection (include/sail_hip.h; the kernels are sail_temporal.hip) ---------------------------------------
int sail_temporal_defaults(sail_temporal_params* p) {
  if (!p) return SAIL_E_INVALID;
  p->cap = 32.0f;
  p->pos_tol = 0.05f;
  p->display = SAIL_FILTER_COLOR;
  p->gamma_c = 2.2f;
  return SAIL_OK;
}

}  // extern "C"

namespace {

int temporalParams(sail_ctx* c, const char* who, const sail_temporal_params* params, sail_temporal_params* p) {
  sail_temporal_defaults(p);
  if (params) *p = *params;
  if (!std::isfinite(p->cap) || p->cap < 1.0f || !std::isfinite(p->pos_tol) || !(p->pos_tol > 0.0f) ||
      p->display < SAIL_FILTER_COLOR || p->display > SAIL_FILTER_TONEMAPPING)
    return fail(c, SAIL_E_INVALID, "%s: bad parameters (cap %g finite and >= 1, pos_tol %g finite and > 0, display %d of 0..2)",
                who, (double)p->cap, (double)p->pos_tol, p->display);
  return SAIL_OK;
}

// what every temporal call refuses on one device's context
int temporalState(sail_ctx* c, const char* who) {
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "%s: no scene (call sail_set_scene first)", who);
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "%s: SAIL_ACCUM_COMPAT8 stores 8-bit frames, which carry no sample count to blend with", who);
  return SAIL_OK;
}

size_t temporalTiles(const sail_ctx* c) { return (size_t)((c->W + 15) / 16) * (size_t)((c->H + 15) / 16); }
uint32_t* temporalOut8(const sail_ctx* c) { return (uint32_t*)((char*)c->tpWork + (size_t)c->W * c->H * 80); }
uint32_t* temporalCounts(const sail_ctx* c) { return temporalOut8(c) + (size_t)c->W * c->H; }

int ensureTemporal(sail_ctx* c) {
  if (c->tpWork) return SAIL_OK;
  const size_t np = (size_t)c->W * c->H;
  // five float4 maps (16 B each) | rgba8 (4 B) per pixel, then three counts per tile
  if (int rc = allocOnce(c, &c->tpWork, np * 84 + temporalTiles(c) * 12, "temporal maps")) return rc;
  float4* base = (float4*)c->tpWork;
  c->tpGcur = base; c->tpGprev = base + np; c->tpHist = base + 2 * np; c->tpR = base + 3 * np; c->tpOut = base + 4 * np;
  return SAIL_OK;
}

// the G-buffer pass's arguments for a view: the corner directions of a sample without jitter
int gbufferArgs(sail_ctx* c, const char* who, const double mvp[16], const float eye[3], SailGbufferArgs* A) {
  float inv[16];
  if (sail_jitter_inverse(mvp, 0.0, 0.0, c->W, c->H, inv) != SAIL_OK)
    return fail(c, SAIL_E_INVALID, "%s: the camera matrix is singular", who);
  memset(A, 0, sizeof *A);
  A->prims = c->prims; A->n = c->n;
  cornerDirs(inv, eye, A->d);
  memcpy(A->eye, eye, sizeof A->eye);
  A->W = c->W; A->H = c->H;
  return SAIL_OK;
}

uint64_t sumTiles(const std::vector<uint32_t>& v, size_t from, size_t count) {
  uint64_t s = 0;
  for (size_t i = 0; i < count; i++) s += v[from + i];
  return s;
}

}  // namespace

extern "C" {

int sail_gbuffer(sail_ctx* c, const double mvp[16], const float eye[3], float* rays6, int32_t* id, float* t, float* xyz) {
  if (!c) return SAIL_E_INVALID;
  if (!mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_gbuffer: mvp and eye are required");
  if (!c->subs.empty()) return relay(c, sail_gbuffer(c->subs[0], mvp, eye, rays6, id, t, xyz), c->subs[0]);
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_gbuffer: no scene (call sail_set_scene first)");
  SailGbufferArgs A;
  if (int rc = gbufferArgs(c, "sail_gbuffer", mvp, eye, &A)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t np = (size_t)c->W * c->H;
  void* work = nullptr;  // G (16 B) | rays (24 B) | t (4 B) per pixel
  if (hipMalloc(&work, np * 44) != hipSuccess) return fail(c, SAIL_E_OOM, "G-buffer scratch");
  A.G = (float4*)work;
  A.rays = rays6 ? (float*)((char*)work + np * 16) : nullptr;
  A.t = t ? (float*)((char*)work + np * 40) : nullptr;
  std::vector<float> g((id || xyz) ? np * 4 : 0);
  hipError_t e = sail_launch_gbuffer(A, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && !g.empty()) e = hipMemcpy(g.data(), A.G, np * 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess && rays6) e = hipMemcpy(rays6, A.rays, np * 24, hipMemcpyDeviceToHost);
  if (e == hipSuccess && t) e = hipMemcpy(t, A.t, np * 4, hipMemcpyDeviceToHost);
  (void)hipFree(work);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_gbuffer: %s", hipGetErrorString(e));
  for (size_t i = 0; i < np && !g.empty(); i++) {
    if (id) id[i] = (int32_t)g[4 * i + 3];
    if (xyz) { xyz[3 * i] = g[4 * i]; xyz[3 * i + 1] = g[4 * i + 1]; xyz[3 * i + 2] = g[4 * i + 2]; }
  }
  return SAIL_OK;
}

int sail_temporal_begin(sail_ctx* c, const double mvp[16], const float eye[3], const sail_temporal_params* params,
                        sail_temporal_info* info) {
  if (!c) return SAIL_E_INVALID;
  sail_temporal_params p;
  if (int rc = temporalParams(c, "sail_temporal_begin", params, &p)) return rc;
  if (!mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_temporal_begin: mvp and eye are required");
  if (!c->subs.empty()) {  // device 0's reduced frame and scene, like sail_filter
    if (int rc = loadIncomplete(c, "sail_temporal_begin")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_temporal_begin(c->subs[0], mvp, eye, &p, info), c->subs[0]);
  }
  if (int rc = temporalState(c, "sail_temporal_begin")) return rc;
  SailGbufferArgs A;
  if (int rc = gbufferArgs(c, "sail_temporal_begin", mvp, eye, &A)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (int rc = ensureTemporal(c)) return rc;
  const bool moved = c->tpMotionPending;
  if (moved) {  // before anything is committed: a begin that fails keeps it all
    const int rows = c->n > 0 ? c->n : 1;
    if (int rc = growBuffer(c, &c->tpMotionDev, &c->tpMotionDevRows, rows, sizeof(float4) * (size_t)rows, "object motion table"))
      return rc;
  }
  if (c->tpHaveCur) {  // commit the view that was current
    std::swap(c->tpHist, c->tpOut);
    std::swap(c->tpGprev, c->tpGcur);
    if (c->tpMom) std::swap(c->tpMhist, c->tpMout);
    c->tpPrev = c->tpCur;
    c->tpHavePrev = true;
    c->tpHaveCur = false;
  }
  const size_t nt = temporalTiles(c), np = (size_t)c->W * c->H;
  uint32_t* cnt = temporalCounts(c);
  A.G = c->tpGcur;
  SailReprojectArgs B;
  memset(&B, 0, sizeof B);
  B.Gcur = c->tpGcur; B.Gprev = c->tpGprev; B.hist = c->tpHist; B.out = c->tpR;
  B.tileHit = cnt; B.tileHist = cnt + nt;
  for (int j = 0; j < 4; j++) { B.Mp[0][j] = c->tpPrev.m[j]; B.Mp[1][j] = c->tpPrev.m[4 + j]; B.Mp[2][j] = c->tpPrev.m[12 + j]; }
  memcpy(B.eyePrev, c->tpPrev.eye, sizeof B.eyePrev);
  B.tol2 = p.pos_tol * p.pos_tol;
  B.W = c->W; B.H = c->H;
  B.haveHist = c->tpHavePrev;
  // an object motion is pending (sail_move_objects): the moved kernels, with the table uploaded ahead of them
  B.motion = c->tpMotionDev; B.n = c->n; B.mc = c->tpMotionCap;
  c->tpResolved = false;
  // moment tracking: the same gather over Mhist, timed with the reproject pass
  const int nev = c->tpMom ? 4 : 3;
  SailReprojectArgs M = B;
  M.hist = c->tpMhist; M.out = c->tpMR;
  M.tileHit = nullptr; M.tileHist = nullptr;
  PooledEvents ev(c, nev);
  if (ev.rc) return ev.rc;
  hipError_t e = hipSuccess;
  if (moved && c->n > 0)
    e = hipMemcpyAsync(c->tpMotionDev, c->tpMotion.data(), sizeof(float4) * (size_t)c->n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = sail_launch_gbuffer(A, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = sail_launch_reproject(B, moved, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[2], c->stream);
  if (c->tpMom) {
    if (e == hipSuccess) e = sail_launch_moment_reproject(M, moved, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[3], c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->tpMout, c->tpMR, np * 16, hipMemcpyDeviceToDevice, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(c->tpOut, c->tpR, np * 16, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  float ms[3] = {};
  for (int i = 0; i + 1 < nev && e == hipSuccess; i++) e = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  ms[1] += ms[2];  // the moment reproject, when it ran
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = hipMemcpy(host.data(), cnt, nt * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_temporal_begin: %s", hipGetErrorString(e));
  for (int i = 0; i < 16; i++) c->tpCur.m[i] = (float)mvp[i];
  memcpy(c->tpCur.eye, eye, sizeof c->tpCur.eye);
  c->tpHaveCur = true;
  clearMotion(c);  // consumed: the next begin is today's unless the rows move again
  c->tpHitPixels = sumTiles(host, 0, nt);
  if (info) {
    memset(info, 0, sizeof *info);
    info->k = c->k;
    info->hit_pixels = c->tpHitPixels;
    info->history_pixels = sumTiles(host, nt, nt);
    info->kernel_ms = (double)ms[0] + (double)ms[1];
    info->pass_ms[0] = ms[0]; info->pass_ms[1] = ms[1];
  }
  return SAIL_OK;
}

int sail_temporal_resolve(sail_ctx* c, const sail_temporal_params* params, float* out_rgba, uint8_t* out_rgba8,
                          sail_temporal_info* info) {
  if (!c) return SAIL_E_INVALID;
  sail_temporal_params p;
  if (int rc = temporalParams(c, "sail_temporal_resolve", params, &p)) return rc;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_temporal_resolve")) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, sail_temporal_resolve(c->subs[0], &p, out_rgba, out_rgba8, info), c->subs[0]);
  }
  if (int rc = temporalState(c, "sail_temporal_resolve")) return rc;
  if (!c->tpHaveCur || !c->tpWork)
    return fail(c, SAIL_E_STATE, "sail_temporal_resolve: no current view (sail_temporal_begin first; a new scene drops it)");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t nt = temporalTiles(c), np = (size_t)c->W * c->H;
  uint32_t* cnt = temporalCounts(c);
  SailResolveArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.R = c->tpR; A.Out = c->tpOut;
  A.out8 = out_rgba8 ? temporalOut8(c) : nullptr;
  A.tileHist = cnt + nt; A.tileBad = cnt + 2 * nt;
  A.W = c->W; A.H = c->H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k;
  A.cap = p.cap; A.display = p.display; A.gammaC = p.gamma_c;
  PooledEvents ev(c, 2);
  if (ev.rc) return ev.rc;
  float ms = 0.0f;
  hipError_t e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = sail_launch_temporal_resolve(A, c->stream);
  if (c->tpMom && e == hipSuccess) {  // moment tracking: blended like the colour, timed with it
    SailMomentResolveArgs M;
    memset(&M, 0, sizeof M);
    M.S = A.S; M.MR = c->tpMR; M.Mout = c->tpMout;
    M.W = c->W; M.H = c->H; M.mix = A.mix; M.kf = A.kf; M.cap = A.cap;
    e = sail_launch_moment_resolve(M, c->stream);
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = hipMemcpy(host.data(), cnt + nt, nt * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_rgba) e = hipMemcpy(out_rgba, c->tpOut, np * 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_rgba8) e = hipMemcpy(out_rgba8, A.out8, np * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_temporal_resolve: %s", hipGetErrorString(e));
  c->tpResolved = true;
  if (info) {
    memset(info, 0, sizeof *info);
    info->k = c->k;
    info->hit_pixels = c->tpHitPixels;
    info->history_pixels = sumTiles(host, 0, nt);
    info->nonfinite = sumTiles(host, nt, nt);
    info->kernel_ms = ms;
    info->pass_ms[2] = ms;
  }
  return SAIL_OK;
}

int sail_temporal_read(sail_ctx* c, int which, float* out) {
  if (!c) return SAIL_E_INVALID;
  if (!out || which < SAIL_TEMPORAL_G_CUR || which > SAIL_TEMPORAL_OUT)
    return fail(c, SAIL_E_INVALID, "sail_temporal_read: map %d of 0..4 and an output are required", which);
  if (!c->subs.empty()) return relay(c, sail_temporal_read(c->subs[0], which, out), c->subs[0]);
  const bool prev = which == SAIL_TEMPORAL_G_PREV || which == SAIL_TEMPORAL_HIST;
  if (!c->tpWork || !(prev ? c->tpHavePrev : c->tpHaveCur))
    return fail(c, SAIL_E_STATE, "sail_temporal_read: map %d needs a %s view (a new scene drops both)", which,
                prev ? "committed" : "current");
  const float4* maps[5] = {c->tpGcur, c->tpGprev, c->tpHist, c->tpR, c->tpOut};
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, maps[which], (size_t)c->W * c->H * 16, hipMemcpyDeviceToHost));
  return SAIL_OK;
}

int sail_temporal_load_history(sail_ctx* c, const float* hist, const float* g, const double mvp_prev[16],
                               const float eye_prev[3]) {
  if (!c) return SAIL_E_INVALID;
  if (!hist || !g || !mvp_prev || !eye_prev)
    return fail(c, SAIL_E_INVALID, "sail_temporal_load_history: hist, g, mvp_prev and eye_prev are required");
  if (!c->subs.empty()) return relay(c, sail_temporal_load_history(c->subs[0], hist, g, mvp_prev, eye_prev), c->subs[0]);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = ensureTemporal(c)) return rc;
  const size_t bytes = (size_t)c->W * c->H * 16;
  HIPCHK(c, hipMemcpy(c->tpHist, hist, bytes, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->tpGprev, g, bytes, hipMemcpyHostToDevice));
  for (int i = 0; i < 16; i++) c->tpPrev.m[i] = (float)mvp_prev[i];
  memcpy(c->tpPrev.eye, eye_prev, sizeof c->tpPrev.eye);
  c->tpHavePrev = true;
  c->tpHaveCur = false;
  c->tpResolved = false;
  clearMotion(c);  // a loaded history belongs to the rows as they are now
  if (c->tpMom) {  // the loaded history carries no moments
    HIPCHK(c, hipMemsetAsync(c->tpMhist, 0, bytes, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return SAIL_OK;
}

// ---- moment tracking and the temporal filter (include/sail_hip.h; the kernels are sail_tfilter.hip) ---------------------------
int sail_temporal_moments(sail_ctx* c, int on) {
  // the arguments first, so that they can be checked without a device (a NULL context's message: sail_last_error(NULL))
  if (on != 0 && on != 1) return fail(c, SAIL_E_INVALID, "sail_temporal_moments: on must be 0 or 1, not %d", on);
  if (!c) return fail(c, SAIL_E_INVALID, "sail_temporal_moments: a context is required");
  if (!c->subs.empty()) return relay(c, sail_temporal_moments(c->subs[0], on), c->subs[0]);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!on) {
    if (c->tpMom) HIPCHK(c, hipFree(c->tpMom));
    c->tpMom = nullptr;
    c->tpMhist = c->tpMR = c->tpMout = nullptr;
    return SAIL_OK;
  }
  if (c->tpMom) return SAIL_OK;
  const size_t np = (size_t)c->W * c->H;
  // three float4 maps (16 B each) per pixel, then the filter's count of temporal pixels per tile
  if (int rc = allocOnce(c, &c->tpMom, np * 48 + temporalTiles(c) * 4, "moment maps")) return rc;
  float4* base = (float4*)c->tpMom;
  c->tpMhist = base; c->tpMR = base + np; c->tpMout = base + 2 * np;
  HIPCHK(c, zeroMoments(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAIL_OK;
}

int sail_temporal_load_moments(sail_ctx* c, const float* mom) {
  if (!c) return SAIL_E_INVALID;
  if (!mom) return fail(c, SAIL_E_INVALID, "sail_temporal_load_moments: mom is required");
  if (!c->subs.empty()) return relay(c, sail_temporal_load_moments(c->subs[0], mom), c->subs[0]);
  if (!c->tpMom)
    return fail(c, SAIL_E_STATE, "sail_temporal_load_moments: moment tracking is off (sail_temporal_moments first)");
  if (!c->tpHavePrev || c->tpHaveCur)
    return fail(c, SAIL_E_STATE, "sail_temporal_load_moments: needs a committed history and no current view (right after sail_temporal_load_history)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->tpMhist, mom, (size_t)c->W * c->H * 16, hipMemcpyHostToDevice));
  return SAIL_OK;
}

int sail_temporal_read_moments(sail_ctx* c, int which, float* out) {
  if (!out || which < SAIL_TEMPORAL_M_HIST || which > SAIL_TEMPORAL_M_OUT)
    return fail(c, SAIL_E_INVALID, "sail_temporal_read_moments: map %d of 0..2 and an output are required", which);
  if (!c) return fail(c, SAIL_E_INVALID, "sail_temporal_read_moments: a context is required");
  if (!c->subs.empty()) return relay(c, sail_temporal_read_moments(c->subs[0], which, out), c->subs[0]);
  if (!c->tpMom)
    return fail(c, SAIL_E_STATE, "sail_temporal_read_moments: moment tracking is off (sail_temporal_moments first)");
  const bool prev = which == SAIL_TEMPORAL_M_HIST;
  if (!c->tpWork || !(prev ? c->tpHavePrev : c->tpHaveCur))
    return fail(c, SAIL_E_STATE, "sail_temporal_read_moments: map %d needs a %s view (a new scene drops both)", which,
                prev ? "committed" : "current");
  const float4* maps[3] = {c->tpMhist, c->tpMR, c->tpMout};
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, maps[which], (size_t)c->W * c->H * 16, hipMemcpyDeviceToHost));
  return SAIL_OK;
}

int sail_temporal_filter_defaults(sail_tfilter_params* p) {
  if (!p) return SAIL_E_INVALID;
  p->iterations = 4;
  p->sigma_l = 4.0f;
  p->sigma_x = 0.2f;
  p->min_hist = 4.0f;
  p->display = SAIL_FILTER_COLOR;
  p->gamma_c = 2.2f;
  return SAIL_OK;
}

}  // extern "C"

namespace {

// sail_temporal_filter (demod = false: amin is not read, no map is needed) and sail_temporal_filter_albedo
int tfilterCall(sail_ctx* c, const char* who, bool demod, const sail_tfilter_params* params, float amin, float* out_rgba,
                float* out_var, uint8_t* out_rgba8, sail_tfilter_info* info) {
  // the parameters first, so that they can be checked without a device (a NULL context's message: sail_last_error(NULL))
  sail_tfilter_params p;
  sail_temporal_filter_defaults(&p);
  if (params) p = *params;
  if (p.iterations < 1 || p.iterations > 6 || !(p.sigma_l > 0.0f) || !std::isfinite(p.sigma_l) || !(p.sigma_x > 0.0f) ||
      !std::isfinite(p.sigma_x) || !std::isfinite(p.min_hist) || p.min_hist < 1.0f || p.display < SAIL_FILTER_COLOR ||
      p.display > SAIL_FILTER_TONEMAPPING)
    return fail(c, SAIL_E_INVALID, "%s: bad parameters (iterations %d of 1..6, sigma_l %g and sigma_x %g finite and > 0, min_hist %g finite and >= 1, display %d of 0..2)",
                who, p.iterations, (double)p.sigma_l, (double)p.sigma_x, (double)p.min_hist, p.display);
  if (demod && !aminOk(amin)) return fail(c, SAIL_E_INVALID, "%s: amin %g must be finite and > 0", who, (double)amin);
  if (!c) return fail(c, SAIL_E_INVALID, "%s: a context is required", who);
  if (!c->subs.empty()) {  // device 0's reduced frame, AOV and temporal maps, like sail_denoise
    if (int rc = loadIncomplete(c, who)) return rc;
    if (int rc = groupReduce(c)) return rc;
    return relay(c, tfilterCall(c->subs[0], who, demod, &p, amin, out_rgba, out_var, out_rgba8, info), c->subs[0]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (!c->tpMom)
    return fail(c, SAIL_E_STATE, "%s: moment tracking is off (sail_temporal_moments first)", who);
  if (!c->aovN || !c->aovP)
    return fail(c, SAIL_E_STATE, "%s: reads the normal and position AOVs (create with SAIL_FLAG_AOV)", who);
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "%s: SAIL_ACCUM_COMPAT8 stores 8-bit frames, which carry no sample count to blend with", who);
  if (!c->tpHaveCur || !c->tpWork)
    return fail(c, SAIL_E_STATE, "%s: no current view (sail_temporal_begin first; a new scene drops it)", who);
  if (!c->tpResolved)
    return fail(c, SAIL_E_STATE, "%s: the current view is not resolved (sail_temporal_resolve first)", who);
  if (c->k == 0)
    return fail(c, SAIL_E_STATE, "%s: no sample of the current view (k = 0: the AOVs belong to another view)", who);
  if (demod && (!c->albHave || !c->albMap))
    return fail(c, SAIL_E_STATE, "%s: no albedo map (sail_albedo or sail_albedo_load first; new rows drop it)", who);
  if (demod && memcmp(&c->albView, &c->tpCur, sizeof c->albView) != 0)
    return fail(c, SAIL_E_STATE, "%s: the albedo map belongs to another view than the current temporal view", who);
  const size_t nt = temporalTiles(c), np = (size_t)c->W * c->H;
  if (int rc = ensureDenoiseWork(c)) return rc;
  const DenoiseWork w = denoiseWork(c);  // sail_denoise's work buffers; the count of temporal pixels sits behind the moments
  uint32_t* dTmp = (uint32_t*)((char*)c->tpMom + np * 48);
  SailTfilterPrepareArgs A;
  memset(&A, 0, sizeof A);
  A.Out = c->tpOut; A.Mout = c->tpMout; A.S = shownAccum(c); A.N = shownAovN(c); A.X = shownAovP(c);
  A.cv = w.cv[0]; A.g0 = w.g0; A.g1 = w.g1; A.tileBad = w.bad; A.tileTemporal = dTmp;
  A.W = c->W; A.H = c->H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k;
  A.minHist = p.min_hist;
  const float sx2 = p.sigma_x * 2.0f;
  A.sx0 = sx2 * sx2;
  float ms[8] = {}, total = 0.0f;
  int rc = SAIL_OK;
  SailTfilterPrepareDemodArgs D;
  memset(&D, 0, sizeof D);
  D.P = A; D.alb = c->albMap; D.amin = amin;
  hipError_t e = runAtrous(c, w, [&] { return demod ? sail_launch_tfilter_prepare_demod(D, c->stream)
                                                      : sail_launch_tfilter_prepare(A, c->stream); },
                           p.iterations, p.sigma_l, p.sigma_x, p.display, p.gamma_c, out_rgba, out_var, out_rgba8, ms, &total,
                           &rc, demod ? c->albMap : nullptr, amin);
  if (rc) return rc;
  std::vector<uint32_t> bad(nt), tmp(nt);
  if (e == hipSuccess) e = hipMemcpy(bad.data(), w.bad, nt * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(tmp.data(), dTmp, nt * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "%s: %s", who, hipGetErrorString(e));
  if (info) {
    memset(info, 0, sizeof *info);
    info->k = c->k;
    info->temporal_pixels = sumTiles(tmp, 0, nt);
    info->spatial_pixels = (uint64_t)np - info->temporal_pixels;
    info->nonfinite = sumTiles(bad, 0, nt);
    info->iterations = p.iterations;
    info->kernel_ms = total;
    for (int i = 0; i <= p.iterations; i++) info->pass_ms[i] = ms[i];
  }
  return SAIL_OK;
}

uint32_t* albedoCounts(const sail_ctx* c) { return (uint32_t*)(c->albMap + (size_t)c->W * c->H); }

// the albedo map and its two counts per tile, allocated on first use
int ensureAlbedo(sail_ctx* c) {
  return allocOnce(c, &c->albMap, (size_t)c->W * c->H * 16 + temporalTiles(c) * 8, "albedo map");
}

void albedoView(sail_ctx* c, const double mvp[16], const float eye[3]) {
  memset(&c->albView, 0, sizeof c->albView);
  for (int i = 0; i < 16; i++) c->albView.m[i] = (float)mvp[i];
  memcpy(c->albView.eye, eye, sizeof c->albView.eye);
}

}  // namespace

extern "C" {

int sail_temporal_filter(sail_ctx* c, const sail_tfilter_params* params, float* out_rgba, float* out_var,
                         uint8_t* out_rgba8, sail_tfilter_info* info) {
  return tfilterCall(c, "sail_temporal_filter", false, params, 0.0f, out_rgba, out_var, out_rgba8, info);
}

int sail_temporal_filter_albedo(sail_ctx* c, const sail_tfilter_params* params, float amin, float* out_rgba, float* out_var,
                                uint8_t* out_rgba8, sail_tfilter_info* info) {
  return tfilterCall(c, "sail_temporal_filter_albedo", true, params, amin, out_rgba, out_var, out_rgba8, info);
}

// ---- the albedo map of a view (include/sail_hip.h; the kernel is sail_albedo.hip) ----------------------------------------------
int sail_albedo(sail_ctx* c, const double mvp[16], const float eye[3], int grid, float* out_rgba, sail_albedo_info* info) {
  if (grid < 1 || grid > 4) return fail(c, SAIL_E_INVALID, "sail_albedo: grid %d of 1..4", grid);
  if (!c) return fail(c, SAIL_E_INVALID, "sail_albedo: a context is required");
  if (!mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_albedo: mvp and eye are required");
  if (!c->subs.empty()) return relay(c, sail_albedo(c->subs[0], mvp, eye, grid, out_rgba, info), c->subs[0]);
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_albedo: no scene (call sail_set_scene first)");
  SailGbufferArgs G;
  if (int rc = gbufferArgs(c, "sail_albedo", mvp, eye, &G)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (int rc = ensureAlbedo(c)) return rc;
  const size_t nt = temporalTiles(c), np = (size_t)c->W * c->H;
  SailAlbedoArgs A;
  memset(&A, 0, sizeof A);
  A.prims = c->prims; A.texparams = c->tp; A.n = c->n; A.tn = c->tn;
  A.texMask = c->plugins.texture_mask;
  memcpy(A.d, G.d, sizeof A.d);
  memcpy(A.eye, eye, sizeof A.eye);
  A.W = c->W; A.H = c->H; A.grid = grid;
  A.A = c->albMap;
  A.tileHit = albedoCounts(c); A.tilePartial = A.tileHit + nt;
  c->albHave = false;  // a call that fails leaves no map
  PooledEvents ev(c, 2);
  if (ev.rc) return ev.rc;
  float ms = 0.0f;
  hipError_t e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = sail_launch_albedo(A, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = hipMemcpy(host.data(), A.tileHit, nt * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_rgba) e = hipMemcpy(out_rgba, c->albMap, np * 16, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_albedo: %s", hipGetErrorString(e));
  albedoView(c, mvp, eye);
  c->albHave = true;
  if (info) {
    memset(info, 0, sizeof *info);
    info->hit_pixels = sumTiles(host, 0, nt);
    info->partial_pixels = sumTiles(host, nt, nt);
    info->grid = grid;
    info->kernel_ms = ms;
  }
  return SAIL_OK;
}

int sail_albedo_load(sail_ctx* c, const float* map, const double mvp[16], const float eye[3]) {
  if (!c) return SAIL_E_INVALID;
  if (!map || !mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_albedo_load: map, mvp and eye are required");
  if (!c->subs.empty()) return relay(c, sail_albedo_load(c->subs[0], map, mvp, eye), c->subs[0]);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = ensureAlbedo(c)) return rc;
  HIPCHK(c, hipMemcpy(c->albMap, map, (size_t)c->W * c->H * 16, hipMemcpyHostToDevice));
  albedoView(c, mvp, eye);
  c->albHave = true;
  return SAIL_OK;
}

int sail_albedo_read(sail_ctx* c, float* out) {
  if (!c) return SAIL_E_INVALID;
  if (!out) return fail(c, SAIL_E_INVALID, "sail_albedo_read: an output is required");
  if (!c->subs.empty()) return relay(c, sail_albedo_read(c->subs[0], out), c->subs[0]);
  if (!c->albHave || !c->albMap)
    return fail(c, SAIL_E_STATE, "sail_albedo_read: no albedo map (sail_albedo or sail_albedo_load first; new rows drop it)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->albMap, (size_t)c->W * c->H * 16, hipMemcpyDeviceToHost));
  return SAIL_OK;
}

int sail_accum_device_ptr(sail_ctx* c, void** ptr, size_t* bytes) {
  if (!c || !ptr || !bytes) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_accum_device_ptr(c->subs[0], ptr, bytes), c->subs[0]);
  if (int rc = flushQueued(c)) return rc;  // the sums the caller's collective will read are queued on this stream
  *ptr = c->accum;
  *bytes = (size_t)c->W * c->H * sizeof(float4);
  return SAIL_OK;
}

int sail_comm_unique_id(char id[128]) {
  if (!id) return SAIL_E_INVALID;
  if (!g_rccl.load()) return fail(nullptr, SAIL_E_RCCL, "librccl not loadable");
  nccl_uid_t u;
  const int r = g_rccl.getUniqueId(&u);
  if (r) return fail(nullptr, SAIL_E_RCCL, "ncclGetUniqueId: %d", r);
  memcpy(id, u.internal, 128);
  return SAIL_OK;
}

int sail_comm_init(sail_ctx* c, const char id[128], int nranks, int rank) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return SAIL_E_INVALID;
  if (!c->subs.empty()) return fail(c, SAIL_E_STATE, "a multi-device context reduces over its own communicator");
  if (!g_rccl.load()) return fail(c, SAIL_E_RCCL, "librccl not loadable");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->comm) {  // a second init replaces the communicator
    HIPCHK(c, hipStreamSynchronize(c->stream));
    g_rccl.commDestroy(c->comm);
    c->comm = nullptr;
    c->commRanks = 0; c->commRank = 0;
  }
  nccl_uid_t u;
  memcpy(u.internal, id, 128);
  const int r = g_rccl.commInitRank(&c->comm, nranks, u, rank);
  if (r) return fail(c, SAIL_E_RCCL, "ncclCommInitRank: %s", g_rccl.errStr ? g_rccl.errStr(r) : "?");
  c->commRanks = nranks; c->commRank = rank;
  return SAIL_OK;
}

int sail_reduce(sail_ctx* c, int root) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (root != 0) return fail(c, SAIL_E_INVALID, "multi-device context: the frame is reduced into device 0");
    if (int rc = loadIncomplete(c, "sail_reduce")) return rc;
    c->dirty = true;  // reduce now even if nothing was rendered since the last one
    return groupReduce(c);
  }
  if (!c->comm) return fail(c, SAIL_E_STATE, "sail_reduce before sail_comm_init");
  if (root < 0 || root >= c->commRanks) return fail(c, SAIL_E_INVALID, "sail_reduce: root %d of %d ranks", root, c->commRanks);
  if (int rc = flushQueued(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const bool isRoot = c->commRank == root;
  const bool aov = c->aovN || c->aovP;
  // a sample split shows the AOVs of the rank that rendered the last sample: the others send -0 maps
  const bool own = planReduce(c->W, c->H, c->rank, c->world, c->partMode, c->k, root).send_own_aovs != 0;
  if (isRoot || (aov && !own)) { if (int rc = ensureFrame(c)) return rc; }
  const size_t np = (size_t)c->W * c->H, count = np * 4;
  if (aov && !own) {
    if (c->frameN) HIPCHK(c, fillNegZero(c->frameN, np, c->stream));
    if (c->frameP) HIPCHK(c, fillNegZero(c->frameP, np, c->stream));
  }
  // out of place into root's frame: every reduce sums the ranks' cumulative accumulators afresh
  float4* sendN = own ? c->aovN : c->frameN;
  float4* sendP = own ? c->aovP : c->frameP;
  int r = g_rccl.groupStart();
  if (r == 0) r = g_rccl.reduce(c->accum, isRoot ? c->frame : c->accum, count, kNcclFloat32, kNcclSum, root, c->comm, c->stream);
  if (r == 0 && c->aovN) r = g_rccl.reduce(sendN, isRoot ? c->frameN : sendN, count, kNcclFloat32, kNcclSum, root, c->comm, c->stream);
  if (r == 0 && c->aovP) r = g_rccl.reduce(sendP, isRoot ? c->frameP : sendP, count, kNcclFloat32, kNcclSum, root, c->comm, c->stream);
  const int r2 = g_rccl.groupEnd();
  if (r || r2) return fail(c, SAIL_E_RCCL, "ncclReduce: %s", g_rccl.errStr ? g_rccl.errStr(r ? r : r2) : "?");
  if (int rc = commCheck(c, c->comm)) return rc;
  c->reduced = isRoot;
  return SAIL_OK;
}

// ---- checkpoint / resume --------------------------------------------------------------------------------------------
int sail_accum_parts(sail_ctx* c, int* parts) {
  if (!c || !parts) return SAIL_E_INVALID;
  *parts = c->subs.empty() ? 1 : (int)c->subs.size();
  return SAIL_OK;
}

int sail_save_accum(sail_ctx* c, int part, float* sums, uint64_t* k) {
  if (!c || !sums || !k) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = loadIncomplete(c, "sail_save_accum")) return rc;
    if (part < 0 || part >= (int)c->subs.size()) return fail(c, SAIL_E_INVALID, "sail_save_accum: part %d of %d", part, (int)c->subs.size());
    return relay(c, sail_save_accum(c->subs[part], 0, sums, k), c->subs[part]);
  }
  if (part != 0) return fail(c, SAIL_E_INVALID, "sail_save_accum: part %d of 1", part);
  if (int rc = sail_sync(c)) return rc;
  HIPCHK(c, hipMemcpy(sums, c->accum, (size_t)c->W * c->H * sizeof(float4), hipMemcpyDeviceToHost));
  *k = c->k;
  return SAIL_OK;
}

int sail_load_accum(sail_ctx* c, int part, const float* sums, uint64_t k) {
  if (!c || !sums || k > (1ull << 53)) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    const int nd = (int)c->subs.size();
    if (part < -1 || part >= nd) return fail(c, SAIL_E_INVALID, "sail_load_accum: part %d of %d", part, nd);
    // one part of a checkpoint: the others must follow with the same k before the frame is used (sail_plan_load_part)
    uint64_t missing = c->loadMissing, loadK = c->loadK;
    if (planLoadPart(&missing, &loadK, nd, part, k) != SAIL_OK)
      return fail(c, SAIL_E_INVALID, "sail_load_accum: part %d has k %llu, the checkpoint being loaded %llu", part,
                  (unsigned long long)k, (unsigned long long)c->loadK);
    for (int i = 0; i < nd; i++) {  // part -1: each device keeps its share of the frame; else one part, every k
      if (part == -1 || part == i) {
        if (int rc = sail_load_accum(c->subs[i], part == -1 ? -1 : 0, sums, k)) return relay(c, rc, c->subs[i]);
      } else {
        c->subs[i]->k = k;
        c->subs[i]->maskSet = false;  // the tile mask goes on every device, as on the ones that load
        c->subs[i]->mask.clear();
        c->subs[i]->frozenAt.clear();
      }
    }
    c->loadMissing = missing;
    c->loadK = loadK;
    c->dirty = true;
    return SAIL_OK;
  }
  if (part != 0 && part != -1) return fail(c, SAIL_E_INVALID, "sail_load_accum: part %d of 1", part);
  if (part == -1 && c->world > 1 && c->partMode == SAIL_PART_SAMPLES && c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_INVALID, "sail_load_accum: a running mean cannot be split by samples");
  HIPCHK(c, hipSetDevice(c->device));
  const bool marked = c->noiseHave;
  if (int rc = resetAccum(c)) return rc;  // queued samples, stats and AOVs restart; the accumulator is replaced
  c->noiseHave = marked;  // a loaded checkpoint continues a render: the noise estimate's mark stays
  std::vector<float> mine;
  const float* src = sums;
  if (part == -1 && c->world > 1) {
    mine.resize((size_t)c->W * c->H * 4);
    keepPart(c->W, c->H, c->rank, c->world, c->partMode, sums, mine.data());
    src = mine.data();
  }
  HIPCHK(c, hipMemcpyAsync(c->accum, src, (size_t)c->W * c->H * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->k = k;
  // this rank's samples among 0 .. k-1 (every one, or those k' = rank mod world of a sample split)
  c->samplesThisRank = planReduce(c->W, c->H, c->rank, c->world, c->partMode, k, 0).samples;
  return SAIL_OK;
}

int sail_jit_compile(const sail_plugins* plugins, int mode, const int32_t* row_types, int rows, void* code,
                     size_t* bytes) {
  if (!plugins || !bytes || mode < SAIL_JIT_MODE_FLAT || mode > SAIL_JIT_MODE_ROOM || rows < 0 ||
      rows > kSailJitMaxRows || (rows > 0 && !row_types))
    return SAIL_E_INVALID;
  // the plugin set's precompiled family, as kernelSetFor decides it for a flat scene of these masks
  const sail_plugins& p = *plugins;
  int set = SAIL_KSET_GENERIC;
  if ((p.shape_mask & ~SAIL_KSET_CORNELL_SHAPES) == 0 && (p.material_mask & ~SAIL_KSET_CORNELL_MATS) == 0 &&
      (p.texture_mask & ~SAIL_KSET_CORNELL_TEX) == 0 && p.light_mask == 0)
    set = SAIL_KSET_CORNELL;
  else if ((p.shape_mask & ~SAIL_KSET_ROOM_SHAPES) == 0)
    set = SAIL_KSET_ROOM;
  SailJitSpec spec;
  spec.ks = p.shape_mask; spec.km = p.material_mask; spec.kt = p.texture_mask; spec.kl = p.light_mask;
  spec.mode = mode;
  spec.waves = jitWaves(mode, mode == SAIL_JIT_MODE_CULL ? SAIL_KSET_GENERIC : set);
  spec.rows = rows;
  for (int i = 0; i < rows; i++) spec.types[i] = row_types[i];
  std::string err;
  if (sail_jit_code("gfx950", spec, code, bytes, &err))
    return fail(nullptr, SAIL_E_INVALID, "sail_jit_compile: %s", err.c_str());
  return SAIL_OK;
}

int sail_jit_prebuild(const float* objects, int n, const float* texparams, int tn, const float* lights, int ln,
                      const sail_plugins* plugins, const char* arch, const char* dir, int* built) {
  if (n < 0 || tn < 0 || ln < 0 || (n > 0 && !objects) || (tn > 0 && !texparams) || (ln > 0 && !lights) || !plugins ||
      !arch || (n > 0 && tn < 1))
    return fail(nullptr, SAIL_E_INVALID, "sail_jit_prebuild: bad arguments");
  (void)lights;
  // the spec a context with the product's defaults derives for this scene (jitSpecFor), without a device
  sail_ctx t;
  t.plugins = *plugins;
  t.n = n; t.tn = tn; t.ln = ln;
  t.haveScene = true;
  std::vector<SailPrim> prims;
  int anyHit = 0;
  decodePrims(objects, n, tn, plugins->shape_mask, prims, &anyHit, nullptr);
  fillCats(prims, texparams, tn);  // the rows as sail_set_scene uploads them: the value kernel compiles them in
  for (const SailPrim& q : prims) t.primTypes.push_back(q.type);
  std::vector<uint32_t> rowWords((size_t)n * 32);
  if (n > 0) memcpy(rowWords.data(), prims.data(), sizeof(SailPrim) * (size_t)n);
  SailJitSpec spec;
  int mode = 0;
  if (built) *built = 0;
  if (!jitSpecFor(&t, &spec, &mode)) return SAIL_OK;  // the scene gets no run-time kernel
  std::string err;
  // the Cornell form in both shapes: 16 samples in flight (a large share of the frame) and 1 (a rank of 8, jitNsFor)
  const bool cornell = mode == SAIL_JIT_MODE_FLAT && kernelSetFor(&t) == SAIL_KSET_CORNELL;
  for (int ns : {16, 1}) {
    if (cornell) spec.ns = ns;
    if (sail_jit_code_to_dir(arch, spec, dir, &err)) return fail(nullptr, SAIL_E_INVALID, "sail_jit_prebuild: %s", err.c_str());
    // and the value kernel a context loads once the scene has settled, where the spec has one
    SailJitSpec vspec;
    if (valueSpecFor(spec, rowWords, texparams, tn, t.jit, &vspec) && sail_jit_code_to_dir(arch, vspec, dir, &err))
      return fail(nullptr, SAIL_E_INVALID, "sail_jit_prebuild: %s", err.c_str());
    if (!cornell) break;
  }
  if (built) *built = 1;
  return SAIL_OK;
}

int sail_plan_settle(uint64_t settled, int after) { return settledFor(settled, after) ? 1 : 0; }

int sail_jit_resident(int* code_objects, int* modules) {
  if (!code_objects || !modules) return SAIL_E_INVALID;
  sail_jit_resident_values(code_objects, modules);
  return SAIL_OK;
}

int sail_jit_value_key(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                       const char* arch, uint64_t* key, char* defs, size_t* defs_len) {
  return sail_jit_spec_key(objects, n, texparams, tn, plugins, arch, -1, 1, key, defs, defs_len);
}

int sail_jit_spec_key(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                      const char* arch, int jit, int value, uint64_t* key, char* defs, size_t* defs_len) {
  if (n < 1 || tn < 1 || !objects || !texparams || !plugins || !arch || !key)
    return fail(nullptr, SAIL_E_INVALID, "sail_jit_spec_key: bad arguments");
  // as sail_jit_prebuild: the spec a context with these switches (else the product's defaults) derives, without a device
  sail_ctx t;
  if (jit >= 0) t.jit = jit;
  t.plugins = *plugins;
  t.n = n; t.tn = tn;
  t.haveScene = true;
  std::vector<SailPrim> prims;
  int anyHit = 0;
  decodePrims(objects, n, tn, plugins->shape_mask, prims, &anyHit, nullptr);
  fillCats(prims, texparams, tn);
  for (const SailPrim& q : prims) t.primTypes.push_back(q.type);
  std::vector<uint32_t> rowWords((size_t)n * 32);
  memcpy(rowWords.data(), prims.data(), sizeof(SailPrim) * (size_t)n);
  SailJitSpec spec, vspec;
  int mode = 0;
  *key = 0;
  if (!jitSpecFor(&t, &spec, &mode) || (value && !valueSpecFor(spec, rowWords, texparams, tn, t.jit, &vspec))) {
    if (defs_len) *defs_len = 0;
    return SAIL_OK;  // the scene gets no such kernel
  }
  std::string text, err;
  if (sail_jit_key(arch, value ? vspec : spec, key, &text, &err))
    return fail(nullptr, SAIL_E_INVALID, "sail_jit_spec_key: %s", err.c_str());
  if (defs_len) {
    const size_t have = *defs_len;
    *defs_len = text.size() + 1;
    if (defs && have >= text.size() + 1) memcpy(defs, text.c_str(), text.size() + 1);
  }
  return SAIL_OK;
}

int sail_prim_bounds(const float* objects, int n, int tn, float* out) {
  if (n < 0 || (n > 0 && (!objects || !out))) return SAIL_E_INVALID;
  std::vector<SailPrim> prims;
  int anyHit = 0;
  decodePrims(objects, n, tn, ~0u, prims, &anyHit, nullptr);
  for (int i = 0; i < n; i++) {
    const SailPrim& p = prims[(size_t)i];
    for (int k = 0; k < 3; k++) {
      out[6 * i + k] = p.type ? p.a[18 + k] : INFINITY;
      out[6 * i + 3 + k] = p.type ? p.a[21 + k] : -INFINITY;
    }
  }
  return SAIL_OK;
}

int sail_plan_last_bounce(const float* objects, int n, const float* texparams, int tn, const sail_plugins* plugins,
                          int kernel_lights, uint32_t* quiet_rows, int* skip_sort) {
  if (n < 0 || tn < 0 || (n > 0 && !objects) || (tn > 0 && !texparams) || !plugins || !quiet_rows || !skip_sort ||
      (n > 0 && tn < 1))
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_last_bounce: bad arguments");
  std::vector<SailPrim> prims;
  int anyHit = 0;
  decodePrims(objects, n, tn, plugins->shape_mask, prims, &anyHit, nullptr);
  fillCats(prims, texparams, tn);
  lastBounceRows(prims, texparams, tn, plugins->material_mask, kernel_lights != 0, quiet_rows, skip_sort);
  return SAIL_OK;
}

int sail_partition_tiles(int width, int height, int rank, int world, int* out, int capacity) {
  if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || capacity < 0) return SAIL_E_INVALID;
  const int tx = (width + 63) / 64, ty = (height + 63) / 64;
  int count = 0;
  for (int t = rank; t < tx * ty; t += world) {
    if (out && count < capacity) {
      const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
      out[4 * count + 0] = x0;
      out[4 * count + 1] = y0;
      out[4 * count + 2] = (width - x0) < 64 ? (width - x0) : 64;
      out[4 * count + 3] = (height - y0) < 64 ? (height - y0) : 64;
    }
    count++;
  }
  return count;
}

int sail_plan_reduce(int width, int height, int rank, int world, int mode, uint64_t k, int root, sail_reduce_plan* out) {
  if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || !out ||
      (mode != SAIL_PART_TILES && mode != SAIL_PART_SAMPLES))
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_reduce: bad arguments");
  *out = planReduce(width, height, rank, world, mode, k, root);
  return SAIL_OK;
}

int sail_plan_keep(int width, int height, int rank, int world, int mode, const float* sums, float* out) {
  if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || !sums || !out ||
      (mode != SAIL_PART_TILES && mode != SAIL_PART_SAMPLES))
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_keep: bad arguments");
  keepPart(width, height, rank, world, mode, sums, out);
  return SAIL_OK;
}

int sail_plan_load_part(uint64_t* missing, uint64_t* k, int parts, int part, uint64_t k_part) {
  if (!missing || !k) return fail(nullptr, SAIL_E_INVALID, "sail_plan_load_part: bad arguments");
  if (int rc = planLoadPart(missing, k, parts, part, k_part))
    return fail(nullptr, rc, "sail_plan_load_part: part %d of %d (index %llu, checkpoint %llu)", part, parts,
                (unsigned long long)k_part, (unsigned long long)*k);
  return SAIL_OK;
}

int sail_math_probe(int fn, const float* x, const float* y, float* out, int count) {
  if (!x || !y || !out || count < 0) return SAIL_E_INVALID;
  if (count == 0) return SAIL_OK;
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  const size_t b = sizeof(float) * count;
  if (hipMalloc(&dx, b) != hipSuccess || hipMalloc(&dy, b) != hipSuccess || hipMalloc(&dout, b) != hipSuccess) {
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    return fail(nullptr, SAIL_E_OOM, "math probe buffers");
  }
  hipError_t e = hipMemcpy(dx, x, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dy, y, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    e = sail_launch_math(fn, dx, dy, dout, count);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, b, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dout);
  if (e != hipSuccess) return fail(nullptr, SAIL_E_HIP, "math probe: %s", hipGetErrorString(e));
  return SAIL_OK;
}

}  // extern "C"
