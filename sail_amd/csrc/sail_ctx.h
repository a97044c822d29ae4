// sail_ctx.h — what the host files of libsail_hip.so share: the context, its run-time-kernel slot, the error, allocation
// and event helpers, and the launch wrappers defined beside the kernels. Internal; the C ABI is include/sail_hip.h.
//   sail_capi.cpp      context life cycle, scene decode and upload, the kernel slots, render, readback, filter, pick
//   sail_plan.cpp      kernel choice and launch shape as pure functions of plain facts (sail_plan.h; no context, no HIP)
//   sail_multi.cpp     RCCL binding, multi-device reduce, checkpoint parts
//   sail_converge.cpp  noise estimate, render-until, tile mask, adaptive sampling
//   sail_post.cpp      a-trous denoiser, reprojection, moment tracking, temporal filter, albedo map, guide maps
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/sail_hip.h"
#include "sail_device.h"

// launch wrappers defined next to the kernels (sail_trace_sets.hip, sail_wavefront.hip, sail_frame.hip)
hipError_t sail_launch_trace(const SailTraceArgs& A, int blocks, hipStream_t s);
// sail_jit.cpp: the trace kernel pair compiled at run time for exactly one plugin set (on the current device)
#include "sail_jit.h"
#include "sail_plan.h"
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
// sail_guides.hip: the guide maps of a view
#include "sail_guides.h"
hipError_t sail_launch_guides(const SailGuidesArgs& A, hipStream_t s);

// what follows is shared between the host files only: none of it is exported from the library
#pragma GCC visibility push(hidden)

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
extern Rccl g_rccl;  // sail_multi.cpp

// union of the primitives' finite bounds and its diagonal (sceneBox)
struct SceneBox { double lo[3], hi[3]; double diag; };
// the view a map of sail_post.cpp belongs to (setView, sameView): P*MV in f32, row-major, and the eye
struct View { float m[16]; float eye[3]; };

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
  int device = 0;
  // what the policy of sail_plan.h reads: the scene (counts, plugin masks, row shape ids), the switches, the share
  SceneFacts facts;
  PlanSwitches sw;
  ShareFacts share;
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
  bool haveScene = false;
  int shadowAnyHit = 0;
  // the rows' last-bounce classes (lastBounceRows) for a kernel without ([0]) and with ([1]) a light plugin compiled in,
  // re-derived whenever the rows are decoded (sail_set_scene, sail_update_objects: texParams and plugin masks change
  // only with the former); launchTrace passes the pair of the kernel it launches
  uint32_t lastQuietRows[2] = {0u, 0u};
  int lastSkipSort[2] = {0, 0};
  std::vector<unsigned long long> typeMasksHost;  // staging for the per-chunk type masks (async copy source)
  int lastGroups = 1;         // the last trace launch: sample groups (sail_kernel_name)
  bool lastWavefront = false;
  int cullFma = 1;       // SAIL_CULL_FMA=0: always the plain pre-cull form (tests)
  double primExtent = INFINITY;  // largest |padded bound| coordinate (inf: some primitive is unbounded)
  SceneBox scene{};              // union of the primitives' finite bounds (padPrimBounds)
  // The scene's run-time kernel (refreshJit), compiled for its plugin set and its rows' types. Until it is loaded the
  // precompiled kernel of the scene's set serves (same results); a launch waits up to jitWait ms for it
  // (SAIL_DEBUG_JIT_WAIT; -1 until it is built). Its error is the one sail_get_kernel_info reports.
  JitSlot typesSlot;
  int jitWait = 0;
  // The value kernel, a second tier on top of the scene's run-time kernel (refreshValues): the same spec with the rows'
  // and the texParams table's words compiled in, asked for once `settled` samples were rendered since the rows last
  // changed (rowsChanged in sail_capi.cpp, a new types spec; not sail_reset or the camera). A launch uses it when
  // it is loaded and never waits for it (sw.jitValuesAfter).
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
  float4* wf = nullptr;  // the wavefront split's path state: 11 float4 arrays of wfSlots
  size_t wfSlots = 0;
  float* stage = nullptr;    // sample-group staging, allocated on first use
  size_t stageBytes = 0;
  int accumMode = SAIL_ACCUM_SUM;
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
  // rowsChanged drops both unless its caller keeps them (sail_move_objects). On a multi-device context device
  // 0's sub-context holds it.
  void* tpWork = nullptr;
  float4 *tpGcur = nullptr, *tpGprev = nullptr, *tpHist = nullptr, *tpR = nullptr, *tpOut = nullptr;
  bool tpHaveCur = false, tpHavePrev = false;
  View tpCur{}, tpPrev{};
  uint64_t tpHitPixels = 0;
  // Moment tracking (sail_temporal_moments): one block of three float4 maps (mu1, mu2, mm, 0) and a count per tile,
  // allocated when tracking is switched on and freed when it is switched off; the pointers are swapped with the colour
  // maps'. tpResolved: the current view has been resolved (sail_temporal_filter needs its Out and Mout).
  void* tpMom = nullptr;
  float4 *tpMhist = nullptr, *tpMR = nullptr, *tpMout = nullptr;
  bool tpResolved = false;
  // Object motion pending for the next sail_temporal_begin (sail_move_objects): tpMotion is the table D, n rows of
  // (d.xyz, 0), the sum of the moves since the last begin; tpMotionCap is mc (+inf: none). tpMotionDev is D's device copy,
  // allocated on first use and uploaded by the begin that consumes it. rowsChanged (with the views) and
  // sail_temporal_load_history clear the pending state; on a multi-device context device 0's sub-context holds it.
  bool tpMotionPending = false;
  std::vector<float> tpMotion;
  float tpMotionCap = INFINITY;
  float4* tpMotionDev = nullptr;
  int tpMotionDevRows = 0;
  // Albedo map (sail_albedo / sail_albedo_load): one float4 map and two counts per 16x16 tile, allocated on first use,
  // with the view it belongs to, kept as the temporal views are. rowsChanged always invalidates it (the rows it shows
  // are gone); on a multi-device context device 0's sub-context holds it.
  float4* albMap = nullptr;
  bool albHave = false;
  View albView{};
  // Guide maps (sail_guides / sail_guides_load): two float4 maps (Ng, then Xg) and three counts per 16x16 tile in one
  // block, allocated on first use, with the view they belong to, kept and invalidated as the albedo map is. useGuides
  // (sail_use_guides): the four filters read them in the AOVs' place. On a multi-device context device 0's sub-context
  // holds both.
  float4* guideMaps = nullptr;
  bool guideHave = false;
  bool useGuides = false;
  View guideView{};
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

// sets the context's message (sail_last_error; a null context: the creating thread's) and returns `code` (sail_capi.cpp)
int fail(sail_ctx* c, int code, const char* fmt, ...);
// a multi-device context's call failed in one of its sub-contexts: carry that context's message up
inline int relay(sail_ctx* c, int rc, const sail_ctx* sub) {
  if (rc != SAIL_OK && sub && c != sub) c->err = sub->err;
  return rc;
}
// a part-wise checkpoint load still missing parts (sail_load_accum): refuse whatever would see the half-loaded frame
inline int loadIncomplete(sail_ctx* c, const char* what) {
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

// the context's pool of timing events (sail_capi.cpp): collectEvents adds up the launches that finished
int collectEvents(sail_ctx* c);
int getEvent(sail_ctx* c, hipEvent_t* ev);
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

// sail_capi.cpp
void cornerDirs(const float* M, const float* eye, float out[4][3]);
int resetAccum(sail_ctx* c);
int flushQueued(sail_ctx* c);
// sail_multi.cpp
int commCheck(sail_ctx* c, nccl_comm_t comm);
int groupCommCheck(sail_ctx* g);
int groupReduce(sail_ctx* g);
int reducedFrame(sail_ctx* g, const char* what);
// sail_post.cpp
hipError_t zeroMoments(sail_ctx* c);
void clearMotion(sail_ctx* c);
// the first-use buffers each file owns, freed by sail_destroy
void freeMulti(sail_ctx* c);
void freeConverge(sail_ctx* c);
void freePost(sail_ctx* c);

// the buffers readback / filter show: the last reduced frame while it is current, else this rank's own
inline const float4* shownAccum(const sail_ctx* c) { return c->reduced ? c->frame : c->accum; }
inline const float4* shownAovN(const sail_ctx* c) { return c->reduced && c->frameN ? c->frameN : c->aovN; }
inline const float4* shownAovP(const sail_ctx* c) { return c->reduced && c->frameP ? c->frameP : c->aovP; }
// the frame's pixels and its 16x16 tiles (the post passes keep a count or more per tile)
inline size_t pixels(const sail_ctx* c) { return (size_t)c->share.W * c->share.H; }
inline size_t tiles16(const sail_ctx* c) { return (size_t)((c->share.W + 15) / 16) * (size_t)((c->share.H + 15) / 16); }

#pragma GCC visibility pop
