// sail_plan.h — the host's measured policy as pure functions of plain facts (sail_plan.cpp): which precompiled kernel set
// and which run-time kernel spec a scene gets, the samples in flight, the samples per launch, and the shape of one trace
// launch. No context, no device, no HIP call: sail_capi.cpp feeds them from a sail_ctx, the device-free entry points
// (sail_jit_prebuild, sail_jit_spec_key, sail_jit_compile, sail_plan_launch) from their arguments.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include <hip/hip_runtime.h>  // float4, hipFunction_t: the types of the two headers below, no call
#include "../../include/sail_hip.h"
#include "sail_device.h"
#include "sail_jit.h"

// what the policy reads of a scene (sail_set_scene's counts and plugin masks, and the decoded rows' shape ids)
struct SceneFacts {
  sail_plugins plugins{};
  int n = 0, tn = 0, ln = 0;
  std::vector<int> primTypes;  // decoded shape id of each row (run-time kernels compiled for the scene's rows)
};

// the switches of sail_set_debug and sail_set_launch_samples that the policy reads, with the product's defaults
struct PlanSwitches {
  int jit = 59;  // SAIL_DEBUG_JIT bits: which scenes get a run-time kernel (jitSpecFor; instrumented in the phase build)
  int cullMinPrims = 8;  // scenes with at least this many primitives use the padded-box pre-cull
  int forceGeneric = 0;  // SAIL_FORCE_GENERIC=1: always launch the all-plugin kernel (tests)
  int jitNs = 0;  // SAIL_DEBUG_JIT_NS: samples in flight of the run-time kernels (0: the form's default, jitNsFor)
  int jitNt = 0;  // SAIL_DEBUG_JIT_NT: threads per workgroup of the run-time kernels (0: the form's own)
  int forceGroups = 0;   // SAIL_SAMPLE_GROUPS=g: fixed sample-group count (tests); 0 = by occupancy
  int flatGroupRounds = 36;  // sample groups: residency rounds queued per launch (flat kernels, SAIL_DEBUG_GROUP_ROUNDS)
  int cullGroupRounds = 64;  // the same for the pre-cull kernel's 1,024-thread workgroups
  int wavefront = 0;     // SAIL_DEBUG_WAVEFRONT: the pre-cull path by the wavefront split (study)
  // samples per launch (sail_set_launch_samples); 0 = by form (launchSamples): 64 measured C2 +0.7 %, C3 +0.5 %, C4/C5
  // +-0.2 % over 32 (profiles/r04_launch_spp*)
  int launchSpp = 0;
  // SAIL_DEBUG_JIT_VALUES_AFTER: 0 at once, < 0 never; 256 is a policy value, not tuned -- it only has to keep scenes in
  // motion and few-sample renders from compiling (settledFor)
  int jitValuesAfter = 256;
};
// One of the sail_set_debug options above into `sw`, checked as sail_set_debug checks it: null, or why the value is
// refused (an option that is no switch of the policy is refused as unknown)
const char* setSwitch(PlanSwitches* sw, int option, int value);

// a context's share of the frame and the device it runs on
struct ShareFacts {
  int W = 0, H = 0;
  int rank = 0, world = 1, partMode = SAIL_PART_TILES;
  int numCUs = 256;
};

// A share on either side of kCornellMinRounds for the callers that have no frame (sail_jit_prebuild builds the kernels of
// both, sail_jit_spec_key reports the small one's): no tiles at all, and a whole 1080p frame on 256 CUs
inline ShareFacts smallShare() { return ShareFacts{}; }
inline ShareFacts largeShare() {
  ShareFacts sh;
  sh.W = 1920; sh.H = 1080;
  return sh;
}

bool cornellSet(uint32_t ks, uint32_t km, uint32_t kt, uint32_t kl);
int kernelSetFor(const SceneFacts& f, const PlanSwitches& sw);
// the sample-group stage's cap (12 B per owned pixel per staged sample): 8 GiB
constexpr size_t kStageCapBytes = (size_t)8 << 30;
int jitWaves(int mode, int kernelSet);
int partitionTiles(const ShareFacts& sh, int* tilesX, int* tilesY);
// The Cornell form holds 16 samples in flight, and its launch runs unsplit, while the tiles it traces queue at least this
// many residency rounds (shareRounds): jitNsFor asks it of the share, planLaunch of the tiles a mask leaves active
constexpr double kCornellMinRounds = 12.0;
double shareRounds(int tiles, int numCUs);
int jitNsFor(const ShareFacts& sh, int mode, int kernelSet);
int jitNtFor(int mode, int kernelSet);
bool jitSpecFor(const SceneFacts& f, const PlanSwitches& sw, const ShareFacts& sh, SailJitSpec* out, int* mode);
bool settledFor(uint64_t settled, int after);
void lastBounceRows(const std::vector<SailPrim>& prims, const float* tp, int tn, uint32_t matMask, bool lights,
                    uint32_t* quietRows, int* skipSort);
bool valueSpecFor(const SailJitSpec& types, const std::vector<uint32_t>& rowWords, const float* tp, int tn, int jit,
                  SailJitSpec* out);
// types: the spec of the scene's run-time kernel while the context holds one whose build has not failed, else null
int launchSamples(const PlanSwitches& sw, const SailJitSpec* types);
// whether launches of the scene go by the wavefront split (no run-time kernel runs then)
bool wavefrontFor(const SceneFacts& f, const PlanSwitches& sw);

// One launch of launchTrace: nspp samples over `owned` tiles (the share's, or under a tile mask its active ones)
struct LaunchChunk {
  int nspp = 0, owned = 0;
  bool masked = false;        // a tile mask is set
  bool cullFmaOk = false;     // the fused pre-cull form is safe for this eye and scene (sail_capi.cpp cullFmaOk)
  bool eyeNearScene = false;  // primary rays may use the pre-cull (sail_capi.cpp eyeNearScene)
  const SailJitSpec* run = nullptr;  // the run-time kernel that will run, or null: the precompiled kernel of the set
};
struct LaunchPlan {
  int kernelSet = 0;     // SAIL_KSET_*
  int cullPrims = 0;     // 0 flat, 1 the plain pre-cull form, 2 the fused one
  int cullPrimary = 0;
  bool wavefront = false;
  int ns = 1;            // samples of each pixel in flight per workgroup
  int sampleGroups = 1, groupSpp = 0, groupHome = 0;
  bool staged = false;   // the groups' samples go through the stage and sail_accum_kernel adds them
  // a run-time kernel: `grid` workgroups of `threads`; a precompiled kernel: `grid` counts 256-thread blocks, as
  // sail_launch_trace takes them (it launches grid * 256 / threads workgroups of `threads`); the wavefront split: every
  // pass of sail_launch_wavefront
  unsigned grid = 0, threads = 0;
  bool kernelLights = false;  // the kernel has a light plugin compiled in: indexes sail_ctx.lastQuietRows / lastSkipSort
};
LaunchPlan planLaunch(const SceneFacts& f, const PlanSwitches& sw, const ShareFacts& sh, const LaunchChunk& k);
