// sail_plan.cpp — the host's measured policy (sail_plan.h): every number here was bought with a benchmark round, and the
// comments say which. Pure functions of plain facts; tests/test_launch_plan.py states them through sail_plan_launch.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "sail_plan.h"

// nothing below may name the context (tests/test_launch_plan.py compiles this file alone)
#pragma GCC poison sail_ctx

const char* setSwitch(PlanSwitches* sw, int option, int value) {
  switch (option) {
    case SAIL_DEBUG_CULL_MIN_PRIMS: sw->cullMinPrims = value; break;
    case SAIL_DEBUG_FORCE_GENERIC: sw->forceGeneric = value; break;
    case SAIL_DEBUG_SAMPLE_GROUPS: sw->forceGroups = value; break;
    case SAIL_DEBUG_WAVEFRONT: sw->wavefront = value; break;
    case SAIL_DEBUG_JIT: sw->jit = value; break;
    case SAIL_DEBUG_JIT_NT:
      if (value != 0 && value != 128 && value != 256 && value != 512 && value != 1024)
        return "threads per workgroup must be 0 (default), 128, 256, 512 or 1024";
      sw->jitNt = value;
      break;
    case SAIL_DEBUG_JIT_NS:
      if (value != 0 && value != 1 && value != 4 && value != 16) return "samples in flight must be 0 (default), 1, 4 or 16";
      sw->jitNs = value;
      break;
    case SAIL_DEBUG_JIT_VALUES_AFTER: sw->jitValuesAfter = value; break;
    case SAIL_DEBUG_GROUP_ROUNDS:
      if (value <= 0) return "group rounds must be > 0";
      sw->flatGroupRounds = value;
      break;
    case SAIL_DEBUG_CULL_GROUP_ROUNDS:
      if (value <= 0) return "group rounds must be > 0";
      sw->cullGroupRounds = value;
      break;
    default: return "unknown option";
  }
  return nullptr;
}

// the Cornell box's own plugin set (cubes, spheres, the box; matte and mirror; no textures, no light plugin)
bool cornellSet(uint32_t ks, uint32_t km, uint32_t kt, uint32_t kl) {
  return (ks & ~SAIL_KSET_CORNELL_SHAPES) == 0 && (km & ~SAIL_KSET_CORNELL_MATS) == 0 && (kt & ~SAIL_KSET_CORNELL_TEX) == 0 &&
         kl == 0;
}
// the smallest precompiled plugin-set kernel that covers the scene (sail_device.h SAIL_KSET_*)
// (the Cornell kernel samples no light: it serves scenes without light rows, whatever light plugins their mask names)
int kernelSetFor(const SceneFacts& f, const PlanSwitches& sw) {
  if (sw.forceGeneric || f.n >= sw.cullMinPrims) return SAIL_KSET_GENERIC;
  const sail_plugins& p = f.plugins;
  if (f.ln == 0 && cornellSet(p.shape_mask, p.material_mask, p.texture_mask, 0u)) return SAIL_KSET_CORNELL;
  if ((p.shape_mask & ~SAIL_KSET_ROOM_SHAPES) == 0) return SAIL_KSET_ROOM;
  return SAIL_KSET_GENERIC;
}

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
int partitionTiles(const ShareFacts& sh, int* tilesX, int* tilesY) {
  const int tx = (sh.W + 63) / 64, ty = (sh.H + 63) / 64;
  *tilesX = tx; *tilesY = ty;
  if (sh.partMode == SAIL_PART_SAMPLES) return tx * ty;
  const int total = tx * ty;
  return sh.rank < total ? (total - sh.rank + sh.world - 1) / sh.world : 0;
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
// residency rounds of 512-thread workgroups at 8 waves per SIMD (4,096 / 32 pixels = 128 workgroups per tile)
double shareRounds(int tiles, int numCUs) { return (double)tiles * 128.0 / ((double)numCUs * 4.0); }
int jitNsFor(const ShareFacts& sh, int mode, int kernelSet) {
  if (mode == SAIL_JIT_MODE_FLAT && kernelSet == SAIL_KSET_CORNELL) {
    int tx, ty;
    return shareRounds(partitionTiles(sh, &tx, &ty), sh.numCUs) >= kCornellMinRounds ? 16 : 1;
  }
  if (mode == SAIL_JIT_MODE_ROOM || mode == SAIL_JIT_MODE_CULL) return 4;
  return 1;
}
int jitNtFor(int mode, int kernelSet) {
  return (mode == SAIL_JIT_MODE_FLAT && kernelSet == SAIL_KSET_CORNELL) ? 512 : 0;
}
// The run-time kernel spec of a scene under the switches, for a share of the frame, or false when none applies.
// SAIL_DEBUG_JIT bits (include/sail_hip.h): 1 flat scenes outside the Cornell and room sets, 2 pre-cull scenes, 4 room-set
// scenes, 8 the flat scenes of bit 1 in the room form, 16 flat scenes compiled for their rows as well (any flat scene),
// 32 the row-shading form of the value kernel (valueSpecFor), 64 the value kernel without its deferred Sphere row.
bool jitSpecFor(const SceneFacts& f, const PlanSwitches& sw, const ShareFacts& sh, SailJitSpec* out, int* mode) {
  if (!sw.jit || sw.forceGeneric) return false;
  const int set = kernelSetFor(f, sw);
  const bool rows = (sw.jit & 16) && f.n >= 1 && f.n <= kSailJitMaxRows && f.n < sw.cullMinPrims &&
                    (int)f.primTypes.size() == f.n;
  int m;
  if (set == SAIL_KSET_GENERIC && f.n >= sw.cullMinPrims) {
    if (!(sw.jit & 2)) return false;
    m = SAIL_JIT_MODE_CULL;
  } else if (set == SAIL_KSET_GENERIC) {
    if (!(sw.jit & 1) && !rows) return false;
    m = (sw.jit & 8) ? SAIL_JIT_MODE_ROOM : SAIL_JIT_MODE_FLAT;
  } else if (set == SAIL_KSET_ROOM) {
    if (!(sw.jit & 4) && !rows) return false;
    m = SAIL_JIT_MODE_ROOM;
  } else {
    if (!rows) return false;  // the Cornell kernel's set is the Cornell box's own
    m = SAIL_JIT_MODE_FLAT;
  }
  const sail_plugins& p = f.plugins;
  SailJitSpec spec;
  spec.ks = p.shape_mask; spec.km = p.material_mask; spec.kt = p.texture_mask; spec.kl = p.light_mask;
  spec.mode = m;
  spec.waves = jitWaves(m, set);
  spec.ldsFit = (m == SAIL_JIT_MODE_CULL && f.n <= SAIL_CULL_LDS_ROWS && f.tn <= SAIL_CULL_LDS_TP) ? 1 : 0;
  spec.ns = sw.jitNs ? sw.jitNs : jitNsFor(sh, m, set);
  spec.nt = sw.jitNt ? sw.jitNt : jitNtFor(m, set);
  if (sailJitThreads(spec) / spec.ns < 16) spec.ns = 4;  // at least 16 pixels per workgroup
  if (rows && m != SAIL_JIT_MODE_CULL) {
    spec.rows = f.n;
    for (int i = 0; i < f.n; i++) spec.types[i] = f.primTypes[i];
    for (int i = 0; i < f.n; i++)
      if (spec.types[i] < 1 || !((spec.ks >> spec.types[i]) & 1u)) spec.rows = 0;  // a row no compiled shape hits
    if (!spec.rows) for (int& t : spec.types) t = 0;
    // the room form copies both tables into LDS (C3 +2.8 %, UI +2.2 %; the Cornell form measured -0.5 %)
    if (spec.rows && m == SAIL_JIT_MODE_ROOM && f.tn >= 1 && f.tn <= kSailJitMaxFlatTp) spec.tn = f.tn;
  }
  *out = spec;
  *mode = m;
  return true;
}
// Whether the value kernel of a scene that rendered `settled` samples since its rows changed is asked for now
// (sail_plan_settle; after: SAIL_DEBUG_JIT_VALUES_AFTER)
bool settledFor(uint64_t settled, int after) { return after >= 0 && settled >= (uint64_t)after; }
// What a path's last bounce can add at a hit on each row (SailTraceArgs.lastQuietRows / lastSkipSort), decided with
// the kernel's own tests and f32 operations on the values it reads (sail_shade.h shadeLast: emission, matCat,
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
  constexpr float kEps = 1e-5f, kInvPI = 0.3183098861837907f;  // sail_geom.h
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
// (SAIL_JIT_ROWSHADE in sail_geom.h); bit 64 (inverted: the default leaves it clear) takes the deferred Sphere row away.
bool valueSpecFor(const SailJitSpec& types, const std::vector<uint32_t>& rowWords, const float* tp, int tn, int jit, SailJitSpec* out) {
  if (!cornellSet(types.ks, types.km, types.kt, types.kl) || types.mode != SAIL_JIT_MODE_FLAT || types.rows <= 0 ||
      types.tn != 0 || tn < 0 || tn > kSailJitMaxFlatTp || rowWords.size() != (size_t)types.rows * 32 || (tn > 0 && !tp))
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
  // The scene's first Sphere row is deferred (its root solve runs after the path sort, SAIL_JIT_ROWDEFER in sail_geom.h),
  // whatever the row-shading switch and the row count; bit 64 asks for the kernel without it.
  out->rowDefer = -1;
  if (!(jit & 64))
    for (int i = types.rows - 1; i >= 0; i--)
      if (types.types[i] == SAIL_SPHERE) out->rowDefer = i;
  return true;
}
// Samples per launch when the host has not fixed them: the Cornell form holding 16 samples in flight runs a whole
// 1,024-sample frame in one launch (its waves live 16 times longer, so their per-wave start -- the spill stores of the
// loop-invariant registers among it -- is paid 16 times less often: C1 Gseg/s at 64 / 128 / 256 / 1,024 samples per
// launch 97.26 / 97.73 / 97.99 / 98.36, profiles/r05_launch_*.jsonl); everything else 64 (sample groups stage a launch's
// samples, which a larger launch would push past the stage's cap).
int launchSamples(const PlanSwitches& sw, const SailJitSpec* types) {
  if (sw.launchSpp > 0) return sw.launchSpp;
  return (types && types->ns >= 16) ? 1024 : 64;
}
bool wavefrontFor(const SceneFacts& f, const PlanSwitches& sw) {
  return sw.wavefront && kernelSetFor(f, sw) == SAIL_KSET_GENERIC && f.n >= sw.cullMinPrims;
}

LaunchPlan planLaunch(const SceneFacts& f, const PlanSwitches& sw, const ShareFacts& sh, const LaunchChunk& k) {
  LaunchPlan P;
  const int owned = k.owned, nspp = k.nspp;
  // The stage holds 12 B per owned pixel per staged sample. It is capped (kStageCapBytes): a launch that would need
  // more runs one workgroup per block (no stage).
  const long long stageStride = (long long)owned * 4096;
  const int stageSpp = (int)std::max<long long>(1, (long long)(kStageCapBytes / ((size_t)stageStride * 12)));
  P.cullPrims = f.n >= sw.cullMinPrims ? (k.cullFmaOk ? 2 : 1) : 0;
  P.cullPrimary = k.eyeNearScene ? 1 : 0;
  P.kernelSet = kernelSetFor(f, sw);
  // Sample groups: a rank's share of a small frame is too few workgroups to fill the device (1/8 of 1080p
  // = 1,016 workgroups = 4 waves per SIMD); split the launch's samples over G workgroups per block so
  // that about 4 rounds of 7-wave-per-SIMD residency are queued, and add the staged samples in order.
  P.wavefront = wavefrontFor(f, sw);
  const SailJitSpec* run = P.wavefront ? nullptr : k.run;  // none under the wavefront switch
  // samples of each pixel in flight per workgroup (the run-time kernels' spec; the precompiled kernels hold one):
  // NS times the workgroups of one sample in flight, each NS times shorter
  const int ns = run ? run->ns : 1;
  P.ns = ns;
  // the last bounce's row classes for the light plugins compiled into the kernel that runs (shadeLast's kLights)
  P.kernelLights = run ? run->kl != 0u : P.kernelSet != SAIL_KSET_CORNELL;
  int G = 1;
  if (sw.forceGroups > 0) {
    G = sw.forceGroups;
  } else if (P.kernelSet == SAIL_KSET_GENERIC && P.cullPrims) {
    // The pre-cull kernel's workgroups are 1,024 threads, two per CU at 8 waves per SIMD. Its per-workgroup cost
    // varies with the primitives a 16x64 strip sees, so a grid of few rounds ends in a long tail (1/8 of C4: 1,020
    // workgroups = 2 rounds, 0.92 of the one-GPU rate per GPU): below 6 rounds, split the samples so that about 8
    // rounds are queued (the grouped kernel is 1,024 threads too; measured 0.95 at N = 8 with 4 groups).
    // Round 3: more groups pay at any frame size (a shorter tail per launch); C4 at N = 1: G = 1 / 2 / 4 9.96 / 10.06
    // / 10.12 Gseg/s (gpurun_out/r03o), so about SAIL_CULL_GROUP_ROUNDS rounds are queued.
    const double rounds = (double)owned * 4.0 * ns / (double)(sh.numCUs * 2);
    if (rounds < (double)sw.cullGroupRounds) G = (int)ceil((double)sw.cullGroupRounds / rounds);
  } else {
    // Round 3: splitting pays at full frame size too (shorter launch tails): C2 at N = 1 with G = 1 / 2 / 4 / 8 / 16
    // 89.3 / 89.7 / 90.9 / 91.6 / 91.4 Gseg/s, C5 87.0 / 89.3 / 90.9 / 91.6 / 91.9, C3 29.2 / 28.6 / 29.2 / 29.5 / 29.4;
    // at N = 8 (C2) G = 8 / 16 / 32 85 / 87 / 88 (gpurun_out/r03o). About 36 rounds of 7-wave residency are queued.
    const long long waves = (long long)owned * 16 * 4 * ns;
    const long long target = (long long)sh.numCUs * 4 * 7 * sw.flatGroupRounds;
    G = (int)((target + waves - 1) / waves);
    // the Cornell form holds 16 samples in flight only while its share queues enough workgroups (jitNsFor), and then
    // runs unsplit: staged groups lost 2-3 % per GPU at N = 4 and 8 (profiles/r05_scale_groups_c2.jsonl)
    // (under a tile mask that leaves too few active tiles for that, the kernel still holds its 16 samples, so the launch
    // is split after all: rate_by_active_tiles against rate_by_active_tiles_unsplit in profiles/adaptive_1080p.json)
    const bool fewActive = k.masked && shareRounds(owned, sh.numCUs) < kCornellMinRounds;
    if (ns >= 16 && !fewActive) G = 1;
  }
  if (G > nspp) G = nspp;
  if (G < 1) G = 1;
  if (nspp > stageSpp) G = 1;  // the stage would pass its cap
  P.groupSpp = (nspp + G - 1) / G;
  // whole steps of the workgroup's samples in flight: a group of 11 samples at 4 in flight would idle a quarter of
  // the lanes in its last step (C4 per GPU at N = 2 and 4: 12.6 Gseg/s against 13.4, profiles/r05_scale_groups_c4.jsonl)
  if (ns > 1 && P.groupSpp < nspp && sw.forceGroups <= 0) P.groupSpp = ((P.groupSpp + ns - 1) / ns) * ns;
  P.sampleGroups = (nspp + P.groupSpp - 1) / P.groupSpp;
  P.groupHome = (run ? run->mode == SAIL_JIT_MODE_ROOM : SAIL_GROUP_HOME_FOR(P.kernelSet)) ? 1 : 0;
  if (P.wavefront) {  // one sample per pass, straight into the accumulator
    P.sampleGroups = 1; P.groupSpp = nspp;
  }
  P.staged = P.sampleGroups > 1;
  if (P.wavefront) {
    P.grid = (unsigned)owned * 16u; P.threads = 256u;  // sail_launch_wavefront: 4,096 slots per owned tile
  } else if (run) {
    const unsigned nt = (unsigned)sailJitThreads(*run);
    const unsigned px = nt / (unsigned)ns;                            // pixels per workgroup
    P.grid = (unsigned)owned * (4096u / px) * (unsigned)P.sampleGroups; P.threads = nt;
  } else {
    P.grid = (unsigned)(owned * 16 * P.sampleGroups);
    P.threads = (P.kernelSet == SAIL_KSET_GENERIC && P.cullPrims) ? 1024u : 256u;  // sail_trace_sets.hip SAIL_*_NT
  }
  return P;
}
