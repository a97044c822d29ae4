// sail_trace.hip — the MI355X (gfx950) trace megakernel: the path loop (traceTileCompact) with its tile bookkeeping, and
// the macro that instantiates the trace kernels. This is the file a run-time compile includes (sail_jit.cpp); with
// SAIL_JIT defined it instantiates that one kernel pair, without it nothing: the precompiled plugin sets are
// sail_trace_sets.hip's. The shapes and hit records are in sail_geom.h, the shading in sail_shade.h. These files and
// the headers they include are the text embedded in the library (sail_amd/gen_jit_src.py) and hashed into every
// run-time kernel's cache key, so nothing a run-time kernel does not compile belongs in them.
//
// Re-implements the per-pixel loop of Sail's generated trace fragment program
// (src/shader/main/fstrace.glsl:6-17 -> trace/path.glsl:16-38 -> generated intersectObjects /
// material / light_sample / getSurfaceColor, shader.*.js).
//
// MI355X design:
//  * one lane = one pixel; a 256-thread workgroup covers a 16x16 pixel block, each wave a coherent 16x4 strip;
//    the grid walks only this rank's 64x64 partition tiles (interleaved t % world);
//  * all `spp` samples of a launch loop inside the lane with the radiance sum / running mean in
//    registers: HBM sees one float4 read + one float4 write per pixel per launch;
//  * the scene is decoded once on the host into 128-B primitive records; the primitive loop index is
//    wave-uniform, so every record field arrives through the scalar cache into SGPRs (no LDS copy, no
//    VGPRs), and material/texture/light rows are read with per-lane indices from L1/L2;
//  * intersectObjects is split into a t-only pass over all primitives and ONE full hit record
//    (normal, dpdu/dpdv, UV, texture) for the closest primitive; the reference builds the full record
//    for every primitive hit (shader.shape.js:44-50). The strict-`<`, first-index tie rule and every
//    f32 operation up to t are kept, so results are bit-identical to the oracle's restatement;
//  * per-sample camera corners and seeds arrive precomputed (SailSample, scalar loads);
//  * all f32 math follows the reference expression order with contraction off; transcendentals use
//    the bit-defined spec in sail_math.h.
#ifndef SAIL_TRACE_HIP
#define SAIL_TRACE_HIP
#if !defined(__HIPCC_RTC__)  // hipRTC (the per-plugin-set kernels, sail_jit.cpp) provides the HIP runtime and stdint
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "sail_device.h"
#include "sail_geom.h"
#include "sail_scan.h"
#include "sail_shade.h"

// Round 4 pruned every measured-and-rejected variant out of these files (their numbers stay in DESIGN.md §6 and
// profiles/r0*_variants_*.jsonl). What remains is what the four plugin-set kernels run; choices that differ between
// kernels are compile-time constants of the kernel template (CULL, KS, ...), not build switches. The one build switch
// left, SAIL_PHASE_TIMING, is instrumentation: tests/test_gpu_parity.py renders through its build too.

#if defined(SAIL_PHASE_TIMING) && SAIL_PHASE_TIMING
// the phase-timing build's per-phase wave-cycle sums: C linkage, so that a run-time compiled module's own copy can be
// found by name (sail_jit_phase_read)
extern "C" __device__ unsigned long long g_sailPhase[12];
__device__ unsigned long long g_sailPhase[12];
#endif

namespace {

// the workgroup's 16x16 block and sample range: blockIdx.x = group * (ownedTiles * 16) + block. Ungrouped
// launches (one workgroup per block, every sample) are a separate compile-time instance, so they carry none of
// the group bookkeeping in registers (sample groups add VGPR/SGPR spills to the flat kernels otherwise).
struct TileWork { int ownedTile, sub, kBeg, kEnd, bid; };
// The global 64x64 tile of the launch's owned tile `ownedTile` (< A.ownedTiles): the partition's, or in a MASKED instance
// (a launch under sail_set_active_tiles' tile mask) the entry of the ascending table of the rank's active tiles.
// Workgroup-uniform: one scalar load where the tile is computed, nothing of it lives on. Slots (stage, wavefront state)
// stay indexed by ownedTile. MASKED is a compile-time instance like GROUPED: the unmasked kernels never read
// A.tileMap, so their text is what it was without masks (a run-time select moved C2 by -0.1 % through register
// allocation alone).
template <bool MASKED>
D int ownedTileIndex(const SailTraceArgs& A, int ownedTile) {
  if constexpr (MASKED) return A.tileMap[ownedTile];
  else return A.rank + ownedTile * A.world;
}
// A workgroup's pixel block: PX pixels (NT threads / NS samples in flight per pixel), BW x BH, 4096 / PX per 64x64 tile:
// 16 x NT/16 strips with one sample in flight (NT = 256: 16 x 16; the pre-cull kernels' 1,024: 16 x 64), square blocks
// otherwise (8 x 8 or 4 x 4 pixels x 4 or 16 samples)
template <int PX> struct BlockGeo {
  static constexpr int kBW = PX >= 128 ? 16 : (PX >= 32 ? 8 : 4);
  static constexpr int kBH = PX / kBW;
  static constexpr int kPerRow = 64 / kBW;  // blocks per tile row
  static constexpr int kPer = 4096 / PX;     // blocks per tile
  static_assert(kBW * kBH == PX && PX >= 16 && 4096 % PX == 0 && kBW * kPerRow == 64, "pixel block shape");
};
template <bool GROUPED, int PX = 256>
D TileWork tileWork(const SailTraceArgs& A) {
  constexpr int kPer = BlockGeo<PX>::kPer;
  TileWork w;
  if (GROUPED) {
    const int nb = A.ownedTiles * kPer;
    const int bid = (int)blockIdx.x % nb, group = (int)blockIdx.x / nb;
    w.bid = bid;
    w.kBeg = group * A.groupSpp;
    w.kEnd = w.kBeg + A.groupSpp < A.spp ? w.kBeg + A.groupSpp : A.spp;
  } else {
    w.bid = (int)blockIdx.x;
    w.kBeg = 0;
    w.kEnd = A.spp;
  }
  w.ownedTile = w.bid / kPer; w.sub = w.bid % kPer;
  return w;
}
// The staged radiance of sample k at pixel p of block bid (groups after the first; the first group, which holds
// the launch's first samples, adds its own to the accumulator directly): stage planes 3k..3k+2, in the slot order
// the accumulation pass (sail_frame.hip accumStaged) reads -- slot (ownedTile * 16 + block16) * 256 + (y mod 16) * 16 +
// (x mod 16) -- whatever the block
template <int PX = 256>
D void stageSample(const SailTraceArgs& A, int k, int bid, int p, V3 e) {
  using G = BlockGeo<PX>;
  size_t slot;
  if (PX == 256 && G::kBW == 16) {
    slot = (size_t)bid * 256 + p;
  } else {
    const int ownedTile = bid / G::kPer, sub = bid % G::kPer;
    const int ly = (sub / G::kPerRow) * G::kBH + p / G::kBW, lx = (sub % G::kPerRow) * G::kBW + p % G::kBW;
    slot = ((size_t)ownedTile * 16 + (size_t)((ly >> 4) * 4 + (lx >> 4))) * 256 + (size_t)((ly & 15) * 16 + (lx & 15));
  }
  // three planes per sample (12 B per pixel instead of a float4's 16)
  float* const st = A.stage + (size_t)k * 3u * (size_t)A.stageStride + slot;
  st[0] = e.x;
  st[A.stageStride] = e.y;
  st[2 * A.stageStride] = e.z;
}

}  // namespace

// Path compaction: after every primitive sweep the workgroup's 256 live paths are sorted through LDS by
// (shape type, material) so that the hit record and the shading, the divergent half of a bounce, run on
// waves of like paths; dead paths drop out, so whole waves idle past the end of the live range. A path's
// state (ray, throughput, radiance, pixel, sweep result: 18 words) migrates between lanes; every path's
// arithmetic is unchanged, so the result is bit-identical to the unsorted kernel. The radiance of a sample
// goes back to the pixel's own lane through LDS before it is accumulated, in sample order.
// The sort key is the winning primitive row for scenes of fewer than 64 rows, else (material, shape) material-major:
// matte paths, which alone run the light sample and its shadow sweep, share waves (C4 +5.2 %; ordering the by-row key
// the same way through a host rank table: C3 -2.8 %).
// After the sort, a wave whose live paths have different sort keys runs at issue priority kPrioMixed (C3 +7.3 %).
// Path state moves through LDS packed: three float4 per path in the flat kernels (ds_*_b128), six float2 in the
// pre-cull kernel (ds_*_b64), the local hit point recomputed; the flat kernels keep each pixel's radiance as one float4
// (measured with priority 2, Gseg/s C1 / C3 / C4: six float2 89.6 / 29.0 / 9.40, three float4 90.0 / 29.0 / 9.10,
// + float4 radiance 90.1 / 29.15 / 9.10 and 90.3 / 29.15 / 9.10; unpacked, no priority 86.0 / 26.3 / 9.04).
// The sort's prefix sum over the key counts is six DPP adds (sail_scan.h).
// Barriers per bounce: two in the pre-cull and room kernels (every wave scans double-buffered counts itself), three in
// the Cornell kernel (one wave scans). Bit-identical; with the DPP scan and the live count by readlane C2 -1.0 % with
// two, C3 +1.1 % (twice), C4 +1.3-1.7 %. Deferring each sample's read-back past the next sample's first barrier (no
// end-of-sample barriers) was bit-identical and slower: C2 -2.3 %, C3 -6.6 %, C4 -2.2 %.
// The pre-cull kernel copies scenes of at most kCullLdsRows rows into LDS per workgroup, and its candidate loops, hit
// record and light sampler read their per-lane rows from there (C4 +4.3 %), with texParams tables of at most
// kCullLdsTp rows as well (+8.8 % together). 72 + 136 rows keep the block at 79.9 KB: two 1,024-thread workgroups per
// CU. The same copies in the flat kernels lost (C2 -6 %, C3 +-0).
// Compacted shadow rays (pre-cull kernel): lit matte paths leave their shadow rays in the sort buffer (compacted, after
// a barrier that ends the bounce's gathers) and the workgroup's first threads trace them, so waves whose lanes have no
// shadow ray (non-matte, unlit, contribution +0) do no shadow sweep; the radiance slot holds the shadowed outcome until
// the tracing thread writes the lit one. Measured (gpurun_out/r03m, bit-identical): C4 +3.1 % (spills 74 -> 105
// VGPRs); in the room kernel C3 -25 % (its spills 41 -> 85).
// NT threads per workgroup: a 16 x NT/16 pixel block, 4096/NT blocks per 64x64 tile. A larger workgroup sorts a
// larger pool of paths (fewer mixed waves) at the price of a wider barrier.
constexpr int kCullLdsRows = SAIL_CULL_LDS_ROWS, kCullLdsTp = SAIL_CULL_LDS_TP;
// A pre-cull kernel compiled at run time for a scene whose tables fit (SAIL_JIT_LDSFIT) copies them unconditionally:
// the per-lane row and texParams pointers are then known to point into LDS, so those reads are ds_read instead of flat
// loads, which also wait on every outstanding vector-memory load, scratch reloads included (C4 +3.1 %,
// profiles/r04_cull_ldsfit.jsonl).
#if defined(SAIL_JIT) && SAIL_JIT_LDSFIT
constexpr bool kLdsFitAll = true;
#else
constexpr bool kLdsFitAll = false;
#endif
// A flat kernel compiled for the scene's rows (kRows > 0) and its texParams row count (SAIL_JIT_TN > 0, at most 32 so
// that the Cornell form keeps 8 workgroups per CU) copies both tables into LDS the same way: the per-lane row reads of
// mixed waves' hit records and the material / texture reads become ds_read, off the counter the scratch reloads wait
// on (C3 +2.8 %, UI +2.2 %, profiles/r04_flat_lds.jsonl; the host asks for it in the room form only: the Cornell form
// measured -0.5 %). Round 3's flat-kernel copies were conditional (flat loads) and lost.
#if defined(SAIL_JIT) && defined(SAIL_JIT_TN) && SAIL_JIT_TN > 0
constexpr int kFlatTp = SAIL_JIT_TN;
#else
constexpr int kFlatTp = 0;
#endif
constexpr int kPrioMixed = 2;
// NS samples of each pixel in flight per workgroup (1, 4 or 16): the workgroup's NT lanes hold NT / NS pixels x NS samples
// (lane li: sample slot li / PX of pixel li % PX), so one workgroup finishes a launch's samples of its block NS times
// sooner. The short units end a launch with a short tail without splitting the samples over workgroups (sample groups:
// every sample's radiance staged in HBM and added in order by the accumulation pass); each pixel's NS radiances of a
// step wait in LDS and its lane adds them in sample order, so the sums are those of one sample at a time, bit for bit.
template <bool CULL, bool GROUPED, uint32_t KS, uint32_t KM, uint32_t KT, uint32_t KL, int NT, bool FAM, int NS = 1, bool MASKED = false>
__device__ __forceinline__ void traceTileCompact(const SailTraceArgs& A) {
  static_assert(NT == 128 || NT == 256 || NT == 512 || NT == 1024, "workgroups of 2, 4, 8 or 16 waves");
  static_assert(NS == 1 || NS == 4 || NS == 16, "samples in flight");
  constexpr int kPX = NT / NS;  // pixels per workgroup
  using G = BlockGeo<kPX>;
  constexpr int kKeys = 64;                // key = 1 + type * 5 + material category (types 0..9) < 64
  constexpr int kPack = CULL ? 1 : 2;
  constexpr bool kE4 = !CULL;
  // packed path state, 2: three float4 per path -- ray o + d.x, d.yz + throughput.xy, throughput.z + distance +
  // pixel | row << 10 + key (ds_write_b128 / ds_read_b128: 3 + 3 LDS instructions instead of 15 + 15); 1: six
  // float2 (ds_*_b64); the local hit point is recomputed (hitRecord<true>). The unused form is one element.
  __shared__ float4 sSt4[kPack == 2 ? 3 : 1][kPack == 2 ? NT : 1];
  __shared__ float2 sSt2[kPack == 1 ? 6 : 1][kPack == 1 ? NT : 1];
  // each pixel's radiance: one float4 (one ds_read_b128 / ds_write_b128) or three floats
  __shared__ float4 sE4[kE4 ? NT : 1];
  __shared__ float sE[kE4 ? 1 : 3][kE4 ? 1 : NT];
  auto E_LOAD = [&](int i) -> V3 {
    if constexpr (kE4) return v3(sE4[i].x, sE4[i].y, sE4[i].z);
    else return v3(sE[0][i], sE[1][i], sE[2][i]);
  };
  auto E_STORE = [&](int i, const V3& v) {
    if constexpr (kE4) sE4[i] = make_float4(v.x, v.y, v.z, 0.0f);
    else { sE[0][i] = v.x; sE[1][i] = v.y; sE[2][i] = v.z; }
  };
  constexpr bool kShCompact = CULL && KL != 0u;
  __shared__ int sShCnt[2];
  int shph = 0;
  constexpr bool twoBar = CULL || FAM;
  constexpr bool kSort1 = CULL || FAM;  // sort the paths at the first bounce too
  constexpr bool kGatherAll = !CULL;    // after a sort every lane gathers, live or not (the gather below says why)
  __shared__ int sCnt2[twoBar ? 2 : 1][kKeys];  // [0] alone in the three-barrier sort
  __shared__ int sStart[twoBar ? 1 : kKeys + 1];
  const TileWork tw = tileWork<GROUPED, kPX>(A);
  const int ownedTile = tw.ownedTile;
  if (ownedTile >= A.ownedTiles) return;  // uniform over the workgroup
  const int sub = tw.sub;
  const int tile = ownedTileIndex<MASKED>(A, ownedTile);
  const int tx = tile % A.tilesX, ty = tile / A.tilesX;
  const int li = threadIdx.x, lane = li & 63, wave = li >> 6;
  const int x0 = tx * 64 + (sub % G::kPerRow) * G::kBW, y0 = ty * 64 + (sub / G::kPerRow) * G::kBH;
  // a path's home slot (the lane it started on) names its pixel and its sample slot
  auto homeX = [&](int h) { return x0 + (h % kPX) % G::kBW; };
  auto homeY = [&](int h) { return y0 + (h % kPX) / G::kBW; };
  const int mySlot = li / kPX;
  const int x = homeX(li), y = homeY(li);
  const bool valid = x < A.W && y < A.H;   // ragged tiles: invalid lanes still serve migrated paths

  Ctx c;
  c.tp = A.texparams; c.lt = A.lights; c.lightObjRow = A.lightObjRow; c.typeMasks = A.typeMasks;
  c.prims = A.prims;
  c.cprims = A.prims;
  c.tpl = A.texparams;
  c.rowCopy = false;
  c.tpCopy = false;
  c.n = A.n; c.tn = A.tn; c.ln = A.ln;
  c.matMask = A.matMask; c.texMask = A.texMask; c.lightMask = A.lightMask;
  c.fcx = 0.0f; c.fcy = 0.0f;
  c.shadowAnyHit = A.shadowAnyHit;
  c.cullPrims = CULL ? 1 : 0;
  c.cullFma = CULL && A.cullPrims == 2;
  c.cullPrimary = A.cullPrimary;
  c.kShapes = KS; c.kMats = KM; c.kTex = KT; c.kLights = KL;

  if (li < (twoBar ? 2 : 1) * kKeys) sCnt2[li / kKeys][li % kKeys] = 0;
  if (li < 2) sShCnt[li] = 0;
  // the pre-cull kernel's candidate loops, hit record and light sampler read rows per lane: from an LDS copy of the
  // scene when it fits
  constexpr int kLdsRows = CULL ? kCullLdsRows : (!CULL && kFlatTp > 0 && kRows > 0 ? kRows : 0);
  c.rowCopy = kLdsRows > 0;
  __shared__ float4 sPrimL[kLdsRows > 0 ? kLdsRows * (int)(sizeof(SailPrim) / 16) : 1];
  constexpr bool kFlatLds = !CULL && kFlatTp > 0 && kRows > 0;
  if constexpr (kLdsFitAll) {
    if (A.n > kLdsRows || A.tn > kCullLdsTp) return;  // never launched so (sail_capi.cpp jitSpecFor); uniform
  }
  if constexpr (kFlatLds) {
    if (A.n != kRows || A.tn != kFlatTp) return;  // never launched so (sail_capi.cpp jitSpecFor); uniform
  }
#if SAIL_ROWVALS
  if (A.n != kRows || A.tn != kTpC) return;  // never launched so (sail_capi.cpp valueSpecFor); uniform
#endif
  if constexpr (kLdsRows > 0) {
    if (kLdsFitAll || kFlatLds || A.n <= kLdsRows) {  // uniform
      const float4* src = reinterpret_cast<const float4*>(A.prims);
      const int nv = A.n * (int)(sizeof(SailPrim) / 16);
      for (int i = li; i < nv; i += NT) sPrimL[i] = src[i];
      c.cprims = reinterpret_cast<const SailPrim*>(sPrimL);
    }
  }
  constexpr int kLdsTp = CULL ? kCullLdsTp : (!CULL && kFlatTp > 0 && kRows > 0 ? kFlatTp : 0);
  c.tpCopy = kLdsTp > 0;
  __shared__ float4 sTpL[kLdsTp > 0 ? kLdsTp * 4 : 1];
  if constexpr (kLdsTp > 0) {
    if (kLdsFitAll || kFlatLds || A.tn <= kLdsTp) {  // uniform
      const float4* src = reinterpret_cast<const float4*>(A.texparams);
      for (int i = li; i < A.tn * 4; i += NT) sTpL[i] = src[i];
      c.tpl = reinterpret_cast<const float*>(sTpL);
    }
  }
  int ph = 0;
  // the seeds of the step's NS samples (NS > 1: a gathered path reads its own)
  __shared__ float sSeed[NS];
  if (NS > 1 && li < NS) sSeed[li] = constRow<SailSample>(A.samples, min(tw.kBeg + li, tw.kEnd - 1)).seed;
  __syncthreads();
  // sort key: the winning primitive row when there are few enough rows (no row reads for the key, and a wave's
  // paths share their primitive and material rows; C2 +3.7 %, C3 +1.2 %), else (shape type, material category).
  // A waterfall over the wave's rows with the row index in an SGPR (scalar row loads) was measured: the
  // duplicated shading body doubled the spills, C2 -40 %.
  const bool byPrim = A.n < kKeys;
  const size_t pixG = (size_t)y * A.W + x;
  constexpr bool grouped = GROUPED;
  // a room-family kernel's first group accumulates its samples itself (SailTraceArgs.groupHome)
  constexpr bool kHome = FAM && !CULL;
  const bool home = !grouped || (kHome && tw.kBeg == 0);
  const bool pixLane = li < kPX;  // the lane that adds its pixel's samples (every lane when NS == 1)
  // the pixel's running accumulator: in registers, or, with samples in flight (flat forms), in an LDS slot of its lane
  // (the Cornell form: 32 float4, 512 B; the room form measured more spills with it), so that no VGPR stays live across the sample loop for it
  constexpr bool kAccLds = NS >= 16 && !CULL;
  __shared__ float4 sAcc[kAccLds ? kPX : 1];
  float4 acc = (valid && home && pixLane) ? A.accum[pixG] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (kAccLds) {
    if (pixLane) sAcc[li] = acc;  // read back only by this lane
  }
  const float s = ((float)x + 0.5f) / (float)A.W, t = ((float)y + 0.5f) / (float)A.H;
  const bool tri0 = s + t <= 1.0f;
  const V3 eye = v3(A.eye[0], A.eye[1], A.eye[2]);
  // the exact segment counter: per wave in scalar registers in the pre-cull kernels (popcount of the live-lane ballot
  // at each bounce; C4 +1.8 %, profiles/r04_live_state.jsonl), per lane in the flat ones (there the scalar form measured
  // C1 -0.2 %, C3 -0.6 %)
  unsigned segs = 0;
  unsigned long long segsW = 0;
  PhaseClock pc;
#if SAIL_PHASE_TIMING
  for (int q = 0; q < 12; q++) pc.acc[q] = 0;
  pc.t = __builtin_amdgcn_s_memtime();
#endif
  for (int k = tw.kBeg; k < tw.kEnd; k += NS) {
    const int ks = k + mySlot;  // this lane's sample (NS == 1: k, uniform)
    const bool inRange = NS == 1 || ks < tw.kEnd;
    const SailSample& S = constRow<SailSample>(A.samples, NS == 1 ? k : (inRange ? ks : k));
    const bool aovs = A.aovN || A.aovP;  // AOVs of the launch's last sample
    bool alive = valid && inRange;
    int pixel = li;  // the path's home slot
    auto pathSeed = [&](int h) { if constexpr (NS == 1) return S.seed; else return sSeed[h / kPX]; };
    // a flat form's path carries its segment (origin, direction) alone: the reciprocals of a direction are built where
    // the segment is swept, below, and die with the sweep, so neither the sort nor the shading holds registers for
    // them. The pre-cull form carries the ray with its reciprocals (PathRay in sail_geom.h says why).
    typename PathRay<CULL>::type ray;
    {
      const V3 d0 = v3(S.d[0][0], S.d[0][1], S.d[0][2]), d1 = v3(S.d[1][0], S.d[1][1], S.d[1][2]);
      const V3 d2 = v3(S.d[2][0], S.d[2][1], S.d[2][2]), d3 = v3(S.d[3][0], S.d[3][1], S.d[3][2]);
      nextRay(ray, eye, tri0 ? (d0 + (d2 - d0) * s + (d1 - d0) * t) : (d3 + (d1 - d3) * (1.0f - s) + (d2 - d3) * (1.0f - t)));
    }
    V3 fpdf = v3s(1.0f);
    // the path's radiance lives in LDS at its pixel: one path per pixel, updated in bounce order
    E_STORE(li, v3s(0.0f));
    for (int depth = 1; depth <= A.maxBounces; depth++) {
      Sweep sw;
      sw.best = kMaxDistance; sw.bi = -1; sw.bhl = v3s(0.0f);
      int key = 0;
      if constexpr (CULL) segsW += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(alive));
#if SAIL_ROWDEFER
      // The deferred row (sail_geom.h kDeferRow): at a bounce that sorts and is not the last (the last needs the true winner
      // for the quiet-row test and may skip the sort), a candidate of that row travels under the row's key with its
      // winner among the other rows -- alive even when that is a miss -- and the row's waves finish its test after the
      // gather (sphereResolve). Its segment is counted here, at its sweep.
      static_assert(!CULL && !FAM && kRows < kKeys, "a deferred row: in the flat form, sorted by winning row");
      const bool deferB = depth > 1 && depth < A.maxBounces;  // uniform
      bool cand = false;
#endif
      if (alive) {
        if constexpr (!CULL) segs++;
        const Ray& rr = sweptRay(ray);  // flat forms: rcp_rn of the three components here, once per traced segment
#if SAIL_ROWDEFER
        sw = sweepRayDefer(c, rr, deferB, cand);
#else
        sw = sweepRay(c, rr, depth == 1);
#endif
#if SAIL_ROWDEFER
        if (cand) {
          key = 1 + kDeferRow;
        } else
#endif
        if (sw.best >= kMaxDistance) {  // the path leaves the scene: its radiance is final
          if (depth == 1 && aovs && k + pixel / kPX == A.spp - 1) {  // fstrace.glsl:15-16 with n = p = 0 (GLSL: undefined)
            const size_t g = (size_t)homeY(pixel) * A.W + homeX(pixel);
            const V3 qn = v3s(0.0f) / 2.0f + 0.5f, qp = normalize(v3s(0.0f));
            if (A.aovN) A.aovN[g] = make_float4(qn.x, qn.y, qn.z, 1.0f);
            if (A.aovP) A.aovP[g] = make_float4(qp.x, qp.y, qp.z, 1.0f);
          }
          alive = false;
        } else if (byPrim) {
          key = 1 + sw.bi;
          // the room form compiled for rows with a Cornellbox sorts its hits by face, the normal / wall-colour chains'
          // first true test on the same hit point the record computes, so that a wave's box records take one face
          // branch (UI +3.4 %; the Cornell form measured -5.5 %: its 512-path pool splits into too many partial waves,
          // profiles/r05_facekey_*.jsonl)
          if constexpr (FAM && !CULL && kCornellRow >= 0) {
            if (sw.bi == kCornellRow) {
              const SailPrim& cp = PRIM(c, kCornellRow);
              const V3 h = ray.o + sw.best * ray.d, mn = P3(cp, 0), mx = P3(cp, 3);
              const int face = h.x < mn.x + 0.0001f ? 0 : h.x > mx.x - 0.0001f ? 1 : h.y < mn.y + 0.0001f ? 2
                             : h.y > mx.y - 0.0001f ? 3 : h.z < mn.z + 0.0001f ? 4 : 5;
              key = 1 + kRows + face;
            }
          }
        } else {
          const SailPrim& p = PRIM(c, sw.bi);
          int mc = matCat(p);
          mc = (mc >= 0 && mc < 5) ? mc : 0;
          key = 1 + mc * 10 + p.type;
        }
      }
      // The last bounce (Cornell and all-plugin forms): only the path's radiance is read after it, and a hit on a
      // quiet row (SailTraceArgs.lastQuietRows, classified by the host) adds exactly +0 * throughput whatever its hit
      // record holds. Such a path ends here, on the lane that has carried it since the last gather (which also made the last
      // store to its pixel's radiance): shadeLast's e + (emission + direct) * fpdf with both terms +0 -- the multiply and
      // the add are made, so a non-finite throughput gives the same NaN -- and then it is dead to the sort, the hit
      // record and the shading like a path that left the scene. Its segment is counted above. The lanes of the AOV
      // sample keep their first-bounce record. Measured bit-identical (profiles/r07_last_quiet.jsonl): C2 +3.2 %,
      // C5 +1.2 %; the room form is left as it was: its light plugins keep every matte row out of this, and with the
      // test compiled in C3 lost 1.0 % (three runs each, spread 0.1 %).
      const bool lastB = !CULL && !FAM && depth == A.maxBounces;  // uniform
      if constexpr (!CULL && !FAM) {
        if (lastB) __builtin_amdgcn_s_setprio(0);  // most waves gather no path below: none keeps a raised priority
        if (lastB && alive && ((A.lastQuietRows >> (sw.bi & 31)) & 1u) != 0u &&
            !(depth == 1 && aovs && k + pixel / kPX == A.spp - 1)) {
          E_STORE(pixel, E_LOAD(pixel) + v3s(0.0f) * fpdf);
          alive = false;
          key = 0;
        }
      }
      PHASE_MARK(pc, 0);
      // ---- counting sort of the live paths by key (LDS atomics for the per-key rank, one wave scans)
      int rank = 0;
      int nAlive;
      // the pre-cull form alone gathers under `if (alive)` (see the gather below): there a lane's old path state is dead
      // after the scatter (a live lane gathers a new one, a dead lane reads none), and says so, or the compiler keeps it
      // live across the sort for the lanes that gather nothing
      auto dropState = [&]() {
        if constexpr (!kGatherAll) {
          ray.o = v3s(0.0f); ray.d = v3s(0.0f); dropRcp(ray);
          fpdf = v3s(0.0f); sw.best = 0.0f; sw.bi = 0; pixel = 0;
        }
      };
      // a path's state into sorted slot d
      auto scatterTo = [&](int d) {
        if constexpr (kPack == 2) {
          sSt4[0][d] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.d.x);
          sSt4[1][d] = make_float4(ray.d.y, ray.d.z, fpdf.x, fpdf.y);
          sSt4[2][d] = make_float4(fpdf.z, sw.best, __int_as_float(pixel | (sw.bi << 10)), __int_as_float(key));
        } else {
          sSt2[0][d] = make_float2(ray.o.x, ray.o.y); sSt2[1][d] = make_float2(ray.o.z, ray.d.x);
          sSt2[2][d] = make_float2(ray.d.y, ray.d.z); sSt2[3][d] = make_float2(fpdf.x, fpdf.y);
          sSt2[4][d] = make_float2(fpdf.z, sw.best);
          sSt2[5][d] = make_float2(__int_as_float(pixel | (sw.bi << 10)), __int_as_float(key));
        }
      };
      // the flat-form kernels (Cornell box, all-plugin) leave the first bounce unsorted: primary rays of a 16 x 4 strip
      // mostly hit one row already and none is dead yet, so each lane keeps its own pixel's path (C1 +1.1 %; the room
      // and pre-cull kernels keep the sort, where skipping it measured C3 -1.6 %, C4 -9.2 %:
      // profiles/r04_skip_sort1.jsonl)
      // lastSkipSort: every row that is not quiet is an emitter whose hit shadeLast accepts, so the few paths left
      // after the quiet ones ended are not sorted: each lane keeps the path it holds. A sort skipped leaves the count
      // buffers as the last sort cleared them and ph where it was, so the next sample's sorts alternate on as before.
      const bool sortNow = (kSort1 || depth > 1) && !(lastB && A.lastSkipSort != 0);
      if (sortNow) {
      if constexpr (twoBar) {
      // every wave scans the counts itself (the start of a lane's key by a cross-lane read), so no barrier
      // between the scan and the scatter; the counts alternate between two buffers, the one just read being
      // cleared by wave 0 after the scatter barrier, two bounces before it is counted into again
      if (alive) rank = atomicAdd(&sCnt2[ph][key], 1);
      PHASE_MARK(pc, 7);  // rank atomics
      __syncthreads();
      PHASE_MARK(pc, 8);  // barrier 1 wait
      {
        const int v = sCnt2[ph][lane];
        const int incl = waveScanIncl(v);
        nAlive = __builtin_amdgcn_readlane(incl, 63);
        const int start = __shfl(incl - v, key, 64);
        if (alive) scatterTo(start + rank);
        dropState();
      }
      PHASE_MARK(pc, 9);  // scan + scatter
      __syncthreads();
      PHASE_MARK(pc, 10);  // barrier 2 wait
      if (wave == 0) sCnt2[ph][lane] = 0;
      ph ^= 1;
      } else {
      int* const sCnt = sCnt2[0];
      if (alive) rank = atomicAdd(&sCnt[key], 1);
      PHASE_MARK(pc, 7);  // rank atomics
      __syncthreads();
      PHASE_MARK(pc, 8);  // barrier 1 wait
      if (wave == 0) {
        const int v = sCnt[lane];
        const int incl = waveScanIncl(v);
        sStart[lane] = incl - v;
        if (lane == 63) sStart[kKeys] = incl;
        sCnt[lane] = 0;
      }
      PHASE_MARK(pc, 9);  // scan
      __syncthreads();
      PHASE_MARK(pc, 10);  // barrier 2 wait
      nAlive = sStart[kKeys];
      if (alive) scatterTo(sStart[key] + rank);
      dropState();
      PHASE_MARK(pc, 9);  // scatter
      __syncthreads();
      PHASE_MARK(pc, 10);  // barrier 3 wait
      }
      alive = li < nAlive;
      }
      ShadowPending sp;
      sp.pending = false;
      V3 eLit = v3s(0.0f);
      int keyG = 0;  // the gathered path's sort key
      PHASE_MARK(pc, 9);
      // After a sort every lane of a flat form (Cornell, room, all-plugin) reads and unpacks the packed state of its sorted
      // slot, the lanes past the live range too: theirs is a slot nobody wrote this bounce (stale or never-written LDS,
      // inside the array), and nothing reads what they unpack -- every use of the state is under `if (alive)` below. A
      // gather under `if (alive)` leaves those lanes their old state, which the compiler keeps live across the sort and
      // merges with the gathered one unless fifteen zero moves per sorted bounce end it (dropState). An unsorted bounce
      // keeps its registers. Measured: C2 +0.9 % by this alone, C3 +0.5 % with the segment-only
      // path; the room form's spills did not move. The pre-cull form keeps its gather under `if (alive)` and its
      // dropState: with every lane gathering (and the segment-only path) its grouped kernel spilled 86 VGPRs for 80
      // and C4 lost 1.3 % (spread 0.6 %), and a fully dead wave there would issue six LDS reads it now skips.
      // (a macro, one text for both places: as a lambda the same text cost the pre-cull kernel 9 more spilled VGPRs
      // and C4 0.7 %)
#define SAIL_GATHER()                                                                                            \
        if constexpr (kPack == 2) {                                                                              \
          const float4 q0 = sSt4[0][li], q1 = sSt4[1][li], q2 = sSt4[2][li];                                     \
          const int pk = __float_as_int(q2.z);                                                                   \
          keyG = __float_as_int(q2.w);                                                                           \
          ray.o = v3(q0.x, q0.y, q0.z);                                                                          \
          ray.d = v3(q0.w, q1.x, q1.y);                                                                          \
          fpdf = v3(q1.z, q1.w, q2.x);                                                                           \
          sw.best = q2.y;                                                                                        \
          pixel = pk & 1023;                                                                                     \
          sw.bi = pk >> 10;                                                                                      \
          sw.bhl = v3s(0.0f);  /* recomputed by hitRecord<true> */                                               \
        } else {                                                                                                 \
          const float2 q0 = sSt2[0][li], q1 = sSt2[1][li], q2 = sSt2[2][li], q3 = sSt2[3][li], q4 = sSt2[4][li]; \
          const int pk = __float_as_int(sSt2[5][li].x);                                                          \
          keyG = __float_as_int(sSt2[5][li].y);                                                                  \
          ray.o = v3(q0.x, q0.y, q1.x);                                                                          \
          ray.d = v3(q1.y, q2.x, q2.y);                                                                          \
          fpdf = v3(q3.x, q3.y, q4.x);                                                                           \
          sw.best = q4.y;                                                                                        \
          pixel = pk & 1023;                                                                                     \
          sw.bi = pk >> 10;                                                                                      \
          sw.bhl = v3s(0.0f);  /* recomputed by hitRecord<true> */                                               \
        }
      if constexpr (kGatherAll) {
        if (!sortNow) keyG = key;
        else { SAIL_GATHER() }
      }
      if (alive) {
        if constexpr (!kGatherAll) {
          if (!sortNow) keyG = key;
          else { SAIL_GATHER() }
          dropRcp(ray);
        }
#undef SAIL_GATHER
        {  // a wave whose live paths have different sort keys runs several hit-record / material branches: raise its
           // issue priority so that its workgroup's next barrier is not held up by it (the other waves wait there)
          const int k0 = __builtin_amdgcn_readfirstlane(keyG);
          const bool mixedW = __builtin_amdgcn_ballot_w64(keyG != k0) != 0ull;
          if (mixedW) __builtin_amdgcn_s_setprio(kPrioMixed);
          else __builtin_amdgcn_s_setprio(0);
        }
#if SAIL_ROWDEFER
        // the deferred row's paths: candidates finish the row's test (sweep time in the phase build); one left without
        // a winner ends here like a path that left the scene -- its radiance is final in LDS, and no AOV is due past
        // the first bounce. The record and shading below see the resolved winner.
        if (deferB) {  // uniform
          PHASE_MARK(pc, 1);
          if (keyG == 1 + kDeferRow) sphereResolve(c, ray, sw);
          if (sw.best >= kMaxDistance) alive = false;
          PHASE_MARK(pc, 0);
        }
#endif
        if (alive) {  // still: a deferred candidate may have ended just above (without a deferred row, always)
        c.fcx = (float)homeX(pixel) + 0.5f;
        c.fcy = (float)homeY(pixel) + 0.5f;
        const float seed = pathSeed(pixel) + (float)depth;
        // the rest of the bounce behind the hit record `ins` (one text for both forms below: no arithmetic restated)
#define SAIL_BOUNCE_REST(ins, Q)                                                                   \
        PHASE_MARK(pc, 1);                                                                         \
        if (depth == 1 && aovs && k + pixel / kPX == A.spp - 1) {                                  \
          const size_t g = (size_t)homeY(pixel) * A.W + homeX(pixel);                              \
          const V3 qn = ins.normal / 2.0f + 0.5f, qp = normalize(ins.hit);                         \
          if (A.aovN) A.aovN[g] = make_float4(qn.x, qn.y, qn.z, 1.0f);                             \
          if (A.aovP) A.aovP[g] = make_float4(qp.x, qp.y, qp.z, 1.0f);                             \
        }                                                                                          \
        V3 e = (Q) ? v3s(0.0f) : E_LOAD(pixel); /* Q: a quiet row's copy (kRowQuietMask) */        \
        if (!(!CULL && depth == A.maxBounces && shadeLast(c, ins, seed, fpdf, e))) {               \
          if constexpr (kShCompact) {                                                              \
            shadeBounceP(c, ins, ray, seed, fpdf, e, pc, sp); /* e: the dark outcome */            \
            eLit = sp.eLit;                                                                        \
          } else {                                                                                 \
            shadeBounce(c, ins, ray, seed, fpdf, e, pc);                                           \
          }                                                                                        \
        }                                                                                          \
        if constexpr (!(Q)) E_STORE(pixel, e);
#if SAIL_ROWSHADE
        // a row-uniform wave runs it in its row's branch, on that row's constants (bounceU)
        bounceU<true, FAM && !CULL>(c, ray, sw,
                                    [&](const Hit& ins, auto quiet) __attribute__((always_inline)) {
          SAIL_BOUNCE_REST(ins, decltype(quiet)::value)
        });
#else
        const Hit ins = hitRecordU<true, FAM && !CULL>(c, ray, sw);
        SAIL_BOUNCE_REST(ins, false)
#endif
#undef SAIL_BOUNCE_REST
        }
      }
      if constexpr (kShCompact) {
        if (c.ln > 0) {  // uniform
          const bool pend = alive && sp.pending;
          __syncthreads();  // every gather of this bounce is done: the sort buffer takes the shadow rays
          const unsigned long long bm = __builtin_amdgcn_ballot_w64(pend);
          if (bm != 0ull) {  // uniform over the wave
            int base = 0;
            if (lane == 0) base = atomicAdd(&sShCnt[shph], __popcll(bm));
            base = __shfl(base, 0, 64);
            if (pend) {
              const int d = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
              const V3 o = sp.hit, dl = sp.toLight;
              if constexpr (kPack == 2) {
                sSt4[0][d] = make_float4(o.x, o.y, o.z, dl.x);
                sSt4[1][d] = make_float4(dl.y, dl.z, eLit.x, eLit.y);
                sSt4[2][d] = make_float4(eLit.z, __int_as_float(pixel), 0.0f, 0.0f);
              } else {
                sSt2[0][d] = make_float2(o.x, o.y); sSt2[1][d] = make_float2(o.z, dl.x);
                sSt2[2][d] = make_float2(dl.y, dl.z); sSt2[3][d] = make_float2(eLit.x, eLit.y);
                sSt2[4][d] = make_float2(eLit.z, __int_as_float(pixel));
              }
            }
          }
          __syncthreads();
          const int nSh = sShCnt[shph];
          if (li == 0) sShCnt[shph ^ 1] = 0;  // the previous bounce's count: every read of it is done
          shph ^= 1;
          if (li < nSh) {  // testShadow(Ray(hit, toLight)) of the light sample (shader.light.js:24-31)
            V3 o, dl, el;
            int pix;
            if constexpr (kPack == 2) {
              const float4 q0 = sSt4[0][li], q1 = sSt4[1][li], q2 = sSt4[2][li];
              o = v3(q0.x, q0.y, q0.z); dl = v3(q0.w, q1.x, q1.y); el = v3(q1.z, q1.w, q2.x);
              pix = __float_as_int(q2.y);
            } else {
              const float2 q0 = sSt2[0][li], q1 = sSt2[1][li], q2 = sSt2[2][li], q3 = sSt2[3][li], q4 = sSt2[4][li];
              o = v3(q0.x, q0.y, q1.x); dl = v3(q1.y, q2.x, q2.y); el = v3(q3.x, q3.y, q4.x);
              pix = __float_as_int(q4.y);
            }
            if (!testShadow(c, mkRay(o, dl))) E_STORE(pix, el);
          }
        }
      }
    }
    __syncthreads();
    if constexpr (NS == 1) {
      if (valid) {
        const V3 er = E_LOAD(li);
        if (!home) stageSample<kPX>(A, k, tw.bid, li, er);
        else accumulateSample(acc, er, S, A.accumMode);
      }
    } else {
      if (valid && pixLane) {  // the pixel's samples of this step, in sample order
        if constexpr (kAccLds) acc = sAcc[li];
        for (int j = 0; j < NS && k + j < tw.kEnd; j++) {
          const V3 er = E_LOAD(j * kPX + li);
          if (!home) stageSample<kPX>(A, k + j, tw.bid, li, er);
          else accumulateSample(acc, er, constRow<SailSample>(A.samples, k + j), A.accumMode);
        }
        if constexpr (kAccLds) sAcc[li] = acc;
      }
      if (li < NS && k + NS + li < tw.kEnd) sSeed[li] = constRow<SailSample>(A.samples, k + NS + li).seed;
    }
    __syncthreads();
    PHASE_MARK(pc, 11);  // sample end: barriers, accumulation / staging
  }
  if constexpr (kAccLds) {
    if (pixLane) acc = sAcc[li];
  }
  if (valid && home && pixLane) A.accum[pixG] = acc;
#if SAIL_PHASE_TIMING
  if (lane == 0)
    for (int q = 0; q < 12; q++) atomicAdd(&g_sailPhase[q], pc.acc[q]);
#endif
  if (A.segCounter) {
    unsigned long long v = segsW;
    if constexpr (!CULL) {
      v = segs;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    }
    if (lane == 0) atomicAdd(&A.segCounter[(blockIdx.x * 4u + (unsigned)wave) % SAIL_SEG_SLOTS], v);
  }
}
// Path compaction (traceTileCompact) in every plugin-set kernel: C2 +6 %, C3 +12 %, C4 +10 % (measured;
// earlier builds with more live state lost to spills in the flat kernels).
// Each plugin set has an ungrouped kernel (one workgroup per 16 x NT/16 block, every sample) and a _grouped one
// (sample groups: G workgroups per block, staged radiance added by the accumulation pass), and a _masked instance of
// each for launches under a tile mask (ownedTileIndex). Launch bounds: waves per SIMD and threads per workgroup, chosen
// by the occupancy sweeps of DESIGN.md §5 (the launch wrapper in sail_trace_sets.hip sizes the grids).
// fam: the room family's choices for a flat kernel -- the two-barrier sort, the first sample group accumulating its
// samples itself (SailTraceArgs.groupHome) and one box record for Cube and Cornellbox.
#define SAIL_TRACE_KERNELS_NS(name, waves, cull, ks, km, kt, kl, nt, gnt, fam, ns, masked)                         \
  extern "C" __global__ void __launch_bounds__(nt, waves) name(SailTraceArgs A) {                                \
    traceTileCompact<cull, false, ks, km, kt, kl, nt, fam, ns, masked>(A);                                       \
  }                                                                                                              \
  extern "C" __global__ void __launch_bounds__(gnt, waves) name##_grouped(SailTraceArgs A) {                     \
    traceTileCompact<cull, true, ks, km, kt, kl, gnt, fam, ns, masked>(A);                                       \
  }
#if defined(SAIL_JIT)
// A per-plugin-set kernel compiled at run time by hipRTC (sail_jit.cpp), like the reference's per-scene program
// (tracerConfig -> Generator.generate, src/scene/scene.js:70-112, src/shader/generator.js:107-123): the plugin masks,
// the pre-cull choice, the family and the launch bounds arrive as macros, and only this kernel pair is compiled.
#ifndef SAIL_JIT_NS
#define SAIL_JIT_NS 1
#endif
// SAIL_JIT_MASKED 1: the pair a launch under a tile mask runs, a module of its own under the same kernel names
#ifndef SAIL_JIT_MASKED
#define SAIL_JIT_MASKED 0
#endif
#if SAIL_JIT_CULL
SAIL_TRACE_KERNELS_NS(sail_trace_kernel_cull_jit, SAIL_JIT_WAVES, true, SAIL_JIT_KS, SAIL_JIT_KM, SAIL_JIT_KT, SAIL_JIT_KL,
                      SAIL_JIT_NT, SAIL_JIT_NT, false, SAIL_JIT_NS, SAIL_JIT_MASKED != 0)
#else
SAIL_TRACE_KERNELS_NS(sail_trace_kernel_jit, SAIL_JIT_WAVES, false, SAIL_JIT_KS, SAIL_JIT_KM, SAIL_JIT_KT, SAIL_JIT_KL,
                      SAIL_JIT_NT, SAIL_JIT_NT, SAIL_JIT_FAM != 0, SAIL_JIT_NS, SAIL_JIT_MASKED != 0)
#endif
#endif  // SAIL_JIT
#endif  // SAIL_TRACE_HIP
