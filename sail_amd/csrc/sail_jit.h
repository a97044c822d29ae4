// sail_jit.h — what one run-time compiled trace kernel pair is specialised to (sail_jit.cpp, used by sail_plan.cpp and sail_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

constexpr int kSailJitMaxRows = 8;  // scenes of at most this many rows can be compiled for their rows (flat path)
constexpr int kSailJitMaxFlatTp = 32;  // flat forms copy texParams tables of at most this many rows into LDS
constexpr int kSailJitRowRecordMax = 3;  // value kernels of at most this many rows: a hit record per row (sail_geom.h kRowRecordMax)
struct SailJitSpec {
  uint32_t ks = 0, km = 0, kt = 0, kl = 0;  // plugin masks: shapes, materials, textures, lights
  int mode = 0;                             // sail_jit_mode (include/sail_hip.h): 0 flat, 1 pre-cull, 2 room family
  int waves = 6;                            // launch bounds: waves per SIMD
  int rows = 0;                             // > 0: the scene's row count, with each row's shape id in types
  int ldsFit = 0;                           // pre-cull: the scene's tables fit the LDS copies (SAIL_CULL_LDS_*)
  int tn = 0;                               // flat forms with rows: the texParams row count (LDS copies), 0 = none
  int ns = 1;                               // samples of each pixel in flight per workgroup (1, 4, 16: traceTileCompact)
  int nt = 0;                               // threads per workgroup (128 .. 1,024); 0 = the form's own (1,024 pre-cull, 256)
  int types[kSailJitMaxRows] = {};
  // A value kernel (flat form with rows, SAIL_JIT_ROWVALS in sail_geom.h): the words of the decoded rows (rows x 32,
  // the bytes of the SailPrim array the host uploads) and of the texParams table (16 per row, at most kSailJitMaxFlatTp
  // rows; may be none). Both empty: the types kernel. Compared and keyed as words, never as floats: +0 / -0 and two NaN
  // payloads are different kernels.
  std::vector<uint32_t> rowWords, tpWords;
  // rowForm 1: a value kernel of at most kSailJitRowRecordMax rows in the row-shading form (SAIL_JIT_ROWSHADE in
  // sail_geom.h; SAIL_DEBUG_JIT bit 32). rowShade: the rows (bit i: row i) whose row-uniform waves run the rest of the
  // bounce in their row's branch, on the row's material constants; rowQuiet: those of them whose copy leaves the
  // radiance alone (quiet rows, sail_plan.cpp lastBounceRows). Both 0: the kernel is the plain value kernel's code.
  // All 0 in every types spec.
  int rowForm = 0, rowShade = 0, rowQuiet = 0;
  // >= 0: a value kernel that defers this Sphere row's root solve past the path sort (SAIL_JIT_ROWDEFER in sail_geom.h;
  // SAIL_DEBUG_JIT bit 64 asks for the kernel without it). -1: none, and in every types spec.
  int rowDefer = -1;
  // 1: the MASKED instances of the spec's kernel pair (sail_trace.hip ownedTileIndex), which a launch under a tile mask
  // runs: a module of its own, built when a context first launches under a mask
  int masked = 0;
};
bool sailJitSpecEqual(const SailJitSpec& a, const SailJitSpec& b);
// threads per workgroup of the spec's kernels
inline int sailJitThreads(const SailJitSpec& s) { return s.nt ? s.nt : (s.mode == 1 ? 1024 : 256); }

// A loaded kernel pair and where its code object came from.
struct SailJitKernel {
  hipFunction_t plain = nullptr, grouped = nullptr;
  uint64_t buildId = 0;     // FNV-1a 64 of the code object, its compilation-unit id masked (sail_jit.cpp codeId)
  double compileMs = 0.0;   // hipRTC time of the code object (0 when it came from a disk cache)
  int fromCache = 0;        // 1: the user's on-disk cache, 2: the cache shipped next to the library
};
// The kernel pair for `spec` on `device` (made current). The code object is built on a background thread at the first
// request (disk caches first, then hipRTC), outside every lock the launch path takes. Returns 0 with the loaded pair;
// 1 while the code object is still being built and wait_ms allows no more waiting (wait_ms < 0: wait until it is done);
// -1 with a message when it cannot be built or loaded (the caller then runs the precompiled kernel, same results).
int sail_jit_kernels(int device, const SailJitSpec& spec, int wait_ms, SailJitKernel* out, std::string* err);
// A context's claim on the kernel of `spec` on `device` (delta +1 when it adopts the spec, -1 when it drops it): a queued
// build of a spec no context holds any more is skipped by the build worker, so the scene's current kernel never waits
// behind builds of specs that a newer scene, partition or switch replaced.
// Dropping the last hold on a value spec (rowWords not empty) also unloads its modules and frees its code object in
// memory (the object stays in the disk caches): the caller synchronises the streams that ran it first.
void sail_jit_hold(int device, const SailJitSpec& spec, int delta);
// host only: the code object for `arch`, built by the same path (sail_jit_compile, sail_jit_prebuild); blocks
int sail_jit_code(const char* arch, const SailJitSpec& spec, void* code, size_t* bytes, std::string* err);
// the on-disk code-object cache directory: nullptr = the default ($XDG_CACHE_HOME or $HOME/.cache, /sail_amd/jit),
// "" = none (sail_set_jit_cache); `dir` of sail_jit_code / prebuild when it is not null
void sail_jit_set_cache_dir(const char* dir);
// The user's cache keeps at most this many value-kernel objects (a scene at rest in a new pose is a new object): writing
// one more deletes the oldest by modification time. 32 is a choice, not a measurement. Value objects live in a directory
// of their own beside each cache directory (<dir>-values), so types kernels are not counted and never deleted by this
// rule; the cache shipped with the library is never pruned.
constexpr int kSailJitMaxValueObjects = 32;
int sail_jit_code_to_dir(const char* arch, const SailJitSpec& spec, const char* dir, std::string* err);
// FNV-1a 64 of the library image plus a precompiled kernel's name: the build identity of a precompiled kernel
uint64_t sail_precompiled_build_id(const char* kernel);
// host only: the disk caches' key of `spec` for `arch` and, when defs is not null, the source prefix it is compiled with
// (no compile; -1 for an invalid spec)
int sail_jit_key(const char* arch, const SailJitSpec& spec, uint64_t* key, std::string* defs, std::string* err);
// what the process keeps of value kernels: code objects in memory and loaded modules (all devices). Both fall back as
// the last hold on a value spec is dropped (sail_jit_hold), so they are bounded by the contexts that hold one.
void sail_jit_resident_values(int* code_objects, int* modules);
