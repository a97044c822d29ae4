// sail_geom.h — the geometry of the trace kernels: the vector and ray types, the scene context (Ctx) and the row tables
// of the value kernels, the textures the hit records evaluate, every shape's intersector and hit record, the candidate
// sweep of the pre-cull kernel, and the hit-record and row-shading dispatch. Part of a run-time kernel's text
// (sail_amd/gen_jit_src.py): an edit here changes every run-time kernel's cache key. sail_temporal.hip, sail_albedo.hip
// and the picker (sail_frame.hip) use mkRay, primT, constRow and hitRecordU from here.
#pragma once
#if !defined(__HIPCC_RTC__)  // hipRTC (the per-plugin-set kernels, sail_jit.cpp) provides the HIP runtime and stdint
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "sail_device.h"
#include "sail_math.h"

using namespace sm;

#define D __device__ __forceinline__

namespace {

constexpr float kMaxDistance = 1e5f, kEps = 1e-5f, kOneMinusEps = 0.9999f, kInf = 1e5f;
constexpr float kPI = 3.141592653589793f, kInvPI = 0.3183098861837907f;
constexpr float kPiOver2 = 1.570796326794896f, kPiOver4 = 0.785398163397448f;

struct V3 { float x, y, z; };
struct V2 { float x, y; };
D V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
D V3 v3s(float s) { return v3(s, s, s); }
D V2 v2(float x, float y) { V2 r; r.x = x; r.y = y; return r; }
D V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
D V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
D V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
// GLSL division (sail_math.h fdiv: a * RN(1/b)); a vector over a scalar shares one reciprocal
D V3 operator/(V3 a, V3 b) { return v3(fdiv(a.x, b.x), fdiv(a.y, b.y), fdiv(a.z, b.z)); }
D V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
D V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
D V3 operator/(V3 a, float s) { const float r = rcp_rn(s); return v3(a.x * r, a.y * r, a.z * r); }
D V3 operator+(V3 a, float s) { return v3(a.x + s, a.y + s, a.z + s); }
D V3 operator-(V3 a, float s) { return v3(a.x - s, a.y - s, a.z - s); }
D V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
D V2 operator*(float s, V2 a) { return v2(s * a.x, s * a.y); }
D float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
D float length(V3 v) { return sqrtf_(dot(v, v)); }
D V3 normalize(V3 v) { return v / length(v); }
D V3 vmin(V3 a, V3 b) { return v3(fmin_(a.x, b.x), fmin_(a.y, b.y), fmin_(a.z, b.z)); }
D V3 vmax(V3 a, V3 b) { return v3(fmax_(a.x, b.x), fmax_(a.y, b.y), fmax_(a.z, b.z)); }
D V3 vclamp01(V3 x) { return v3(clamp_(x.x, 0.0f, 1.0f), clamp_(x.y, 0.0f, 1.0f), clamp_(x.z, 0.0f, 1.0f)); }
D bool isBlack(V3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }
D V3 reflect_(V3 I, V3 N) { return I - (2.0f * dot(N, I)) * N; }
D V3 refract_(V3 I, V3 N, float eta) {
  const float dni = dot(N, I);
  const float k = 1.0f - eta * eta * (1.0f - dni * dni);
  if (k < 0.0f) return v3s(0.0f);
  return eta * I - (eta * dni + sqrtf_(k)) * N;
}
D V3 worldToLocal(V3 v, V3 ns, V3 ss, V3 ts) { return v3(dot(v, ss), dot(v, ts), dot(v, ns)); }
D V3 localToWorld(V3 v, V3 ns, V3 ss, V3 ts) {
  return v3(ss.x * v.x + ts.x * v.y + ns.x * v.z, ss.y * v.x + ts.y * v.y + ns.y * v.z,
            ss.z * v.x + ts.z * v.y + ns.z * v.z);
}
// Box faces (Cube, Cornellbox): normal, dpdu, dpdv, ss and ts all have components in {0, +-1}, so every product of
// their dot products, cross products and frame changes is exact, and each a*b + c rounds once: written fma(a, b, c),
// bit for bit the unfused sum (the zero-sum sign rule of fma is the addition's; 0 * inf / NaN is NaN either way).
// Measured bit-identical with ~20 fewer VALU per box-face bounce: C2 -1.2 %, C3 -0.8 % (the second shading-frame
// branch costs more than it saves there), C4 +0.9 %: the pre-cull kernel only (Hit.axis).
D float dotX(V3 a, V3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
D V3 crossX(V3 a, V3 b) {
  return v3(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x)));
}
D V3 localToWorldX(V3 v, V3 ns, V3 ss, V3 ts) {
  return v3(fma_(ns.x, v.z, fma_(ts.x, v.y, ss.x * v.x)), fma_(ns.y, v.z, fma_(ts.y, v.y, ss.y * v.x)),
            fma_(ns.z, v.z, fma_(ts.z, v.y, ss.z * v.x)));
}
// OBJECT_SPACE_N/S/T (define.glsl:62-64): the full dot products of the reference, so -0 / NaN propagate the same.
// A product with an exact 0 is exact (a signed zero, or NaN), so "a*0 + b" rounds once either way and is written
// fma(a, 0, b): bit for bit the same sum (the zero-sum sign rule of fma is the addition's) in fewer instructions.
D V3 W2L(V3 v) {  // (dot(v, (0,0,-1)), dot(v, (1,0,0)), dot(v, (0,1,0)))
  return v3(fma_(v.y, 0.0f, v.x * 0.0f) - v.z, fma_(v.z, 0.0f, fma_(v.y, 0.0f, v.x)), fma_(v.z, 0.0f, fma_(v.x, 0.0f, v.y)));
}
D V3 L2W(V3 v) {  // (0,0,-1) v.x + (1,0,0) v.y + (0,1,0) v.z, row by row as localToWorld sums them
  return v3(fma_(v.z, 0.0f, fma_(v.x, 0.0f, v.y)), fma_(v.y, 0.0f, v.x * 0.0f) + v.z, fma_(v.z, 0.0f, fma_(v.y, 0.0f, -v.x)));
}
D bool equalZero(float x) { return x < 1e-3f && x > -1e-3f; }
D float sgn(int rev) { return rev ? -1.0f : 1.0f; }

// utility.glsl:37-51, whole (PART 0) or in two parts for a sweep that defers a sphere's roots (sphereT below): 1 the
// discriminant alone (false when it is negative), 2 the roots of a discriminant that is not negative
template <int PART>
D bool quadratic(float A, float B, float C, float& t0, float& t1, float& discrim) {
  if constexpr (PART != 2) {
    discrim = B * B - 4.0f * A * C;
    if (discrim < 0.0f) return false;
  }
  if constexpr (PART != 1) {
    const float rootDiscrim = sqrtf_(discrim);
    float q;
    if (B < 0.0f) q = -0.5f * (B - rootDiscrim);
    else q = -0.5f * (B + rootDiscrim);
    t0 = fdiv(q, A);
    t1 = fdiv(C, q);
    if (t0 > t1) { const float tmp = t0; t0 = t1; t1 = tmp; }
  }
  return true;
}
D bool quadratic(float A, float B, float C, float& t0, float& t1) {
  float discrim = 0.0f;
  return quadratic<0>(A, B, C, t0, t1, discrim);
}

// A path segment: origin and direction. It is what the path loop carries from bounce to bounce, what the packed path
// state moves through LDS, and all that a hit record or the shading reads of a ray.
struct Seg { V3 o, d; };
// A ray carries the reciprocals of its direction: every slab test divides by the same three components, and
// under the GLSL division spec a / d.x is a * RN(1/d.x), so a slab is six subtractions and six multiplies.
// In the flat forms it is built (mkRay) where it is swept and lives no longer than the sweep; the pre-cull form carries
// it (PathRay below).
struct Ray : Seg { float rx, ry, rz; };
D Ray mkRay(V3 o, V3 d) {
  Ray r; r.o = o; r.d = d;
  // one range guard for the three components (rcp_rn guards each)
  const float mx = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)), mn = fminf(fminf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
  // wave-uniform: the IEEE reciprocals (equal to the Newton step in range) for every lane when some lane is out of range
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(mn >= 0x1p-126f && mx <= 0x1p126f)) == 0ull, 1)) {
    const float y0 = __builtin_amdgcn_rcpf(d.x), y1 = __builtin_amdgcn_rcpf(d.y), y2 = __builtin_amdgcn_rcpf(d.z);
    r.rx = fma_(fma_(-d.x, y0, 1.0f), y0, y0);
    r.ry = fma_(fma_(-d.y, y1, 1.0f), y1, y1);
    r.rz = fma_(fma_(-d.z, y2, 1.0f), y2, y2);
  } else {
    r.rx = 1.0f / d.x; r.ry = 1.0f / d.y; r.rz = 1.0f / d.z;
  }
  return r;
}
// What a path carries from bounce to bounce, by kernel form (traceTileCompact):
//  * flat forms (Cornell, room, all-plugin): the segment alone. The reciprocals are built inside the sweep's `if (alive)`
//    and die there, so the sort and the shading hold no registers for them and nothing zeroes them (value kernel of
//    the Cornell box: 161 VALU and 18 v_rcp_f32 fewer in the code, 1 spilled VGPR fewer; C2 +0.8 % on top of the
//    all-lane gather, C5 +1.8 % and C3 +0.5 % with it: DESIGN.md, round 19). The same rcp_rn of the same three values
//    once per traced segment; the last bounce's shading no longer computes a dead ray's.
//  * pre-cull form: the ray with its reciprocals, built by the shading (mkRay) and zeroed after the gather, as before.
//    Its kernel spills 80 VGPRs as it is, and the segment form raised that to 98 and lost 0.75 % on C4 (spread 0.6 %).
// One text serves both through these overloads: the segment's next value, the ray to sweep, the end of the reciprocals.
template <bool CARRY_RCP> struct PathRay { using type = Seg; };
template <> struct PathRay<true> { using type = Ray; };
D void nextRay(Seg& r, V3 o, V3 d) { r.o = o; r.d = d; }
D void nextRay(Ray& r, V3 o, V3 d) { r = mkRay(o, d); }
D Ray sweptRay(const Seg& r) { return mkRay(r.o, r.d); }
D const Ray& sweptRay(const Ray& r) { return r; }
D void dropRcp(Seg&) {}
D void dropRcp(Ray& r) { r.rx = r.ry = r.rz = 0.0f; }  // not used past the sweep: the next ray is rebuilt by mkRay
struct Hit {
  float d; V3 hit, normal, dpdu, dpdv; bool into; int matRow; V3 sc, emission; int matCategory;
  float nd;  // dot(geometric normal before the into flip, ray direction)
  bool axis; // box face in the pre-cull kernel: normal / dpdu / dpdv components in {0, +-1} (dotX, crossX)
};
struct Ctx {
  const float* tp; const float* lt; const int32_t* lightObjRow; const SailPrim* prims;
  const SailPrim* cprims;  // rows for the candidate loops' per-lane reads: an LDS copy when it fits (kCullLdsRows)
  const float* tpl;        // texParams rows, an LDS copy when they fit (kCullLdsTp)
  bool rowCopy, tpCopy;    // per-lane hit-record / light-sampler row reads and texParams reads go through cprims / tpl
  const unsigned long long* typeMasks;
  int n, tn, ln;
  uint32_t matMask, texMask, lightMask;
  float fcx, fcy;
  int shadowAnyHit;
  int cullPrims;
  int cullFma;     // the candidate sweep's pre-cull in the fused form (padHitFMask)
  int cullPrimary; // primary rays may use the pre-cull (the eye is near the scene)
  // plugin sets compiled into this kernel instantiation (compile-time constants after inlining): the
  // reference generates one GLSL program per scene plugin set (shader.js combinefs); this build precompiles
  // kernels for plugin subsets and dispatches the smallest one that covers the scene
  uint32_t kShapes, kMats, kTex, kLights;
};
#define HAS(set, id) (((set) >> (id)) & 1u)

// Scene rows are read through the constant address space: the kernels also store to global memory (AOVs,
// stage, accumulator) through pointers the compiler cannot prove disjoint from the scene, and without this
// a wave-uniform primitive read becomes a per-lane vector load (VGPRs + TA cycles) instead of a scalar load.
template <typename T> using ConstAS = const __attribute__((address_space(4))) T;
template <typename T> D const T& constRow(const T* base, int i) { return *(const T*)((ConstAS<T>*)base + i); }
// A flat kernel compiled at run time for a settled scene's row values (SAIL_JIT_ROWVALS, sail_jit.cpp; the host asks for
// it once the rows have stood still for a while, sail_capi.cpp refreshValues) carries the decoded rows and the
// texParams table as word lists in its source prefix: the bytes of the arrays the host uploads, bit for bit (-0, NaN
// payloads, denormals). gfx950 has no scalar float ALU, so every wave-uniform float expression on row data (mn + 1e-4,
// c - rad, rad * rad, rev ? -nd : nd) is a VALU instruction per wave and bounce, and the loaded rows live in SGPRs that
// spill through v_writelane: with the rows constant, those expressions fold and the loads go. Same operations on the
// same operands, so the frames are those of the types kernel (tests/test_gpu_jit_values.py).
#if defined(SAIL_JIT) && defined(SAIL_JIT_ROWVALS) && SAIL_JIT_ROWVALS && SAIL_JIT_N > 0
#define SAIL_ROWVALS 1
template <class... T> constexpr int wordCount(T...) { return (int)sizeof...(T); }
static_assert(sizeof(SailPrim) == 128, "a row is 32 words");
static_assert(wordCount(SAIL_JIT_ROW_WORDS) == SAIL_JIT_N * 32, "32 words per row");
constexpr int kTpC = SAIL_JIT_TPN;  // texParams rows compiled in (0: the scene has none)
static_assert(wordCount(SAIL_JIT_TP_WORDS) == (kTpC > 0 ? kTpC * 16 : 1), "16 words per texParams row");
struct PrimWordsC { uint32_t w[SAIL_JIT_N * 32]; };
struct PrimTabC { SailPrim r[SAIL_JIT_N]; };
struct TpWordsC { uint32_t w[kTpC > 0 ? kTpC * 16 : 1]; };
struct TpTabC { float v[kTpC > 0 ? kTpC * 16 : 1]; };
constexpr PrimWordsC kPrimW = {{SAIL_JIT_ROW_WORDS}};
constexpr TpWordsC kTpW = {{SAIL_JIT_TP_WORDS}};
constexpr PrimTabC kPrimTab = __builtin_bit_cast(PrimTabC, kPrimW);
constexpr TpTabC kTpTab = __builtin_bit_cast(TpTabC, kTpW);
#define PRIM(c, i) (kPrimTab.r[(i)])
#else
#define SAIL_ROWVALS 0
#define PRIM(c, i) constRow<SailPrim>((c).prims, (i))
#endif
// Row shading (SAIL_JIT_ROWSHADE = a mask of rows, in a value kernel of at most kRowRecordMax rows; SAIL_DEBUG_JIT bit
// 32): a row-uniform wave of a row in the mask runs the rest of its bounce -- AOV store, radiance update, BSDF sample,
// next ray -- inside its row's branch of the hit record (bounceU), so that the row's material category, matRow,
// texParams values, rev and emission words are constants of that copy of the shading too. Mixed waves and the other
// rows' waves keep the one generic body. The host names the quiet rows (sail_capi.cpp valueSpecFor: a copy for every
// row measured -4.8 % on C2, copies for the quiet rows +6.7 %); a mask of 0 is the plain value kernel's text.
#if SAIL_ROWVALS && defined(SAIL_JIT_ROWSHADE) && SAIL_JIT_ROWSHADE
#define SAIL_ROWSHADE 1
#else
#define SAIL_ROWSHADE 0
#endif
// A deferred row (SAIL_JIT_ROWDEFER = the index of a Sphere row of a flat value kernel; absent or -1: none; SAIL_DEBUG_JIT
// bit 64 leaves it out). At the bounces that sort their paths and are not the last, the sweep runs only the head of
// that row's sphereT. A lane whose discriminant is not negative is a candidate: it is sorted under the sphere's key with
// its winner among the other rows, and the sphere's waves run the tail after the gather (sphereResolve), where nearly
// every lane needs it, instead of nearly every wave of the sweep running it for one lane in ten. Same operations on
// the same operands, and the sweep's strict-`<`, first-index rule decides between the sphere and the provisional winner.
#if defined(SAIL_JIT_ROWDEFER) && SAIL_JIT_ROWDEFER >= 0
#define SAIL_ROWDEFER 1
static_assert(SAIL_ROWVALS, "a deferred row: in a value kernel");
static_assert(!SAIL_JIT_CULL && !SAIL_JIT_FAM, "a deferred row: in the flat form");
constexpr int kDeferRow = SAIL_JIT_ROWDEFER;
#else
#define SAIL_ROWDEFER 0
constexpr int kDeferRow = -1;
#endif

D V3 P3(const SailPrim& p, int k) { return v3(p.a[k], p.a[k + 1], p.a[k + 2]); }
D float TP(const Ctx& c, int row, int col) {
#if SAIL_ROWVALS
  return kTpTab.v[row * 16 + col];
#else
  if (c.tpCopy) return c.tpl[row * 16 + col];  // kernels with table copies in LDS (compile-time)
  return constRow<float>(c.tp, row * 16 + col);
#endif
}
D V3 TP3(const Ctx& c, int row, int col) { return v3(TP(c, row, col), TP(c, row, col + 1), TP(c, row, col + 2)); }

// ---- textures (shader.texture.js:22-29) ----------------------------------------------------------------
// The pre-cull kernel's two checkerboards share uv / size and its floor, so a wave holding both runs them once (same
// operations). Measured (bit-identical, profiles/r03_variants_tex_shared.jsonl, three rounds): C3 -1.4 %, C4 +0.7 %
// (its 64 rows mix both textures in most waves), so the flat kernels keep one branch per texture.
// UNIFORM_COLOR ignores uv, so hit records skip the UV arithmetic (atan2/acos/divides) for it
D int matCat(const SailPrim& p) { return (int)(short)(p.cats & 0xffff); }
D int texCat(const SailPrim& p) { return p.cats >> 16; }
D bool needsUV(const SailPrim& p) { return texCat(p) != SAIL_TEX_UNIFORM; }
D V3 getSurfaceColor(const Ctx& c, V2 uv, const SailPrim& p) {
  const int texRow = p.texRow, cat = texCat(p);
  if (cat == SAIL_TEX_UNIFORM) return TP3(c, texRow, 1);
  if (cat < 0 || cat >= 32 || !((c.texMask >> cat) & 1u)) return v3s(0.0f);
  // c.cullPrims is a compile-time constant in every kernel (the pre-cull ones set 1)
  if (c.cullPrims &&
      ((cat == SAIL_TEX_CHECKERBOARD && HAS(c.kTex, SAIL_TEX_CHECKERBOARD)) ||
       (cat == SAIL_TEX_CHECKERBOARD2 && HAS(c.kTex, SAIL_TEX_CHECKERBOARD2)))) {
    const bool cb1 = cat == SAIL_TEX_CHECKERBOARD;
    const float size = cb1 ? TP(c, texRow, 1) : TP(c, texRow, 7);
    const float sx = fdiv(uv.x, size), sy = fdiv(uv.y, size);
    const float qx = floorf(sx), qy = floorf(sy);
    if (cb1) {
      const float width = fdiv(0.5f * TP(c, texRow, 2), size);
      const float fx = sx - qx, fy = sy - qy;
      const bool in_outline = (fx < width || fx > 1.0f - width) || (fy < width || fy > 1.0f - width);
      return in_outline ? v3s(0.5f) : v3s(1.0f);
    }
    return (to_int(qx + qy) % 2 == 0) ? TP3(c, texRow, 1) : TP3(c, texRow, 4);
  }
  switch (cat) {
    case SAIL_TEX_CHECKERBOARD: if (!HAS(c.kTex, SAIL_TEX_CHECKERBOARD)) break; {
      const float size = TP(c, texRow, 1), lineWidth = TP(c, texRow, 2);
      const float width = fdiv(0.5f * lineWidth, size);
      const float fx = fdiv(uv.x, size) - floorf(fdiv(uv.x, size)), fy = fdiv(uv.y, size) - floorf(fdiv(uv.y, size));
      const bool in_outline = (fx < width || fx > 1.0f - width) || (fy < width || fy > 1.0f - width);
      return in_outline ? v3s(0.5f) : v3s(1.0f);
    }
    case SAIL_TEX_CHECKERBOARD2: if (!HAS(c.kTex, SAIL_TEX_CHECKERBOARD2)) break; {
      const float size = TP(c, texRow, 7);
      const float qx = floorf(fdiv(uv.x, size)), qy = floorf(fdiv(uv.y, size));
      return (to_int(qx + qy) % 2 == 0) ? TP3(c, texRow, 1) : TP3(c, texRow, 4);
    }
    case SAIL_TEX_BILERP: if (!HAS(c.kTex, SAIL_TEX_BILERP)) break; {
      const V3 c00 = TP3(c, texRow, 1), c01 = TP3(c, texRow, 4), c10 = TP3(c, texRow, 7), c11 = TP3(c, texRow, 10);
      return (1.0f - uv.x) * (1.0f - uv.y) * c00 + (1.0f - uv.x) * (uv.y) * c01 + (uv.x) * (1.0f - uv.y) * c10 +
             (uv.x) * (uv.y) * c11;
    }
    case SAIL_TEX_MIXF: if (!HAS(c.kTex, SAIL_TEX_MIXF)) break; {
      const float amount = TP(c, texRow, 7);
      return (1.0f - amount) * TP3(c, texRow, 1) + amount * TP3(c, texRow, 4);
    }
    case SAIL_TEX_SCALE: if (!HAS(c.kTex, SAIL_TEX_SCALE)) break; return TP3(c, texRow, 1) * TP3(c, texRow, 4);
    case SAIL_TEX_UVF: if (!HAS(c.kTex, SAIL_TEX_UVF)) break; return v3(uv.x - floorf(uv.x), uv.y - floorf(uv.y), 0.0f);
    default: break;
  }
  return v3s(0.0f);
}

// ---- slab boxes: cube.glsl:65-87, cornellbox.glsl:67-90, boundbox.glsl:6-17 ------------------------------
struct Slab { float tNear, tFar; };
D Slab slab(V3 bmin, V3 bmax, const Ray& r) {
  const V3 a0 = bmin - r.o, a1 = bmax - r.o;
  const V3 tMin = v3(a0.x * r.rx, a0.y * r.ry, a0.z * r.rz);  // (bmin - o) / d
  const V3 tMax = v3(a1.x * r.rx, a1.y * r.ry, a1.z * r.rz);
  const V3 t1 = vmin(tMin, tMax), t2 = vmax(tMin, tMax);
  Slab s;
  s.tNear = fmax_(fmax_(t1.x, t1.y), t1.z);
  s.tFar = fmin_(fmin_(t2.x, t2.y), t2.z);
  return s;
}
// Boundbox(max, min) constructor order (boundbox.glsl:1-4): the `min` member is the 2nd argument
D bool testBoundbox(const Ray& r, V3 bmax, V3 bmin) {
  const Slab s = slab(bmin, bmax, r);
  if (s.tNear < 0.0f && s.tFar < 0.0f) return false;
  return s.tNear < s.tFar;
}
D float cubeT(const SailPrim& p, const Ray& r) {
  const Slab s = slab(P3(p, 0), P3(p, 3), r);
  float t = -1.0f;
  if (s.tNear > kEps && s.tNear < s.tFar) t = s.tNear;
  else if (s.tNear < s.tFar) t = s.tFar;
  return (t > kEps) ? t : kMaxDistance;
}
D float cornellT(const SailPrim& p, const Ray& r) {
  const Slab s = slab(P3(p, 0), P3(p, 3), r);
  float t = -1.0f;
  if (s.tNear < s.tFar) t = s.tFar;
  return (t > kEps) ? t : kMaxDistance;
}
D V3 normalForCube(V3 hit, const SailPrim& p) {  // cube.glsl:25-38
  const float c = sgn(p.rev);
  const V3 mn = P3(p, 0), mx = P3(p, 3);
  if (hit.x < mn.x + 0.0001f) return c * v3(-1.0f, 0.0f, 0.0f);
  else if (hit.x > mx.x - 0.0001f) return c * v3(1.0f, 0.0f, 0.0f);
  else if (hit.y < mn.y + 0.0001f) return c * v3(0.0f, -1.0f, 0.0f);
  else if (hit.y > mx.y - 0.0001f) return c * v3(0.0f, 1.0f, 0.0f);
  else if (hit.z < mn.z + 0.0001f) return c * v3(0.0f, 0.0f, -1.0f);
  return c * v3(0.0f, 0.0f, 1.0f);
}
D V3 normalForCornellbox(V3 hit, const SailPrim& p) {  // cornellbox.glsl:39-51
  const V3 mn = P3(p, 0), mx = P3(p, 3);
  if (hit.x < mn.x + 0.0001f) return v3(-1.0f, 0.0f, 0.0f);
  else if (hit.x > mx.x - 0.0001f) return v3(1.0f, 0.0f, 0.0f);
  else if (hit.y < mn.y + 0.0001f) return v3(0.0f, -1.0f, 0.0f);
  else if (hit.y > mx.y - 0.0001f) return v3(0.0f, 1.0f, 0.0f);
  else if (hit.z < mn.z + 0.0001f) return v3(0.0f, 0.0f, -1.0f);
  return v3(0.0f, 0.0f, 1.0f);
}
D void dpdBox(V3 normal, V3& dpdu, V3& dpdv) {
  const V3 n = normal;  // cross(n, (1,0,0)) / cross(n, (0,1,0)) with the exact zero products folded (see W2L)
  if (fabsf(n.x) < 0.5f) dpdu = v3(fma_(n.y, 0.0f, n.z * -0.0f), fma_(n.x, -0.0f, n.z), fma_(n.x, 0.0f, -n.y));
  else dpdu = v3(fma_(n.y, 0.0f, -n.z), fma_(n.z, 0.0f, n.x * -0.0f), fma_(n.y, -0.0f, n.x));
  dpdv = cross(normal, dpdu);
}
D void cubeHit(const Ctx& c, const SailPrim& p, const Seg& r, float t, Hit& h) {
  h.hit = r.o + t * r.d;
  h.normal = normalForCube(r.o + t * r.d, p);
  dpdBox(h.normal, h.dpdu, h.dpdv);
  V2 uv = v2(0.0f, 0.0f);
  if (needsUV(p)) {
    const V3 mn = P3(p, 0), mx = P3(p, 3);
    const V3 tr = mx - mn, hh = h.hit - mn;  // getCubeUV cube.glsl:54-63
    if (hh.x < mn.x + 0.0001f || hh.x > mx.x - 0.0001f) uv = v2(fdiv(hh.y, tr.y), fdiv(hh.z, tr.z));
    else if (hh.y < mn.y + 0.0001f || hh.y > mx.y - 0.0001f) uv = v2(fdiv(hh.x, tr.x), fdiv(hh.z, tr.z));
    else uv = v2(fdiv(hh.x, tr.x), fdiv(hh.y, tr.y));
  }
  h.sc = getSurfaceColor(c, uv, p);
}
// The wall colour chain (cornellbox.glsl:53-65) tests the same face conditions in the same order as the normal
// chain (:39-51), except its last test, z > mn.z + 0.0001 where the normal's is z < mn.z + 0.0001: one chain sets
// both (z < t excludes z > t; after it the colour test is made as written). Same values, each face test once:
// 1 = one branch chain, 2 = branch-free selects. Bit-identical but slower (C2 -4.7 % / -3.8 %: more constant moves per
// branch and more spills), so the default keeps the reference's two chains.
D void cornellHit(const SailPrim& p, const Seg& r, float t, Hit& h) {
  h.hit = r.o + t * r.d;
  h.normal = -normalForCornellbox(r.o + t * r.d, p);
  dpdBox(h.normal, h.dpdu, h.dpdv);
  const V3 mn = P3(p, 0), mx = P3(p, 3), x = h.hit;
  if (x.x < mn.x + 0.0001f) h.sc = v3(0.25f, 0.75f, 0.25f);
  else if (x.x > mx.x - 0.0001f) h.sc = v3(0.25f, 0.25f, 0.75f);
  else if (x.y < mn.y + 0.0001f) h.sc = v3s(1.0f);
  else if (x.y > mx.y - 0.0001f) h.sc = v3s(1.0f);
  else if (x.z > mn.z + 0.0001f) h.sc = v3s(1.0f);
  else h.sc = v3s(0.0f);
}

// The room kernel's one hit record for both axis-aligned box shapes (a wave holding Cube and Cornellbox lanes runs one
// face chain instead of two). The face chains test the same conditions; the Cube's normal is sgn(rev) * n and the
// Cornellbox's is -n == -1 * n bit for bit (zeros included); only the surface colour differs (texture vs wall chain).
// Measured (bit-identical, profiles/r03_variants_box_unified*.jsonl): room kernel C3 +0.7 %; every kernel C2 -0.8 %,
// C4 +0.1 %; only in mixed waves C2 +-0.2 %, C3 -0.7 %, so the room kernel alone takes it.
D void boxHit(const Ctx& c, const SailPrim& p, const Seg& r, float t, Hit& h, bool cornell) {
  h.hit = r.o + t * r.d;
  const float s = cornell ? -1.0f : sgn(p.rev);
  h.normal = s * normalForCornellbox(r.o + t * r.d, p);
  dpdBox(h.normal, h.dpdu, h.dpdv);
  const V3 mn = P3(p, 0), mx = P3(p, 3), x = h.hit;
  if (cornell) {
    if (x.x < mn.x + 0.0001f) h.sc = v3(0.25f, 0.75f, 0.25f);
    else if (x.x > mx.x - 0.0001f) h.sc = v3(0.25f, 0.25f, 0.75f);
    else if (x.y < mn.y + 0.0001f) h.sc = v3s(1.0f);
    else if (x.y > mx.y - 0.0001f) h.sc = v3s(1.0f);
    else if (x.z > mn.z + 0.0001f) h.sc = v3s(1.0f);
    else h.sc = v3s(0.0f);
  } else {
    V2 uv = v2(0.0f, 0.0f);
    if (needsUV(p)) {
      const V3 tr = mx - mn, hh = h.hit - mn;  // getCubeUV cube.glsl:54-63
      if (hh.x < mn.x + 0.0001f || hh.x > mx.x - 0.0001f) uv = v2(fdiv(hh.y, tr.y), fdiv(hh.z, tr.z));
      else if (hh.y < mn.y + 0.0001f || hh.y > mx.y - 0.0001f) uv = v2(fdiv(hh.x, tr.x), fdiv(hh.z, tr.z));
      else uv = v2(fdiv(hh.x, tr.x), fdiv(hh.y, tr.y));
    }
    h.sc = getSurfaceColor(c, uv, p);
  }
}

// The quadrics' bounding-box test (testBoundboxFor*) and their root search are both pure predicates on the
// ray, so their order is free: the discriminant rejects most rays more cheaply than the six-divide slab test,
// and only candidate hits pay the exact slab test (same results; C3 +4 %, C4 +5 %, measured).
// ---- sphere.glsl:45-86 ---------------------------------------------------------------------------------------
// In two parts. The head, up to the discriminant, is what every ray pays; the tail -- the square root, the two divides,
// the root choice and the slab test -- is what only a ray whose discriminant is not negative runs. sphereT is the head
// followed by the tail; a sweep that defers the row (SAIL_JIT_ROWDEFER below) runs the head in the sweep and the tail
// after the path sort, on the same operands.
// One text, three uses (PART): 0 the whole test; 1 the head alone, which fills q and returns kMaxDistance for a
// negative discriminant, else 0; 2 the tail, from a q whose discriminant is not negative.
struct SphereQuad { V3 o, d; float a, b, cc, discrim; };
template <int PART>
D float sphereT(const SailPrim& p, const Ray& r0, V3* hitOut, SphereQuad& q) {
  const V3 c = P3(p, 0);
  const float rad = p.a[3];
  float t1 = 0.0f, t2 = 0.0f;
  if constexpr (PART != 2) {
    q.d = W2L(r0.d); q.o = W2L(r0.o - c);
    q.a = dot(q.d, q.d); q.b = 2.0f * dot(q.o, q.d); q.cc = dot(q.o, q.o) - rad * rad;
    if (!quadratic<1>(q.a, q.b, q.cc, t1, t2, q.discrim)) return kMaxDistance;
  }
  if constexpr (PART == 1) return 0.0f;
  quadratic<2>(q.a, q.b, q.cc, t1, t2, q.discrim);
  if (t2 < kEps) return kMaxDistance;
  float t = t1;
  if (t1 < kEps) t = t2;
  if (t >= kMaxDistance) return kMaxDistance;
  if (!testBoundbox(r0, c - v3s(rad), c + v3s(rad))) return kMaxDistance;
  if (hitOut) *hitOut = q.o + t * q.d;
  return t;
}
D float sphereT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  SphereQuad q;
  return sphereT<0>(p, r0, hitOut, q);
}
D float phiOf(float y, float x) {
  float phi = atan2f_(y, x);
  if (phi < 0.0f) phi += 2.0f * kPI;
  return phi;
}
D V3 dpduRot(V3 hit) { return v3(-2.0f * kPI * hit.y, 2.0f * kPI * hit.x, 0.0f); }
// cross(a, b) with a.z == 0 (crossZa) or b.z == 0 (crossZb), the exact zero products folded as in W2L
D V3 crossZa(V3 a, V3 b) {
  return v3(fma_(b.y, -0.0f, a.y * b.z), fma_(b.x, 0.0f, -(a.x * b.z)), a.x * b.y - a.y * b.x);
}
D V3 crossZb(V3 a, V3 b) {
  return v3(fma_(a.y, 0.0f, -(a.z * b.y)), fma_(a.x, -0.0f, a.z * b.x), a.x * b.y - a.y * b.x);
}
D void sphereHit(const Ctx& c, const SailPrim& p, V3 hl, Hit& h) {
  const float rad = p.a[3];
  // theta of the UV and of computeDpDForSphere (:33-43) are the same value: the pole guard touches x only
  const float theta = acosf_(clamp_(fdiv(hl.z, rad), -1.0f, 1.0f));
  V2 uv = v2(0.0f, 0.0f);
  if (needsUV(p)) {
    V3 hit = hl;
    if (hit.x == 0.0f && hit.y == 0.0f) hit.x = 1e-5f * rad;
    uv = v2(fdiv(phiOf(hit.y, hit.x), 2.0f * kPI), fdiv(theta, kPI));
  }
  const float th2 = theta;
  const float zRadius = sqrtf_(hl.x * hl.x + hl.y * hl.y);
  const float invZRadius = rcp_rn(zRadius);
  const float cosPhi = hl.x * invZRadius, sinPhi = hl.y * invZRadius;
  const V3 dpdu = dpduRot(hl);
  const V3 dpdv = kPI * v3(hl.z * cosPhi, hl.z * sinPhi, -rad * sinf_(th2));
  const V3 nl = normalize(crossZb(dpdv, dpdu));  // dpdu.z == 0
  h.sc = getSurfaceColor(c, uv, p);
  h.hit = L2W(hl) + P3(p, 0);
  h.normal = L2W(nl);
  h.dpdu = L2W(dpdu);
  h.dpdv = L2W(dpdv);
}

// ---- rectangle.glsl:32-63 ---------------------------------------------------------------------------------
struct RectFrame { V3 dpdu, dpdv, normal, ss, ts; float maxX, maxY; };
D RectFrame rectFrame(const SailPrim& p) {  // rectangle.glsl:32-44; the divides/roots are per scene (host)
  RectFrame f;
  const V3 mn = P3(p, 0), mx = P3(p, 3);
  f.dpdu = v3(mx.x - mn.x, 0.0f, 0.0f);
  f.dpdv = v3(0.0f, mx.y - mn.y, mx.z - mn.z);
  f.normal = P3(p, 6); f.ss = P3(p, 9); f.ts = P3(p, 12);
  f.maxX = p.a[15]; f.maxY = p.a[16];
  return f;
}
D float rectT(const SailPrim& p, const Ray& r, V3* hitOut) {
  const RectFrame f = rectFrame(p);
  const V3 d = worldToLocal(r.d, f.normal, f.ss, f.ts);
  const V3 o = worldToLocal(r.o - P3(p, 0), f.normal, f.ss, f.ts);
  if (d.z == 0.0f) return kMaxDistance;
  const float t = fdiv(-o.z, d.z);
  if (t < kEps) return kMaxDistance;
  const V3 hit = o + t * d;
  if (hit.x > f.maxX || hit.y > f.maxY || hit.x < -kEps || hit.y < -kEps) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
D void rectHit(const Ctx& c, const SailPrim& p, V3 hl, Hit& h) {
  const RectFrame f = rectFrame(p);
  h.dpdu = f.dpdu; h.dpdv = f.dpdv; h.normal = f.normal;
  h.sc = getSurfaceColor(c, needsUV(p) ? v2(fdiv(hl.x, f.maxX), fdiv(hl.y, f.maxY)) : v2(0.0f, 0.0f), p);
  h.hit = localToWorld(hl, f.normal, f.ss, f.ts) + P3(p, 0);
}

// ---- cone.glsl:48-99 / cylinder.glsl:40-90 / hyperboloid.glsl:60-111 / paraboloid.glsl:51-103 ---------------
// shared tail: two-root retry against the z range, then the MAX_DISTANCE test
D bool rootPick(float t1, float t2, V3 o, V3 d, float zlo, float zhi, bool epsLo, float& t, V3& hit) {
  t = t1;
  if (t1 < kEps) t = t2;
  hit = o + t * d;
  const bool out = epsLo ? (hit.z < -kEps || hit.z > zhi) : (hit.z < zlo || hit.z > zhi);
  if (out) {
    if (t == t2) return false;
    t = t2;
    hit = o + t * d;
    const bool out2 = epsLo ? (hit.z < -kEps || hit.z > zhi) : (hit.z < zlo || hit.z > zhi);
    if (out2) return false;
  }
  return t < kMaxDistance;
}
D float coneT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  const V3 pp = P3(p, 0);
  const float h = p.a[3], rad = p.a[4];
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  const float k = p.a[5];  // (rad / h)^2, per scene
  const float a = d.x * d.x + d.y * d.y - k * d.z * d.z;
  const float b = 2.0f * (d.x * o.x + d.y * o.y - k * d.z * (o.z - h));
  const float cc = o.x * o.x + o.y * o.y - k * (o.z - h) * (o.z - h);
  float t1 = 0.0f, t2 = 0.0f, t; V3 hit;
  if (!quadratic(a, b, cc, t1, t2)) return kMaxDistance;
  if (t2 < -kEps) return kMaxDistance;
  if (!rootPick(t1, t2, o, d, 0.0f, h, true, t, hit)) return kMaxDistance;
  if (!testBoundbox(r0, pp - v3(rad, 0.0f, rad), pp + v3(rad, h, rad))) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
D float cylinderT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  const V3 pp = P3(p, 0);
  const float h = p.a[3], rad = p.a[4];
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  const float a = d.x * d.x + d.y * d.y;
  const float b = 2.0f * (d.x * o.x + d.y * o.y);
  const float cc = o.x * o.x + o.y * o.y - rad * rad;
  float t1 = 0.0f, t2 = 0.0f, t; V3 hit;
  if (!quadratic(a, b, cc, t1, t2)) return kMaxDistance;
  if (t2 < -kEps) return kMaxDistance;
  if (!rootPick(t1, t2, o, d, 0.0f, h, true, t, hit)) return kMaxDistance;
  if (!testBoundbox(r0, pp - v3(rad, 0.0f, rad), pp + v3(rad, h, rad))) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
D float hypT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  const V3 pp = P3(p, 0);
  const float ah = p.a[9], ch = p.a[10];
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  const float a = ah * d.x * d.x + ah * d.y * d.y - ch * d.z * d.z;
  const float b = 2.0f * (ah * d.x * o.x + ah * d.y * o.y - ch * d.z * o.z);
  const float cc = ah * o.x * o.x + ah * o.y * o.y - ch * o.z * o.z - 1.0f;
  float t1 = 0.0f, t2 = 0.0f, t; V3 hit;
  if (!quadratic(a, b, cc, t1, t2)) return kMaxDistance;
  if (t2 < -kEps) return kMaxDistance;
  const float zMin = p.a[12], zMax = p.a[13];
  if (!rootPick(t1, t2, o, d, zMin, zMax, false, t, hit)) return kMaxDistance;
  {  // testBoundboxForHyperboloid :13-24 (rMax, zMin, zMax per scene)
    const float rMax = p.a[11], zMin = p.a[12], zMax = p.a[13];
    if (!testBoundbox(r0, pp - v3(rMax, -zMin, rMax), pp + v3(rMax, zMax, rMax))) return kMaxDistance;
  }
  if (hitOut) *hitOut = hit;
  return t;
}
D float paraT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  const V3 pp = P3(p, 0);
  const float z0 = p.a[3], z1 = p.a[4], rad = p.a[5];
  const float zMin = fmin_(z0, z1), zMax = fmax_(z0, z1);
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  const float k = p.a[6];  // zMax / (rad * rad), per scene
  const float a = k * (d.x * d.x + d.y * d.y);
  const float b = 2.0f * k * (d.x * o.x + d.y * o.y) - d.z;
  const float cc = k * (o.x * o.x + o.y * o.y) - o.z;
  float t1 = 0.0f, t2 = 0.0f, t; V3 hit;
  if (!quadratic(a, b, cc, t1, t2)) return kMaxDistance;
  if (t2 < -kEps) return kMaxDistance;
  if (!rootPick(t1, t2, o, d, zMin, zMax, false, t, hit)) return kMaxDistance;
  if (!testBoundbox(r0, pp - v3(rad, -zMin, rad), pp + v3(rad, zMax, rad))) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
D float diskT(const SailPrim& p, const Ray& r0, V3* hitOut) {  // disk.glsl:36-75
  const V3 pp = P3(p, 0);
  const float rad = p.a[3], ri = p.a[4];
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  if (d.z == 0.0f) return kMaxDistance;
  const float t = fdiv(-o.z, d.z);
  if (t <= 0.0f) return kMaxDistance;
  const V3 hit = o + t * d;
  const float dist2 = hit.x * hit.x + hit.y * hit.y;
  if (dist2 > rad * rad || dist2 < ri * ri) return kMaxDistance;
  if (t >= kMaxDistance) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
// The pre-cull kernel's candidate sweep tests cones, cylinders, hyperboloids and paraboloids in one
// loop (quadT) instead of one loop per type. A wave then runs max-over-lanes(quadric candidates) iterations instead
// of the sum over the four types of max-over-lanes(candidates of the type). Per type only the coefficients and the
// z-range / box parameters differ; the ray transform, the root solve, rootPick and the box test are shared. Same
// operations on the same values as coneT / cylinderT / hypT / paraT (box test last). Candidates are visited out of
// row order either way (the take rule keeps the in-order winner).
// Measured (bit-identical, profiles/r03_variants_quad_shared.jsonl, three rounds): C4 +0.9 %; with the sphere in the
// same loop (its own root rule) -5.4 %, with the planar disk -0.6 %.
D float quadT(const SailPrim& p, const Ray& r0, V3* hitOut) {
  const int ty = p.type;
  const V3 pp = P3(p, 0);
  const V3 d = W2L(r0.d), o = W2L(r0.o - pp);
  float a, b, cc, zlo, zhi, bA, bB, bC;
  bool epsLo;
  if (ty == SAIL_CONE) {
    const float h = p.a[3], rad = p.a[4], k = p.a[5];
    a = d.x * d.x + d.y * d.y - k * d.z * d.z;
    b = 2.0f * (d.x * o.x + d.y * o.y - k * d.z * (o.z - h));
    cc = o.x * o.x + o.y * o.y - k * (o.z - h) * (o.z - h);
    zlo = 0.0f; zhi = h; epsLo = true; bA = rad; bB = 0.0f; bC = h;
  } else if (ty == SAIL_CYLINDER) {
    const float h = p.a[3], rad = p.a[4];
    a = d.x * d.x + d.y * d.y;
    b = 2.0f * (d.x * o.x + d.y * o.y);
    cc = o.x * o.x + o.y * o.y - rad * rad;
    zlo = 0.0f; zhi = h; epsLo = true; bA = rad; bB = 0.0f; bC = h;
  } else if (ty == SAIL_HYPERBOLOID) {
    const float ah = p.a[9], ch = p.a[10];
    a = ah * d.x * d.x + ah * d.y * d.y - ch * d.z * d.z;
    b = 2.0f * (ah * d.x * o.x + ah * d.y * o.y - ch * d.z * o.z);
    cc = ah * o.x * o.x + ah * o.y * o.y - ch * o.z * o.z - 1.0f;
    zlo = p.a[12]; zhi = p.a[13]; epsLo = false; bA = p.a[11]; bB = -p.a[12]; bC = p.a[13];
  } else {  // SAIL_PARABOLOID
    const float z0 = p.a[3], z1 = p.a[4], rad = p.a[5];
    const float zMin = fmin_(z0, z1), zMax = fmax_(z0, z1);
    const float k = p.a[6];
    a = k * (d.x * d.x + d.y * d.y);
    b = 2.0f * k * (d.x * o.x + d.y * o.y) - d.z;
    cc = k * (o.x * o.x + o.y * o.y) - o.z;
    zlo = zMin; zhi = zMax; epsLo = false; bA = rad; bB = -zMin; bC = zMax;
  }
  float t1 = 0.0f, t2 = 0.0f, t; V3 hit;
  if (!quadratic(a, b, cc, t1, t2)) return kMaxDistance;
  if (t2 < -kEps) return kMaxDistance;
  if (!rootPick(t1, t2, o, d, zlo, zhi, epsLo, t, hit)) return kMaxDistance;
  if (!testBoundbox(r0, pp - v3(bA, bB, bA), pp + v3(bA, bC, bA))) return kMaxDistance;
  if (hitOut) *hitOut = hit;
  return t;
}
// local-space tail shared by the quadrics and the disk: normal from dpdu x dpdv, texture, back to world
// dpdu is dpduRot(hit) for every caller (z == 0)
D void finishLocal(const Ctx& c, const SailPrim& p, V3 hl, V2 uv, V3 dpdu, V3 dpdv, Hit& h) {
  const V3 nl = normalize(crossZa(dpdu, dpdv));
  h.sc = getSurfaceColor(c, uv, p);
  h.hit = L2W(hl) + P3(p, 0);
  h.normal = L2W(nl);
  h.dpdu = L2W(dpdu);
  h.dpdv = L2W(dpdv);
}
D void coneHit(const Ctx& c, const SailPrim& p, V3 hit, Hit& h) {
  const float hh = p.a[3];
  const V2 uv = needsUV(p) ? v2(fdiv(phiOf(hit.y, hit.x), 2.0f * kPI), fdiv(hit.z, hh)) : v2(0.0f, 0.0f);
  const float vv = fdiv(hit.z, hh);
  const V3 dpdv = v3(fdiv(-hit.x, 1.0f - vv), fdiv(-hit.y, 1.0f - vv), hh);
  finishLocal(c, p, hit, uv, dpduRot(hit), dpdv, h);
}
D void cylinderHit(const Ctx& c, const SailPrim& p, V3 hit, Hit& h) {
  const float hh = p.a[3];
  const V2 uv = needsUV(p) ? v2(fdiv(phiOf(hit.y, hit.x), 2.0f * kPI), fdiv(hit.z, hh)) : v2(0.0f, 0.0f);
  finishLocal(c, p, hit, uv, dpduRot(hit), v3(0.0f, 0.0f, hh), h);
}
D void hypDpD(V3 hit, V3 p1, V3 p2, float phi, V3& dpdu, V3& dpdv) {  // hyperboloid.glsl:41-46
  float sinPhi, cosPhi; sincosf_(phi, sinPhi, cosPhi);
  dpdu = dpduRot(hit);
  dpdv = v3((p2.x - p1.x) * cosPhi - (p2.y - p1.y) * sinPhi, (p2.x - p1.x) * sinPhi + (p2.y - p1.y) * cosPhi, p2.z - p1.z);
}
D void hypHit(const Ctx& c, const SailPrim& p, V3 hit, Hit& h) {
  const V3 p1 = P3(p, 3), p2 = P3(p, 6);
  const float v = fdiv(hit.z - p1.z, p2.z - p1.z);
  const V3 pr = (1.0f - v) * p1 + v * p2;
  const float phi = phiOf(pr.x * hit.y - hit.x * pr.y, hit.x * pr.x + hit.y * pr.y);
  const float u = fdiv(phi, 2.0f * kPI);
  V3 dpdu, dpdv;
  hypDpD(hit, p1, p2, phi, dpdu, dpdv);
  finishLocal(c, p, hit, v2(u, v), dpdu, dpdv, h);
}
D void paraDpD(V3 hit, float zMax, float zMin, V3& dpdu, V3& dpdv) {  // paraboloid.glsl:35-40
  dpdu = dpduRot(hit);
  dpdv = (zMax - zMin) * v3(fdiv(hit.x, 2.0f * hit.z), fdiv(hit.y, 2.0f * hit.z), 1.0f);
}
D void paraHit(const Ctx& c, const SailPrim& p, V3 hit, Hit& h) {
  const float zMin = fmin_(p.a[3], p.a[4]), zMax = fmax_(p.a[3], p.a[4]);
  const V2 uv = needsUV(p) ? v2(fdiv(phiOf(hit.y, hit.x), 2.0f * kPI), fdiv(hit.z - zMin, zMax - zMin)) : v2(0.0f, 0.0f);
  V3 dpdu, dpdv;
  paraDpD(hit, zMax, zMin, dpdu, dpdv);
  finishLocal(c, p, hit, uv, dpdu, dpdv, h);
}
D void diskHit(const Ctx& c, const SailPrim& p, V3 hit, Hit& h) {
  const float rad = p.a[3], ri = p.a[4];
  const float dist2 = hit.x * hit.x + hit.y * hit.y;
  V2 uv = v2(0.0f, 0.0f);
  if (needsUV(p)) {
    const float rHit = sqrtf_(dist2);
    const float oneMinusV = fdiv(rHit - ri, rad - ri);
    uv = v2(fdiv(phiOf(hit.y, hit.x), 2.0f * kPI), 1.0f - oneMinusV);
  }
  const V3 dpdv = v3(hit.x, hit.y, 0.0f) * (ri - rad) / sqrtf_(dist2);
  finishLocal(c, p, hit, uv, dpduRot(hit), dpdv, h);
}
// localHit, the pre-cull kernel's one hit record for the six local-space shapes (sphere, cone, cylinder, hyperboloid, paraboloid,
// disk). Each computes the same tail -- the azimuth phiOf (atan2) of its UV, dpdu = dpduRot(hit), a normalised cross,
// the texture and four local-to-world transforms -- so a wave whose lanes hit different shape types (the pre-cull
// kernel sorts by material, then shape) runs that tail once instead of once per type. Per type only the phi
// arguments, the v coordinate, dpdv and the cross order differ. Same operations on the same values as sphereHit and
// the finishLocal callers above. Measured (bit-identical, profiles/r03_variants_local_shared.jsonl, three rounds):
// pre-cull kernel C4 +3.3 %, C2/C3 unchanged; only its mixed waves +3.2 %; every kernel C4 +3.1 %, C3 -0.8 %.
D void localHit(const Ctx& c, const SailPrim& p, V3 hl, Hit& h) {
  const int ty = p.type;
  const bool nUV = needsUV(p);
  // the azimuth's arguments: (y, x) of the hit, the sphere's pole guard, the hyperboloid's rotated frame
  float py = hl.y, px = hl.x, theta = 0.0f, hv = 0.0f;
  V3 p1 = v3s(0.0f), p2 = v3s(0.0f);
  bool needPhi = nUV;
  if (ty == SAIL_SPHERE) {
    theta = acosf_(clamp_(fdiv(hl.z, p.a[3]), -1.0f, 1.0f));
    if (hl.x == 0.0f && hl.y == 0.0f) px = 1e-5f * p.a[3];
  } else if (ty == SAIL_HYPERBOLOID) {
    p1 = P3(p, 3); p2 = P3(p, 6);
    hv = fdiv(hl.z - p1.z, p2.z - p1.z);
    const V3 pr = (1.0f - hv) * p1 + hv * p2;
    py = pr.x * hl.y - hl.x * pr.y; px = hl.x * pr.x + hl.y * pr.y;
    needPhi = true;
  }
  float phi = 0.0f, u = 0.0f;
  if (needPhi) { phi = phiOf(py, px); u = fdiv(phi, 2.0f * kPI); }
  V2 uv = v2(0.0f, 0.0f);
  const V3 dpdu = dpduRot(hl);
  V3 dpdv, nc;
  switch (ty) {
    case SAIL_SPHERE: {
      const float rad = p.a[3];
      if (nUV) uv = v2(u, fdiv(theta, kPI));
      const float zRadius = sqrtf_(hl.x * hl.x + hl.y * hl.y);
      const float invZRadius = rcp_rn(zRadius);
      const float cosPhi = hl.x * invZRadius, sinPhi = hl.y * invZRadius;
      dpdv = kPI * v3(hl.z * cosPhi, hl.z * sinPhi, -rad * sinf_(theta));
      nc = crossZb(dpdv, dpdu);
      break;
    }
    case SAIL_CONE: {
      const float hh = p.a[3];
      if (nUV) uv = v2(u, fdiv(hl.z, hh));
      const float vv = fdiv(hl.z, hh);
      dpdv = v3(fdiv(-hl.x, 1.0f - vv), fdiv(-hl.y, 1.0f - vv), hh);
      nc = crossZa(dpdu, dpdv);
      break;
    }
    case SAIL_CYLINDER: {
      const float hh = p.a[3];
      if (nUV) uv = v2(u, fdiv(hl.z, hh));
      dpdv = v3(0.0f, 0.0f, hh);
      nc = crossZa(dpdu, dpdv);
      break;
    }
    case SAIL_HYPERBOLOID: {
      uv = v2(u, hv);
      float sinPhi, cosPhi; sincosf_(phi, sinPhi, cosPhi);
      dpdv = v3((p2.x - p1.x) * cosPhi - (p2.y - p1.y) * sinPhi, (p2.x - p1.x) * sinPhi + (p2.y - p1.y) * cosPhi, p2.z - p1.z);
      nc = crossZa(dpdu, dpdv);
      break;
    }
    case SAIL_PARABOLOID: {
      const float zMin = fmin_(p.a[3], p.a[4]), zMax = fmax_(p.a[3], p.a[4]);
      if (nUV) uv = v2(u, fdiv(hl.z - zMin, zMax - zMin));
      dpdv = (zMax - zMin) * v3(fdiv(hl.x, 2.0f * hl.z), fdiv(hl.y, 2.0f * hl.z), 1.0f);
      nc = crossZa(dpdu, dpdv);
      break;
    }
    default: {  // SAIL_DISK
      const float rad = p.a[3], ri = p.a[4];
      const float dist2 = hl.x * hl.x + hl.y * hl.y;
      if (nUV) {
        const float rHit = sqrtf_(dist2);
        const float oneMinusV = fdiv(rHit - ri, rad - ri);
        uv = v2(u, 1.0f - oneMinusV);
      }
      dpdv = v3(hl.x, hl.y, 0.0f) * (ri - rad) / sqrtf_(dist2);
      nc = crossZa(dpdu, dpdv);
      break;
    }
  }
  const V3 nl = normalize(nc);
  h.sc = getSurfaceColor(c, uv, p);
  h.hit = L2W(hl) + P3(p, 0);
  h.normal = L2W(nl);
  h.dpdu = L2W(dpdu);
  h.dpdv = L2W(dpdv);
}

// hl (may be null): the local-space hit point of the shapes whose hit record starts from it
// type: the row's shape id (p.type, or a compile-time constant in a kernel compiled for the scene's rows)
D float primTy(const Ctx& c, int type, const SailPrim& p, const Ray& r, V3* hl) {
  switch (type) {
    case SAIL_CUBE: if (HAS(c.kShapes, SAIL_CUBE)) return cubeT(p, r); break;
    case SAIL_SPHERE: if (HAS(c.kShapes, SAIL_SPHERE)) return sphereT(p, r, hl); break;
    case SAIL_RECTANGLE: if (HAS(c.kShapes, SAIL_RECTANGLE)) return rectT(p, r, hl); break;
    case SAIL_CONE: if (HAS(c.kShapes, SAIL_CONE)) return coneT(p, r, hl); break;
    case SAIL_CYLINDER: if (HAS(c.kShapes, SAIL_CYLINDER)) return cylinderT(p, r, hl); break;
    case SAIL_DISK: if (HAS(c.kShapes, SAIL_DISK)) return diskT(p, r, hl); break;
    case SAIL_HYPERBOLOID: if (HAS(c.kShapes, SAIL_HYPERBOLOID)) return hypT(p, r, hl); break;
    case SAIL_PARABOLOID: if (HAS(c.kShapes, SAIL_PARABOLOID)) return paraT(p, r, hl); break;
    case SAIL_CORNELLBOX: if (HAS(c.kShapes, SAIL_CORNELLBOX)) return cornellT(p, r); break;
    default: break;
  }
  return kMaxDistance;
}
D float primT(const Ctx& c, const SailPrim& p, const Ray& r, V3* hl) { return primTy(c, p.type, p, r, hl); }

// A kernel compiled at run time for the scene's primitive rows (sail_jit.cpp, SAIL_JIT_N > 0) knows their count and
// shape types: the flat sweeps become straight-line code over the rows, each row's intersection test chosen at compile
// time (no per-row type dispatch, no loop). Same operations in the same order as the loops below (measured on the
// Cornell box, tools/study/c1_struct.py: C1 +1.9 %).
#if defined(SAIL_JIT) && SAIL_JIT_N > 0
constexpr int kRows = SAIL_JIT_N;
constexpr int kRowType[SAIL_JIT_N] = {SAIL_JIT_TYPES};
#else
constexpr int kRows = 0;
constexpr int kRowType[1] = {0};
#endif
// the row of the scene's Cornellbox in a kernel compiled for its rows (-1: none)
constexpr int cornellRowOf() {
  for (int i = 0; i < kRows; i++)
    if (kRowType[i] == SAIL_CORNELLBOX) return i;
  return -1;
}
constexpr int kCornellRow = cornellRowOf();
template <int I>
D void sweepRows(const Ctx& c, const Ray& r, float& best, int& bi, V3& bhl) {
  if constexpr (I < kRows) {
    V3 hl = v3s(0.0f);
    const float t = primTy(c, kRowType[I], PRIM(c, I), r, &hl);
    if (t < best) { best = t; bi = I; bhl = hl; }
    sweepRows<I + 1>(c, r, best, bi, bhl);
  }
}
template <int I>
D void closestRows(const Ctx& c, const Ray& r, float& best) {
  if constexpr (I < kRows) {
    const float t = primTy(c, kRowType[I], PRIM(c, I), r, nullptr);
    if (t < best) {
      best = t;
      if (c.shadowAnyHit && best > kEps && best < kOneMinusEps) return;  // as closestT's loop
    }
    closestRows<I + 1>(c, r, best);
  }
}

// Cheap conservative pre-cull: the ray against the primitive's padded bounds in f32 (sail_capi.cpp
// padPrimBounds). It rejects only rays that miss the padded box or enter it beyond the closest distance so
// far (with margin); such a primitive's exact test could only return a miss or a larger distance.
D bool padHit(const SailPrim& p, const Ray& r, float best) {
  const float ix = r.rx, iy = r.ry, iz = r.rz;
  const float x0 = (p.a[18] - r.o.x) * ix, x1 = (p.a[21] - r.o.x) * ix;
  const float y0 = (p.a[19] - r.o.y) * iy, y1 = (p.a[22] - r.o.y) * iy;
  const float z0 = (p.a[20] - r.o.z) * iz, z1 = (p.a[23] - r.o.z) * iz;
  const float tmin = fmax_(fmax_(fmin_(x0, x1), fmin_(y0, y1)), fmin_(z0, z1));
  const float tmax = fmin_(fmin_(fmax_(x0, x1), fmax_(y0, y1)), fmax_(z0, z1));
  return !(tmin > tmax) && !(tmax < 0.0f) && !(tmin > best * 1.0001f + 1e-4f);
}


// ---- candidate sweep (pre-cull kernel) ----------------------------------------------------------------------
// In the uniform sweep a wave runs a primitive's exact test whenever any lane passes its pre-cull; on C4
// (67 primitives, incoherent bounce rays) that is 35 % of the (wave, primitive) pairs with 4.7 of 53 lanes
// passing. Here every lane first collects its candidates of a 64-row chunk into a bit mask (uniform pre-cull
// loop, scalar row reads), then, one shape type at a time, each lane tests its own next candidate of that
// type: the wave runs max-over-lanes iterations instead of one per primitive any lane needs. Candidates are
// visited out of row order, so a hit replaces the best one when it is nearer, or equally near with a lower
// row -- the winner of the in-order "t < best" sweep. Pre-culled rows cannot win (padHit), nor tie.
// Candidate loops without exec-mask nesting (idle lanes test a real row of the type, `take` keeps them out) were
// bit-identical and C4 -0.8 % (the idle lanes' own branches cost more than the saved masking).
// candidate masks built from descending rows shifted into two 32-bit halves (one select + one v_lshl_or per
// row instead of a 64-bit shift, two moves, two selects and two ors): C4 +2.7 %. Packing the x/y slab
// arithmetic of padHit into v_pk_add_f32 / v_pk_mul_f32 was measured at -3.4 %.
// Fused pre-cull form (A.cullPrims == 2): each slab plane as fma(a, R, -RN(o R)), 2 FMAs per axis instead of
// 2 subtractions + 2 multiplies, o R hoisted per ray. Against the plain form each plane moves by at most
// |o| 2^-24 (the host enables it only while that is far inside the padding: sail_capi.cpp cullFmaOk). The
// reciprocals are clamped to +-1e30 first: for an axis-parallel ray (R = +-inf) the plain form gives the
// slab (+-inf, +-inf) while a R - o R would be inf - inf = NaN, which min/max then drop from one side only
// (measured: 1.4 M rays of one C4 frame culled wrongly without the clamp). NaN reciprocals stay NaN.
struct CullRay { float rx, ry, rz, ox, oy, oz; };
D float clampRcp(float v) { return fabsf(v) > 1e30f ? __builtin_copysignf(1e30f, v) : v; }
D CullRay cullRay(const Ray& r) {
  CullRay q;
  q.rx = clampRcp(r.rx); q.ry = clampRcp(r.ry); q.rz = clampRcp(r.rz);
  q.ox = -(r.o.x * q.rx); q.oy = -(r.o.y * q.ry); q.oz = -(r.o.z * q.rz);
  return q;
}
// Mask build in the fused form, B = best * 1.0001 + 1e-4 (> 0) computed once per chunk by the caller. The row's
// outcome is the compare's own lane mask: the bit is
// shifted in by one v_addc (v + v + carry, the carry-in being that lane mask) instead of a select and a v_lshl_or,
// and min(tmax, B) is one v_min_f32 -- the compiler's own fold of the three tests, which re-canonicalised the
// loop-invariant B on every row (tmax and B are arithmetic results, never signalling NaNs, so the plain hardware
// min is the same value). Two fewer VALU per row of the ~20 of each pre-cull test.
D unsigned long long padHitFMask(const SailPrim& p, const CullRay& q, float B) {
  const float x0 = fma_(p.a[18], q.rx, q.ox), x1 = fma_(p.a[21], q.rx, q.ox);
  const float y0 = fma_(p.a[19], q.ry, q.oy), y1 = fma_(p.a[22], q.ry, q.oy);
  const float z0 = fma_(p.a[20], q.rz, q.oz), z1 = fma_(p.a[23], q.rz, q.oz);
  const float tmin = fmax_(fmax_(fmin_(x0, x1), fmin_(y0, y1)), fmin_(z0, z1));
  const float tmax = fmin_(fmin_(fmax_(x0, x1), fmax_(y0, y1)), fmax_(z0, z1));
  float mB;
  __asm__("v_min_f32 %0, %1, %2" : "=v"(mB) : "v"(tmax), "v"(B));
  // !(tmin > tmax) && !(tmin > B) == !(tmin > min(tmax, B)): a NaN tmax leaves B on either side
  return __builtin_amdgcn_ballot_w64(!(tmin > mB)) & __builtin_amdgcn_ballot_w64(!(tmax < 0.0f));
}
D unsigned shiftInMask(unsigned v, unsigned long long laneMask) {
  unsigned r;
  unsigned long long carryOut;
  __asm__("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carryOut) : "v"(v), "s"(laneMask));
  return r;
}
// one 64-row chunk's candidate mask: descending rows shifted into two 32-bit halves (one v_addc per row in the fused
// form; one select and one v_lshl_or per row in the plain one)
template <bool FUSED>
D unsigned long long chunkMask(const Ctx& c, const Ray& r, const CullRay& q, int base, int cnt, float bound) {
  unsigned lo = 0u, hi = 0u;
  const float B = bound * 1.0001f + 1e-4f;
  if (FUSED) {
    // four rows per step (their bounds requested by scalar loads together, fewer waits; C4 +1.7 %,
    // profiles/r04_cull_unroll.jsonl), the bits shifted in the same descending order as one row per step
    int j = cnt - 1;
    for (; j >= 35; j -= 4) {
      const unsigned long long m0 = padHitFMask(PRIM(c, base + j), q, B), m1 = padHitFMask(PRIM(c, base + j - 1), q, B);
      const unsigned long long m2 = padHitFMask(PRIM(c, base + j - 2), q, B), m3 = padHitFMask(PRIM(c, base + j - 3), q, B);
      hi = shiftInMask(shiftInMask(shiftInMask(shiftInMask(hi, m0), m1), m2), m3);
    }
    for (; j >= 32; j--) hi = shiftInMask(hi, padHitFMask(PRIM(c, base + j), q, B));
    j = (cnt < 32 ? cnt : 32) - 1;
    for (; j >= 3; j -= 4) {
      const unsigned long long m0 = padHitFMask(PRIM(c, base + j), q, B), m1 = padHitFMask(PRIM(c, base + j - 1), q, B);
      const unsigned long long m2 = padHitFMask(PRIM(c, base + j - 2), q, B), m3 = padHitFMask(PRIM(c, base + j - 3), q, B);
      lo = shiftInMask(shiftInMask(shiftInMask(shiftInMask(lo, m0), m1), m2), m3);
    }
    for (; j >= 0; j--) lo = shiftInMask(lo, padHitFMask(PRIM(c, base + j), q, B));
    return ((unsigned long long)hi << 32) | lo;
  }
  for (int j = cnt - 1; j >= 32; j--) hi = (hi << 1) | (padHit(PRIM(c, base + j), r, bound) ? 1u : 0u);
  for (int j = (cnt < 32 ? cnt : 32) - 1; j >= 0; j--) lo = (lo << 1) | (padHit(PRIM(c, base + j), r, bound) ? 1u : 0u);
  return ((unsigned long long)hi << 32) | lo;
}
template <int T> D float typedT(const SailPrim& p, const Ray& r, V3* hl) {
  if constexpr (T == SAIL_CUBE) return cubeT(p, r);
  else if constexpr (T == SAIL_SPHERE) return sphereT(p, r, hl);
  else if constexpr (T == SAIL_RECTANGLE) return rectT(p, r, hl);
  else if constexpr (T == SAIL_CONE) return coneT(p, r, hl);
  else if constexpr (T == SAIL_CYLINDER) return cylinderT(p, r, hl);
  else if constexpr (T == SAIL_DISK) return diskT(p, r, hl);
  else if constexpr (T == SAIL_HYPERBOLOID) return hypT(p, r, hl);
  else if constexpr (T == SAIL_PARABOLOID) return paraT(p, r, hl);
  else if constexpr (T == SAIL_CORNELLBOX) return cornellT(p, r);
  else return kMaxDistance;
}
// HIT = false (shadow rays): only the closest distance is read, so neither the winner's row nor its local hit point
// is kept, and an equally near candidate changes nothing (a tie leaves the distance's value as it is; +-0 compare
// equal and both fail the caller's d > EPSILON). Four fewer live registers in the shadow sweep, where the
// shading state is live.
template <int T, bool HIT>
D void candType(const Ctx& c, const Ray& r, int base, unsigned long long cand, float& best, int& bi, V3& bhl) {
  if (!HAS(c.kShapes, T)) return;
  const unsigned long long tm = constRow<unsigned long long>(c.typeMasks, (base >> 6) * 16 + T);
  unsigned long long m = cand & tm;
  while (__ballot(m != 0ull)) {
    if (m != 0ull) {
      const int i = base + __builtin_ctzll(m);
      m &= m - 1ull;
      const SailPrim& p = c.cprims[i];
      if (HIT) {
        V3 hl = v3s(0.0f);
        const float t = typedT<T>(p, r, &hl);
        if (t < best || (t == best && i < bi)) { best = t; bi = i; bhl = hl; }
      } else {
        const float t = typedT<T>(p, r, nullptr);
        if (t < best) best = t;
      }
    }
  }
}
// the four quadric types' candidates in one loop (quadT)
template <bool HIT>
D void candQuad(const Ctx& c, const Ray& r, int base, unsigned long long cand, float& best, int& bi, V3& bhl) {
  const uint32_t kq = c.kShapes & ((1u << SAIL_CONE) | (1u << SAIL_CYLINDER) | (1u << SAIL_HYPERBOLOID) |
                                   (1u << SAIL_PARABOLOID));
  if (kq == 0u) return;
  const unsigned long long* tms = c.typeMasks + (base >> 6) * 16;
  unsigned long long tm = 0ull;
  if (HAS(kq, SAIL_CONE)) tm |= constRow<unsigned long long>(tms, SAIL_CONE);
  if (HAS(kq, SAIL_CYLINDER)) tm |= constRow<unsigned long long>(tms, SAIL_CYLINDER);
  if (HAS(kq, SAIL_HYPERBOLOID)) tm |= constRow<unsigned long long>(tms, SAIL_HYPERBOLOID);
  if (HAS(kq, SAIL_PARABOLOID)) tm |= constRow<unsigned long long>(tms, SAIL_PARABOLOID);
  unsigned long long m = cand & tm;
  while (__ballot(m != 0ull)) {
    if (m != 0ull) {
      const int i = base + __builtin_ctzll(m);
      m &= m - 1ull;
      const SailPrim& p = c.cprims[i];
      if (HIT) {
        V3 hl = v3s(0.0f);
        const float t = quadT(p, r, &hl);
        if (t < best || (t == best && i < bi)) { best = t; bi = i; bhl = hl; }
      } else {
        const float t = quadT(p, r, nullptr);
        if (t < best) best = t;
      }
    }
  }
}
// limit: the pre-cull distance bound before any hit (kMaxDistance, or 1 for shadow rays: see closestT)
template <bool HIT>
D void candSweep(const Ctx& c, const Ray& r, float limit, float& best, int& bi, V3& bhl) {
  const CullRay q = cullRay(r);
  for (int base = 0; base < c.n; base += 64) {
    const int cnt = c.n - base < 64 ? c.n - base : 64;
    const float bound = fmin_(best, limit);
    const unsigned long long cand =
        c.cullFma ? chunkMask<true>(c, r, q, base, cnt, bound) : chunkMask<false>(c, r, q, base, cnt, bound);
    candType<SAIL_CUBE, HIT>(c, r, base, cand, best, bi, bhl);
    candType<SAIL_CORNELLBOX, HIT>(c, r, base, cand, best, bi, bhl);
    candType<SAIL_RECTANGLE, HIT>(c, r, base, cand, best, bi, bhl);
    candType<SAIL_DISK, HIT>(c, r, base, cand, best, bi, bhl);
    candType<SAIL_SPHERE, HIT>(c, r, base, cand, best, bi, bhl);
    candQuad<HIT>(c, r, base, cand, best, bi, bhl);
  }
}

// closest distance only (shadow rays, testShadow shader.light.js:24-31). The caller only asks whether the
// closest distance lies in (EPSILON, 1 - EPSILON): a primitive whose padded box starts beyond 1 cannot change
// that answer (if it were the closest, every distance would be >= 1 - EPSILON), so the pre-cull bound
// starts at 1 instead of MAX_DISTANCE. Returned distances beyond that bound are not exact.
D float closestT(const Ctx& c, const Ray& r) {
  float best = kMaxDistance;
  if (c.cullPrims && !c.shadowAnyHit) {
    int bi = -1; V3 bhl = v3s(0.0f);
    candSweep<false>(c, r, 1.0f, best, bi, bhl);
    return best;
  }
  if constexpr (kRows > 0) {
    if (!c.cullPrims) {  // compile-time: the flat kernels
      closestRows<0>(c, r, best);
      return best;
    }
  }
  for (int i = 0; i < c.n; i++) {
    if (c.cullPrims && !padHit(PRIM(c, i), r, fmin_(best, 1.0f))) continue;
    const float t = primT(c, PRIM(c, i), r, nullptr);
    if (t < best) {
      best = t;
      if (c.shadowAnyHit && best > kEps && best < kOneMinusEps) break;  // exact: no prim returns t <= EPSILON
    }
  }
  return best;
}

// generated intersectObjects (shader.shape.js:28-51), split in two: one sweep keeps the winner's distance and
// local hit point, then one full record is built for the winner alone
struct Sweep { float best; int bi; V3 bhl; };
// primary: a camera ray, pre-culled only when the eye is near the scene (SailTraceArgs.cullPrimary)
D Sweep sweepRay(const Ctx& c, const Ray& r, bool primary) {
  float best = kMaxDistance;
  int bi = -1;
  V3 bhl = v3s(0.0f);
  const bool cull = c.cullPrims && (!primary || c.cullPrimary);
  if (cull) {
    candSweep<true>(c, r, kMaxDistance, best, bi, bhl);
    Sweep sw; sw.best = best; sw.bi = bi; sw.bhl = bhl;
    return sw;
  }
  if constexpr (kRows > 0) {
    if (!c.cullPrims) {  // compile-time: the flat kernels
      sweepRows<0>(c, r, best, bi, bhl);
      Sweep sw; sw.best = best; sw.bi = bi; sw.bhl = bhl;
      return sw;
    }
  }
  for (int i = 0; i < c.n; i++) {
    V3 hl = v3s(0.0f);
    const float t = primT(c, PRIM(c, i), r, &hl);
    if (t < best) { best = t; bi = i; bhl = hl; }
  }
  Sweep sw; sw.best = best; sw.bi = bi; sw.bhl = bhl;
  return sw;
}
#if SAIL_ROWDEFER
static_assert(kDeferRow < kRows && kRowType[kDeferRow] == SAIL_SPHERE && HAS(SAIL_JIT_KS, SAIL_SPHERE),
              "the deferred row is a Sphere the kernel intersects");
// The deferring sweep: the other rows in order as sweepRows, row kDeferRow's head only. cand: the discriminant is not
// negative (written so that a NaN one stays a candidate, as sphereT does not reject it), and the ray is not one whose
// origin is outside the sphere and which moves away from it. For b > 0 and cc > 0 quadratic takes q = -0.5 (b + root)
// with b + root > 0, so q <= -0, and t0 = q RN(1/a), t1 = cc RN(1/q) are each <= -0 or NaN: the tail either returns
// kMaxDistance at its t2 < kEps test or goes on with a NaN t and returns kMaxDistance or that NaN, and neither passes
// the sweep's t < best (tests/test_sphere_defer_host.py). That keeps the mirror's own reflected rays, the one large
// class of false candidates, out of the sphere's waves.
// defer (wave-uniform): this bounce defers; otherwise row kDeferRow's head is followed by its tail, which is sphereT. One
// text for both, so that the other rows' tests are in the kernel once.
template <int I>
D void sweepRowsDefer(const Ctx& c, const Ray& r, bool defer, float& best, int& bi, V3& bhl, bool& cand) {
  if constexpr (I < kRows) {
    if constexpr (I == kDeferRow) {
      SphereQuad q;
      const bool live = sphereT<1>(PRIM(c, I), r, nullptr, q) < kMaxDistance;  // the discriminant is not negative
      if (defer) {
        cand = live && !(q.b > 0.0f && q.cc > 0.0f);
      } else if (live) {
        V3 hl = v3s(0.0f);
        const float t = sphereT<2>(PRIM(c, I), r, &hl, q);
        if (t < best) { best = t; bi = I; bhl = hl; }
      }
    } else {
      V3 hl = v3s(0.0f);
      const float t = primTy(c, kRowType[I], PRIM(c, I), r, &hl);
      if (t < best) { best = t; bi = I; bhl = hl; }
    }
    sweepRowsDefer<I + 1>(c, r, defer, best, bi, bhl, cand);
  }
}
D Sweep sweepRayDefer(const Ctx& c, const Ray& r, bool defer, bool& cand) {
  Sweep sw;
  sw.best = kMaxDistance; sw.bi = -1; sw.bhl = v3s(0.0f);
  cand = false;
  sweepRowsDefer<0>(c, r, defer, sw.best, sw.bi, sw.bhl, cand);
  return sw;
}
// A gathered candidate's tail, on the ray it was sorted with: the head's expressions again (the packed path state
// carries the segment, not a, b, cc), the ray's reciprocals again (mkRay: the path carries none), then the tail. The
// sphere wins iff the in-order sweep would have taken it: nearer than the provisional winner, or as near with a
// lower row index (the candidate sweep's rule for a row visited out of order, candType).
D void sphereResolve(const Ctx& c, const Seg& r, Sweep& sw) {
  const SailPrim& p = PRIM(c, kDeferRow);
  const Ray rr = mkRay(r.o, r.d);
  // the discriminant is the sweep's, bit for bit (the same operations on the same operands): not negative, so the whole
  // test is the head followed by the tail
  SphereQuad q;
  const float t = sphereT<0>(p, rr, nullptr, q);
  if (t < sw.best || (t == sw.best && kDeferRow < sw.bi)) { sw.best = t; sw.bi = kDeferRow; }
}
#endif
// The winner's local hit point from the ray and its distance: every local-space intersect above ends with
// hit = o + t * d on the same local o and d (W2L of the ray for the quadrics and the disk, the rectangle's frame), so
// this is the sweep's own value bit for bit -- the compacting kernels recompute it instead of moving it through LDS
// (packed path state, traceTileCompact).
D V3 quadLocalHit(const SailPrim& p, const Seg& r, float t) {
  const V3 d = W2L(r.d), o = W2L(r.o - P3(p, 0));
  return o + t * d;
}
D V3 rectLocalHit(const SailPrim& p, const Seg& r, float t) {
  const RectFrame f = rectFrame(p);
  const V3 d = worldToLocal(r.d, f.normal, f.ss, f.ts);
  const V3 o = worldToLocal(r.o - P3(p, 0), f.normal, f.ss, f.ts);
  return o + t * d;
}
// BOXU: the room family's one box record for Cube and Cornellbox (boxHit)
template <bool RECOMP_HL = false, bool BOXU = false>
D Hit hitRecord(const Ctx& c, const Seg& r, const Sweep& sw) {
  const float best = sw.best;
  const int bi = sw.bi;
  Hit h;
  h.d = best;
  // precondition: bi >= 0 is a sweep winner, so its shape is compiled into this kernel (primT returns
  // MAX_DISTANCE for any other row, which never wins): no zero record is needed on any path -- a divergent
  // zero default would be materialised for every lane before the dispatch
  const SailPrim& p = c.rowCopy ? c.cprims[bi] : PRIM(c, bi);
#define BHL (RECOMP_HL ? quadLocalHit(p, r, best) : sw.bhl)
  // compile-time constants: the room kernel's shared box record (boxHit), the pre-cull kernel's shared local-space
  // record (localHit)
  constexpr bool boxU = BOXU;
  const bool localU = c.cullPrims != 0;
  const uint32_t kLocal = c.kShapes & ((1u << SAIL_SPHERE) | (1u << SAIL_CONE) | (1u << SAIL_CYLINDER) |
                                       (1u << SAIL_HYPERBOLOID) | (1u << SAIL_PARABOLOID) | (1u << SAIL_DISK));
  if (boxU && ((HAS(c.kShapes, SAIL_CUBE) && p.type == SAIL_CUBE) ||
               (HAS(c.kShapes, SAIL_CORNELLBOX) && p.type == SAIL_CORNELLBOX))) {
    boxHit(c, p, r, best, h, HAS(c.kShapes, SAIL_CORNELLBOX) && p.type == SAIL_CORNELLBOX);
  } else if (localU && ((kLocal >> p.type) & 1u)) {
    localHit(c, p, BHL, h);
  } else
  switch (p.type) {
    case SAIL_CUBE: if (!boxU && HAS(c.kShapes, SAIL_CUBE)) { cubeHit(c, p, r, best, h); break; } __builtin_unreachable();
    case SAIL_SPHERE: if (!localU && HAS(c.kShapes, SAIL_SPHERE)) { sphereHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_RECTANGLE: if (HAS(c.kShapes, SAIL_RECTANGLE)) { rectHit(c, p, RECOMP_HL ? rectLocalHit(p, r, best) : sw.bhl, h); break; } __builtin_unreachable();
    case SAIL_CONE: if (!localU && HAS(c.kShapes, SAIL_CONE)) { coneHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_CYLINDER: if (!localU && HAS(c.kShapes, SAIL_CYLINDER)) { cylinderHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_DISK: if (!localU && HAS(c.kShapes, SAIL_DISK)) { diskHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_HYPERBOLOID: if (!localU && HAS(c.kShapes, SAIL_HYPERBOLOID)) { hypHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_PARABOLOID: if (!localU && HAS(c.kShapes, SAIL_PARABOLOID)) { paraHit(c, p, BHL, h); break; } __builtin_unreachable();
    case SAIL_CORNELLBOX: if (!boxU && HAS(c.kShapes, SAIL_CORNELLBOX)) { cornellHit(p, r, best, h); break; } __builtin_unreachable();
    default: __builtin_unreachable();
  }
#undef BHL
  h.matRow = p.matRow;
  h.emission = v3(p.em[0], p.em[1], p.em[2]);
  // faceObj test (shader.shape.js:47-49) on sgn(rev) * normal: (-n).d is exactly -(n.d) (negated products,
  // round-to-nearest is symmetric), so one dot product serves it and the into test below
  h.axis = c.cullPrims && (p.type == SAIL_CUBE || p.type == SAIL_CORNELLBOX);
  const float nd = h.axis ? dotX(h.normal, r.d) : dot(h.normal, r.d);
  if (!((p.rev ? -nd : nd) < -kEps)) h.emission = v3s(0.0f);
  h.matCategory = matCat(p);
  h.into = nd < -kEps;
  h.nd = nd;
  if (!h.into) h.normal = -h.normal;
  return h;
}
// wave-uniform winner: the same record with the row index in an SGPR (scalar row loads)
#if SAIL_ROWVALS
// Scenes of at most this many rows get one hit-record instance per row in a kernel compiled for their values (each
// folds to one shape, one material category, constant operands); with more rows the per-row copies outgrow what they
// save, and only the sweep, the key, the AOV and quiet-row reads take the constants (the one generic record then reads
// its row from the constant table). Measured on C1 variants at 1080p, ms per 1,024-sample frame, types kernel /
// generic record on constant rows / a record per row (profiles/r08_rowmax.jsonl): 3 rows 161.6 / 157.5 / 155.6,
// 4 rows 174.7 / 169.2 / 173.2, 5 rows 178.1 / 171.4 / 173.7, 7 rows 202.2 / 193.8 / 205.1.
constexpr int kRowRecordMax = 3;
// the record of row I for the lanes whose winner it is: pick by the scalar row index (U) or per lane
template <int I, bool U, bool RECOMP_HL, bool BOXU>
D void hitRecordRows(const Ctx& c, const Seg& r, const Sweep& sw, int b0, Hit& h) {
  if constexpr (I + 1 < kRows) {
    if ((U ? b0 : sw.bi) != I) { hitRecordRows<I + 1, U, RECOMP_HL, BOXU>(c, r, sw, b0, h); return; }
  }
  Sweep su = sw;
  su.bi = I;  // a winner is one of the kernel's rows (hitRecord's precondition): the last row needs no test
  h = hitRecord<RECOMP_HL, BOXU>(c, r, su);
}
#endif
template <bool RECOMP_HL = false, bool BOXU = false>
D Hit hitRecordU(const Ctx& c, const Seg& r, const Sweep& sw) {
  const int b0 = __builtin_amdgcn_readfirstlane(sw.bi);
#if SAIL_ROWVALS
  if constexpr (kRows <= kRowRecordMax) {
    Hit h;
    if (__all(sw.bi == b0)) hitRecordRows<0, true, RECOMP_HL, BOXU>(c, r, sw, b0, h);
    else hitRecordRows<0, false, RECOMP_HL, BOXU>(c, r, sw, b0, h);
    return h;
  }
#endif
  if (__all(sw.bi == b0)) {
    Sweep su = sw;
    su.bi = b0;
    return hitRecord<RECOMP_HL, BOXU>(c, r, su);
  }
  return hitRecord<RECOMP_HL, BOXU>(c, r, sw);
}
#if SAIL_ROWSHADE
static_assert(kRows <= kRowRecordMax, "row shading rides on the per-row hit records");
// rest(hit record): the remainder of the bounce. A row-uniform wave whose row is in kRowShadeMask runs it in the branch
// of its row, behind that row's record (the same functions on the same operands in the same order: only operands become
// constants); every other wave runs the one generic copy behind its record(s), as after hitRecordU.
constexpr unsigned kRowShadeMask = SAIL_JIT_ROWSHADE;  // bit i: row i has a shading copy of its own
// Quiet rows (SAIL_JIT_ROWQUIET, the host's lastBounceRows class for a kernel without a light plugin): the emission words
// are +0 and the row is not a matte, or a Lambertian one of constant colour(s) with finite f = (kd * sc) / pi. A hit on
// such a row updates the radiance by e + (emission + direct) * throughput with emission + direct = +0 + fma(f, 0, 0)
// = +0 exactly, at every bounce (shadeBounce and shadeLast make the same update). That sum is e, bit for bit:
//  * the throughput is finite: it starts at 1 and is only ever multiplied by vclamp01 results, which lie in [0, 1]
//    (clamp_ of a NaN is 0), so +0 * throughput is +0 or -0, never NaN;
//  * e is never -0: it starts at +0, every later value is a sum, and a sum is -0 only if both terms are -0;
//  * x + (+-0) = x for every x but -0 (NaN payloads pass through the add unchanged: the operand is already quiet, being
//    a sum itself).
// So the row's own copy neither loads nor stores the radiance: its update runs on a dummy and is dead code.
constexpr unsigned kRowQuietMask = SAIL_JIT_ROWQUIET;
static_assert(kRowQuietMask == 0u || SAIL_JIT_KL == 0u, "quiet rows: no light plugin compiled in");
static_assert((kRowQuietMask & ~kRowShadeMask) == 0u, "quiet rows are rows with a copy of their own");
template <bool Q> struct QuietTag { static constexpr bool value = Q; };
template <int I, bool RECOMP_HL, bool BOXU, class Rest>
D bool bounceRows(const Ctx& c, const Seg& r, const Sweep& sw, int b0, Hit& h, Rest&& rest) {
  if constexpr (I + 1 < kRows) {
    if (b0 != I) return bounceRows<I + 1, RECOMP_HL, BOXU>(c, r, sw, b0, h, rest);
  }
  Sweep su = sw;
  su.bi = I;
  h = hitRecord<RECOMP_HL, BOXU>(c, r, su);
  if constexpr (((kRowShadeMask >> I) & 1u) != 0u) {
    rest(h, QuietTag<((kRowQuietMask >> I) & 1u) != 0u>{});
    return true;
  }
  return false;
}
template <bool RECOMP_HL, bool BOXU, class Rest>
D void bounceU(const Ctx& c, const Seg& r, const Sweep& sw, Rest&& rest) {
  const int b0 = __builtin_amdgcn_readfirstlane(sw.bi);
  Hit h;
  if (__all(sw.bi == b0)) {
    if (bounceRows<0, RECOMP_HL, BOXU>(c, r, sw, b0, h, rest)) return;
  } else {
    hitRecordRows<0, false, RECOMP_HL, BOXU>(c, r, sw, b0, h);
  }
  rest(h, QuietTag<false>{});
}
#endif

}  // namespace
