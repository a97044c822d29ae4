// sail_capi.cpp — libsail_hip.so: the context's life cycle, scene decode and upload, the run-time kernels' slots and the
// trace launch (which kernel and what shape: sail_plan.cpp), readback, display filter, picking. What it shares with the
// other host files (sail_multi.cpp: RCCL and multi-device reduce, checkpoints; sail_converge.cpp: noise estimate,
// render-until, tile mask; sail_post.cpp: denoiser, reprojection, temporal filter, albedo map) is in sail_ctx.h.
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
#include "sail_ctx.h"

namespace {

thread_local std::string g_create_error;

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

int fail(sail_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

namespace {

// The rows changed, or the spec their value kernel was derived from: the hold on the value spec goes (a queued build of it
// is skipped, a finished one stays in the caches for a scene that returns to this pose), its masked twin's first, launches
// run the types kernel again, and the settle count restarts.
void dropValues(sail_ctx* c) {
  c->valueTwin.drop(c->device, c->stream);
  c->valueSlot.drop(c->device, c->stream);
  c->settled = 0;
}
// Ask for the scene's value kernel once it has settled (after every refreshJit, and between and after launches): the build
// starts in the background, or the object loads here when a disk cache has it, as refreshJit does for the types kernel.
// When it fails the types kernel serves.
void refreshValues(sail_ctx* c) {
  if (!c->subs.empty() || c->valueSlot.have || !c->typesSlot.have || !settledFor(c->settled, c->sw.jitValuesAfter)) return;
  SailJitSpec spec;
  if (!valueSpecFor(c->typesSlot.spec, c->rowWords, c->tpRows.data(), c->facts.tn, c->sw.jit, &spec)) return;
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
  const bool have = c->haveScene && jitSpecFor(c->facts, c->sw, c->share, &spec, &mode);
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
// the spec launchSamples goes by: the scene's run-time kernel while one is held whose build has not failed
const SailJitSpec* heldTypes(const sail_ctx* c) {
  const JitSlot& t = c->typesSlot;
  return (t.have && t.state != SAIL_KERNEL_JIT_FAILED) ? &t.spec : nullptr;
}
// the tiles a launch traces, and their in-frame pixels: the share, or with a tile mask its active tiles (tileMap)
int ownedTiles(const sail_ctx* c, int* tilesX, int* tilesY) {
  const int part = partitionTiles(c->share, tilesX, tilesY);
  return c->maskSet ? c->maskTiles : part;
}
long long ownedPixels(const sail_ctx* c) {
  if (c->maskSet) return c->maskPixels;
  int tx, ty;
  const ShareFacts& sh = c->share;
  const int owned = partitionTiles(sh, &tx, &ty);
  long long px = 0;
  const int w = (sh.partMode == SAIL_PART_SAMPLES) ? 1 : sh.world, r = (sh.partMode == SAIL_PART_SAMPLES) ? 0 : sh.rank;
  for (int j = 0; j < owned; j++) {
    const int t = r + j * w;
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    const int cw = (sh.W - x0) < 64 ? (sh.W - x0) : 64, ch = (sh.H - y0) < 64 ? (sh.H - y0) : 64;
    px += (long long)cw * ch;
  }
  return px;
}

}  // namespace

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
  const size_t bytes = (size_t)c->share.W * c->share.H * sizeof(float4);
  HIPCHK(c, hipMemsetAsync(c->accum, 0, bytes, c->stream));
  if (c->aovN) HIPCHK(c, hipMemsetAsync(c->aovN, 0, bytes, c->stream));
  if (c->aovP) HIPCHK(c, hipMemsetAsync(c->aovP, 0, bytes, c->stream));
  if ((c->aovN || c->aovP) && c->share.partMode == SAIL_PART_TILES && c->share.world > 1)
    HIPCHK(c, sail_launch_negzero_unowned(c->aovN, c->aovP, c->share.W, c->share.H, c->share.rank, c->share.world, c->stream));
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

namespace {

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

// The fused pre-cull form (sail_geom.h padHitFMask) tests each slab plane as fma(a, R, -RN(o R)): the plane
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

// One decoded scene, as sail_set_scene uploads it and as the device-free entry points derive kernels from it: the rows
// with their category words filled, their shape ids, their words (32 per row: what a value kernel compiles in), whether
// a shadow ray may stop at any hit, and the scene box
struct DecodedScene {
  std::vector<SailPrim> prims;
  std::vector<int> types;
  std::vector<uint32_t> rowWords;
  int anyHit = 1;
  SceneBox box{};
};
DecodedScene decodeScene(const float* objects, int n, const float* texparams, int tn, const sail_plugins& plugins) {
  DecodedScene d;
  decodePrims(objects, n, tn, plugins.shape_mask, d.prims, &d.anyHit, &d.box);
  fillCats(d.prims, texparams, tn);
  for (const SailPrim& q : d.prims) d.types.push_back(q.type);
  d.rowWords.resize((size_t)n * 32);
  if (n > 0) memcpy(d.rowWords.data(), d.prims.data(), sizeof(SailPrim) * (size_t)n);
  return d;
}
// the policy's facts of a decoded scene (ln: the light rows of sail_set_scene)
SceneFacts sceneFacts(const DecodedScene& d, int tn, int ln, const sail_plugins& plugins) {
  SceneFacts f;
  f.plugins = plugins;
  f.n = (int)d.prims.size(); f.tn = tn; f.ln = ln;
  f.primTypes = d.types;
  return f;
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
  const long long stageStride = (long long)owned * 4096;  // the stage's floats per staged sample and colour
  const int L = launchSamples(c->sw, heldTypes(c));
  for (int s0 = 0; s0 < count; s0 += L) {
    const int nspp = (count - s0) < L ? (count - s0) : L;
    SailTraceArgs A;
    memset(&A, 0, sizeof A);
    A.prims = c->prims; A.typeMasks = reinterpret_cast<const unsigned long long*>(c->prims + c->facts.n);
    A.texparams = c->tp; A.lights = c->lt; A.lightObjRow = c->lightObjRow;
    A.samples = dev + s0;
    A.accum = c->accum; A.aovN = c->aovN; A.aovP = c->aovP; A.segCounter = c->segCounter;
    A.W = c->share.W; A.H = c->share.H; A.n = c->facts.n; A.tn = c->facts.tn; A.ln = c->facts.ln;
    const sail_plugins& pl = c->facts.plugins;
    A.matMask = pl.material_mask; A.texMask = pl.texture_mask; A.lightMask = pl.light_mask;
    A.maxBounces = maxBounces; A.spp = nspp; A.accumMode = c->accumMode;
    A.tilesX = tx; A.tilesY = ty;
    A.world = (c->share.partMode == SAIL_PART_SAMPLES) ? 1 : c->share.world;
    A.rank = (c->share.partMode == SAIL_PART_SAMPLES) ? 0 : c->share.rank;
    A.ownedTiles = owned;
    A.tileMap = c->maskSet ? c->tileMap : nullptr;
    A.shadowAnyHit = c->shadowAnyHit;
    memcpy(A.eye, c->eyeCache, sizeof A.eye);
    refreshValues(c);  // the settle count may have crossed its threshold with the launch before
    const JitSlot* run = runningSlot(c, A.tileMap != nullptr, wavefrontFor(c->facts, c->sw));
    LaunchChunk chunk;
    chunk.nspp = nspp; chunk.owned = owned; chunk.masked = c->maskSet;
    chunk.cullFmaOk = cullFmaOk(c); chunk.eyeNearScene = eyeNearScene(c) != 0;
    chunk.run = run ? &run->spec : nullptr;
    const LaunchPlan P = planLaunch(c->facts, c->sw, c->share, chunk);
    A.cullPrims = P.cullPrims; A.cullPrimary = P.cullPrimary; A.kernelSet = P.kernelSet;
    A.lastQuietRows = P.cullPrims ? 0u : c->lastQuietRows[P.kernelLights];
    A.lastSkipSort = P.cullPrims ? 0 : c->lastSkipSort[P.kernelLights];
    A.groupSpp = P.groupSpp; A.sampleGroups = P.sampleGroups; A.groupHome = P.groupHome;
    A.stageStride = stageStride;
    if (P.staged) {  // sized for this launch's samples (it grows to the largest launch seen)
      const size_t need = (size_t)A.stageStride * (size_t)nspp * 3 * sizeof(float);
      if ((rc = growBuffer(c, &c->stage, &c->stageBytes, need, need, "sample-group stage"))) return rc;
      A.stage = c->stage;
    }
    SailWfState WS;
    memset(&WS, 0, sizeof WS);
    if (P.wavefront) {
      const size_t slots = (size_t)owned * 4096;
      if ((rc = growBuffer(c, &c->wf, &c->wfSlots, slots, slots * 11 * sizeof(float4), "wavefront state"))) return rc;
      float4* b = c->wf;
      WS.o = b; WS.d = b + c->wfSlots; WS.f = b + 2 * c->wfSlots; WS.e = b + 3 * c->wfSlots; WS.s = b + 4 * c->wfSlots;
      for (int i = 0; i < 6; i++) WS.sp[i] = b + (5 + i) * c->wfSlots;
    }
    hipEvent_t e0, e1;
    if ((rc = getEvent(c, &e0)) || (rc = getEvent(c, &e1))) return rc;
    HIPCHK(c, hipEventRecord(e0, c->stream));
    if (P.wavefront) {
      HIPCHK(c, sail_launch_wavefront(A, WS, c->stream));
    } else {
      if (run) {
        void* args[] = {&A};
        HIPCHK(c, hipModuleLaunchKernel(P.staged ? run->k.grouped : run->k.plain, P.grid, 1, 1, P.threads, 1, 1, 0, c->stream,
                                        args, nullptr));
        c->lastJit = true;
        c->lastJitMode = run->spec.mode;
        c->lastBuildId = run->k.buildId;
      } else {
        HIPCHK(c, sail_launch_trace(A, (int)P.grid, c->stream));
        c->lastJit = false;
      }
      if (P.staged) HIPCHK(c, sail_launch_accum(A, owned * 16, c->stream));
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    c->pending.emplace_back(e0, e1);
    c->lastGroups = A.sampleGroups;
    c->lastMasked = A.tileMap != nullptr;
    c->lastWavefront = P.wavefront;
    c->launches++;
    c->nominalSegments += (uint64_t)px * (uint64_t)nspp * (uint64_t)maxBounces;
    c->settled += (uint64_t)nspp;
  }
  refreshValues(c);
  return SAIL_OK;
}

}  // namespace

// Launch the queued one-sample frames of sail_render as one launch sequence (launchTrace splits it into launches of
// launchSpp samples). Their sample index and counts were taken when they were queued.
int flushQueued(sail_ctx* c) {
  if (c->queued.empty()) return SAIL_OK;
  std::vector<SailSample> q;
  q.swap(c->queued);
  HIPCHK(c, hipSetDevice(c->device));
  return launchTrace(c, q.data(), (int)q.size(), c->queuedBounces);
}

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
  const int set = kernelSetFor(c->facts, c->sw);
  const char* k = set == SAIL_KSET_CORNELL ? "sail_trace_kernel_cornell"
                  : set == SAIL_KSET_ROOM ? "sail_trace_kernel_room"
                  : (c->facts.n >= c->sw.cullMinPrims ? "sail_trace_kernel_cull" : "sail_trace_kernel");
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
  c->device = device; c->share.W = width; c->share.H = height; c->flags = flags;
  auto bail = [&](int code, const char* what) {
    g_create_error = std::string("sail_create: ") + what;
    sail_destroy(c);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(SAIL_E_HIP, "hipSetDevice");
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->share.numCUs = cus;
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
  void* bufs[] = {c->accum, c->aovN, c->aovP, c->filterOut, c->filterOut8, c->stage, c->segCounter, c->prims, c->tp, c->lt,
                  c->lightObjRow, c->samples, c->wf};
  for (void* b : bufs) if (b) (void)hipFree(b);
  freeMulti(c);  // every other file frees the first-use buffers it owns
  freeConverge(c);
  freePost(c);
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
  g->share.W = width; g->share.H = height; g->flags = flags; g->device = dev[0];
  g->share.world = n_devices;
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
    case SAIL_DEBUG_CULL_FMA: c->cullFma = value; break;
    case SAIL_DEBUG_JIT_WAIT:
      if (value < -1) return fail(c, SAIL_E_INVALID, "sail_set_debug: jit wait must be >= -1");
      c->jitWait = value;
      break;
    default: {  // a switch of the policy (sail_plan.h)
      const int jitWas = c->sw.jit;
      if (const char* why = setSwitch(&c->sw, option, value))
        return fail(c, SAIL_E_INVALID, "sail_set_debug: option %d: %s", option, why);
      // the value kernel's other form, derived anew below (refreshValues), or never a value kernel: back to the types
      // kernel; the rows did not move: the count stays
      if (((jitWas ^ c->sw.jit) & (32 | 64)) || (option == SAIL_DEBUG_JIT_VALUES_AFTER && value < 0)) {
        const uint64_t settled = c->settled;
        dropValues(c);
        c->settled = settled;
      }
    }
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
static int uploadPrims(sail_ctx* c, const DecodedScene& d) {
  const std::vector<SailPrim>& prims = d.prims;
  const int n = (int)prims.size();
  if (n <= 0) return SAIL_OK;
  const size_t chunks = (size_t)(n + 63) / 64;
  c->typeMasksHost.assign(chunks * 16, 0ull);
  for (int i = 0; i < n; i++)
    if (prims[i].type >= 0 && prims[i].type < 16) c->typeMasksHost[(size_t)(i / 64) * 16 + prims[i].type] |= 1ull << (i % 64);
  HIPCHK(c, hipMemcpyAsync(c->prims, prims.data(), sizeof(SailPrim) * n, hipMemcpyHostToDevice, c->stream));
  c->rowWords = d.rowWords;  // what a value kernel compiles in (refreshValues)
  HIPCHK(c, hipMemcpyAsync(c->prims + n, c->typeMasksHost.data(), chunks * 16 * sizeof(unsigned long long),
                           hipMemcpyHostToDevice, c->stream));
  return SAIL_OK;
}

// Decode the rows for the context's plugin set and derive what follows them: the rows' shape ids, the last-bounce classes
// for a kernel without and with a light plugin, and the scene's extent
static DecodedScene decodeRows(sail_ctx* c, const float* objects, int n, const float* texparams, int tn) {
  DecodedScene d = decodeScene(objects, n, texparams, tn, c->facts.plugins);
  c->shadowAnyHit = d.anyHit;
  c->scene = d.box;
  c->facts.primTypes = d.types;  // a kernel compiled for the rows follows them
  for (int l = 0; l < 2; l++)
    lastBounceRows(d.prims, texparams, tn, c->facts.plugins.material_mask, l != 0, &c->lastQuietRows[l], &c->lastSkipSort[l]);
  c->primExtent = primExtent(d.prims);
  return d;
}

// What a context forgets when its rows change (sail_set_scene, sail_update_objects, sail_move_objects), written once.
// The albedo map and the guide maps show the rows as they were, whoever moved them. The temporal views' ids and positions are stale, and
// with them the pending motion and the moments, unless the caller records how the rows moved (keepTemporal:
// sail_move_objects on a context with temporal state). The value kernel has the old rows' words compiled in: it goes and
// the settle count restarts; a drag keeps the types kernel, a changed shape type or plugin set starts the new rows'
// kernel building in the background (Tracer.update links the scene's program, tracer.js:42-90) while the precompiled
// kernel of the set serves. The accumulation restarts (resetAccum: the mark, the tile mask, "resolved").
static int rowsChanged(sail_ctx* c, bool keepTemporal) {
  c->albHave = false;
  c->guideHave = false;
  if (!keepTemporal) {
    c->tpHaveCur = c->tpHavePrev = c->tpResolved = false;
    clearMotion(c);
    HIPCHK(c, zeroMoments(c));
  }
  dropValues(c);
  refreshJit(c);
  refreshValues(c);
  return resetAccum(c);
}

int sail_set_scene(sail_ctx* c, const float* objects, int n, const float* texparams, int tn, const float* lights,
                   int ln, const sail_plugins* plugins) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs)
      if (int rc = sail_set_scene(s, objects, n, texparams, tn, lights, ln, plugins)) return relay(c, rc, s);
    c->haveScene = true; c->facts.n = n; c->facts.tn = tn; c->facts.ln = ln; c->dirty = false;
    c->loadMissing = 0;  // every device's accumulation restarted: a half-loaded checkpoint is abandoned
    return SAIL_OK;
  }
  if (n < 0 || tn < 0 || ln < 0 || (n > 0 && !objects) || (tn > 0 && !texparams) || (ln > 0 && !lights) || !plugins)
    return fail(c, SAIL_E_INVALID, "sail_set_scene: bad arguments (n=%d tn=%d ln=%d)", n, tn, ln);
  if (n > 0 && tn < 1) return fail(c, SAIL_E_INVALID, "sail_set_scene: objects need texParams rows");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->facts.plugins = *plugins;
  c->lastGroups = 1;
  c->lastWavefront = false;
  c->lastJit = false;
  const DecodedScene prims = decodeRows(c, objects, n, texparams, tn);
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
  c->facts.n = n; c->facts.tn = tn; c->facts.ln = ln;
  c->haveScene = true;
  return rowsChanged(c, false);
}

// New rows for a single-device context whose arguments have been checked: sail_update_objects (the temporal state goes,
// its ids and positions are stale) and sail_move_objects (it stays: the caller records how the rows moved)
static int updateRows(sail_ctx* c, const float* objects, int n, bool keepTemporal) {
  HIPCHK(c, hipSetDevice(c->device));
  const DecodedScene prims = decodeRows(c, objects, n, c->tpRows.data(), c->facts.tn);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = uploadPrims(c, prims)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->objectsRows.assign(objects, objects + (size_t)n * 18);
  return rowsChanged(c, keepTemporal);
}

int sail_update_objects(sail_ctx* c, const float* objects, int n) {
  if (c && !c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_update_objects(s, objects, n)) return relay(c, rc, s);
    c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (!c || !c->haveScene) return c ? fail(c, SAIL_E_STATE, "sail_update_objects before sail_set_scene") : SAIL_E_INVALID;
  if (n != c->facts.n || !objects) return fail(c, SAIL_E_INVALID, "sail_update_objects: n must stay %d", c->facts.n);
  return updateRows(c, objects, n, false);
}

int sail_move_objects(sail_ctx* c, const float* objects, int n, const float* motion, float hist_cap) {
  if (!c) return SAIL_E_INVALID;
  // everything is checked before anything changes: a refused call leaves rows, accumulator and temporal state alone
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_move_objects before sail_set_scene");
  if (n != c->facts.n || !objects) return fail(c, SAIL_E_INVALID, "sail_move_objects: n must stay %d", c->facts.n);
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

int sail_set_accum_mode(sail_ctx* c, int mode) {
  if (!c) return SAIL_E_INVALID;
  if (mode < SAIL_ACCUM_SUM || mode > SAIL_ACCUM_COMPAT8) return fail(c, SAIL_E_INVALID, "accum mode %d", mode);
  if (!c->subs.empty()) {
    for (sail_ctx* s : c->subs) if (int rc = sail_set_accum_mode(s, mode)) return relay(c, rc, s);
    c->accumMode = mode; c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (mode != SAIL_ACCUM_SUM && c->share.partMode == SAIL_PART_SAMPLES && c->share.world > 1)
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
    c->share.partMode = mode; c->dirty = false;
    c->loadMissing = 0;
    return SAIL_OK;
  }
  if (world < 1 || rank < 0 || rank >= world || (mode != SAIL_PART_TILES && mode != SAIL_PART_SAMPLES))
    return fail(c, SAIL_E_INVALID, "partition rank=%d world=%d mode=%d", rank, world, mode);
  if (mode == SAIL_PART_SAMPLES && world > 1 && c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_INVALID, "sample partition needs SAIL_ACCUM_SUM");
  HIPCHK(c, hipSetDevice(c->device));
  c->share.rank = rank; c->share.world = world; c->share.partMode = mode;
  refreshJit(c);  // the Cornell form's samples in flight follow the share of the frame (jitNsFor)
  refreshValues(c);
  return resetAccum(c);
}

int sail_set_launch_samples(sail_ctx* c, int spp) {
  if (!c) return SAIL_E_INVALID;
  if (spp < 0 || spp > 1 << 20) return fail(c, SAIL_E_INVALID, "launch samples %d", spp);  // 0: by form
  for (sail_ctx* s : c->subs) if (int rc = sail_set_launch_samples(s, spp)) return relay(c, rc, s);
  if (int rc = flushQueued(c)) return rc;
  c->sw.launchSpp = spp;
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
    if (c->share.partMode == SAIL_PART_SAMPLES && c->share.world > 1 && (int)(k % (uint64_t)c->share.world) != c->share.rank) continue;
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
  if (!(c->share.partMode == SAIL_PART_SAMPLES && c->share.world > 1 && (int)(k % (uint64_t)c->share.world) != c->share.rank)) {
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
  if ((int)c->queued.size() >= (c->sw.launchSpp > 0 ? c->sw.launchSpp : 64)) return flushQueued(c);
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
    if (int rc = reducedFrame(c, "sail_read_accum")) return rc;
    return relay(c, sail_read_accum(c->subs[0], rgba), c->subs[0]);
  }
  int rc = sail_sync(c);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(rgba, shownAccum(c), (size_t)c->share.W * c->share.H * sizeof(float4), hipMemcpyDeviceToHost));
  return SAIL_OK;
}

int sail_readback(sail_ctx* c, float* rgba, float* normal, float* position) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {
    if (int rc = reducedFrame(c, "sail_readback")) return rc;
    return relay(c, sail_readback(c->subs[0], rgba, normal, position), c->subs[0]);
  }
  int rc = sail_sync(c);
  if (rc) return rc;
  const size_t np = (size_t)c->share.W * c->share.H, bytes = np * sizeof(float4);
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
    if (int rc = reducedFrame(c, "sail_filter")) return rc;
    return relay(c, sail_filter(c->subs[0], kind, weights16, rx, ry, gammaC, out, out8), c->subs[0]);
  }
  if (kind < SAIL_FILTER_COLOR || kind > SAIL_FILTER_POSITION || (kind == SAIL_FILTER_WINDOW && !weights16))
    return fail(c, SAIL_E_INVALID, "sail_filter: kind %d", kind);
  if (kind >= SAIL_FILTER_WAVELET && !c->aovN)
    return fail(c, SAIL_E_STATE, "sail_filter: kind %d reads the AOVs (create with SAIL_FLAG_AOV)", kind);
  HIPCHK(c, hipSetDevice(c->device));
  int rc = sail_sync(c);
  if (rc) return rc;
  const size_t np = (size_t)c->share.W * c->share.H;
  if (out && (rc = allocOnce(c, &c->filterOut, np * sizeof(float4), "filter output"))) return rc;
  if (out8 && (rc = allocOnce(c, &c->filterOut8, np * 4, "filter output"))) return rc;
  float4* dOut = out ? c->filterOut : nullptr;
  uint8_t* dOut8 = out8 ? c->filterOut8 : nullptr;
  SailFilterArgs A;
  memset(&A, 0, sizeof A);
  A.accum = shownAccum(c); A.aovN = shownAovN(c); A.aovP = shownAovP(c);
  A.out = dOut; A.out8 = dOut8; A.W = c->share.W; A.H = c->share.H; A.kind = kind; A.accumMode = c->accumMode;
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
  if (e == hipSuccess) e = sail_launch_pick(c->prims, c->facts.n, dRays, count, dIdx, dT, c->stream);
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
      s->samples = c->share.partMode == SAIL_PART_SAMPLES ? s->samples + q.samples : q.samples;
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

int sail_jit_compile(const sail_plugins* plugins, int mode, const int32_t* row_types, int rows, void* code,
                     size_t* bytes) {
  if (!plugins || !bytes || mode < SAIL_JIT_MODE_FLAT || mode > SAIL_JIT_MODE_ROOM || rows < 0 ||
      rows > kSailJitMaxRows || (rows > 0 && !row_types))
    return SAIL_E_INVALID;
  // the plugin set's precompiled family, as kernelSetFor decides it for a flat scene of these masks (a light plugin
  // named stands for light rows)
  const sail_plugins& p = *plugins;
  const int set = cornellSet(p.shape_mask, p.material_mask, p.texture_mask, p.light_mask) ? SAIL_KSET_CORNELL
                  : (p.shape_mask & ~SAIL_KSET_ROOM_SHAPES) == 0                          ? SAIL_KSET_ROOM
                                                                                          : SAIL_KSET_GENERIC;
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
  // the specs a context with the product's defaults derives for this scene (jitSpecFor), without a device: for a large
  // share of the frame and for a small one, which differ for the Cornell form alone (16 samples in flight and 1, jitNsFor)
  const DecodedScene d = decodeScene(objects, n, texparams, tn, *plugins);
  const SceneFacts f = sceneFacts(d, tn, ln, *plugins);
  const PlanSwitches sw;
  if (built) *built = 0;
  SailJitSpec first;
  bool any = false;
  for (const ShareFacts& sh : {largeShare(), smallShare()}) {
    SailJitSpec spec;
    int mode = 0;
    if (!jitSpecFor(f, sw, sh, &spec, &mode)) return SAIL_OK;  // the scene gets no run-time kernel
    if (any && sailJitSpecEqual(spec, first)) break;  // one shape serves both shares
    first = spec;
    any = true;
    std::string err;
    if (sail_jit_code_to_dir(arch, spec, dir, &err)) return fail(nullptr, SAIL_E_INVALID, "sail_jit_prebuild: %s", err.c_str());
    // and the value kernel a context loads once the scene has settled, where the spec has one
    SailJitSpec vspec;
    if (valueSpecFor(spec, d.rowWords, texparams, tn, sw.jit, &vspec) && sail_jit_code_to_dir(arch, vspec, dir, &err))
      return fail(nullptr, SAIL_E_INVALID, "sail_jit_prebuild: %s", err.c_str());
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
  // as sail_jit_prebuild: the spec a context with these switches (else the product's defaults) derives, without a device,
  // for a small share of the frame (the Cornell form holding 1 sample in flight) and a scene without light rows
  const DecodedScene d = decodeScene(objects, n, texparams, tn, *plugins);
  const SceneFacts f = sceneFacts(d, tn, 0, *plugins);
  PlanSwitches sw;
  if (jit >= 0) sw.jit = jit;
  SailJitSpec spec, vspec;
  int mode = 0;
  *key = 0;
  if (!jitSpecFor(f, sw, smallShare(), &spec, &mode) || (value && !valueSpecFor(spec, d.rowWords, texparams, tn, sw.jit, &vspec))) {
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
  const DecodedScene d = decodeScene(objects, n, texparams, tn, *plugins);
  lastBounceRows(d.prims, texparams, tn, plugins->material_mask, kernel_lights != 0, quiet_rows, skip_sort);
  return SAIL_OK;
}

int sail_plan_launch(const sail_launch_facts* in, sail_launch_plan* out) {
  if (!in || !out) return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: bad arguments");
  const sail_launch_facts& q = *in;
  if (q.n < 1 || q.tn < 1 || q.ln < 0 || !q.objects || !q.texparams || !q.plugins)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: bad scene (n=%d tn=%d ln=%d)", q.n, q.tn, q.ln);
  if (q.width <= 0 || q.height <= 0 || q.width > 32768 || q.height > 32768 || q.world < 1 || q.rank < 0 || q.rank >= q.world ||
      (q.part_mode != SAIL_PART_TILES && q.part_mode != SAIL_PART_SAMPLES) || q.compute_units < 1)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: bad share (%dx%d rank %d of %d, mode %d, %d CUs)", q.width, q.height,
                q.rank, q.world, q.part_mode, q.compute_units);
  if (q.nspp < 1 || q.launch_spp < 0 || q.tier < SAIL_LAUNCH_TIER_NONE || q.tier > SAIL_LAUNCH_TIER_VALUE)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: bad launch (nspp=%d launch_spp=%d tier=%d)", q.nspp, q.launch_spp, q.tier);
  PlanSwitches sw;
  sw.launchSpp = q.launch_spp;
  for (int o = 0; o < 16; o++)
    if ((q.debug_set >> o) & 1u)
      if (const char* why = setSwitch(&sw, o, q.debug[o]))
        return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: option %d: %s", o, why);
  ShareFacts sh;
  sh.W = q.width; sh.H = q.height; sh.rank = q.rank; sh.world = q.world; sh.partMode = q.part_mode; sh.numCUs = q.compute_units;
  int tx, ty;
  const int share = partitionTiles(sh, &tx, &ty);
  if (q.active_tiles > share || share < 1 || q.active_tiles == 0)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: no tile to trace (%d active of the share's %d)", q.active_tiles, share);
  const DecodedScene d = decodeScene(q.objects, q.n, q.texparams, q.tn, *q.plugins);
  const SceneFacts f = sceneFacts(d, q.tn, q.ln, *q.plugins);
  // the kernel that runs, as a context derives it: the types spec of the scene and share, and the value spec on top
  SailJitSpec types, value;
  int mode = 0;
  const bool haveTypes = jitSpecFor(f, sw, sh, &types, &mode);
  if (q.tier >= SAIL_LAUNCH_TIER_TYPES && !haveTypes)
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: the scene gets no run-time kernel under these switches");
  if (q.tier == SAIL_LAUNCH_TIER_VALUE && !valueSpecFor(types, d.rowWords, q.texparams, q.tn, sw.jit, &value))
    return fail(nullptr, SAIL_E_INVALID, "sail_plan_launch: the scene gets no value kernel under these switches");
  LaunchChunk k;
  k.nspp = q.nspp;
  k.masked = q.active_tiles > 0;
  k.owned = k.masked ? q.active_tiles : share;
  k.cullFmaOk = q.cull_fma_ok != 0; k.eyeNearScene = q.eye_near_scene != 0;
  k.run = q.tier == SAIL_LAUNCH_TIER_VALUE ? &value : (q.tier == SAIL_LAUNCH_TIER_TYPES ? &types : nullptr);
  const LaunchPlan P = planLaunch(f, sw, sh, k);
  memset(out, 0, sizeof *out);
  out->kernel_set = P.kernelSet; out->cull_prims = P.cullPrims; out->cull_primary = P.cullPrimary;
  out->wavefront = P.wavefront; out->ns = P.ns;
  out->sample_groups = P.sampleGroups; out->group_spp = P.groupSpp; out->group_home = P.groupHome; out->staged = P.staged;
  out->grid = P.grid; out->threads = P.threads;
  out->kernel_lights = P.kernelLights;
  out->jit_mode = (k.run && !P.wavefront) ? k.run->mode : -1;
  out->launch_samples = launchSamples(sw, haveTypes ? &types : nullptr);
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
