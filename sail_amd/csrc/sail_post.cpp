// sail_post.cpp — the passes over a rendered frame: the a-trous denoiser (sail_denoise.hip), camera- and object-motion
// reprojection (sail_temporal.hip), moment tracking and the temporal filter (sail_tfilter.hip), the albedo map
// (sail_albedo.hip), the guide maps (sail_guides.hip). The context is sail_ctx.h's; sail_capi.cpp's rowsChanged says what of this new rows invalidate.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "sail_ctx.h"

namespace {

// ---- the work blocks' layouts ---------------------------------------------------------------------------------------------------
// Every block is arrays of np pixels or nt 16x16 tiles, back to back, the widest element first (each array is aligned to
// its own type). A block is described once, by a carve() that names its arrays in order: with a null base a Carve only
// adds up the bytes, so the size that is allocated (workBytes) and the typed pointers (workAt) cannot disagree.
struct Carve {
  char* base;
  size_t off = 0;
  template <class T> constexpr void operator()(T*& p, size_t count) {
    p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
  }
};
template <class L> constexpr size_t workBytes(size_t np, size_t nt) {
  Carve k{nullptr};
  L l{};
  l.carve(k, np, nt);
  return k.off;
}
template <class L> L workAt(const sail_ctx* c, void* base) {
  Carve k{(char*)base};
  L l{};
  l.carve(k, pixels(c), tiles16(c));
  return l;
}
// allocated on first use and kept for the context's life
template <class L, class T> int ensureWork(sail_ctx* c, T** block, const char* what) {
  return allocOnce(c, block, workBytes<L>(pixels(c), tiles16(c)), what);
}

// the a-trous passes' work buffers (sail_denoise and sail_temporal_filter share them; sail_ctx.denoiseWork)
struct DenoiseWork {
  float4 *cv[2], *g0;
  float2* g1;
  float* var;
  uint32_t *u8, *bad;
  constexpr void carve(Carve& k, size_t np, size_t nt) { k(cv[0], np); k(cv[1], np); k(g0, np); k(g1, np); k(var, np); k(u8, np); k(bad, nt); }
};
// the temporal maps (tpWork): `maps` in the order the context's pointers start in, G_cur, G_prev, Hist, R, Out (a
// committed view swaps those, never these); the RGBA8 map; the counts of begin (hit, hist) and resolve (hist, bad)
struct TemporalWork {
  float4* maps[5];
  uint32_t *out8, *tileHit, *tileHist, *tileBad;
  constexpr void carve(Carve& k, size_t np, size_t nt) {
    for (float4*& m : maps) k(m, np);
    k(out8, np); k(tileHit, nt); k(tileHist, nt); k(tileBad, nt);
  }
};
// the moment maps (tpMom) as the context's pointers start, Mhist, MR, Mout, and the filter's count of temporal pixels
struct MomentWork {
  float4* maps[3];
  uint32_t* tileTemporal;
  constexpr void carve(Carve& k, size_t np, size_t nt) {
    for (float4*& m : maps) k(m, np);
    k(tileTemporal, nt);
  }
};
struct AlbedoWork {  // albMap
  float4* map;
  uint32_t *tileHit, *tilePartial;
  constexpr void carve(Carve& k, size_t np, size_t nt) { k(map, np); k(tileHit, nt); k(tilePartial, nt); }
};
struct GuideWork {  // guideMaps
  float4 *n, *x;
  uint32_t *tileHit, *tileFollowed, *tileTruncated;
  constexpr void carve(Carve& k, size_t np, size_t nt) { k(n, np); k(x, np); k(tileHit, nt); k(tileFollowed, nt); k(tileTruncated, nt); }
};
struct GbufferScratch {  // sail_gbuffer's own, freed by the call
  float4* G;
  float (*rays)[6];
  float* t;
  constexpr void carve(Carve& k, size_t np, size_t) { k(G, np); k(rays, np); k(t, np); }
};
template <class L> constexpr bool sized(size_t perPixel, size_t perTile) {
  return workBytes<L>(1, 1) == perPixel + perTile && workBytes<L>(33 * 17, 3 * 2) == perPixel * (33 * 17) + perTile * (3 * 2);
}
static_assert(sized<DenoiseWork>(64, 4) && sized<TemporalWork>(84, 12) && sized<MomentWork>(48, 4) &&
                  sized<AlbedoWork>(16, 8) && sized<GuideWork>(32, 12) && sized<GbufferScratch>(44, 0),
              "a work block's size is part of what the context allocates per frame: it does not change");

DenoiseWork denoiseWork(const sail_ctx* c) { return workAt<DenoiseWork>(c, c->denoiseWork); }
TemporalWork temporalWork(const sail_ctx* c) { return workAt<TemporalWork>(c, c->tpWork); }
MomentWork momentWork(const sail_ctx* c) { return workAt<MomentWork>(c, c->tpMom); }
AlbedoWork albedoWork(const sail_ctx* c) { return workAt<AlbedoWork>(c, c->albMap); }
GuideWork guideWork(const sail_ctx* c) { return workAt<GuideWork>(c, c->guideMaps); }

// ---- what the calls share -------------------------------------------------------------------------------------------------------
void setView(View* v, const double mvp[16], const float eye[3]) {
  memset(v, 0, sizeof *v);
  for (int i = 0; i < 16; i++) v->m[i] = (float)mvp[i];
  memcpy(v->eye, eye, sizeof v->eye);
}
bool sameView(const View& a, const View& b) { return memcmp(&a, &b, sizeof a) == 0; }

template <class T> hipError_t toHost(void* host, const T* dev, size_t count) {
  return hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
}
// the tail of every read and load call: the stream idle, then one blocking copy of `count` float4 texels
int moveMap(sail_ctx* c, void* dst, const void* src, size_t count, hipMemcpyKind kind) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, src, count * sizeof(float4), kind));
  return SAIL_OK;
}
int readMap(sail_ctx* c, const float4* dev, float* host, size_t count) { return moveMap(c, host, dev, count, hipMemcpyDeviceToHost); }
int loadMap(sail_ctx* c, float4* dev, const float* host, size_t count) { return moveMap(c, dev, host, count, hipMemcpyHostToDevice); }

// Times the passes of one call on the context's stream, on top of PooledEvents: mark() records the next event, run()
// launches or copies, and both do nothing once a step has failed (e carries the first failure). finish() synchronises
// the stream and gives ms[i], the time between marks i and i + 1, and the time from the first mark to the last.
struct PassTimer {
  sail_ctx* c;
  PooledEvents ev;
  int marks = 0;
  hipError_t e = hipSuccess;
  PassTimer(sail_ctx* ctx, int want) : c(ctx), ev(ctx, want) {}
  int rc() const { return ev.rc; }  // the pool could not give the events: nothing was started
  void mark() { if (e == hipSuccess) e = hipEventRecord(ev[marks++], c->stream); }
  template <class Step> void run(Step step) { if (e == hipSuccess) e = step(); }
  hipError_t finish(float* ms, float* total = nullptr) {
    run([&] { return hipStreamSynchronize(c->stream); });
    for (int i = 0; i + 1 < marks; i++) run([&] { return hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]); });
    if (total) run([&] { return hipEventElapsedTime(total, ev[0], ev[marks - 1]); });
    return e;
  }
  template <class Step> hipError_t one(Step step, float* ms) { mark(); run(step); mark(); return finish(ms); }  // one span
};

// What sail_denoise and sail_temporal_filter share: `prepare` launches the pass that fills (cv[0], g0, g1) and the
// per-tile counts, then the a-trous passes run with steps 1, 2, 4, ..., an event round every pass (ms[0] = prepare,
// ms[1..] = the passes; T holds iterations + 2 events); the stream is synchronised and the outputs that are asked for are
// copied back.
// With a map `alb` (the demodulated calls) the last pass is the remodulating instance.
template <class Prepare>
hipError_t runAtrous(sail_ctx* c, PassTimer& T, const DenoiseWork& w, Prepare prepare, int iterations, float sigma_l,
                     float sigma_x, int display, float gamma_c, float* out_rgba, float* out_var, uint8_t* out_rgba8,
                     float ms[8], float* total, const float4* alb = nullptr, float amin = 0.0f) {
  const size_t np = pixels(c);
  T.mark();
  T.run(prepare);
  T.mark();
  int cur = 0;
  for (int it = 0; it < iterations && T.e == hipSuccess; it++) {
    const bool last = it == iterations - 1;
    SailDenoiseAtrousArgs B;
    memset(&B, 0, sizeof B);
    B.src = w.cv[cur];
    B.dst = (last && !out_rgba) ? nullptr : w.cv[cur ^ 1];
    B.g0 = w.g0; B.g1 = w.g1;
    B.outVar = (last && out_var) ? w.var : nullptr;
    B.out8 = (last && out_rgba8) ? w.u8 : nullptr;
    B.W = c->share.W; B.H = c->share.H;
    B.step = 1 << it;
    B.last = last;
    B.sl2 = sigma_l * sigma_l;
    const float sx = sigma_x * (float)B.step;
    B.sxs = sx * sx;
    B.display = display; B.gammaC = gamma_c;
    SailDenoiseAtrousRemodArgs R;
    memset(&R, 0, sizeof R);
    R.P = B; R.alb = alb; R.amin = amin;
    T.run([&] { return (last && alb) ? sail_launch_denoise_atrous_remod(R, c->stream) : sail_launch_denoise_atrous(B, c->stream); });
    T.mark();
    cur ^= 1;
  }
  hipError_t e = T.finish(ms, total);
  if (e == hipSuccess && out_rgba) e = toHost(out_rgba, w.cv[cur], np);
  if (e == hipSuccess && out_var) e = toHost(out_var, w.var, np);
  if (e == hipSuccess && out_rgba8) e = toHost(out_rgba8, w.u8, np);
  return e;
}

}  // namespace

// the three moment maps of a context that tracks them (sail_temporal_moments), zeroed on its stream
hipError_t zeroMoments(sail_ctx* c) {
  if (!c->tpMom) return hipSuccess;
  return hipMemsetAsync(c->tpMom, 0, workBytes<MomentWork>(pixels(c), 0), c->stream);  // the maps, not the tile counts
}

// nothing is pending for the next sail_temporal_begin any more (sail_move_objects)
void clearMotion(sail_ctx* c) {
  c->tpMotionPending = false;
  c->tpMotion.clear();
  c->tpMotionCap = INFINITY;
}

void freePost(sail_ctx* c) {
  for (void* b : {c->denoiseWork, c->tpWork, c->tpMom, (void*)c->tpMotionDev, (void*)c->albMap, (void*)c->guideMaps}) if (b) (void)hipFree(b);
}

extern "C" {

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

// The normal and position maps a filter reads: the shown AOVs, or with sail_use_guides the guide maps (Ng, then Xg)
const float4* filterN(const sail_ctx* c) { return c->useGuides ? guideWork(c).n : shownAovN(c); }
const float4* filterX(const sail_ctx* c) { return c->useGuides ? guideWork(c).x : shownAovP(c); }
// what a filter refuses about them (temporal: the maps must belong to the current temporal view)
int filterGuides(sail_ctx* c, const char* who, bool temporal) {
  if (!c->useGuides) return SAIL_OK;
  if (!c->guideHave || !c->guideMaps)
    return fail(c, SAIL_E_STATE, "%s: no guide maps (sail_guides or sail_guides_load first; new rows drop them)", who);
  if (temporal && !sameView(c->guideView, c->tpCur))
    return fail(c, SAIL_E_STATE, "%s: the guide maps belong to another view than the current temporal view", who);
  return SAIL_OK;
}

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
    if (int rc = reducedFrame(c, who)) return rc;
    return relay(c, denoiseCall(c->subs[0], who, demod, &p, amin, out_rgba, out_var, out_rgba8, info), c->subs[0]);
  }
  if (!c->useGuides && (!c->aovN || !c->aovP))
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
  if (int rc = filterGuides(c, who, false)) return rc;
  const size_t nt = tiles16(c);
  if (int rc = ensureWork<DenoiseWork>(c, &c->denoiseWork, "denoise work buffers")) return rc;
  const DenoiseWork w = denoiseWork(c);
  SailDenoisePrepareArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.P = c->noiseMark; A.N = filterN(c); A.X = filterX(c);
  A.cv = w.cv[0]; A.g0 = w.g0; A.g1 = w.g1; A.tileBad = w.bad;
  A.W = c->share.W; A.H = c->share.H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k; A.hf = (float)c->noiseK;
  float ms[8] = {}, total = 0.0f;
  SailDenoisePrepareDemodArgs D;
  memset(&D, 0, sizeof D);
  D.P = A; D.alb = c->albMap; D.amin = amin;
  PassTimer T(c, p.iterations + 2);
  if (T.rc()) return T.rc();
  hipError_t e = runAtrous(c, T, w, [&] { return demod ? sail_launch_denoise_prepare_demod(D, c->stream)
                                                         : sail_launch_denoise_prepare(A, c->stream); },
                           p.iterations, p.sigma_l, p.sigma_x, p.display, p.gamma_c, out_rgba, out_var, out_rgba8, ms, &total,
                           demod ? c->albMap : nullptr, amin);
  std::vector<uint32_t> bad(nt);
  if (e == hipSuccess) e = toHost(bad.data(), w.bad, nt);
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

int ensureTemporal(sail_ctx* c) {
  if (c->tpWork) return SAIL_OK;
  if (int rc = ensureWork<TemporalWork>(c, &c->tpWork, "temporal maps")) return rc;
  const TemporalWork w = temporalWork(c);
  c->tpGcur = w.maps[0]; c->tpGprev = w.maps[1]; c->tpHist = w.maps[2]; c->tpR = w.maps[3]; c->tpOut = w.maps[4];
  return SAIL_OK;
}

// what a view pass takes (sail_view.h): the scene's rows and, for a view, the corner directions of a sample without jitter
int viewArgs(sail_ctx* c, const char* who, const double mvp[16], const float eye[3], SailViewArgs* V) {
  float inv[16];
  if (sail_jitter_inverse(mvp, 0.0, 0.0, c->share.W, c->share.H, inv) != SAIL_OK)
    return fail(c, SAIL_E_INVALID, "%s: the camera matrix is singular", who);
  memset(V, 0, sizeof *V);
  V->prims = c->prims; V->n = c->facts.n;
  cornerDirs(inv, eye, V->d);
  memcpy(V->eye, eye, sizeof V->eye);
  V->W = c->share.W; V->H = c->share.H;
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
  memset(&A, 0, sizeof A);
  if (int rc = viewArgs(c, "sail_gbuffer", mvp, eye, &A.V)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t np = pixels(c);
  void* work = nullptr;
  if (hipMalloc(&work, workBytes<GbufferScratch>(np, 0)) != hipSuccess) return fail(c, SAIL_E_OOM, "G-buffer scratch");
  const GbufferScratch w = workAt<GbufferScratch>(c, work);
  A.G = w.G;
  A.rays = rays6 ? *w.rays : nullptr;
  A.t = t ? w.t : nullptr;
  std::vector<float4> g((id || xyz) ? np : 0);
  hipError_t e = sail_launch_gbuffer(A, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && !g.empty()) e = toHost(g.data(), w.G, np);
  if (e == hipSuccess && rays6) e = toHost(rays6, w.rays, np);
  if (e == hipSuccess && t) e = toHost(t, w.t, np);
  (void)hipFree(work);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_gbuffer: %s", hipGetErrorString(e));
  for (size_t i = 0; i < np && !g.empty(); i++) {
    if (id) id[i] = (int32_t)g[i].w;
    if (xyz) { xyz[3 * i] = g[i].x; xyz[3 * i + 1] = g[i].y; xyz[3 * i + 2] = g[i].z; }
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
    if (int rc = reducedFrame(c, "sail_temporal_begin")) return rc;
    return relay(c, sail_temporal_begin(c->subs[0], mvp, eye, &p, info), c->subs[0]);
  }
  if (int rc = temporalState(c, "sail_temporal_begin")) return rc;
  SailGbufferArgs A;
  memset(&A, 0, sizeof A);
  if (int rc = viewArgs(c, "sail_temporal_begin", mvp, eye, &A.V)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (int rc = ensureTemporal(c)) return rc;
  const bool moved = c->tpMotionPending;
  if (moved) {  // before anything is committed: a begin that fails keeps it all
    const int rows = c->facts.n > 0 ? c->facts.n : 1;
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
  const size_t nt = tiles16(c), np = pixels(c);
  const TemporalWork w = temporalWork(c);
  A.G = c->tpGcur;
  SailReprojectArgs B;
  memset(&B, 0, sizeof B);
  B.Gcur = c->tpGcur; B.Gprev = c->tpGprev; B.hist = c->tpHist; B.out = c->tpR;
  B.tileHit = w.tileHit; B.tileHist = w.tileHist;
  for (int j = 0; j < 4; j++) { B.Mp[0][j] = c->tpPrev.m[j]; B.Mp[1][j] = c->tpPrev.m[4 + j]; B.Mp[2][j] = c->tpPrev.m[12 + j]; }
  memcpy(B.eyePrev, c->tpPrev.eye, sizeof B.eyePrev);
  B.tol2 = p.pos_tol * p.pos_tol;
  B.W = c->share.W; B.H = c->share.H;
  B.haveHist = c->tpHavePrev;
  // an object motion is pending (sail_move_objects): the moved kernels, with the table uploaded ahead of them
  B.motion = c->tpMotionDev; B.n = c->facts.n; B.mc = c->tpMotionCap;
  c->tpResolved = false;
  // moment tracking: the same gather over Mhist, timed with the reproject pass
  SailReprojectArgs M = B;
  M.hist = c->tpMhist; M.out = c->tpMR;
  M.tileHit = nullptr; M.tileHist = nullptr;
  PassTimer T(c, c->tpMom ? 4 : 3);
  if (T.rc()) return T.rc();
  const auto copyMap = [&](float4* dst, const float4* src) { return hipMemcpyAsync(dst, src, np * sizeof(float4), hipMemcpyDeviceToDevice, c->stream); };
  if (moved && c->facts.n > 0)
    T.run([&] { return hipMemcpyAsync(c->tpMotionDev, c->tpMotion.data(), sizeof(float4) * (size_t)c->facts.n, hipMemcpyHostToDevice, c->stream); });
  T.mark();
  T.run([&] { return sail_launch_gbuffer(A, c->stream); });
  T.mark();
  T.run([&] { return sail_launch_reproject(B, moved, c->stream); });
  T.mark();
  if (c->tpMom) {
    T.run([&] { return sail_launch_moment_reproject(M, moved, c->stream); });
    T.mark();
    T.run([&] { return copyMap(c->tpMout, c->tpMR); });
  }
  T.run([&] { return copyMap(c->tpOut, c->tpR); });
  float ms[3] = {};
  hipError_t e = T.finish(ms);
  ms[1] += ms[2];  // the moment reproject, when it ran
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = toHost(host.data(), w.tileHit, nt * 2);  // and tileHist behind it
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_temporal_begin: %s", hipGetErrorString(e));
  setView(&c->tpCur, mvp, eye);
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
    if (int rc = reducedFrame(c, "sail_temporal_resolve")) return rc;
    return relay(c, sail_temporal_resolve(c->subs[0], &p, out_rgba, out_rgba8, info), c->subs[0]);
  }
  if (int rc = temporalState(c, "sail_temporal_resolve")) return rc;
  if (!c->tpHaveCur || !c->tpWork)
    return fail(c, SAIL_E_STATE, "sail_temporal_resolve: no current view (sail_temporal_begin first; a new scene drops it)");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t nt = tiles16(c), np = pixels(c);
  const TemporalWork w = temporalWork(c);
  SailResolveArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.R = c->tpR; A.Out = c->tpOut;
  A.out8 = out_rgba8 ? w.out8 : nullptr;
  A.tileHist = w.tileHist; A.tileBad = w.tileBad;
  A.W = c->share.W; A.H = c->share.H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k;
  A.cap = p.cap; A.display = p.display; A.gammaC = p.gamma_c;
  SailMomentResolveArgs M;  // moment tracking: blended like the colour, timed with it
  memset(&M, 0, sizeof M);
  M.S = A.S; M.MR = c->tpMR; M.Mout = c->tpMout;
  M.W = c->share.W; M.H = c->share.H; M.mix = A.mix; M.kf = A.kf; M.cap = A.cap;
  PassTimer T(c, 2);
  if (T.rc()) return T.rc();
  float ms = 0.0f;
  hipError_t e = T.one([&] {
    const hipError_t r = sail_launch_temporal_resolve(A, c->stream);
    return (r == hipSuccess && c->tpMom) ? sail_launch_moment_resolve(M, c->stream) : r;
  }, &ms);
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = toHost(host.data(), w.tileHist, nt * 2);  // and tileBad behind it
  if (e == hipSuccess && out_rgba) e = toHost(out_rgba, c->tpOut, np);
  if (e == hipSuccess && out_rgba8) e = toHost(out_rgba8, w.out8, np);
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
  return readMap(c, maps[which], out, pixels(c));
}

int sail_temporal_load_history(sail_ctx* c, const float* hist, const float* g, const double mvp_prev[16],
                               const float eye_prev[3]) {
  if (!c) return SAIL_E_INVALID;
  if (!hist || !g || !mvp_prev || !eye_prev)
    return fail(c, SAIL_E_INVALID, "sail_temporal_load_history: hist, g, mvp_prev and eye_prev are required");
  if (!c->subs.empty()) return relay(c, sail_temporal_load_history(c->subs[0], hist, g, mvp_prev, eye_prev), c->subs[0]);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensureTemporal(c)) return rc;
  if (int rc = loadMap(c, c->tpHist, hist, pixels(c))) return rc;
  if (int rc = loadMap(c, c->tpGprev, g, pixels(c))) return rc;
  setView(&c->tpPrev, mvp_prev, eye_prev);
  c->tpHavePrev = true;
  c->tpHaveCur = false;
  c->tpResolved = false;
  clearMotion(c);  // a loaded history belongs to the rows as they are now
  if (c->tpMom) {  // the loaded history carries no moments
    HIPCHK(c, hipMemsetAsync(c->tpMhist, 0, pixels(c) * sizeof(float4), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return SAIL_OK;
}

int sail_temporal_pending_motion(sail_ctx* c, float* motion, float* hist_cap, int* pending) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_temporal_pending_motion(c->subs[0], motion, hist_cap, pending), c->subs[0]);
  for (int r = 0; motion && r < c->facts.n; r++)
    for (int j = 0; j < 3; j++) motion[r * 3 + j] = c->tpMotionPending ? c->tpMotion[(size_t)r * 4 + j] : 0.0f;
  if (hist_cap) *hist_cap = c->tpMotionPending ? c->tpMotionCap : INFINITY;
  if (pending) *pending = c->tpMotionPending ? 1 : 0;
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
  if (int rc = ensureWork<MomentWork>(c, &c->tpMom, "moment maps")) return rc;
  const MomentWork w = momentWork(c);
  c->tpMhist = w.maps[0]; c->tpMR = w.maps[1]; c->tpMout = w.maps[2];
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
  return loadMap(c, c->tpMhist, mom, pixels(c));
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
  return readMap(c, maps[which], out, pixels(c));
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
    if (int rc = reducedFrame(c, who)) return rc;
    return relay(c, tfilterCall(c->subs[0], who, demod, &p, amin, out_rgba, out_var, out_rgba8, info), c->subs[0]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (!c->tpMom)
    return fail(c, SAIL_E_STATE, "%s: moment tracking is off (sail_temporal_moments first)", who);
  if (!c->useGuides && (!c->aovN || !c->aovP))
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
  if (demod && !sameView(c->albView, c->tpCur))
    return fail(c, SAIL_E_STATE, "%s: the albedo map belongs to another view than the current temporal view", who);
  if (int rc = filterGuides(c, who, true)) return rc;
  const size_t nt = tiles16(c), np = pixels(c);
  if (int rc = ensureWork<DenoiseWork>(c, &c->denoiseWork, "denoise work buffers")) return rc;
  const DenoiseWork w = denoiseWork(c);  // sail_denoise's work buffers; the count of temporal pixels sits behind the moments
  uint32_t* dTmp = momentWork(c).tileTemporal;
  SailTfilterPrepareArgs A;
  memset(&A, 0, sizeof A);
  A.Out = c->tpOut; A.Mout = c->tpMout; A.S = shownAccum(c); A.N = filterN(c); A.X = filterX(c);
  A.cv = w.cv[0]; A.g0 = w.g0; A.g1 = w.g1; A.tileBad = w.bad; A.tileTemporal = dTmp;
  A.W = c->share.W; A.H = c->share.H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k;
  A.minHist = p.min_hist;
  const float sx2 = p.sigma_x * 2.0f;
  A.sx0 = sx2 * sx2;
  float ms[8] = {}, total = 0.0f;
  SailTfilterPrepareDemodArgs D;
  memset(&D, 0, sizeof D);
  D.P = A; D.alb = c->albMap; D.amin = amin;
  PassTimer T(c, p.iterations + 2);
  if (T.rc()) return T.rc();
  hipError_t e = runAtrous(c, T, w, [&] { return demod ? sail_launch_tfilter_prepare_demod(D, c->stream)
                                                         : sail_launch_tfilter_prepare(A, c->stream); },
                           p.iterations, p.sigma_l, p.sigma_x, p.display, p.gamma_c, out_rgba, out_var, out_rgba8, ms, &total,
                           demod ? c->albMap : nullptr, amin);
  std::vector<uint32_t> bad(nt), tmp(nt);
  if (e == hipSuccess) e = toHost(bad.data(), w.bad, nt);
  if (e == hipSuccess) e = toHost(tmp.data(), dTmp, nt);
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

int ensureAlbedo(sail_ctx* c) { return ensureWork<AlbedoWork>(c, &c->albMap, "albedo map"); }
int ensureGuides(sail_ctx* c) { return ensureWork<GuideWork>(c, &c->guideMaps, "guide maps"); }

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
  SailAlbedoArgs A;
  memset(&A, 0, sizeof A);
  if (int rc = viewArgs(c, "sail_albedo", mvp, eye, &A.V)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (int rc = ensureAlbedo(c)) return rc;
  const size_t nt = tiles16(c);
  const AlbedoWork w = albedoWork(c);
  A.texparams = c->tp; A.tn = c->facts.tn;
  A.texMask = c->facts.plugins.texture_mask;
  A.grid = grid;
  A.A = w.map;
  A.tileHit = w.tileHit; A.tilePartial = w.tilePartial;
  c->albHave = false;  // a call that fails leaves no map
  PassTimer T(c, 2);
  if (T.rc()) return T.rc();
  float ms = 0.0f;
  hipError_t e = T.one([&] { return sail_launch_albedo(A, c->stream); }, &ms);
  std::vector<uint32_t> host(nt * 2);
  if (e == hipSuccess) e = toHost(host.data(), w.tileHit, nt * 2);  // and tilePartial behind it
  if (e == hipSuccess && out_rgba) e = toHost(out_rgba, w.map, pixels(c));
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_albedo: %s", hipGetErrorString(e));
  setView(&c->albView, mvp, eye);
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
  if (int rc = ensureAlbedo(c)) return rc;
  if (int rc = loadMap(c, c->albMap, map, pixels(c))) return rc;
  setView(&c->albView, mvp, eye);
  c->albHave = true;
  return SAIL_OK;
}

int sail_albedo_read(sail_ctx* c, float* out) {
  if (!c) return SAIL_E_INVALID;
  if (!out) return fail(c, SAIL_E_INVALID, "sail_albedo_read: an output is required");
  if (!c->subs.empty()) return relay(c, sail_albedo_read(c->subs[0], out), c->subs[0]);
  if (!c->albHave || !c->albMap)
    return fail(c, SAIL_E_STATE, "sail_albedo_read: no albedo map (sail_albedo or sail_albedo_load first; new rows drop it)");
  return readMap(c, c->albMap, out, pixels(c));
}

// ---- the guide maps of a view (include/sail_hip.h; the kernel is sail_guides.hip) ----------------------------------------------
int sail_guides(sail_ctx* c, const double mvp[16], const float eye[3], int depth, float* out_n, float* out_x,
                sail_guides_info* info) {
  if (depth < 0 || depth > 8) return fail(c, SAIL_E_INVALID, "sail_guides: depth %d of 0..8", depth);
  if (!c) return fail(c, SAIL_E_INVALID, "sail_guides: a context is required");
  if (!mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_guides: mvp and eye are required");
  if (!c->subs.empty()) return relay(c, sail_guides(c->subs[0], mvp, eye, depth, out_n, out_x, info), c->subs[0]);
  if (!c->haveScene) return fail(c, SAIL_E_STATE, "sail_guides: no scene (call sail_set_scene first)");
  SailGuidesArgs A;
  memset(&A, 0, sizeof A);
  if (int rc = viewArgs(c, "sail_guides", mvp, eye, &A.V)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  if (int rc = ensureGuides(c)) return rc;
  const size_t nt = tiles16(c), np = pixels(c);
  const GuideWork w = guideWork(c);
  A.texparams = c->tp; A.tn = c->facts.tn;
  A.matMask = c->facts.plugins.material_mask; A.texMask = c->facts.plugins.texture_mask;
  A.depth = depth;
  A.Ng = w.n; A.Xg = w.x;
  A.tileHit = w.tileHit; A.tileFollowed = w.tileFollowed; A.tileTruncated = w.tileTruncated;
  c->guideHave = false;  // a call that fails leaves no maps
  PassTimer T(c, 2);
  if (T.rc()) return T.rc();
  float ms = 0.0f;
  hipError_t e = T.one([&] { return sail_launch_guides(A, c->stream); }, &ms);
  std::vector<uint32_t> host(nt * 3);
  if (e == hipSuccess) e = toHost(host.data(), w.tileHit, nt * 3);  // tileFollowed and tileTruncated behind it
  std::vector<float4> ng((info && !out_n) ? np : 0);  // max_depth is read off Ng.w
  float* hn = out_n ? out_n : (ng.empty() ? nullptr : &ng[0].x);
  if (e == hipSuccess && hn) e = toHost(hn, w.n, np);
  if (e == hipSuccess && out_x) e = toHost(out_x, w.x, np);
  if (e != hipSuccess) return fail(c, SAIL_E_HIP, "sail_guides: %s", hipGetErrorString(e));
  setView(&c->guideView, mvp, eye);
  c->guideHave = true;
  if (info) {
    memset(info, 0, sizeof *info);
    info->hit_pixels = sumTiles(host, 0, nt);
    info->followed_pixels = sumTiles(host, nt, nt);
    info->truncated_pixels = sumTiles(host, 2 * nt, nt);
    info->depth = depth;
    for (size_t i = 0; i < np; i++) info->max_depth = std::max(info->max_depth, (int)hn[4 * i + 3]);
    info->kernel_ms = ms;
  }
  return SAIL_OK;
}

int sail_guides_load(sail_ctx* c, const float* n_map, const float* x_map, const double mvp[16], const float eye[3]) {
  if (!c) return SAIL_E_INVALID;
  if (!n_map || !x_map || !mvp || !eye) return fail(c, SAIL_E_INVALID, "sail_guides_load: n_map, x_map, mvp and eye are required");
  if (!c->subs.empty()) return relay(c, sail_guides_load(c->subs[0], n_map, x_map, mvp, eye), c->subs[0]);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensureGuides(c)) return rc;
  const GuideWork w = guideWork(c);
  c->guideHave = false;
  if (int rc = loadMap(c, w.n, n_map, pixels(c))) return rc;
  if (int rc = loadMap(c, w.x, x_map, pixels(c))) return rc;
  setView(&c->guideView, mvp, eye);
  c->guideHave = true;
  return SAIL_OK;
}

int sail_guides_read(sail_ctx* c, int which, float* out) {
  if (!c) return SAIL_E_INVALID;
  if (!out || which < SAIL_GUIDE_N || which > SAIL_GUIDE_X)
    return fail(c, SAIL_E_INVALID, "sail_guides_read: map %d of 0..1 and an output are required", which);
  if (!c->subs.empty()) return relay(c, sail_guides_read(c->subs[0], which, out), c->subs[0]);
  if (!c->guideHave || !c->guideMaps)
    return fail(c, SAIL_E_STATE, "sail_guides_read: no guide maps (sail_guides or sail_guides_load first; new rows drop them)");
  const GuideWork w = guideWork(c);
  return readMap(c, which == SAIL_GUIDE_X ? w.x : w.n, out, pixels(c));
}

int sail_use_guides(sail_ctx* c, int on) {
  if (on != 0 && on != 1) return fail(c, SAIL_E_INVALID, "sail_use_guides: on must be 0 or 1, not %d", on);
  if (!c) return fail(c, SAIL_E_INVALID, "sail_use_guides: a context is required");
  if (!c->subs.empty()) return relay(c, sail_use_guides(c->subs[0], on), c->subs[0]);
  c->useGuides = on != 0;
  return SAIL_OK;
}

}  // extern "C"
