// sail_converge.cpp — when to stop rendering: the noise estimate (sail_noise.hip), sail_render_until, the 64x64 tile mask
// and sail_render_adaptive. The context is sail_ctx.h's; sail_capi.cpp renders and resetAccum drops the mark and the mask.
#include <math.h>
#include <string.h>
#include <vector>
#include "sail_ctx.h"

void freeConverge(sail_ctx* c) {
  for (void* b : {(void*)c->noiseMark, (void*)c->noiseOut, (void*)c->noisePix, (void*)c->tileMap, (void*)c->maskBytes})
    if (b) (void)hipFree(b);
}

extern "C" {

// ---- noise estimate and render-until-converged (include/sail_hip.h; the kernel is sail_noise.hip) -------------------------
int sail_noise_mark(sail_ctx* c) {
  if (!c) return SAIL_E_INVALID;
  if (!c->subs.empty()) {  // device 0's reduced frame, like sail_filter
    if (int rc = reducedFrame(c, "sail_noise_mark")) return rc;
    return relay(c, sail_noise_mark(c->subs[0]), c->subs[0]);
  }
  if (c->accumMode == SAIL_ACCUM_COMPAT8)
    return fail(c, SAIL_E_STATE, "sail_noise_mark: SAIL_ACCUM_COMPAT8 stores 8-bit frames, whose halves cannot be compared");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = sail_sync(c)) return rc;
  const size_t bytes = (size_t)c->share.W * c->share.H * sizeof(float4);
  if (int rc = allocOnce(c, &c->noiseMark, bytes, "noise mark")) return rc;
  if (c->maskSet && c->noiseHave) {  // frozen tiles keep the mark they froze with
    SailNoiseArgs A;
    memset(&A, 0, sizeof A);
    A.S = shownAccum(c); A.P = c->noiseMark;
    A.W = c->share.W; A.H = c->share.H;
    A.active64 = c->maskBytes; A.tiles64X = (c->share.W + 63) / 64;
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
    if (int rc = reducedFrame(c, "sail_noise_estimate")) return rc;
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
  const int tx = (c->share.W + 15) / 16, ty = (c->share.H + 15) / 16;
  const size_t nt = (size_t)tx * ty, np = (size_t)c->share.W * c->share.H;
  if (int rc = allocOnce(c, &c->noiseOut, nt * 8, "noise tiles")) return rc;
  if (pixel_err)
    if (int rc = allocOnce(c, &c->noisePix, np * sizeof(float), "noise map")) return rc;
  SailNoiseArgs A;
  memset(&A, 0, sizeof A);
  A.S = shownAccum(c); A.P = c->noiseMark;
  A.tileSum = c->noiseOut; A.tileBad = (uint32_t*)(c->noiseOut + nt);
  A.pixErr = pixel_err ? c->noisePix : nullptr;
  A.W = c->share.W; A.H = c->share.H;
  A.mix = c->accumMode == SAIL_ACCUM_MIX;
  A.kf = (float)c->k; A.hf = (float)c->noiseK;
  A.remark = remark != 0;
  if (c->maskSet) { A.active64 = c->maskBytes; A.tiles64X = (c->share.W + 63) / 64; }
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
      const int w = c->share.W - i * 16 < 16 ? c->share.W - i * 16 : 16, h = c->share.H - j * 16 < 16 ? c->share.H - j * 16 : 16;
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
    if (int rc = sail_schedule(mvp, c->share.W, c->share.H, (int)*k, spp, inv.data(), seeds.data()))
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
  out->tiles_x = (c->share.W + 15) / 16; out->tiles_y = (c->share.H + 15) / 16;
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
  const int tx = (c->share.W + 63) / 64, ty = (c->share.H + 63) / 64, tiles = tx * ty;
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
  const int w = (c->share.partMode == SAIL_PART_SAMPLES) ? 1 : c->share.world, r = (c->share.partMode == SAIL_PART_SAMPLES) ? 0 : c->share.rank;
  std::vector<int32_t> table;
  long long px = 0;
  for (int t = r; t < tiles; t += w) {
    if (!m[(size_t)t]) continue;
    table.push_back(t);
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    const int cw = (c->share.W - x0) < 64 ? (c->share.W - x0) : 64, ch = (c->share.H - y0) < 64 ? (c->share.H - y0) : 64;
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
  const int tiles = ((c->share.W + 63) / 64) * ((c->share.H + 63) / 64);
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
  const int tx = (c->share.W + 63) / 64, ty = (c->share.H + 63) / 64, tiles = tx * ty;
  const int tx16 = (c->share.W + 15) / 16, ty16 = (c->share.H + 15) / 16;
  auto tilePixels = [&](int t) {
    const int x0 = (t % tx) * 64, y0 = (t / tx) * 64;
    return (uint64_t)((c->share.W - x0) < 64 ? (c->share.W - x0) : 64) * (uint64_t)((c->share.H - y0) < 64 ? (c->share.H - y0) : 64);
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
      if (int rc = sail_plan_adaptive(c->share.W, c->share.H, err16.data(), p.target, p.dilate, active.data(), active.data(), nullptr, &nActive))
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
  out->frame_pixel_samples = (uint64_t)c->share.W * (uint64_t)c->share.H * (k - k0);
  out->kernel_ms = st1.kernel_ms - st0.kernel_ms;
  if (tile_samples)
    for (int t = 0; t < tiles; t++)
      tile_samples[t] = (!h->maskSet || h->mask[(size_t)t]) ? (uint32_t)k : h->frozenAt[(size_t)t];
  if (looks) *looks = nlooks;
  return SAIL_OK;
}

}  // extern "C"
