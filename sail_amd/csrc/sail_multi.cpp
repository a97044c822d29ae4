// sail_multi.cpp — more than one GPU: the RCCL binding, sail_reduce and the multi-device context's reduce into device 0,
// and the checkpoint parts (sail_save_accum / sail_load_accum) with their host-only plans. The context is sail_ctx.h's.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "sail_ctx.h"

Rccl g_rccl;

namespace {

constexpr int kNcclFloat32 = 7, kNcclSum = 0;

// ---- reduced frame (sail_reduce, multi-device contexts) -----------------------------------------------------------
int ensureFrame(sail_ctx* c) {
  const size_t bytes = (size_t)c->share.W * c->share.H * sizeof(float4);
  float4** bufs[3] = {&c->frame, c->aovN ? &c->frameN : nullptr, c->aovP ? &c->frameP : nullptr};
  for (float4** b : bufs) {
    if (!b) continue;
    if (int rc = allocOnce(c, b, bytes, "reduced frame")) return rc;
  }
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
  const bool tiles = g->share.partMode == SAIL_PART_TILES;
  const size_t np = (size_t)g->share.W * g->share.H, bytes = np * sizeof(float4);
  // every device's share of the exchange (sail_plan_reduce: device i = rank i of nd, root 0)
  std::vector<sail_reduce_plan> plan((size_t)nd);
  for (int i = 0; i < nd; i++) plan[i] = planReduce(g->share.W, g->share.H, i, nd, g->share.partMode, r->k, 0);
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

// What every read of a multi-device context starts with: device 0's sub-context then shows the reduced frame.
// (sail_reduce keeps its own form: it sets `dirty` first.)
int reducedFrame(sail_ctx* g, const char* what) {
  if (int rc = loadIncomplete(g, what)) return rc;
  return groupReduce(g);
}

void freeMulti(sail_ctx* c) {
  for (void* b : {(void*)c->frame, (void*)c->frameN, (void*)c->frameP}) if (b) (void)hipFree(b);
}

extern "C" {

int sail_accum_device_ptr(sail_ctx* c, void** ptr, size_t* bytes) {
  if (!c || !ptr || !bytes) return SAIL_E_INVALID;
  if (!c->subs.empty()) return relay(c, sail_accum_device_ptr(c->subs[0], ptr, bytes), c->subs[0]);
  if (int rc = flushQueued(c)) return rc;  // the sums the caller's collective will read are queued on this stream
  *ptr = c->accum;
  *bytes = (size_t)c->share.W * c->share.H * sizeof(float4);
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
  const bool own = planReduce(c->share.W, c->share.H, c->share.rank, c->share.world, c->share.partMode, c->k, root).send_own_aovs != 0;
  if (isRoot || (aov && !own)) { if (int rc = ensureFrame(c)) return rc; }
  const size_t np = (size_t)c->share.W * c->share.H, count = np * 4;
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
  HIPCHK(c, hipMemcpy(sums, c->accum, (size_t)c->share.W * c->share.H * sizeof(float4), hipMemcpyDeviceToHost));
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
  if (part == -1 && c->share.world > 1 && c->share.partMode == SAIL_PART_SAMPLES && c->accumMode != SAIL_ACCUM_SUM)
    return fail(c, SAIL_E_INVALID, "sail_load_accum: a running mean cannot be split by samples");
  HIPCHK(c, hipSetDevice(c->device));
  const bool marked = c->noiseHave;
  if (int rc = resetAccum(c)) return rc;  // queued samples, stats and AOVs restart; the accumulator is replaced
  c->noiseHave = marked;  // a loaded checkpoint continues a render: the noise estimate's mark stays
  std::vector<float> mine;
  const float* src = sums;
  if (part == -1 && c->share.world > 1) {
    mine.resize((size_t)c->share.W * c->share.H * 4);
    keepPart(c->share.W, c->share.H, c->share.rank, c->share.world, c->share.partMode, sums, mine.data());
    src = mine.data();
  }
  HIPCHK(c, hipMemcpyAsync(c->accum, src, (size_t)c->share.W * c->share.H * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->k = k;
  // this rank's samples among 0 .. k-1 (every one, or those k' = rank mod world of a sample split)
  c->samplesThisRank = planReduce(c->share.W, c->share.H, c->share.rank, c->share.world, c->share.partMode, k, 0).samples;
  return SAIL_OK;
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

}  // extern "C"
