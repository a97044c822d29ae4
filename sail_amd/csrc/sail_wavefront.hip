// sail_wavefront.hip — the wavefront split of the pre-cull path: sail_wf_primary, sail_wf_sweep, sail_wf_shade,
// sail_wf_shadow, sail_wf_accum and sail_launch_wavefront. It runs the trace kernels' own sweep, hit record and shading
// (sail_geom.h, sail_shade.h) and sail_trace.hip's tile index. No part of a run-time kernel's text.
#include <hip/hip_runtime.h>
#include "sail_trace.hip"

// ---- wavefront split of the pre-cull path (study switch SAIL_DEBUG_WAVEFRONT; DESIGN.md §9 of round 2) -------------------
// The megakernel keeps each path in registers and LDS across its bounces and sorts the workgroup's paths between the
// sweep and the shading. Here one sample of every owned pixel is traced bounce by bounce with the state in HBM and
// four kernels per bounce pass: the sweep, the hit record + shading (a lit matte path's shadow test deferred), the
// shadow sweep of the deferred tests with the radiance update they hold back, then (per sample) the accumulation.
// Each kernel runs with only its own live state. Same functions, same operations in the same order: bit-identical.
namespace {
struct WfPix { int x, y; bool valid; };
D WfPix wfPixel(const SailTraceArgs& A, long long slot) {
  const int ownedTile = (int)(slot >> 12), local = (int)(slot & 4095);
  WfPix q;
  q.x = q.y = 0;
  q.valid = false;
  if (ownedTile >= A.ownedTiles) return q;  // never past the tile table
  // (the study path selects at run time: its fifteen kernels per sample have no masked instances)
  const int tile = A.tileMap ? ownedTileIndex<true>(A, ownedTile) : ownedTileIndex<false>(A, ownedTile);
  q.x = (tile % A.tilesX) * 64 + (local & 63);
  q.y = (tile / A.tilesX) * 64 + (local >> 6);
  q.valid = q.x < A.W && q.y < A.H;
  return q;
}
D Ctx wfCtx(const SailTraceArgs& A) {
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
  c.cullPrims = 1;
  c.cullFma = A.cullPrims == 2;
  c.cullPrimary = A.cullPrimary;
  c.kShapes = ~0u; c.kMats = ~0u; c.kTex = ~0u; c.kLights = ~0u;
  return c;
}
}  // namespace
// primary rays of sample k
extern "C" __global__ void __launch_bounds__(256) sail_wf_primary(SailTraceArgs A, SailWfState S, int k) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  const WfPix q = wfPixel(A, slot);
  const SailSample& sm = constRow<SailSample>(A.samples, k);
  const float s = ((float)q.x + 0.5f) / (float)A.W, t = ((float)q.y + 0.5f) / (float)A.H;
  const V3 d0 = v3(sm.d[0][0], sm.d[0][1], sm.d[0][2]), d1 = v3(sm.d[1][0], sm.d[1][1], sm.d[1][2]);
  const V3 d2 = v3(sm.d[2][0], sm.d[2][1], sm.d[2][2]), d3 = v3(sm.d[3][0], sm.d[3][1], sm.d[3][2]);
  const V3 dir = (s + t <= 1.0f) ? (d0 + (d2 - d0) * s + (d1 - d0) * t) : (d3 + (d1 - d3) * (1.0f - s) + (d2 - d3) * (1.0f - t));
  S.o[slot] = make_float4(A.eye[0], A.eye[1], A.eye[2], q.valid ? 1.0f : 0.0f);
  S.d[slot] = make_float4(dir.x, dir.y, dir.z, 0.0f);
  S.f[slot] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  S.e[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// the closest-hit sweep of every live path
extern "C" __global__ void __launch_bounds__(256) sail_wf_sweep(SailTraceArgs A, SailWfState S, int k, int depth) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  const float4 o = S.o[slot];
  unsigned seg = 0;
  if (o.w != 0.0f) {
    const Ctx c = wfCtx(A);
    const float4 d = S.d[slot];
    const Ray ray = mkRay(v3(o.x, o.y, o.z), v3(d.x, d.y, d.z));
    const Sweep sw = sweepRay(c, ray, depth == 1);
    seg = 1;
    if (sw.best >= kMaxDistance) {  // the path leaves the scene
      S.o[slot] = make_float4(o.x, o.y, o.z, 0.0f);
      if (depth == 1 && (A.aovN || A.aovP) && k == A.spp - 1) {
        const WfPix q = wfPixel(A, slot);
        const size_t g = (size_t)q.y * A.W + q.x;
        const V3 qn = v3s(0.0f) / 2.0f + 0.5f, qp = normalize(v3s(0.0f));
        if (A.aovN) A.aovN[g] = make_float4(qn.x, qn.y, qn.z, 1.0f);
        if (A.aovP) A.aovP[g] = make_float4(qp.x, qp.y, qp.z, 1.0f);
      }
    } else {
      S.s[slot] = make_float4(sw.best, __int_as_float(sw.bi), 0.0f, 0.0f);
    }
  }
  if (A.segCounter) {
    unsigned long long v = seg;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&A.segCounter[(blockIdx.x * 4u + (threadIdx.x >> 6)) % SAIL_SEG_SLOTS], v);
  }
}
// hit record and shading of every live path; a lit matte path's shadow test and radiance update are deferred
extern "C" __global__ void __launch_bounds__(256) sail_wf_shade(SailTraceArgs A, SailWfState S, int k, int depth) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  const float4 o = S.o[slot];
  if (o.w == 0.0f) { S.sp[0][slot].w = 0.0f; return; }
  Ctx c = wfCtx(A);
  const WfPix q = wfPixel(A, slot);
  c.fcx = (float)q.x + 0.5f; c.fcy = (float)q.y + 0.5f;
  const float4 d = S.d[slot], fp = S.f[slot], ee = S.e[slot], sv = S.s[slot];
  Ray ray;
  ray.o = v3(o.x, o.y, o.z); ray.d = v3(d.x, d.y, d.z); ray.rx = ray.ry = ray.rz = 0.0f;
  Sweep sw;
  sw.best = sv.x; sw.bi = __float_as_int(sv.y); sw.bhl = v3s(0.0f);
  const Hit ins = hitRecord<true>(c, ray, sw);
  if (depth == 1 && (A.aovN || A.aovP) && k == A.spp - 1) {
    const size_t g = (size_t)q.y * A.W + q.x;
    const V3 qn = ins.normal / 2.0f + 0.5f, qp = normalize(ins.hit);
    if (A.aovN) A.aovN[g] = make_float4(qn.x, qn.y, qn.z, 1.0f);
    if (A.aovP) A.aovP[g] = make_float4(qp.x, qp.y, qp.z, 1.0f);
  }
  V3 fpdf = v3(fp.x, fp.y, fp.z), e = v3(ee.x, ee.y, ee.z);
  const float seed = constRow<SailSample>(A.samples, k).seed + (float)depth;
  PhaseClock pc;
  ShadowPending sp;
  shadeBounceP(c, ins, ray, seed, fpdf, e, pc, sp);
  S.e[slot] = make_float4(e.x, e.y, e.z, 0.0f);
  S.f[slot] = make_float4(fpdf.x, fpdf.y, fpdf.z, 0.0f);
  S.o[slot] = make_float4(ray.o.x, ray.o.y, ray.o.z, 1.0f);
  S.d[slot] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f);
  S.sp[0][slot] = make_float4(sp.hit.x, sp.hit.y, sp.hit.z, sp.pending ? 1.0f : 0.0f);
  if (sp.pending) {
    S.sp[1][slot] = make_float4(sp.toLight.x, sp.toLight.y, sp.toLight.z, 0.0f);
    S.sp[2][slot] = make_float4(sp.eLit.x, sp.eLit.y, sp.eLit.z, 0.0f);
  }
}
// the deferred shadow tests (testShadow, shader.light.js:24-31): the radiance holds the blocked outcome of the update,
// replaced by the unblocked one (ShadowPending.eLit) when the ray is not blocked
extern "C" __global__ void __launch_bounds__(256) sail_wf_shadow(SailTraceArgs A, SailWfState S) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  const float4 h = S.sp[0][slot];
  if (h.w == 0.0f) return;
  const Ctx c = wfCtx(A);
  const float4 tl = S.sp[1][slot], el = S.sp[2][slot];
  if (!testShadow(c, mkRay(v3(h.x, h.y, h.z), v3(tl.x, tl.y, tl.z)))) S.e[slot] = make_float4(el.x, el.y, el.z, 0.0f);
}
// sample k's radiance into the accumulator (sample order: one launch per sample)
extern "C" __global__ void __launch_bounds__(256) sail_wf_accum(SailTraceArgs A, SailWfState S, int k) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  const WfPix q = wfPixel(A, slot);
  if (!q.valid) return;
  const size_t pix = (size_t)q.y * A.W + q.x;
  float4 acc = A.accum[pix];
  const float4 ee = S.e[slot];
  accumulateSample(acc, v3(ee.x, ee.y, ee.z), constRow<SailSample>(A.samples, k), A.accumMode);
  A.accum[pix] = acc;
}
hipError_t sail_launch_wavefront(const SailTraceArgs& A, const SailWfState& S, hipStream_t s) {
  const unsigned blocks = (unsigned)A.ownedTiles * 16u;  // 4096 slots per owned tile, 256 per workgroup
  for (int k = 0; k < A.spp; k++) {
    hipLaunchKernelGGL(sail_wf_primary, dim3(blocks), dim3(256), 0, s, A, S, k);
    for (int depth = 1; depth <= A.maxBounces; depth++) {
      hipLaunchKernelGGL(sail_wf_sweep, dim3(blocks), dim3(256), 0, s, A, S, k, depth);
      hipLaunchKernelGGL(sail_wf_shade, dim3(blocks), dim3(256), 0, s, A, S, k, depth);
      hipLaunchKernelGGL(sail_wf_shadow, dim3(blocks), dim3(256), 0, s, A, S);
    }
    hipLaunchKernelGGL(sail_wf_accum, dim3(blocks), dim3(256), 0, s, A, S, k);
  }
  return hipGetLastError();
}

