// sail_frame.hip — the kernels that work on whole frames around the trace kernels, each with its launch wrapper: the
// staged-sample accumulation (sail_accum_kernel), the multi-device sum and the -0 fill of unowned tiles, the display
// filter (sail_filter_kernel: the reference's display pass, main/fsrender.glsl + filter/window.glsl:26-44,
// tonemapping.glsl, gamma.glsl, color.glsl), the picker, the spec-math probe and the phase-timing readout. They use the
// trace kernels' vector types and accumulateSample (sail_geom.h, sail_shade.h), the view passes' first-hit sweep
// (sail_view.h: the picker; included here, never from sail_trace.hip) and sail_trace.hip's tile index
// and g_sailPhase. No part of a run-time kernel's text: an edit here leaves the run-time kernels' cache keys alone.
#include <hip/hip_runtime.h>
#include "sail_trace.hip"
#include "sail_view.h"

// ---- sample groups: add the staged per-sample radiance to the accumulator in sample order ---------------------
namespace {
template <bool MASKED>
D void accumStaged(const SailTraceArgs& A) {
  const int bid = (int)blockIdx.x;
  const int ownedTile = bid >> 4, sub = bid & 15;
  const int tile = ownedTileIndex<MASKED>(A, ownedTile);
  const int tx = tile % A.tilesX, ty = tile / A.tilesX;
  const int li = threadIdx.x;
  const int x = tx * 64 + (sub & 3) * 16 + (li & 15), y = ty * 64 + (sub >> 2) * 16 + (li >> 4);
  if (x >= A.W || y >= A.H) return;
  const size_t pix = (size_t)y * A.W + x;
  float4 acc = A.accum[pix];  // holds the first group's samples already (SAIL_GROUP_HOME)
  const float* st = A.stage + (long long)bid * 256 + li;
  const size_t ss = (size_t)A.stageStride;
  int k = A.groupHome ? A.groupSpp : 0;
  // eight samples' planes loaded ahead of their in-order additions (the pass is HBM-bound: keep loads in flight;
  // 0.189 -> 0.180 ms per C2 launch)
  for (; k + 8 <= A.spp; k += 8) {
    float v[8][3];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float* q = st + (size_t)(k + j) * 3u * ss;
      v[j][0] = q[0]; v[j][1] = q[ss]; v[j][2] = q[2 * ss];
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
      accumulateSample(acc, v3(v[j][0], v[j][1], v[j][2]), constRow<SailSample>(A.samples, k + j), A.accumMode);
  }
  for (; k < A.spp; k++) {
    const float* q = st + (size_t)k * 3u * ss;
    accumulateSample(acc, v3(q[0], q[ss], q[2 * ss]), constRow<SailSample>(A.samples, k), A.accumMode);
  }
  A.accum[pix] = acc;
}
}  // namespace
extern "C" __global__ void __launch_bounds__(256) sail_accum_kernel(SailTraceArgs A) { accumStaged<false>(A); }
extern "C" __global__ void __launch_bounds__(256) sail_accum_kernel_masked(SailTraceArgs A) { accumStaged<true>(A); }

// ---- multi-device frame reduction without RCCL (a multi-device context whose devices are all one GPU) ----------
// dst = ((src0 + src1) + src2) + ...: the sum of the ranks' frames in rank order
extern "C" __global__ void __launch_bounds__(256) sail_sum_kernel(SailSumArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  float4 v = A.src[0][i];
  for (int k = 1; k < A.nsrc; k++) {
    const float4 w = A.src[k][i];
    v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
  }
  A.dst[i] = v;
}
// AOV maps of a tile-partitioned rank hold -0 outside its tiles: x + (-0) == x for every x (+0, -0 and NaN
// included), so the sum over ranks reproduces the owning rank's AOV bits exactly (a +0 fill would turn -0 into +0)
extern "C" __global__ void __launch_bounds__(256) sail_negzero_unowned_kernel(float4* a, float4* b, int W, int H,
                                                                             int rank, int world) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const int tilesX = (W + 63) / 64;
  const int tile = (y >> 6) * tilesX + (x >> 6);
  if (tile % world == rank) return;
  const float4 nz = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
  const size_t pix = (size_t)y * W + x;
  if (a) a[pix] = nz;
  if (b) b[pix] = nz;
}

// ---- display filter (fsrender.glsl + filter/*.glsl), W x H generalisation of the 512 x 512 pass ---------------------
// Every map is sampled as the reference's frame textures are: LINEAR, default REPEAT wrap (webgl.js:153-156),
// RGB (texture() returns alpha 1). The colour map is the mean image (SUM accumulators divided per texel).
namespace {
D int wrapi(int i, int size) { int m = i % size; return m < 0 ? m + size : m; }
struct Tap { int xa, xb, ya, yb; float a, b; };
D Tap tapAt(int W, int H, float u, float v) {
  const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  Tap t;
  t.a = fx - x0f; t.b = fy - y0f;
  const int xi = (int)x0f, yi = (int)y0f;
  t.xa = wrapi(xi, W); t.xb = wrapi(xi + 1, W); t.ya = wrapi(yi, H); t.yb = wrapi(yi + 1, H);
  return t;
}
D V3 texel(const SailFilterArgs& A, const float4* img, bool mean, int x, int y) {
  const float4 v = img[(size_t)y * A.W + x];
  if (mean && A.accumMode == 0) {  // each texel's own count (a reduced tile frame may mix counts; 0: unrendered)
    const float cnt = v.w > 0.0f ? v.w : 1.0f;
    return v3(v.x / cnt, v.y / cnt, v.z / cnt);
  }
  return v3(v.x, v.y, v.z);
}
D V3 bilerp(V3 t00, V3 t10, V3 t01, V3 t11, float a, float b) {
  const V3 c0 = t00 * (1.0f - a) + t10 * a, c1 = t01 * (1.0f - a) + t11 * a;
  return c0 * (1.0f - b) + c1 * b;
}
D V3 sample(const SailFilterArgs& A, const float4* img, bool mean, float u, float v) {
  const Tap t = tapAt(A.W, A.H, u, v);
  return bilerp(texel(A, img, mean, t.xa, t.ya), texel(A, img, mean, t.xb, t.ya), texel(A, img, mean, t.xa, t.yb),
                texel(A, img, mean, t.xb, t.yb), t.a, t.b);
}
D float dot4(V3 t, float w) { return t.x * t.x + t.y * t.y + t.z * t.z + w * w; }
// window filters: the workgroup's 16x16 pixels plus a halo of mean texels staged in LDS once (one divide per
// texel instead of one per tap read); taps that would leave the tile read global memory as before
constexpr int kFiltMaxT = 32;
struct FiltTile { const float* r; const float* g; const float* b; int x0, y0, T; };
D V3 sampleTile(const SailFilterArgs& A, const FiltTile& tl, float u, float v) {
  const float fx = u * (float)A.W - 0.5f, fy = v * (float)A.H - 0.5f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float a = fx - x0f, b = fy - y0f;
  const int lx = (int)x0f - tl.x0, ly = (int)y0f - tl.y0;
  if (lx < 0 || ly < 0 || lx + 1 >= tl.T || ly + 1 >= tl.T) return sample(A, A.accum, true, u, v);
  const int i00 = ly * tl.T + lx, i01 = i00 + tl.T;
  return bilerp(v3(tl.r[i00], tl.g[i00], tl.b[i00]), v3(tl.r[i00 + 1], tl.g[i00 + 1], tl.b[i00 + 1]),
                v3(tl.r[i01], tl.g[i01], tl.b[i01]), v3(tl.r[i01 + 1], tl.g[i01 + 1], tl.b[i01 + 1]), a, b);
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) sail_filter_kernel(SailFilterArgs A) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  __shared__ float sTR[kFiltMaxT * kFiltMaxT], sTG[kFiltMaxT * kFiltMaxT], sTB[kFiltMaxT * kFiltMaxT];
  FiltTile tl;
  tl.r = sTR; tl.g = sTG; tl.b = sTB;
  tl.T = 16 + 2 * A.halo;
  tl.x0 = (int)blockIdx.x * 16 - A.halo; tl.y0 = (int)blockIdx.y * 16 - A.halo;
  if (A.kind == 3 && A.halo > 0) {  // uniform over the grid
    for (int i = threadIdx.x; i < tl.T * tl.T; i += 256) {
      const int ly = i / tl.T, lx = i - ly * tl.T;
      const V3 m = texel(A, A.accum, true, wrapi(tl.x0 + lx, A.W), wrapi(tl.y0 + ly, A.H));  // REPEAT wrap
      sTR[i] = m.x; sTG[i] = m.y; sTB[i] = m.z;
    }
    __syncthreads();
  }
  if (x >= A.W || y >= A.H) return;
  const float tcx = ((float)x + 0.5f) / (float)A.W, tcy = ((float)y + 0.5f) / (float)A.H;
  float o[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  if (A.kind <= 2) {  // color.glsl / gamma.glsl / tonemapping.glsl
    const V3 cv = sample(A, A.accum, true, tcx, tcy);
    const float col[3] = {cv.x, cv.y, cv.z};
    for (int c = 0; c < 3; c++) {
      if (A.kind == 0) o[c] = col[c];
      else if (A.kind == 1) o[c] = powf_(col[c], rcp_rn(A.gammaC));
      else {
        const float xx = fmax_(0.0f, col[c] - 0.004f);
        o[c] = fdiv(xx * (6.2f * xx + 0.5f), xx * (6.2f * xx + 1.7f) + 0.06f);
      }
    }
  } else if (A.kind == 3) {  // window.glsl:1-44, FILTER_WINDOW_WIDTH 4
    V3 acc = v3s(0.0f);
    float weightSum = 0.0f;
    for (int i = 0; i < 4; i++) {
      for (int j = 0; j < 4; j++) {
        const float wi = fdiv(((float)j + 0.5f) * A.rx, 4.0f), wj = fdiv(((float)i + 0.5f) * A.ry, 4.0f);
        const float ox = fdiv(wi, (float)A.W), oy = fdiv(wj, (float)A.H);
        V3 tmp = v3s(0.0f);
        int count = 0;
        for (int q = 0; q < 4; q++) {
          const float u = (q < 2) ? tcx + ox : tcx - ox;
          const float v = (q & 1) ? tcy - oy : tcy + oy;
          if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) continue;
          count++;
          tmp = tmp + (A.halo > 0 ? sampleTile(A, tl, u, v) : sample(A, A.accum, true, u, v));
        }
        const float weight = A.weights[i * j + j];
        weightSum += weight * (float)count;
        acc = acc + tmp * weight;
      }
    }
    o[0] = fdiv(acc.x, weightSum); o[1] = fdiv(acc.y, weightSum); o[2] = fdiv(acc.z, weightSum);
  } else if (A.kind == 4) {  // wavelet.glsl:5-54 (edge-avoiding a-trous over the colour and position maps)
    const V3 cval = sample(A, A.accum, true, tcx, tcy);
    const V3 pval = sample(A, A.aovP, false, tcx, tcy);
    // the reference reads normalMap (nval, ntmp) but never uses it: its "normal" weight reuses the colour
    // difference (wavelet.glsl:11-12)
    const float hk[5] = {0.375f, 0.25f, 0.0625f, 0.0625f, 0.25f};
    const float dW = (float)A.W, dH = (float)A.H, dW2 = dW * 2.5f, dH2 = dH * 2.5f;  // 512, 1280 at 512^2
    float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float weightSum = 0.0f;
    for (int n = 0; n < 3; n++) {
      const float stepwidth = powf_(2.0f, (float)n) - 1.0f;
      const int div = to_int(stepwidth) + 1;
      int count = 0;
      for (int i = 0; i < 5; i++) {
        for (int j = 0; j < 5; j++, count++) {
          const int delt = abs(count - 12);
          float h = 0.0f;
          if (delt % div == 0) h = hk[(delt / div) % 5];
          if (h == 0.0f) continue;
          const float u = (tcx - fdiv(A.rx, dW)) + fdiv(((float)j + 0.5f) * A.rx, dW2);
          const float v = (tcy - fdiv(A.ry, dH)) + fdiv(((float)i + 0.5f) * A.ry, dH2);
          const V3 ctmp = sample(A, A.accum, true, u, v);
          const V3 t = cval - ctmp;
          const float tw = 1.0f - 1.0f;
          const float c_w = fmin_(expf_(fdiv(-(dot4(t, tw)), 4.0f)), 1.0f);
          const float d2 = fmax_(fdiv(dot4(t, tw), stepwidth * stepwidth), 0.0f);
          const float n_w = fmin_(expf_(fdiv(-(d2), 128.0f)), 1.0f);
          const V3 tp = pval - sample(A, A.aovP, false, u, v);
          const float p_w = fmin_(expf_(fdiv(-(dot4(tp, tw)), 1.0f)), 1.0f);
          const float weight = c_w * n_w * p_w * h;
          weightSum += weight;
          col[0] += ctmp.x * weight; col[1] += ctmp.y * weight; col[2] += ctmp.z * weight; col[3] += 1.0f * weight;
        }
      }
    }
    for (int c = 0; c < 4; c++) o[c] = fdiv(col[c], weightSum);
  } else {  // normal.glsl / position.glsl: the AOV map at the texel
    const V3 m = sample(A, A.kind == 5 ? A.aovN : A.aovP, false, tcx, tcy);
    o[0] = m.x; o[1] = m.y; o[2] = m.z;
  }
  const size_t pix = (size_t)y * A.W + x;
  if (A.out) A.out[pix] = make_float4(o[0], o[1], o[2], o[3]);
  if (A.out8) {
    for (int c = 0; c < 3; c++) A.out8[4 * pix + c] = (uint8_t)(int)(clamp_(o[c], 0.0f, 1.0f) * 255.0f + 0.5f);
    A.out8[4 * pix + 3] = 255;
  }
}

// ---- picking (replaces the CPU picker, src/core/pickup.js:46-66): the view passes' first-hit sweep (sail_view.h)
// for caller-supplied rays; index = the first object row with the smallest distance, -1 on a miss ---------------
extern "C" __global__ void __launch_bounds__(64) sail_pick_kernel(const SailPrim* prims, int n, const float* rays,
                                                                   int count, int32_t* index, float* tOut) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float* q = rays + 6 * (size_t)i;
  const Ray r = mkRay(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]));
  const Sweep sw = sv::firstHit(sv::flatCtx(prims, n, nullptr, 0, 0u, 0u, 0u), prims, n, r);
  index[i] = sw.bi;
  tOut[i] = sw.best;
}

// ---- spec-math probe for the CPU/GPU bit-parity test ----------------------------------------------------------------
extern "C" __global__ void sail_math_kernel(int fn, const float* x, const float* y, float* out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float r = 0.0f;
  switch (fn) {
    case 0: r = sinf_(x[i]); break;
    case 1: r = cosf_(x[i]); break;
    case 2: r = tanf_(x[i]); break;
    case 3: r = atan2f_(y[i], x[i]); break;
    case 4: r = acosf_(x[i]); break;
    case 5: r = powf_(x[i], y[i]); break;
    case 6: r = atanf_(x[i]); break;
    case 7: r = sqrtf_(x[i]); break;
    case 8: r = x[i] / y[i]; break;
    case 9: r = fmin_(x[i], y[i]); break;
    case 10: r = fmax_(x[i], y[i]); break;
    case 11: r = fdiv(x[i], y[i]); break;  // GLSL divide spec
    case 14: r = rcp_rn(x[i]); break;
    case 15: r = sqrt01(x[i]); break;  // callers guarantee [0, 1] or NaN
    case 12: r = clamp_(x[i], 0.0f, 1.0f); break;
    case 13: r = expf_(x[i]); break;
    case 16: r = __int_as_float(to_int(x[i])); break;  // the int's 32 bits, compared as such
    case 17: r = fract_(x[i]); break;
    case 18: r = clamp_(x[i], -1.0f, 1.0f); break;
    default: break;
  }
  out[i] = r;
}

// 1 in the phase-timing build: its run-time kernels are compiled instrumented too (sail_jit.cpp defsFor)
extern const int sail_trace_phase_timing = SAIL_PHASE_TIMING;
#if SAIL_PHASE_TIMING
int sail_jit_phase_read(unsigned long long out[12], int reset);  // sail_jit.cpp: the loaded run-time modules' sums
// phase-timing readout (tools/phase_profile.py): the precompiled kernels' sums plus every loaded run-time module's
extern "C" int sail_phase_read(unsigned long long out[12], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sailPhase), 12 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_sailPhase), z, sizeof z) != hipSuccess) return -1;
  }
  return sail_jit_phase_read(out, reset);
}
#endif

// ---- host launch wrappers (called by sail_capi.cpp and sail_multi.cpp) -----------------------------------------------
hipError_t sail_launch_accum(const SailTraceArgs& A, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(A.tileMap ? sail_accum_kernel_masked : sail_accum_kernel, dim3(blocks), dim3(256), 0, s, A);
  return hipGetLastError();
}
hipError_t sail_launch_sum(const SailSumArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_sum_kernel, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, s, A);
  return hipGetLastError();
}
hipError_t sail_launch_negzero_unowned(float4* a, float4* b, int W, int H, int rank, int world, hipStream_t s) {
  hipLaunchKernelGGL(sail_negzero_unowned_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, a, b, W, H,
                     rank, world);
  return hipGetLastError();
}
hipError_t sail_launch_filter(const SailFilterArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(sail_filter_kernel, dim3((A.W + 15) / 16, (A.H + 15) / 16), dim3(256), 0, s, A);
  return hipGetLastError();
}
hipError_t sail_launch_pick(const SailPrim* prims, int n, const float* rays, int count, int32_t* index, float* t,
                            hipStream_t s) {
  hipLaunchKernelGGL(sail_pick_kernel, dim3((count + 63) / 64), dim3(64), 0, s, prims, n, rays, count, index, t);
  return hipGetLastError();
}
hipError_t sail_launch_math(int fn, const float* x, const float* y, float* out, int count) {
  hipLaunchKernelGGL(sail_math_kernel, dim3((count + 255) / 256), dim3(256), 0, 0, fn, x, y, out, count);
  return hipGetLastError();
}
