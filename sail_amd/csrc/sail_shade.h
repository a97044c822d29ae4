// sail_shade.h — the shading of the trace kernels: the phase clock that shading and the path loop mark, the hash RNG
// and the samplers, sampleGeometry for area lights, Fresnel, microfacet and BSDF, the lights, shadeBounce / shadeLast
// with the deferred-shadow pieces, and the accumulation of one sample. Part of a run-time kernel's text
// (sail_amd/gen_jit_src.py): an edit here changes every run-time kernel's cache key.
#pragma once
#include "sail_geom.h"

namespace {

// ---- optional phase timing (-DSAIL_PHASE_TIMING=1: libsail_hip_phase.so, tools/phase_profile.py): per-wave
// s_memtime deltas per phase of the bounce, summed over the launch; the results are those of the plain build
#ifndef SAIL_PHASE_TIMING
#define SAIL_PHASE_TIMING 0
#endif
#if SAIL_PHASE_TIMING
struct PhaseClock { unsigned long long t, acc[12]; };
#define PHASE_MARK(pc, k) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); (pc).acc[k] += now_ - (pc).t; (pc).t = now_; } while (0)
#else
struct PhaseClock {};
#define PHASE_MARK(pc, k) do { (void)(pc); } while (0)
#endif
// the square root of the warps and BSDF terms whose argument is in [0, 1] by construction (sail_math.h sqrt01)
#define SQRT01(x) sqrt01(x)
// ---- random.glsl:5-18 ---------------------------------------------------------------------------------
D float hash1(const Ctx& c, float seed, float a, float b, float cc) {
  const V3 p = v3(c.fcx + seed, c.fcy + seed, 0.5f + seed);
  return fract_(sinf_(dot(p, v3(a, b, cc))) * 43758.5453f + seed);
}
D V2 random2(const Ctx& c, float seed) {
  return v2(hash1(c, seed, 12.9898f, 78.233f, 151.7182f), hash1(c, seed, 63.7264f, 10.873f, 623.6736f));
}

// ---- sampler.glsl ---------------------------------------------------------------------------------------
D V3 uniformSampleSphere(V2 u) {
  const float z = 1.0f - 2.0f * u.x;
  const float r = SQRT01(1.0f - z * z);
  const float angle = 2.0f * kPI * u.y;
  float s, co; sincosf_(angle, s, co);
  return v3(r * co, r * s, z);
}
D V3 cosineSampleHemisphere(V2 u) {
  const float r = SQRT01(u.x);
  const float angle = 2.0f * kPI * u.y;
  float s, co; sincosf_(angle, s, co);
  return v3(r * co, r * s, SQRT01(1.0f - u.x));
}
D V2 concentricSampleDisk(V2 u) {
  const float uOffset = 2.0f * u.x - 1.0f, vOffset = 2.0f * u.y - 1.0f;
  if (uOffset == 0.0f && vOffset == 0.0f) return v2(0.0f, 0.0f);
  float theta, r;
  if (fabsf(uOffset) > fabsf(vOffset)) { r = uOffset; theta = fdiv(vOffset, uOffset) * kPiOver4; }
  else { r = vOffset; theta = kPiOver2 - fdiv(uOffset, vOffset) * kPiOver4; }
  float s, co; sincosf_(theta, s, co);
  return r * v2(co, s);
}

// ---- sampleGeometry for area lights (shader.shape.js:53-67) -----------------------------------------------------
D V3 sampleGeometry(const Ctx& c, V2 u, int row, V3& normal, float& pdf) {
  normal = v3s(0.0f);
  pdf = 0.0f;
  const SailPrim& p = c.rowCopy ? c.cprims[row] : PRIM(c, row);
  const float s = sgn(p.rev);
  switch (p.type) {
    case SAIL_SPHERE: if (!HAS(c.kShapes, SAIL_SPHERE)) break; {
      const V3 q = uniformSampleSphere(u);
      const float rad = p.a[3];
      pdf = fdiv(kInvPI, rad * rad);
      const V3 res = q * rad + P3(p, 0);
      normal = s * (res - P3(p, 0)) / rad;
      return res;
    }
    case SAIL_RECTANGLE: if (!HAS(c.kShapes, SAIL_RECTANGLE)) break; {
      const V3 mn = P3(p, 0), mx = P3(p, 3);
      const V3 x = v3(mx.x - mn.x, 0.0f, 0.0f), y = v3(0.0f, mx.y - mn.y, mx.z - mn.z);
      pdf = p.a[17];                                   // 1 / (length(x) * length(y)), per scene
      const V3 res = mn + x * u.x + y * u.y;
      normal = s * P3(p, 6);                           // normalize(cross(x, y)) == the frame normal
      return res;
    }
    case SAIL_DISK: if (!HAS(c.kShapes, SAIL_DISK)) break; {
      const V2 pd = concentricSampleDisk(u);
      const V3 pp = P3(p, 0);
      const float rad = p.a[3], ri = p.a[4];
      const V3 res = v3(pd.x * rad + pp.x, pp.y, pd.y * rad + pp.z);
      const float area = 2.0f * kPI * 0.5f * (rad * rad - ri * ri);
      pdf = rcp_rn(area);
      normal = s * v3(0.0f, 1.0f, 0.0f);
      return res;
    }
    case SAIL_CUBE: if (HAS(c.kShapes, SAIL_CUBE)) normal = normalForCube(v3s(0.0f), p); return v3s(0.0f);
    case SAIL_CORNELLBOX: if (HAS(c.kShapes, SAIL_CORNELLBOX)) normal = normalForCornellbox(v3s(0.0f), p); return v3s(0.0f);
    case SAIL_CONE: {  // cone.glsl:38-46 at BLACK
      const V3 hit = v3s(0.0f) - P3(p, 0);
      const float h = p.a[3], rad = p.a[4];
      const float tana = fdiv(rad, h);
      const float dd = sqrtf_(hit.x * hit.x + hit.y * hit.y);
      const float x1 = fdiv(dd, tana), x2 = dd * tana;
      normal = s * normalize(hit - v3(0.0f, 0.0f, h - x1 - x2));
      return v3s(0.0f);
    }
    case SAIL_CYLINDER: if (!HAS(c.kShapes, SAIL_CYLINDER)) break; {
      const V3 pp = P3(p, 0);
      normal = s * normalize(v3(0.0f - pp.x, 0.0f - pp.y, 0.0f));
      return v3s(0.0f);
    }
    case SAIL_HYPERBOLOID: if (!HAS(c.kShapes, SAIL_HYPERBOLOID)) break; {
      const V3 hit = v3s(0.0f), p1 = P3(p, 3), p2 = P3(p, 6);
      const float v = fdiv(hit.z - p1.z, p2.z - p1.z);
      const V3 pr = (1.0f - v) * p1 + v * p2;
      const float phi = phiOf(pr.x * hit.y - hit.x * pr.y, hit.x * pr.x + hit.y * pr.y);
      V3 dpdu, dpdv;
      hypDpD(hit, p1, p2, phi, dpdu, dpdv);
      normal = s * L2W(normalize(cross(dpdu, dpdv)));
      return v3s(0.0f);
    }
    case SAIL_PARABOLOID: if (!HAS(c.kShapes, SAIL_PARABOLOID)) break; {
      const float zMin = fmin_(p.a[3], p.a[4]), zMax = fmax_(p.a[3], p.a[4]);
      V3 dpdu, dpdv;
      paraDpD(v3s(0.0f), zMax, zMin, dpdu, dpdv);
      normal = s * L2W(normalize(cross(dpdu, dpdv)));
      return v3s(0.0f);
    }
    default: break;
  }
  return v3s(0.0f);
}

// ---- ssutility.glsl / fresnel.glsl / microfacet.glsl / bsdf.glsl --------------------------------------------------
D float absCosTheta(V3 w) { return fabsf(w.z); }
D float sin2Theta(V3 w) { return fmax_(0.0f, 1.0f - w.z * w.z); }
D float sinTheta(V3 w) { return SQRT01(sin2Theta(w)); }
D float tan2Theta(V3 w) {
  const float cos2T = w.z * w.z;
  if (cos2T < kEps) return kInf;
  return fdiv(sin2Theta(w), cos2T);
}
D float cosPhi(V3 w) { const float st = sinTheta(w); return equalZero(st) ? 1.0f : clamp_(fdiv(w.x, st), -1.0f, 1.0f); }
D float sinPhi(V3 w) { const float st = sinTheta(w); return equalZero(st) ? 0.0f : clamp_(fdiv(w.y, st), -1.0f, 1.0f); }
D bool sameHemisphere(V3 w, V3 wp) { return w.z * wp.z > kEps; }

D float frDielectric(float cosThetaI, float etaI, float etaT) {
  cosThetaI = clamp_(cosThetaI, -1.0f, 1.0f);
  const float sinThetaI = SQRT01(fmax_(0.0f, 1.0f - cosThetaI * cosThetaI));
  const float sinThetaT = fdiv(etaI, etaT) * sinThetaI;
  if (sinThetaT >= 1.0f) return 1.0f;
  const float cosThetaT = SQRT01(fmax_(0.0f, 1.0f - sinThetaT * sinThetaT));
  const float TI = etaT * cosThetaI, IT = etaI * cosThetaT, II = etaI * cosThetaI, TT = etaT * cosThetaT;
  const float Rparl = fdiv(TI - IT, TI + IT), Rperp = fdiv(II - TT, II + TT);
  return fdiv(Rparl * Rparl + Rperp * Rperp, 2.0f);
}
D V3 frConductor(float cosThetaI, V3 etaI, V3 etaT, V3 k) {
  cosThetaI = clamp_(cosThetaI, -1.0f, 1.0f);
  const V3 eta = etaT / etaI, etak = k / etaI;
  const float cosThetaI2 = cosThetaI * cosThetaI, sinThetaI2 = 1.0f - cosThetaI2;
  const V3 eta2 = eta * eta, etak2 = etak * etak;
  const V3 t0 = eta2 - etak2 - sinThetaI2;
  const V3 s = t0 * t0 + 4.0f * eta2 * etak2;
  const V3 a2plusb2 = v3(sqrtf_(s.x), sqrtf_(s.y), sqrtf_(s.z));
  const V3 t1 = a2plusb2 + cosThetaI2;
  const V3 ah = 0.5f * (a2plusb2 + t0);
  const V3 a = v3(sqrtf_(ah.x), sqrtf_(ah.y), sqrtf_(ah.z));
  const V3 t2 = 2.0f * cosThetaI * a;
  const V3 Rs = (t1 - t2) / (t1 + t2);
  const V3 t3 = cosThetaI2 * a2plusb2 + v3s(sinThetaI2 * sinThetaI2);
  const V3 t4 = t2 * sinThetaI2;
  const V3 Rp = Rs * (t3 - t4) / (t3 + t4);
  return 0.5f * (Rp + Rs);
}
// Fresnel: type 0 noop (WHITE), 1 conductor(etaI=WHITE, eta, k), 2 dielectric(1, eta)
struct Fr { int type; V3 eta, k; float etaT; };
D V3 frEvaluate(const Fr& f, float cosThetaI) {
  if (f.type == 2) return v3s(1.0f) * frDielectric(cosThetaI, 1.0f, f.etaT);
  else if (f.type == 1) return frConductor(cosThetaI, v3s(1.0f), f.eta, f.k);
  return v3s(1.0f);
}
D V3 trSampleWh(V2 u, float ax, float ay, V3 wo) {  // microfacet.glsl:41-59
  float cosT = 0.0f, phi = 2.0f * kPI * u.x;
  float sp, cp;  // sin/cos of the final phi: the anisotropic branch has them already
  if (ax == ay) {
    const float tanTheta2 = fdiv(ax * ax * u.x, 1.0f - u.x);
    cosT = rcp_rn(sqrtf_(1.0f + tanTheta2));
    sincosf_(phi, sp, cp);
  } else {
    phi = atanf_(fdiv(ay, ax) * tanf_(kPiOver2 + 2.0f * kPI * u.x));
    if (u.x > 0.5f) phi += kPI;
    float sP, cP; sincosf_(phi, sP, cP);
    const float ax2 = ax * ax, ay2 = ay * ay;
    const float alpha2 = rcp_rn(fdiv(cP * cP, ax2) + fdiv(sP * sP, ay2));
    const float tanTheta2 = fdiv(alpha2 * u.x, 1.0f - u.x);
    cosT = rcp_rn(sqrtf_(1.0f + tanTheta2));
    sp = sP; cp = cP;
  }
  const float sinT = SQRT01(fmax_(0.0f, 1.0f - cosT * cosT));
  V3 wh = v3(sinT * cp, sinT * sp, cosT);
  if (!sameHemisphere(wo, wh)) wh = -wh;
  return wh;
}
D float trD(float ax, float ay, V3 wh) {  // microfacet.glsl:61-67
  const float t2 = tan2Theta(wh);
  if (t2 >= kInf) return 0.001f;
  const float c2 = wh.z * wh.z;
  const float cos4Theta = c2 * c2;
  const float cp = cosPhi(wh), sp = sinPhi(wh);
  const float e = (fdiv(cp * cp, ax * ax) + fdiv(sp * sp, ay * ay)) * t2;
  return rcp_rn(kPI * ax * ay * cos4Theta * (1.0f + e) * (1.0f + e));
}
D float trPdf(float ax, float ay, V3 wh) { return trD(ax, ay, wh) * absCosTheta(wh); }
D V3 microR_f(V3 R, const Fr& fr, float ax, float ay, V3 wo, V3 wi) {  // bsdf.glsl:168-178
  const float cosThetaO = absCosTheta(wo), cosThetaI = absCosTheta(wi);
  V3 wh = wi + wo;
  if (cosThetaI < kEps || cosThetaO < kEps) return v3s(0.0f);
  if (equalZero(wh.x) && equalZero(wh.y) && equalZero(wh.z)) return v3s(0.0f);
  wh = normalize(wh);
  const V3 F = frEvaluate(fr, dot(wi, wh));
  return R * trD(ax, ay, wh) * F / (4.0f * cosThetaI * cosThetaO);
}
D V3 microR_sample(V3 R, const Fr& fr, float ax, float ay, V2 u, V3 wo, V3& wi, float& pdf) {  // :186-196
  if (wo.z < kEps) return v3s(0.0f);
  const V3 wh = trSampleWh(u, ax, ay, wo);
  wi = reflect_(-wo, wh);
  if (!sameHemisphere(wo, wi)) return v3s(0.0f);
  pdf = fdiv(trPdf(ax, ay, wh), 4.0f * dot(wo, wh));
  return microR_f(R, fr, ax, ay, wo, wi);
}
D V3 microT_f(V3 T, float etaB, bool into, float ax, float ay, V3 wo, V3 wi) {  // :205-224 (etaA = 1)
  if (sameHemisphere(wo, wi)) return v3s(0.0f);
  const float cosThetaO = wo.z, cosThetaI = wi.z;
  if (equalZero(cosThetaI) || equalZero(cosThetaO)) return v3s(0.0f);
  const float eta = into ? fdiv(etaB, 1.0f) : rcp_rn(etaB);
  V3 wh = normalize(wo + wi * eta);
  if (wh.z < -kEps) wh = -wh;
  const float Fd = frDielectric(dot(wo, wh), 1.0f, etaB);
  const float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
  return (1.0f - Fd) * T *
         fabsf(fdiv(eta * eta * trD(ax, ay, wh) * fabsf(dot(wi, wh)) * fabsf(dot(wo, wh)),
                    cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
}
D float microT_pdf(float etaB, bool into, float ax, float ay, V3 wo, V3 wi) {  // :226-235
  if (sameHemisphere(wo, wi)) return 0.001f;
  const float eta = into ? fdiv(etaB, 1.0f) : rcp_rn(etaB);
  const V3 wh = normalize(wo + wi * eta);
  const float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
  const float dwh_dwi = fabsf(fdiv(eta * eta * dot(wi, wh), sqrtDenom * sqrtDenom));
  return trPdf(ax, ay, wh) * dwh_dwi;
}
D V3 microT_sample(V3 T, float etaB, bool into, float ax, float ay, V2 u, V3 wo, V3& wi, float& pdf) {
  if (equalZero(wo.z)) return v3s(0.0f);
  const V3 wh = trSampleWh(u, ax, ay, wo);
  const float eta = into ? rcp_rn(etaB) : fdiv(etaB, 1.0f);
  wi = refract_(-wo, wh, eta);
  pdf = microT_pdf(etaB, into, ax, ay, wo, wi);
  return microT_f(T, etaB, into, ax, ay, wo, wi);
}
D V3 orenNayar_f(V3 R, float A, float B, V3 wo, V3 wi) {  // bsdf.glsl:45-66
  const float sinThetaI = sinTheta(wi), sinThetaO = sinTheta(wo);
  float maxCos = 0.0f;
  if (sinThetaI > kEps && sinThetaO > kEps) {
    const float sinPhiI = sinPhi(wi), cosPhiI = cosPhi(wi), sinPhiO = sinPhi(wo), cosPhiO = cosPhi(wo);
    const float dCos = cosPhiI * cosPhiO + sinPhiI * sinPhiO;
    maxCos = fmax_(0.0f, dCos);
  }
  float sinAlpha, tanBeta;
  if (absCosTheta(wi) > absCosTheta(wo)) { sinAlpha = sinThetaO; tanBeta = fdiv(sinThetaI, absCosTheta(wi)); }
  else { sinAlpha = sinThetaI; tanBeta = fdiv(sinThetaO, absCosTheta(wo)); }
  return R * kInvPI * (A + B * maxCos * sinAlpha * tanBeta);
}

// material() (shader.material.js:21-29): returns fpdf; f only for MATTE (the only consumer, path.glsl:10-11)
D V3 material(const Ctx& c, const Hit& ins, V2 u, V3 wo, V3& wi, V3& f) {
  f = v3s(0.0f);
  wi = v3s(0.0f);
  const int cat = ins.matCategory;
  if (cat < 0 || cat >= 32 || !((c.matMask >> cat) & 1u)) return v3s(0.0f);
  const int m = ins.matRow;
  const V3 sc = ins.sc;
  float pdf = 0.0f;
  V3 fs = v3s(0.0f);
  switch (cat) {
    case SAIL_MATTE: if (!HAS(c.kMats, SAIL_MATTE)) break; {  // matte.glsl:8-37
      const float kd = TP(c, m, 1), sigma = TP(c, m, 2), A = TP(c, m, 3), B = TP(c, m, 4);
      const V3 R = kd * sc;
      wi = cosineSampleHemisphere(u);
      pdf = sameHemisphere(wo, wi) ? absCosTheta(wi) * kInvPI : 0.0f;
      if (sigma < kEps) { fs = R * kInvPI; f = (kd * sc) * kInvPI; }
      else { fs = orenNayar_f(R, A, B, wo, wi); f = orenNayar_f(kd * sc, A, B, wo, wi); }
      break;
    }
    case SAIL_MIRROR: if (!HAS(c.kMats, SAIL_MIRROR)) break; {  // mirror.glsl:5-17, specular_r_sample_f bsdf.glsl:93-98
      const float kr = TP(c, m, 1);
      const V3 R = kr * sc;
      wi = v3(-wo.x, -wo.y, wo.z);
      pdf = 1.0f;
      fs = v3s(1.0f) * R / absCosTheta(wi);
      break;
    }
    case SAIL_METAL: if (!HAS(c.kMats, SAIL_METAL)) break; {  // metal.glsl:8-22
      Fr fr; fr.type = 1; fr.eta = TP3(c, m, 3); fr.k = TP3(c, m, 6); fr.etaT = 0.0f;
      fs = microR_sample(sc, fr, TP(c, m, 1), TP(c, m, 2), u, wo, wi, pdf);
      break;
    }
    case SAIL_GLASS: if (!HAS(c.kMats, SAIL_GLASS)) break; {  // glass.glsl:10-36
      const float kr = TP(c, m, 1), kt = TP(c, m, 2), eta = TP(c, m, 3), ur = TP(c, m, 4), vr = TP(c, m, 5);
      if (ur < kEps && vr < kEps) {  // specular_fr_sample_f bsdf.glsl:141-158
        const float Fd = frDielectric(wo.z, 1.0f, eta);
        if (u.x < Fd) {
          wi = v3(-wo.x, -wo.y, wo.z);
          pdf = 1.0f;
          fs = (kr * sc) / absCosTheta(wi);
        } else {
          const float etaI = ins.into ? 1.0f : eta, etaT = ins.into ? eta : 1.0f;
          wi = refract_(-wo, v3(0.0f, 0.0f, 1.0f), fdiv(etaI, etaT));
          const V3 ft = (kt * sc) * (1.0f - Fd);
          pdf = 1.0f;
          fs = ft / absCosTheta(wi);
        }
      } else {
        const float p = u.x;
        V2 uu = u;
        uu.x = fmin_(u.x * 2.0f - 1.0f, kOneMinusEps);
        if (p < 0.5f) {
          Fr fr; fr.type = 2; fr.etaT = eta; fr.eta = v3s(0.0f); fr.k = v3s(0.0f);
          fs = microR_sample(kr * sc, fr, ur, vr, uu, wo, wi, pdf);
        } else {
          fs = microT_sample(kt * sc, eta, ins.into, ur, vr, uu, wo, wi, pdf);
        }
      }
      break;
    }
    default: break;
  }
  return fs * absCosTheta(wi) / pdf;
}

// ---- lights (shader.light.js:12-22, light/*.glsl) ---------------------------------------------------------------
// (one uniformSampleSphere shared by point lights and sphere area lights was bit-identical and C4 -0.35 %,
// profiles/r03_variants_light_shared.jsonl: the extra light-row read cost more than the second evaluation)
D bool testShadow(const Ctx& c, const Ray& r) {
  const float d = closestT(c, r);
  return d > kEps && d < kOneMinusEps;
}
// The light categories only differ in how they build the shadow ray and the unoccluded contribution; the
// shadow sweep itself (the expensive part) is shared, so a wave whose lanes picked different light kinds
// runs one sweep instead of one per kind. Contribution and visibility are independent pure functions of the
// same inputs, so evaluating the contribution first changes no bit.
// lightPrep: everything of light_sample but its shadow test -- whether the sample is lit, its unoccluded
// contribution and the shadow ray (from the hit point along the unnormalised toLight)
struct LightPrep { bool lit; V3 contrib, toLight; };
D LightPrep lightPrep(const Ctx& c, const Hit& ins, V2 u2) {
  LightPrep lp;
  lp.lit = false; lp.contrib = v3s(0.0f); lp.toLight = v3s(0.0f);
  // randomInt(seed,0,ln) = int(random2(seed).x * ln): the same hash as the BSDF sample's first component
  if (c.kLights == 0) return lp;                              // no light plugin compiled in
  const int index = to_int(u2.x * (float)c.ln);
  if (c.ln <= 0) return lp;
  const int catRow = (index <= 0) ? 0 : c.ln - 1;           // readInt(lights, vec2(0, index)) : integer row coord
  const int cat = to_int(c.lt[catRow * 18]);
  if (cat < 0 || cat >= 32 || !((c.lightMask >> cat) & 1u)) return lp;
  const int row = (c.ln == 1) ? 0 : (index < 0 ? 0 : (index > c.ln - 1 ? c.ln - 1 : index));
  const float* L = c.lt + row * 18;
  V3 contrib = v3s(0.0f), toLight = v3s(0.0f);
  bool lit = false;
  if (cat == SAIL_AREA && HAS(c.kLights, SAIL_AREA)) {  // light/area.glsl
    const V3 em = v3(L[2], L[3], L[4]);
    V3 normal; float pdf;
    const V3 p = sampleGeometry(c, u2, c.lightObjRow[row], normal, pdf);
    toLight = p - ins.hit;
    const V3 nt = normalize(toLight);
    contrib = em * fmax_(0.0f, dot(normal, -nt)) * fmax_(0.0f, dot(nt, ins.normal)) / pdf;
    lit = true;
  } else if (cat == SAIL_POINT && HAS(c.kLights, SAIL_POINT)) {  // light/point.glsl:13-20
    const V3 from = v3(L[1], L[2], L[3]), em = v3(L[4], L[5], L[6]);
    const V3 p = from + uniformSampleSphere(u2) * 0.1f;
    toLight = p - ins.hit;
    contrib = em * fmax_(0.0f, dot(normalize(toLight), ins.normal));
    lit = true;
  } else if (cat == SAIL_SPOT && HAS(c.kLights, SAIL_SPOT)) {  // light/spot.glsl
    const float ctw = L[1], cfs = L[2];
    const V3 from = v3(L[3], L[4], L[5]), em = v3(L[6], L[7], L[8]);
    toLight = from - ins.hit;
    const V3 nt = normalize(toLight);
    const float d = length(toLight);
    float fall;
    {  // falloff spot.glsl:17-27 with w = -normToLight
      const float cT = -(-nt).y;
      if (cT < ctw) fall = 0.0f;
      else if (cT >= cfs) fall = 1.0f;
      else { const float delta = fdiv(cT - ctw, cfs - ctw); const float d2 = delta * delta; fall = d2 * d2; }
    }
    contrib = em * fall * fmax_(0.0f, dot(normalize(toLight), ins.normal)) / (d * d);
    lit = true;
  }
  lp.lit = lit; lp.contrib = contrib; lp.toLight = toLight;
  return lp;
}
// Dead shadow tests: a light sample whose unoccluded contribution is exactly +0 in every channel (the sample behind
// the surface or the light facing away, a spot light's falloff 0) returns that +0 vector whether or not its shadow
// ray is blocked, so the shadow sweep is skipped; any other value (-0, NaN, a nonzero channel) takes the sweep
D bool posZero3(const V3& v) {
  return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z)) == 0u;
}
D V3 lightSample(const Ctx& c, const Hit& ins, V2 u2) {
  const LightPrep lp = lightPrep(c, ins, u2);
  if (!lp.lit) return v3s(0.0f);
  if (posZero3(lp.contrib)) return v3s(0.0f);
  // testShadow(Ray(hit, toLight)) (shader.light.js:24-31): unnormalised direction, no origin offset
  if (testShadow(c, mkRay(ins.hit, lp.toLight))) return v3s(0.0f);
  return lp.contrib;
}

// The path's final bounce: only its radiance is read afterwards (the throughput and the next ray are dead), so the
// BSDF sample is needed there only for f -- the light term's weight, which a matte surface alone sets -- and a
// Lambertian matte f (kd * sc / pi, matte.glsl) does not depend on the sample. shadeLast adds that bounce's
// radiance without the shading frame, BSDF sample or next ray, by the same expression on the same values as
// shadeBounce; it declines (false) for an Oren-Nayar matte, whose f needs the sampled direction, and for any matte
// path when a light plugin is compiled in (its light sample and shadow sweep stay in shadeBounce alone: a second
// inlined shadow sweep multiplied the pre-cull kernel's spills).
// Measured bit-identical: C2 +4.2 %, C3 +2.6 %, C4 -0.6 % (its 12-bounce paths are mostly matte with lights, which
// decline), so every kernel but the pre-cull one takes it.
D bool shadeLast(const Ctx& c, const Hit& ins, float seed, const V3& fpdf, V3& e) {
  const bool matteLit = isBlack(ins.emission) && ins.matCategory == SAIL_MATTE;  // path.glsl:10-11
  if (matteLit && c.kLights != 0) return false;
  V3 f = v3s(0.0f);
  // material()'s matte branch (the plugin in the scene and compiled in)
  if (matteLit && ((c.matMask >> SAIL_MATTE) & 1u) && HAS(c.kMats, SAIL_MATTE)) {
    const float kd = TP(c, ins.matRow, 1), sigma = TP(c, ins.matRow, 2);
    if (!(sigma < kEps)) return false;
    f = (kd * ins.sc) * kInvPI;
  }
  (void)seed;
  V3 direct = v3s(0.0f);
  if (matteLit)  // no light plugin: lightSample is 0, and 0 + 0 * f == fma(f, 0, 0) bit for bit
    direct = v3(fma_(f.x, 0.0f, 0.0f), fma_(f.y, 0.0f, 0.0f), fma_(f.z, 0.0f, 0.0f));
  const V3 sh = ins.emission + direct;
  e = e + sh * fpdf;
  return true;
}

// ---- path.glsl:1-38 ------------------------------------------------------------------------------------------------
// shade() (path.glsl:1-14) + the bounce bookkeeping of trace() (path.glsl:27-36): radiance, throughput, next ray
// A lit matte path's light sample whose shadow test is left to a later pass (the wavefront split, SAIL_DEBUG_WAVEFRONT):
// everything the radiance update e += (emission + light * f) * fpdf needs once the shadow ray's answer is known
// e holds the dark outcome of the radiance update (the light blocked); eLit the unblocked one, to be taken when the
// shadow ray from `hit` along `toLight` is not blocked. Both are shadeBounce's e += (emission + (0 + light * f)) * fpdf.
struct ShadowPending { bool pending; V3 toLight, hit, eLit; };
// DEFER: a lit matte path's shadow ray is handed to onShadow(hit, toLight, eLit) where it is made (so that nothing of it
// stays live through the rest of the bounce) and e takes the blocked outcome
// R: what the path carries, a Seg or a Ray (PathRay, sail_geom.h); the bounce ends with nextRay
template <bool DEFER, class R, class OnShadow>
D void shadeBounceT(const Ctx& c, const Hit& ins, R& ray, float seed, V3& fpdf, V3& e, PhaseClock& pc, OnShadow&& onShadow);
template <class R>
D void shadeBounce(const Ctx& c, const Hit& ins, R& ray, float seed, V3& fpdf, V3& e, PhaseClock& pc) {
  shadeBounceT<false>(c, ins, ray, seed, fpdf, e, pc, [](const V3&, const V3&, const V3&) {});
}
// the deferred shadow ray into a ShadowPending (the pre-cull kernel's compacted shadow rays, the wavefront split)
template <class R>
D void shadeBounceP(const Ctx& c, const Hit& ins, R& ray, float seed, V3& fpdf, V3& e, PhaseClock& pc, ShadowPending& sp) {
  sp.pending = false;
  shadeBounceT<true>(c, ins, ray, seed, fpdf, e, pc, [&](const V3& hit, const V3& toLight, const V3& eLit) {
    sp.pending = true; sp.hit = hit; sp.toLight = toLight; sp.eLit = eLit;
  });
}
template <bool DEFER, class R, class OnShadow>
D void shadeBounceT(const Ctx& c, const Hit& ins, R& ray, float seed, V3& fpdf, V3& e, PhaseClock& pc, OnShadow&& onShadow) {
  {
    // shade()
    // box faces have axis-aligned unit dpdu: dot == 1 exactly, sqrt(1) == 1 and v / 1 == v bit for bit
    // worldToLocal(-ray.d, normal, ss, ts): its z is dot(-d, +-n) = -+(n.d) exactly (negated products, symmetric
    // rounding), already known from the hit record's into test
    const V3 nd3 = -ray.d;
    V3 ss, ts, wo;
    if (ins.axis) {  // box face: unit dpdu (ss = dpdu, as below), exact products
      ss = ins.dpdu;
      ts = crossX(ins.normal, ss);
      wo = v3(dotX(nd3, ss), dotX(nd3, ts), ins.into ? -ins.nd : ins.nd);
    } else {
      const float dd = dot(ins.dpdu, ins.dpdu);
      ss = (dd == 1.0f) ? ins.dpdu : ins.dpdu / sqrtf_(dd);
      ts = cross(ins.normal, ss);
      wo = v3(dot(nd3, ss), dot(nd3, ts), ins.into ? -ins.nd : ins.nd);
    }
    // the hash is evaluated only for materials that consume it (matte/metal/glass; mirror is deterministic)
    PHASE_MARK(pc, 2);  // shading frame
    const V2 u2 = (ins.matCategory != SAIL_MIRROR) ? random2(c, seed) : v2(0.0f, 0.0f);
    PHASE_MARK(pc, 3);  // hash RNG
    V3 wiL, f;
    const V3 mat = material(c, ins, u2, wo, wiL, f);
    const V3 _fpdf = vclamp01(mat);
    const V3 wi = ins.axis ? localToWorldX(wiL, ins.normal, ss, ts) : localToWorld(wiL, ins.normal, ss, ts);
    PHASE_MARK(pc, 4);  // BSDF sample
    V3 direct = v3s(0.0f);
    if (isBlack(ins.emission) && ins.matCategory == SAIL_MATTE) {
      if (c.kLights == 0) {  // no light plugin: lightSample is 0, and 0 + 0 * f == fma(f, 0, 0) bit for bit
        direct = v3(fma_(f.x, 0.0f, 0.0f), fma_(f.y, 0.0f, 0.0f), fma_(f.z, 0.0f, 0.0f));
      } else if (DEFER) {  // lightSample's light prep now; its shadow test later picks one of the two outcomes
        const LightPrep lp = lightPrep(c, ins, u2);
        if (lp.lit && !posZero3(lp.contrib)) {
          V3 dLit = v3s(0.0f);
          dLit = dLit + lp.contrib * f;
          onShadow(ins.hit, lp.toLight, e + (ins.emission + dLit) * fpdf);
        }
        direct = direct + v3s(0.0f) * f;  // the dark outcome (light 0), or no shadow ray at all
      } else {
        direct = direct + lightSample(c, ins, u2) * f;
      }
    }
    PHASE_MARK(pc, 5);  // light sample + shadow ray
    {
      const V3 sh = ins.emission + direct;
      e = e + sh * fpdf;
    }
    fpdf = fpdf * _fpdf;
    const float outdot = ins.axis ? dotX(ins.normal, wi) : dot(ins.normal, wi);
    nextRay(ray, ins.hit + ins.normal * (outdot > kEps ? 0.0001f : -0.0001f), wi);
    PHASE_MARK(pc, 6);  // next ray
  }
}

D float q8(float v) {
  v = clamp_(v, 0.0f, 1.0f);
  return floorf(v * 255.0f + 0.5f) / 255.0f;
}
// fstrace.glsl:13 accumulation of one sample (SUM: running sums + count; MIX / COMPAT8: the reference's
// mix(e, cache, k/(k+1)), COMPAT8 through the UNORM8 frame store)
D void accumulateSample(float4& acc, V3 e, const SailSample& S, int mode) {
  if (mode == 0) {
    acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += 1.0f;
  } else {
    const float w = S.mixw;
    float mx = e.x * (1.0f - w) + acc.x * w, my = e.y * (1.0f - w) + acc.y * w, mz = e.z * (1.0f - w) + acc.z * w;
    if (mode == 2) { mx = q8(mx); my = q8(my); mz = q8(mz); }
    acc.x = mx; acc.y = my; acc.z = mz; acc.w = 1.0f;
  }
}

}  // namespace
