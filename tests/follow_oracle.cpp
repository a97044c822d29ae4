// Test-side shim over the CPU parity oracle: the guide maps' walk (include/sail_hip.h, sail_guides). The oracle's trace()
// loop with the material's random pair fixed at (0.5, 0.5), no radiance, stopping at the first surface that scatters.
// Nothing the oracle exports takes the random pair as an argument, and oracle/ does not change for a test, so this file
// includes the oracle's source and adds one entry point that calls its own intersectObjects, mirror, glass,
// worldToLocal / localToWorld and AOV encoding. Built on first use by tests/guides_ref.py with oracle/build.sh's flags.
// Test infrastructure only.
#include <cmath>
#include "../oracle/sail_oracle.cpp"

// rays: count x 6, the G-buffer pass's. out_n / out_x: count x 4 as Ng / Xg. counts: hit, followed, truncated pixels.
extern "C" int oracle_follow(const float* objects, int n, const float* texparams, int tn, unsigned shape_mask,
                             unsigned mat_mask, unsigned tex_mask, const float* rays, int count, int max_depth,
                             float* out_n, float* out_x, unsigned long long* counts) {
  C.objects.d = objects; C.objects.w = 18; C.objects.h = n;
  C.texParams.d = texparams; C.texParams.w = 16; C.texParams.h = tn;
  C.n = n; C.tn = tn; C.shapeMask = shape_mask; C.matMask = mat_mask; C.texMask = tex_mask;
  counts[0] = counts[1] = counts[2] = 0;
  const V2 u = v2(F(0.5f), F(0.5f));
  for (int i = 0; i < count; i++) {
    const float* q = rays + 6 * i;
    Ray ray = ray_(v3(F(q[0]), F(q[1]), F(q[2])), v3(F(q[3]), F(q[4]), F(q[5])));
    V3 nn = BLACKv, pp = BLACKv;
    int depth = 0, id = -1;
    bool truncated = false;
    for (;;) {
      const Intersect ins = intersectObjects(ray);
      if (ins.d >= F(kMaxDistance)) break;  // path.glsl:22
      nn = ins.normal; pp = ins.hit; id = ins.index;
      const int cat = ins.matCategory;
      bool follow = false;
      if (cat >= 0 && cat < 32 && ((C.matMask >> cat) & 1u)) {  // material()'s plugin test
        if (cat == MIRROR) follow = true;
        else if (cat == GLASS)  // glass.glsl's isSpecular
          follow = readFloat(C.texParams, 4.0f, ins.matIndex, kTexLen) < F(kEps) &&
                   readFloat(C.texParams, 5.0f, ins.matIndex, kTexLen) < F(kEps);
      }
      if (!follow) break;
      if (depth == max_depth) { truncated = true; break; }
      // shade() (path.glsl:1-14) and trace()'s next ray (:33-36)
      const V3 ss = normalize(ins.dpdu), ts = cross(ins.normal, ss);
      const V3 wo = worldToLocal(-ray.dir, ins.normal, ss, ts);
      V3 wi = BLACKv;
      if (cat == MIRROR) (void)mirror(u, ins.matIndex, ins.sc, wo, wi, ins.into);
      else (void)glass(u, ins.matIndex, ins.sc, wo, wi, ins.into);
      wi = localToWorld(wi, ins.normal, ss, ts);
      const F outdot = dot(ins.normal, wi);
      ray.origin = ins.hit + ins.normal * (outdot > F(kEps) ? F(0.0001f) : F(-0.0001f));
      ray.dir = wi;
      depth += 1;
    }
    float* on = out_n + 4 * i;
    float* ox = out_x + 4 * i;
    if (id < 0) {
      on[0] = on[1] = on[2] = 0.5f; on[3] = 0.0f;
      ox[0] = ox[1] = ox[2] = NAN; ox[3] = -1.0f;
      continue;
    }
    const V3 qn = nn / F(2.0f) + F(0.5f), qp = normalize(pp);  // fstrace.glsl:15-16
    on[0] = raw(qn.x); on[1] = raw(qn.y); on[2] = raw(qn.z); on[3] = (float)depth;
    ox[0] = raw(qp.x); ox[1] = raw(qp.y); ox[2] = raw(qp.z); ox[3] = (float)id;
    counts[0] += 1;
    counts[1] += depth > 0;
    counts[2] += truncated;
  }
  return 0;
}
