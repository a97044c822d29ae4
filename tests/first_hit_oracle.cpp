// Test-side shim over the CPU parity oracle: the first hit's object row and surface colour for caller-supplied rays.
// Nothing the oracle exports returns Intersect::sc, and oracle/ does not change for a test, so this file includes the
// oracle's source and adds one entry point next to oracle_pick. Built on first use by tests/albedo_ref.py with
// oracle/build.sh's flags. Test infrastructure only.
#include "../oracle/sail_oracle.cpp"

// oracle_pick with the scene's own texture mask: index = the first row with the smallest d (-1 on a miss), sc = its surface
// colour (3 floats per ray, 0 on a miss)
extern "C" int oracle_first_hit(const float* objects, int n, const float* texparams, int tn, unsigned shape_mask,
                                unsigned tex_mask, const float* rays, int count, int* index, float* sc) {
  C.objects.d = objects; C.objects.w = 18; C.objects.h = n;
  C.texParams.d = texparams; C.texParams.w = 16; C.texParams.h = tn;
  C.n = n; C.tn = tn; C.shapeMask = shape_mask; C.texMask = tex_mask;
  for (int i = 0; i < count; i++) {
    const float* q = rays + 6 * i;
    const Intersect ins = intersectObjects(ray_(v3(F(q[0]), F(q[1]), F(q[2])), v3(F(q[3]), F(q[4]), F(q[5]))));
    const bool hit = ins.d < F(kMaxDistance);
    index[i] = hit ? ins.index : -1;
    sc[3 * i] = hit ? raw(ins.sc.x) : 0.0f;
    sc[3 * i + 1] = hit ? raw(ins.sc.y) : 0.0f;
    sc[3 * i + 2] = hit ? raw(ins.sc.z) : 0.0f;
  }
  return 0;
}
