// sail_napi.cc — Node-API binding of libsail_hip.so (include/sail_hip.h) for the JavaScript host.
// Built against the Node headers of this image (/usr/include/node, N-API 8); links libsail_hip.so with
// an $ORIGIN rpath. Every failing C call becomes a thrown JS Error carrying sail_last_error().
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../../include/sail_hip.h"

namespace {

struct Handle {
  sail_ctx* ctx;
  int W, H;
};

#define NAPI_OK(call)                                              \
  do {                                                             \
    if ((call) != napi_ok) {                                       \
      napi_throw_error(env, nullptr, "N-API call failed: " #call); \
      return nullptr;                                              \
    }                                                              \
  } while (0)

napi_value throwSail(napi_env env, const char* what, int rc, const sail_ctx* c) {
  std::string msg = std::string(what) + " failed (" + std::to_string(rc) + "): " + sail_last_error(c);
  napi_throw_error(env, nullptr, msg.c_str());
  return nullptr;
}

bool args(napi_env env, napi_callback_info info, size_t n, napi_value* out) {
  size_t argc = n;
  if (napi_get_cb_info(env, info, &argc, out, nullptr, nullptr) != napi_ok) return false;
  if (argc < n) {
    napi_throw_type_error(env, nullptr, "not enough arguments");
    return false;
  }
  return true;
}
// at least n arguments, up to cap: those not passed are undefined
bool argsUpTo(napi_env env, napi_callback_info info, size_t n, size_t cap, napi_value* out) {
  size_t argc = cap;
  if (napi_get_cb_info(env, info, &argc, out, nullptr, nullptr) != napi_ok) return false;
  if (argc < n) {
    napi_throw_type_error(env, nullptr, "not enough arguments");
    return false;
  }
  return true;
}
bool getInt(napi_env env, napi_value v, int* out) {
  if (napi_get_value_int32(env, v, out) != napi_ok) { napi_throw_type_error(env, nullptr, "expected a number"); return false; }
  return true;
}
bool getDouble(napi_env env, napi_value v, double* out) {
  if (napi_get_value_double(env, v, out) != napi_ok) { napi_throw_type_error(env, nullptr, "expected a number"); return false; }
  return true;
}
// typed-array view (nullptr for null/undefined when allowed)
template <typename T>
bool getArray(napi_env env, napi_value v, napi_typedarray_type want, T** data, size_t* len, bool nullable = false) {
  napi_valuetype vt;
  napi_typeof(env, v, &vt);
  if (nullable && (vt == napi_null || vt == napi_undefined)) { *data = nullptr; *len = 0; return true; }
  bool is = false;
  napi_is_typedarray(env, v, &is);
  if (!is) { napi_throw_type_error(env, nullptr, "expected a typed array"); return false; }
  napi_typedarray_type t;
  void* p = nullptr;
  napi_value ab;
  size_t off = 0;
  napi_get_typedarray_info(env, v, &t, len, &p, &ab, &off);
  if (t != want) { napi_throw_type_error(env, nullptr, "typed array has the wrong element type"); return false; }
  *data = static_cast<T*>(p);
  return true;
}
bool getHandle(napi_env env, napi_value v, Handle** h) {
  void* p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !static_cast<Handle*>(p)->ctx) {
    napi_throw_error(env, nullptr, "invalid or destroyed renderer context");
    return false;
  }
  *h = static_cast<Handle*>(p);
  return true;
}
napi_value makeF32(napi_env env, const float* src, size_t n) {
  void* data = nullptr;
  napi_value ab, arr;
  napi_create_arraybuffer(env, n * sizeof(float), &data, &ab);
  if (src) memcpy(data, src, n * sizeof(float));
  napi_create_typedarray(env, napi_float32_array, n, ab, 0, &arr);
  return arr;
}
napi_value makeTyped(napi_env env, napi_typedarray_type t, size_t n, size_t elem, void** data) {
  napi_value ab, arr;
  napi_create_arraybuffer(env, n * elem, data, &ab);
  napi_create_typedarray(env, t, n, ab, 0, &arr);
  return arr;
}
napi_value num(napi_env env, double v) { napi_value r; napi_create_double(env, v, &r); return r; }
napi_value undef(napi_env env) { napi_value r; napi_get_undefined(env, &r); return r; }

void finalizeHandle(napi_env, void* data, void*) {
  Handle* h = static_cast<Handle*>(data);
  if (h->ctx) sail_destroy(h->ctx);
  delete h;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
  int n = 0;
  sail_device_count(&n);
  return num(env, n);
}
napi_value AbiVersion(napi_env env, napi_callback_info) { return num(env, sail_abi_version()); }

napi_value Create(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  int w, h, dev, flags;
  if (!getInt(env, a[0], &w) || !getInt(env, a[1], &h) || !getInt(env, a[2], &dev) || !getInt(env, a[3], &flags)) return nullptr;
  sail_ctx* c = nullptr;
  const int rc = sail_create(&c, w, h, dev, (uint32_t)flags);
  if (rc) return throwSail(env, "sail_create", rc, nullptr);
  Handle* hd = new Handle{c, w, h};
  napi_value ext;
  NAPI_OK(napi_create_external(env, hd, finalizeHandle, nullptr, &ext));
  return ext;
}
// (W, H, Int32Array devices, flags): one context over several GPUs (sail_create_multi)
napi_value CreateMulti(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  int w, h, flags;
  int32_t* dev;
  size_t nd;
  if (!getInt(env, a[0], &w) || !getInt(env, a[1], &h) || !getArray(env, a[2], napi_int32_array, &dev, &nd) ||
      !getInt(env, a[3], &flags))
    return nullptr;
  sail_ctx* c = nullptr;
  const int rc = sail_create_multi(&c, w, h, dev, (int)nd, (uint32_t)flags);
  if (rc) return throwSail(env, "sail_create_multi", rc, nullptr);
  Handle* hd = new Handle{c, w, h};
  napi_value ext;
  NAPI_OK(napi_create_external(env, hd, finalizeHandle, nullptr, &ext));
  return ext;
}
napi_value Destroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  void* p = nullptr;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    Handle* h = static_cast<Handle*>(p);
    if (h->ctx) { sail_destroy(h->ctx); h->ctx = nullptr; }
  }
  return undef(env);
}
napi_value SetScene(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!args(env, info, 8, a)) return nullptr;
  Handle* h;
  float *o, *t, *l;
  size_t no, nt, nl;
  int n, tn, ln;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &o, &no) || !getInt(env, a[2], &n) ||
      !getArray(env, a[3], napi_float32_array, &t, &nt) || !getInt(env, a[4], &tn) ||
      !getArray(env, a[5], napi_float32_array, &l, &nl) || !getInt(env, a[6], &ln))
    return nullptr;
  if (no < (size_t)n * 18 || nt < (size_t)tn * 16 || nl < (size_t)ln * 18) {
    napi_throw_range_error(env, nullptr, "scene rows shorter than n/tn/ln");
    return nullptr;
  }
  uint32_t m[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < 4; i++) {
    napi_value e;
    NAPI_OK(napi_get_element(env, a[7], i, &e));
    NAPI_OK(napi_get_value_uint32(env, e, &m[i]));
  }
  sail_plugins pl{m[0], m[1], m[2], m[3]};
  const int rc = sail_set_scene(h->ctx, o, n, t, tn, l, ln, &pl);
  if (rc) return throwSail(env, "sail_set_scene", rc, h->ctx);
  return undef(env);
}
napi_value UpdateObjects(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!args(env, info, 3, a)) return nullptr;
  Handle* h;
  float* o;
  size_t no;
  int n;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &o, &no) || !getInt(env, a[2], &n)) return nullptr;
  if (no < (size_t)n * 18) { napi_throw_range_error(env, nullptr, "object rows shorter than n"); return nullptr; }
  const int rc = sail_update_objects(h->ctx, o, n);
  if (rc) return throwSail(env, "sail_update_objects", rc, h->ctx);
  return undef(env);
}
// moveObjects(ctx, objects, n, motion | null, histCap): sail_move_objects
napi_value MoveObjects(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  float *o, *m = nullptr;
  size_t no, nm = 0;
  int n;
  double cap = 0.0;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &o, &no) || !getInt(env, a[2], &n)) return nullptr;
  if (!getArray(env, a[3], napi_float32_array, &m, &nm, true)) return nullptr;
  NAPI_OK(napi_get_value_double(env, a[4], &cap));
  if (n < 0 || no < (size_t)n * 18 || (m && nm < (size_t)n * 3)) {
    napi_throw_range_error(env, nullptr, "object rows or motion shorter than n");
    return nullptr;
  }
  const int rc = sail_move_objects(h->ctx, o, n, m, (float)cap);
  if (rc) return throwSail(env, "sail_move_objects", rc, h->ctx);
  return undef(env);
}
napi_value IntSetter(napi_env env, napi_callback_info info, int nargs, const char* name,
                     int (*fn3)(sail_ctx*, int, int, int), int (*fn1)(sail_ctx*, int)) {
  napi_value a[4];
  if (!args(env, info, nargs + 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  int v[3] = {0, 0, 0};
  for (int i = 0; i < nargs; i++) if (!getInt(env, a[1 + i], &v[i])) return nullptr;
  const int rc = fn3 ? fn3(h->ctx, v[0], v[1], v[2]) : fn1(h->ctx, v[0]);
  if (rc) return throwSail(env, name, rc, h->ctx);
  return undef(env);
}
napi_value SetAccumMode(napi_env env, napi_callback_info info) { return IntSetter(env, info, 1, "sail_set_accum_mode", nullptr, sail_set_accum_mode); }
napi_value SetLaunchSamples(napi_env env, napi_callback_info info) { return IntSetter(env, info, 1, "sail_set_launch_samples", nullptr, sail_set_launch_samples); }
napi_value SetPartition(napi_env env, napi_callback_info info) { return IntSetter(env, info, 3, "sail_set_partition", sail_set_partition, nullptr); }
int setDebug3(sail_ctx* c, int opt, int val, int) { return sail_set_debug(c, opt, val); }
napi_value SetDebug(napi_env env, napi_callback_info info) { return IntSetter(env, info, 2, "sail_set_debug", setDebug3, nullptr); }
int reduce3(sail_ctx* c, int root, int, int) { return sail_reduce(c, root); }
napi_value Reduce(napi_env env, napi_callback_info info) { return IntSetter(env, info, 1, "sail_reduce", reduce3, nullptr); }

napi_value Render(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  float *inv, *eye;
  size_t ni, ne;
  double seed;
  int b;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &inv, &ni) ||
      !getArray(env, a[2], napi_float32_array, &eye, &ne) || !getDouble(env, a[3], &seed) || !getInt(env, a[4], &b))
    return nullptr;
  if (ni < 16 || ne < 3) { napi_throw_range_error(env, nullptr, "inv_mvp needs 16 and eye 3 floats"); return nullptr; }
  const int rc = sail_render(h->ctx, inv, eye, (float)seed, b);
  if (rc) return throwSail(env, "sail_render", rc, h->ctx);
  return undef(env);
}
napi_value RenderSchedule(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  float *inv, *seeds, *eye;
  size_t ni, ns, ne;
  int b;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &inv, &ni) ||
      !getArray(env, a[2], napi_float32_array, &seeds, &ns) || !getArray(env, a[3], napi_float32_array, &eye, &ne) ||
      !getInt(env, a[4], &b))
    return nullptr;
  if (ni < ns * 16 || ne < 3) { napi_throw_range_error(env, nullptr, "schedule arrays too short"); return nullptr; }
  const int rc = sail_render_schedule(h->ctx, inv, seeds, eye, (int)ns, b);
  if (rc) return throwSail(env, "sail_render_schedule", rc, h->ctx);
  return undef(env);
}
napi_value Simple(napi_env env, napi_callback_info info, int (*fn)(sail_ctx*), const char* name) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  const int rc = fn(h->ctx);
  if (rc) return throwSail(env, name, rc, h->ctx);
  return undef(env);
}
napi_value Reset(napi_env env, napi_callback_info info) { return Simple(env, info, sail_reset, "sail_reset"); }
napi_value Sync(napi_env env, napi_callback_info info) { return Simple(env, info, sail_sync, "sail_sync"); }

napi_value Readback(napi_env env, napi_callback_info info) {  // (ctx, wantAov) -> {rgba, normal?, position?}
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  bool aov = false;
  napi_get_value_bool(env, a[1], &aov);
  const size_t np = (size_t)h->W * h->H * 4;
  void *pr = nullptr, *pn = nullptr, *pp = nullptr;
  napi_value rgba = makeTyped(env, napi_float32_array, np, 4, &pr);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "rgba", rgba));
  if (aov) {
    napi_value nn = makeTyped(env, napi_float32_array, np, 4, &pn), ppv = makeTyped(env, napi_float32_array, np, 4, &pp);
    NAPI_OK(napi_set_named_property(env, out, "normal", nn));
    NAPI_OK(napi_set_named_property(env, out, "position", ppv));
  }
  const int rc = sail_readback(h->ctx, (float*)pr, (float*)pn, (float*)pp);
  if (rc) return throwSail(env, "sail_readback", rc, h->ctx);
  return out;
}
napi_value ReadAccum(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  void* p = nullptr;
  napi_value arr = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &p);
  const int rc = sail_read_accum(h->ctx, (float*)p);
  if (rc) return throwSail(env, "sail_read_accum", rc, h->ctx);
  return arr;
}
// checkpoint / resume (sail_accum_parts, sail_save_accum, sail_load_accum)
napi_value SaveAccum(napi_env env, napi_callback_info info) {  // (ctx) -> {k, parts: [Float32Array]}
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  int parts = 0;
  int rc = sail_accum_parts(h->ctx, &parts);
  if (rc) return throwSail(env, "sail_accum_parts", rc, h->ctx);
  napi_value list, out;
  NAPI_OK(napi_create_array_with_length(env, (size_t)parts, &list));
  uint64_t k = 0;
  for (int i = 0; i < parts; i++) {
    void* p = nullptr;
    napi_value arr = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &p);
    rc = sail_save_accum(h->ctx, i, (float*)p, &k);
    if (rc) return throwSail(env, "sail_save_accum", rc, h->ctx);
    napi_set_element(env, list, (uint32_t)i, arr);
  }
  NAPI_OK(napi_create_object(env, &out));
  napi_set_named_property(env, out, "k", num(env, (double)k));
  napi_set_named_property(env, out, "parts", list);
  return out;
}
napi_value LoadAccum(napi_env env, napi_callback_info info) {  // (ctx, part, Float32Array sums, k)
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  Handle* h;
  int part;
  float* sums;
  size_t n;
  double k;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &part) || !getArray(env, a[2], napi_float32_array, &sums, &n) ||
      !getDouble(env, a[3], &k))
    return nullptr;
  if (n != (size_t)h->W * h->H * 4) { napi_throw_range_error(env, nullptr, "accumulator has the wrong size"); return nullptr; }
  if (!(k >= 0.0 && k <= 9007199254740992.0) || k != (double)(uint64_t)k) {
    napi_throw_range_error(env, nullptr, "sample index must be a non-negative integer");
    return nullptr;
  }
  const int rc = sail_load_accum(h->ctx, part, sums, (uint64_t)k);
  if (rc) return throwSail(env, "sail_load_accum", rc, h->ctx);
  return undef(env);
}
napi_value Filter(napi_env env, napi_callback_info info) {  // (ctx, kind, weights|null, rx, ry, gamma) -> {rgba, rgba8}
  napi_value a[6];
  if (!args(env, info, 6, a)) return nullptr;
  Handle* h;
  int kind;
  float* w;
  size_t nw;
  double rx, ry, g;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &kind) || !getArray(env, a[2], napi_float32_array, &w, &nw, true) ||
      !getDouble(env, a[3], &rx) || !getDouble(env, a[4], &ry) || !getDouble(env, a[5], &g))
    return nullptr;
  if (w && nw < 16) { napi_throw_range_error(env, nullptr, "window weights need 16 floats"); return nullptr; }
  const size_t np = (size_t)h->W * h->H * 4;
  void *pf = nullptr, *p8 = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, np, 4, &pf), u8 = makeTyped(env, napi_uint8_array, np, 1, &p8);
  const int rc = sail_filter(h->ctx, kind, w, (float)rx, (float)ry, (float)g, (float*)pf, (uint8_t*)p8);
  if (rc) return throwSail(env, "sail_filter", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "rgba", f));
  NAPI_OK(napi_set_named_property(env, out, "rgba8", u8));
  return out;
}
napi_value Pick(napi_env env, napi_callback_info info) {  // (ctx, Float32Array rays[6*count]) -> {index, t}
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  float* rays;
  size_t nr;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &rays, &nr)) return nullptr;
  if (nr % 6) { napi_throw_range_error(env, nullptr, "rays need 6 floats each"); return nullptr; }
  const size_t count = nr / 6;
  void *pi = nullptr, *pt = nullptr;
  napi_value idx = makeTyped(env, napi_int32_array, count, 4, &pi), t = makeTyped(env, napi_float32_array, count, 4, &pt);
  const int rc = sail_pick(h->ctx, rays, (int)count, (int32_t*)pi, (float*)pt);
  if (rc) return throwSail(env, "sail_pick", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "index", idx));
  NAPI_OK(napi_set_named_property(env, out, "t", t));
  return out;
}
napi_value Stats(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  sail_stats s;
  const int rc = sail_get_stats(h->ctx, &s);
  if (rc) return throwSail(env, "sail_get_stats", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  napi_set_named_property(env, out, "samples", num(env, (double)s.samples));
  napi_set_named_property(env, out, "segments", num(env, (double)s.segments));
  napi_set_named_property(env, out, "nominalSegments", num(env, (double)s.nominal_segments));
  napi_set_named_property(env, out, "kernelMs", num(env, s.kernel_ms));
  napi_set_named_property(env, out, "lastLaunchMs", num(env, s.last_launch_ms));
  napi_set_named_property(env, out, "launches", num(env, s.launches));
  return out;
}
// noise estimate (sail_noise_mark, sail_noise_estimate, sail_render_until)
napi_value NoiseMark(napi_env env, napi_callback_info info) { return Simple(env, info, sail_noise_mark, "sail_noise_mark"); }
napi_value noiseObject(napi_env env, const sail_noise_info& n) {
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  napi_set_named_property(env, out, "mean", num(env, n.mean));
  napi_set_named_property(env, out, "maxTile", num(env, n.max_tile));
  napi_set_named_property(env, out, "k", num(env, (double)n.k));
  napi_set_named_property(env, out, "kMark", num(env, (double)n.k_mark));
  napi_set_named_property(env, out, "nonfinite", num(env, (double)n.nonfinite));
  napi_set_named_property(env, out, "tilesX", num(env, n.tiles_x));
  napi_set_named_property(env, out, "tilesY", num(env, n.tiles_y));
  napi_set_named_property(env, out, "kernelMs", num(env, n.kernel_ms));
  return out;
}
napi_value Noise(napi_env env, napi_callback_info info) {  // (ctx, remark, wantTiles) -> {mean, maxTile, ..., tileErr?}
  napi_value a[3];
  if (!args(env, info, 3, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  bool remark = false, tiles = false;
  napi_get_value_bool(env, a[1], &remark);
  napi_get_value_bool(env, a[2], &tiles);
  void* pt = nullptr;
  napi_value tileErr = nullptr;
  if (tiles) tileErr = makeTyped(env, napi_float32_array, (size_t)((h->W + 15) / 16) * (size_t)((h->H + 15) / 16), 4, &pt);
  sail_noise_info n;
  const int rc = sail_noise_estimate(h->ctx, &n, (float*)pt, nullptr, remark ? 1 : 0);
  if (rc) return throwSail(env, "sail_noise_estimate", rc, h->ctx);
  napi_value out = noiseObject(env, n);
  if (out && tiles) NAPI_OK(napi_set_named_property(env, out, "tileErr", tileErr));
  return out;
}
// (ctx, mvp f64[16] row-major, eye f32[3], bounces, target, minSpp, maxSpp) -> {k, mean, maxTile, converged, history}
napi_value RenderUntil(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!args(env, info, 7, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  size_t nm, ne;
  int b;
  double target, mn, mx;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float64_array, &m, &nm) ||
      !getArray(env, a[2], napi_float32_array, &eye, &ne) || !getInt(env, a[3], &b) || !getDouble(env, a[4], &target) ||
      !getDouble(env, a[5], &mn) || !getDouble(env, a[6], &mx))
    return nullptr;
  if (nm < 16 || ne < 3) { napi_throw_range_error(env, nullptr, "mvp needs 16 doubles and eye 3 floats"); return nullptr; }
  if (!(mn >= 0.0 && mn <= 2147483647.0 && mx >= 0.0 && mx <= 2147483647.0) || mn != (double)(uint64_t)mn || mx != (double)(uint64_t)mx) {
    napi_throw_range_error(env, nullptr, "minSpp and maxSpp must be non-negative integers below 2^31");
    return nullptr;
  }
  sail_noise_info n;
  sail_until_step hist[64];
  int conv = 0, looks = 0;
  const int rc = sail_render_until(h->ctx, m, eye, b, target, (uint64_t)mn, (uint64_t)mx, &n, &conv, hist, 64, &looks);
  if (rc) return throwSail(env, "sail_render_until", rc, h->ctx);
  napi_value out = noiseObject(env, n);
  if (!out) return nullptr;
  napi_value cv, list;
  NAPI_OK(napi_get_boolean(env, conv != 0, &cv));
  NAPI_OK(napi_set_named_property(env, out, "converged", cv));
  const int nl = looks < 64 ? looks : 64;
  NAPI_OK(napi_create_array_with_length(env, (size_t)nl, &list));
  for (int i = 0; i < nl; i++) {
    napi_value s;
    NAPI_OK(napi_create_object(env, &s));
    napi_set_named_property(env, s, "k", num(env, (double)hist[i].k));
    napi_set_named_property(env, s, "mean", num(env, hist[i].mean));
    napi_set_named_property(env, s, "maxTile", num(env, hist[i].max_tile));
    napi_set_element(env, list, (uint32_t)i, s);
  }
  NAPI_OK(napi_set_named_property(env, out, "history", list));
  return out;
}
// adaptive sampling (sail_set_active_tiles, sail_get_active_tiles, sail_render_adaptive)
// (ctx, Uint8Array of one byte per 64x64 tile | null: no mask)
napi_value SetActiveTiles(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  napi_valuetype vt;
  napi_typeof(env, a[1], &vt);
  uint8_t* m = nullptr;
  size_t n = 0;
  if (!(vt == napi_undefined || vt == napi_null) && !getArray(env, a[1], napi_uint8_array, &m, &n)) return nullptr;
  if (n > 2147483647u) { napi_throw_range_error(env, nullptr, "too many tiles"); return nullptr; }
  const int rc = sail_set_active_tiles(h->ctx, m, (int)n);
  if (rc) return throwSail(env, "sail_set_active_tiles", rc, h->ctx);
  return nullptr;
}
// (ctx) -> Uint8Array, one byte (0 / 1) per 64x64 tile
napi_value GetActiveTiles(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  const size_t tiles = (size_t)((h->W + 63) / 64) * (size_t)((h->H + 63) / 64);
  void* p = nullptr;
  napi_value out = makeTyped(env, napi_uint8_array, tiles, 1, &p);
  if (!out) return nullptr;
  const int rc = sail_get_active_tiles(h->ctx, (uint8_t*)p, (int)tiles, nullptr);
  if (rc) return throwSail(env, "sail_get_active_tiles", rc, h->ctx);
  return out;
}
// (ctx, mvp f64[16] row-major, eye f32[3], bounces, target, minSpp, maxSpp, dilate; undefined or null keeps
// sail_adaptive_defaults' value) -> {k, mean, maxTile, ..., converged, activeTiles, tiles64X, tiles64Y, pixelSamples,
// framePixelSamples, traceMs, history, tileSamples: Uint32Array}
napi_value RenderAdaptive(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!args(env, info, 8, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  size_t nm, ne;
  int b;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float64_array, &m, &nm) ||
      !getArray(env, a[2], napi_float32_array, &eye, &ne) || !getInt(env, a[3], &b))
    return nullptr;
  if (nm < 16 || ne < 3) { napi_throw_range_error(env, nullptr, "mvp needs 16 doubles and eye 3 floats"); return nullptr; }
  sail_adaptive_params p;
  sail_adaptive_defaults(&p);
  double v[4] = {p.target, (double)p.min_spp, (double)p.max_spp, (double)p.dilate};
  for (int i = 0; i < 4; i++) {
    napi_valuetype vt;
    napi_typeof(env, a[4 + i], &vt);
    if (vt == napi_undefined || vt == napi_null) continue;
    if (!getDouble(env, a[4 + i], &v[i])) return nullptr;
  }
  if (!(v[1] >= 0.0 && v[1] <= 2147483647.0 && v[2] >= 0.0 && v[2] <= 2147483647.0) || v[1] != (double)(uint64_t)v[1] ||
      v[2] != (double)(uint64_t)v[2] || !(v[3] == 0.0 || v[3] == 1.0)) {
    napi_throw_range_error(env, nullptr, "minSpp and maxSpp must be non-negative integers below 2^31, dilate 0 or 1");
    return nullptr;
  }
  p.target = v[0]; p.min_spp = (uint64_t)v[1]; p.max_spp = (uint64_t)v[2]; p.dilate = (int)v[3];
  const size_t tiles = (size_t)((h->W + 63) / 64) * (size_t)((h->H + 63) / 64);
  void* pt = nullptr;
  napi_value tileSamples = makeTyped(env, napi_uint32_array, tiles, 4, &pt);
  if (!tileSamples) return nullptr;
  sail_adaptive_info ai;
  sail_until_step hist[64];
  int looks = 0;
  const int rc = sail_render_adaptive(h->ctx, m, eye, b, &p, &ai, hist, 64, &looks, (uint32_t*)pt);
  if (rc) return throwSail(env, "sail_render_adaptive", rc, h->ctx);
  napi_value out = noiseObject(env, ai.noise);
  if (!out) return nullptr;
  napi_value cv, list;
  NAPI_OK(napi_get_boolean(env, ai.converged != 0, &cv));
  NAPI_OK(napi_set_named_property(env, out, "converged", cv));
  napi_set_named_property(env, out, "activeTiles", num(env, ai.active_tiles));
  napi_set_named_property(env, out, "tiles64X", num(env, ai.tiles_x));
  napi_set_named_property(env, out, "tiles64Y", num(env, ai.tiles_y));
  napi_set_named_property(env, out, "pixelSamples", num(env, (double)ai.pixel_samples));
  napi_set_named_property(env, out, "framePixelSamples", num(env, (double)ai.frame_pixel_samples));
  napi_set_named_property(env, out, "traceMs", num(env, ai.kernel_ms));
  const int nl = looks < 64 ? looks : 64;
  NAPI_OK(napi_create_array_with_length(env, (size_t)nl, &list));
  for (int i = 0; i < nl; i++) {
    napi_value s;
    NAPI_OK(napi_create_object(env, &s));
    napi_set_named_property(env, s, "k", num(env, (double)hist[i].k));
    napi_set_named_property(env, s, "mean", num(env, hist[i].mean));
    napi_set_named_property(env, s, "maxTile", num(env, hist[i].max_tile));
    napi_set_element(env, list, (uint32_t)i, s);
  }
  NAPI_OK(napi_set_named_property(env, out, "history", list));
  NAPI_OK(napi_set_named_property(env, out, "tileSamples", tileSamples));
  return out;
}
// an optional amin: undefined or null is the plain call (*have = false)
bool optionalAmin(napi_env env, napi_value v, bool* have, float* amin) {
  napi_valuetype vt;
  napi_typeof(env, v, &vt);
  *have = !(vt == napi_undefined || vt == napi_null);
  double d = 0.0;
  if (*have && !getDouble(env, v, &d)) return false;
  *amin = (float)d;
  return true;
}
// the denoiser (sail_denoise): (ctx, iterations, sigmaL, sigmaX, display, gamma, wantU8[, amin]) -> {rgba, rgba8?, info};
// a parameter that is undefined or null keeps sail_denoise_defaults' value; with amin, sail_denoise_albedo
napi_value Denoise(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!argsUpTo(env, info, 7, 8, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  sail_denoise_params p;
  sail_denoise_defaults(&p);
  double v[5] = {(double)p.iterations, p.sigma_l, p.sigma_x, (double)p.display, p.gamma_c};
  for (int i = 0; i < 5; i++) {
    napi_valuetype vt;
    napi_typeof(env, a[1 + i], &vt);
    if (vt == napi_undefined || vt == napi_null) continue;
    if (!getDouble(env, a[1 + i], &v[i])) return nullptr;
  }
  if (v[0] != (double)(int)v[0] || v[3] != (double)(int)v[3]) {
    napi_throw_range_error(env, nullptr, "iterations and display must be integers");
    return nullptr;
  }
  p.iterations = (int)v[0]; p.sigma_l = (float)v[1]; p.sigma_x = (float)v[2]; p.display = (int)v[3]; p.gamma_c = (float)v[4];
  bool wantU8 = false;
  napi_get_value_bool(env, a[6], &wantU8);
  const size_t np = (size_t)h->W * h->H * 4;
  void *pf = nullptr, *p8 = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, np, 4, &pf), u8 = nullptr;
  if (wantU8) u8 = makeTyped(env, napi_uint8_array, np, 1, &p8);
  bool demod = false;
  float amin = 0.0f;
  if (!optionalAmin(env, a[7], &demod, &amin)) return nullptr;
  sail_denoise_info n;
  const int rc = demod ? sail_denoise_albedo(h->ctx, &p, amin, (float*)pf, nullptr, (uint8_t*)p8, &n)
                       : sail_denoise(h->ctx, &p, (float*)pf, nullptr, (uint8_t*)p8, &n);
  if (rc) return throwSail(env, demod ? "sail_denoise_albedo" : "sail_denoise", rc, h->ctx);
  napi_value out, inf, passes;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_object(env, &inf));
  napi_set_named_property(env, inf, "k", num(env, (double)n.k));
  napi_set_named_property(env, inf, "kMark", num(env, (double)n.k_mark));
  napi_set_named_property(env, inf, "nonfinite", num(env, (double)n.nonfinite));
  napi_set_named_property(env, inf, "iterations", num(env, n.iterations));
  napi_set_named_property(env, inf, "kernelMs", num(env, n.kernel_ms));
  NAPI_OK(napi_create_array_with_length(env, (size_t)n.iterations + 1, &passes));
  for (int i = 0; i <= n.iterations; i++) napi_set_element(env, passes, (uint32_t)i, num(env, n.pass_ms[i]));
  NAPI_OK(napi_set_named_property(env, inf, "passMs", passes));
  NAPI_OK(napi_set_named_property(env, out, "rgba", f));
  if (wantU8) NAPI_OK(napi_set_named_property(env, out, "rgba8", u8));
  NAPI_OK(napi_set_named_property(env, out, "info", inf));
  return out;
}
// ---- camera-motion reprojection (sail_gbuffer, sail_temporal_*) ----
namespace {
bool viewArgs(napi_env env, napi_value mvp, napi_value eye, double** m, float** e) {
  size_t nm, ne;
  if (!getArray(env, mvp, napi_float64_array, m, &nm) || !getArray(env, eye, napi_float32_array, e, &ne)) return false;
  if (nm < 16 || ne < 3) { napi_throw_range_error(env, nullptr, "mvp needs 16 doubles and eye 3 floats"); return false; }
  return true;
}
// cap, posTol, display, gamma from four values; undefined or null keeps sail_temporal_defaults' value
bool temporalParams(napi_env env, const napi_value* a, sail_temporal_params* p) {
  sail_temporal_defaults(p);
  double v[4] = {p->cap, p->pos_tol, (double)p->display, p->gamma_c};
  for (int i = 0; i < 4; i++) {
    napi_valuetype vt;
    napi_typeof(env, a[i], &vt);
    if (vt == napi_undefined || vt == napi_null) continue;
    if (!getDouble(env, a[i], &v[i])) return false;
  }
  if (v[2] != (double)(int)v[2]) { napi_throw_range_error(env, nullptr, "display must be an integer"); return false; }
  p->cap = (float)v[0]; p->pos_tol = (float)v[1]; p->display = (int)v[2]; p->gamma_c = (float)v[3];
  return true;
}
napi_value temporalObject(napi_env env, const sail_temporal_info& n) {
  napi_value out, passes;
  NAPI_OK(napi_create_object(env, &out));
  napi_set_named_property(env, out, "k", num(env, (double)n.k));
  napi_set_named_property(env, out, "hitPixels", num(env, (double)n.hit_pixels));
  napi_set_named_property(env, out, "historyPixels", num(env, (double)n.history_pixels));
  napi_set_named_property(env, out, "nonfinite", num(env, (double)n.nonfinite));
  napi_set_named_property(env, out, "kernelMs", num(env, n.kernel_ms));
  NAPI_OK(napi_create_array_with_length(env, 3, &passes));
  for (int i = 0; i < 3; i++) napi_set_element(env, passes, (uint32_t)i, num(env, n.pass_ms[i]));
  NAPI_OK(napi_set_named_property(env, out, "passMs", passes));
  return out;
}
}  // namespace
// (ctx, mvp f64[16] row-major, eye f32[3]) -> {id: Int32Array, t: Float32Array, xyz: Float32Array (3 per pixel)}
napi_value Gbuffer(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!args(env, info, 3, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  if (!getHandle(env, a[0], &h) || !viewArgs(env, a[1], a[2], &m, &eye)) return nullptr;
  const size_t np = (size_t)h->W * h->H;
  void *pi = nullptr, *pt = nullptr, *px = nullptr;
  napi_value id = makeTyped(env, napi_int32_array, np, 4, &pi), t = makeTyped(env, napi_float32_array, np, 4, &pt),
             xyz = makeTyped(env, napi_float32_array, np * 3, 4, &px);
  const int rc = sail_gbuffer(h->ctx, m, eye, nullptr, (int32_t*)pi, (float*)pt, (float*)px);
  if (rc) return throwSail(env, "sail_gbuffer", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "id", id));
  NAPI_OK(napi_set_named_property(env, out, "t", t));
  NAPI_OK(napi_set_named_property(env, out, "xyz", xyz));
  return out;
}
// (ctx, mvp, eye, cap, posTol) -> {k, hitPixels, historyPixels, nonfinite, kernelMs, passMs}
napi_value TemporalBegin(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  if (!getHandle(env, a[0], &h) || !viewArgs(env, a[1], a[2], &m, &eye)) return nullptr;
  const napi_value none = undef(env);
  const napi_value pv[4] = {a[3], a[4], none, none};
  sail_temporal_params p;
  if (!temporalParams(env, pv, &p)) return nullptr;
  sail_temporal_info n;
  const int rc = sail_temporal_begin(h->ctx, m, eye, &p, &n);
  if (rc) return throwSail(env, "sail_temporal_begin", rc, h->ctx);
  return temporalObject(env, n);
}
// (ctx, cap, posTol, display, gamma, wantF32) -> {rgba8, rgba?, info}
napi_value TemporalResolve(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (!args(env, info, 6, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  sail_temporal_params p;
  if (!temporalParams(env, a + 1, &p)) return nullptr;
  bool wantF32 = false;
  napi_get_value_bool(env, a[5], &wantF32);
  const size_t np = (size_t)h->W * h->H * 4;
  void *pf = nullptr, *p8 = nullptr;
  napi_value u8 = makeTyped(env, napi_uint8_array, np, 1, &p8), f = nullptr;
  if (wantF32) f = makeTyped(env, napi_float32_array, np, 4, &pf);
  sail_temporal_info n;
  const int rc = sail_temporal_resolve(h->ctx, &p, (float*)pf, (uint8_t*)p8, &n);
  if (rc) return throwSail(env, "sail_temporal_resolve", rc, h->ctx);
  napi_value out, inf = temporalObject(env, n);
  if (!inf) return nullptr;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "rgba8", u8));
  if (wantF32) NAPI_OK(napi_set_named_property(env, out, "rgba", f));
  NAPI_OK(napi_set_named_property(env, out, "info", inf));
  return out;
}
// (ctx, which 0..4) -> Float32Array (4 per pixel): G_cur, G_prev, Hist, R or Out
napi_value TemporalRead(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  int which = 0;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &which)) return nullptr;
  void* pf = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pf);
  const int rc = sail_temporal_read(h->ctx, which, (float*)pf);
  if (rc) return throwSail(env, "sail_temporal_read", rc, h->ctx);
  return f;
}
// (ctx, hist f32[W H 4], g f32[W H 4], mvpPrev, eyePrev)
napi_value TemporalLoadHistory(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  float *hist, *g, *eye;
  double* m;
  size_t nh, ng;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &hist, &nh) ||
      !getArray(env, a[2], napi_float32_array, &g, &ng) || !viewArgs(env, a[3], a[4], &m, &eye))
    return nullptr;
  const size_t need = (size_t)h->W * h->H * 4;
  if (nh < need || ng < need) { napi_throw_range_error(env, nullptr, "hist and g need width * height * 4 floats"); return nullptr; }
  const int rc = sail_temporal_load_history(h->ctx, hist, g, m, eye);
  if (rc) return throwSail(env, "sail_temporal_load_history", rc, h->ctx);
  return undef(env);
}
// ---- moment tracking and the temporal filter (sail_temporal_moments, sail_temporal_filter) ----
// (ctx, on)
napi_value TemporalMoments(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  bool on = false;
  if (!getHandle(env, a[0], &h)) return nullptr;
  if (napi_get_value_bool(env, a[1], &on) != napi_ok) {  // anything but a boolean must not silently mean "off"
    napi_throw_type_error(env, nullptr, "temporalMoments: on must be a boolean");
    return nullptr;
  }
  const int rc = sail_temporal_moments(h->ctx, on ? 1 : 0);
  if (rc) return throwSail(env, "sail_temporal_moments", rc, h->ctx);
  return undef(env);
}
// (ctx, mom f32[W H 4])
napi_value TemporalLoadMoments(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  float* mom;
  size_t nm;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &mom, &nm)) return nullptr;
  if (nm < (size_t)h->W * h->H * 4) { napi_throw_range_error(env, nullptr, "mom needs width * height * 4 floats"); return nullptr; }
  const int rc = sail_temporal_load_moments(h->ctx, mom);
  if (rc) return throwSail(env, "sail_temporal_load_moments", rc, h->ctx);
  return undef(env);
}
// (ctx, which 0..2) -> Float32Array (4 per pixel): Mhist, MR or Mout
napi_value TemporalReadMoments(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  int which = 0;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &which)) return nullptr;
  void* pf = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pf);
  const int rc = sail_temporal_read_moments(h->ctx, which, (float*)pf);
  if (rc) return throwSail(env, "sail_temporal_read_moments", rc, h->ctx);
  return f;
}
// () -> {iterations, sigmaL, sigmaX, minHist, display, gamma}: sail_temporal_filter_defaults (host only)
napi_value TemporalFilterDefaults(napi_env env, napi_callback_info info) {
  (void)info;
  sail_tfilter_params p;
  sail_temporal_filter_defaults(&p);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  napi_set_named_property(env, out, "iterations", num(env, p.iterations));
  napi_set_named_property(env, out, "sigmaL", num(env, p.sigma_l));
  napi_set_named_property(env, out, "sigmaX", num(env, p.sigma_x));
  napi_set_named_property(env, out, "minHist", num(env, p.min_hist));
  napi_set_named_property(env, out, "display", num(env, p.display));
  napi_set_named_property(env, out, "gamma", num(env, p.gamma_c));
  return out;
}
// (ctx, iterations, sigmaL, sigmaX, minHist, display, gamma, wantU8[, amin]) -> {rgba, rgba8?, info}; a parameter that is
// undefined or null keeps sail_temporal_filter_defaults' value; with amin, sail_temporal_filter_albedo
napi_value TemporalFilter(napi_env env, napi_callback_info info) {
  napi_value a[9];
  if (!argsUpTo(env, info, 8, 9, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  sail_tfilter_params p;
  sail_temporal_filter_defaults(&p);
  double v[6] = {(double)p.iterations, p.sigma_l, p.sigma_x, p.min_hist, (double)p.display, p.gamma_c};
  for (int i = 0; i < 6; i++) {
    napi_valuetype vt;
    napi_typeof(env, a[1 + i], &vt);
    if (vt == napi_undefined || vt == napi_null) continue;
    if (!getDouble(env, a[1 + i], &v[i])) return nullptr;
  }
  // the range first: converting a double outside int's range is undefined
  const auto small = [](double x) { return x >= -1e6 && x <= 1e6 && x == (double)(int)x; };
  if (!small(v[0]) || !small(v[4])) {
    napi_throw_range_error(env, nullptr, "iterations and display must be integers");
    return nullptr;
  }
  p.iterations = (int)v[0]; p.sigma_l = (float)v[1]; p.sigma_x = (float)v[2]; p.min_hist = (float)v[3];
  p.display = (int)v[4]; p.gamma_c = (float)v[5];
  bool wantU8 = false;
  napi_get_value_bool(env, a[7], &wantU8);
  const size_t np = (size_t)h->W * h->H * 4;
  void *pf = nullptr, *p8 = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, np, 4, &pf), u8 = nullptr;
  if (wantU8) u8 = makeTyped(env, napi_uint8_array, np, 1, &p8);
  bool demod = false;
  float amin = 0.0f;
  if (!optionalAmin(env, a[8], &demod, &amin)) return nullptr;
  sail_tfilter_info n;
  const int rc = demod ? sail_temporal_filter_albedo(h->ctx, &p, amin, (float*)pf, nullptr, (uint8_t*)p8, &n)
                       : sail_temporal_filter(h->ctx, &p, (float*)pf, nullptr, (uint8_t*)p8, &n);
  if (rc) return throwSail(env, demod ? "sail_temporal_filter_albedo" : "sail_temporal_filter", rc, h->ctx);
  napi_value out, inf, passes;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_object(env, &inf));
  napi_set_named_property(env, inf, "k", num(env, (double)n.k));
  napi_set_named_property(env, inf, "temporalPixels", num(env, (double)n.temporal_pixels));
  napi_set_named_property(env, inf, "spatialPixels", num(env, (double)n.spatial_pixels));
  napi_set_named_property(env, inf, "nonfinite", num(env, (double)n.nonfinite));
  napi_set_named_property(env, inf, "iterations", num(env, n.iterations));
  napi_set_named_property(env, inf, "kernelMs", num(env, n.kernel_ms));
  NAPI_OK(napi_create_array_with_length(env, (size_t)n.iterations + 1, &passes));
  for (int i = 0; i <= n.iterations; i++) napi_set_element(env, passes, (uint32_t)i, num(env, n.pass_ms[i]));
  NAPI_OK(napi_set_named_property(env, inf, "passMs", passes));
  NAPI_OK(napi_set_named_property(env, out, "rgba", f));
  if (wantU8) NAPI_OK(napi_set_named_property(env, out, "rgba8", u8));
  NAPI_OK(napi_set_named_property(env, out, "info", inf));
  return out;
}
// (ctx, mvp f64[16] row-major, eye f32[3], grid) -> {rgba: Float32Array (4 per pixel), hitPixels, partialPixels, grid,
// kernelMs}: the albedo map of a view, kept by the context (sail_albedo)
napi_value Albedo(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  int grid = 0;
  if (!getHandle(env, a[0], &h) || !viewArgs(env, a[1], a[2], &m, &eye) || !getInt(env, a[3], &grid)) return nullptr;
  void* pf = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pf);
  sail_albedo_info n;
  const int rc = sail_albedo(h->ctx, m, eye, grid, (float*)pf, &n);
  if (rc) return throwSail(env, "sail_albedo", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "rgba", f));
  napi_set_named_property(env, out, "hitPixels", num(env, (double)n.hit_pixels));
  napi_set_named_property(env, out, "partialPixels", num(env, (double)n.partial_pixels));
  napi_set_named_property(env, out, "grid", num(env, n.grid));
  napi_set_named_property(env, out, "kernelMs", num(env, n.kernel_ms));
  return out;
}
// (ctx, map f32[W H 4], mvp, eye): install a caller's albedo map for a view (sail_albedo_load)
napi_value AlbedoLoad(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  Handle* h;
  float* map;
  size_t len;
  double* m;
  float* eye;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &map, &len) ||
      !viewArgs(env, a[2], a[3], &m, &eye))
    return nullptr;
  if (len < (size_t)h->W * h->H * 4) { napi_throw_range_error(env, nullptr, "the map needs W * H * 4 floats"); return nullptr; }
  const int rc = sail_albedo_load(h->ctx, map, m, eye);
  if (rc) return throwSail(env, "sail_albedo_load", rc, h->ctx);
  return undef(env);
}
// (ctx) -> Float32Array (4 per pixel): the context's albedo map (sail_albedo_read)
napi_value AlbedoRead(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  void* pf = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pf);
  const int rc = sail_albedo_read(h->ctx, (float*)pf);
  if (rc) return throwSail(env, "sail_albedo_read", rc, h->ctx);
  return f;
}
// (ctx, mvp f64[16] row-major, eye f32[3], depth) -> {n, x: Float32Array (4 per pixel), hitPixels, followedPixels,
// truncatedPixels, depth, maxDepth, kernelMs}: the guide maps of a view, kept by the context (sail_guides)
napi_value Guides(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  Handle* h;
  double* m;
  float* eye;
  int depth = 0;
  if (!getHandle(env, a[0], &h) || !viewArgs(env, a[1], a[2], &m, &eye) || !getInt(env, a[3], &depth)) return nullptr;
  void *pn = nullptr, *px = nullptr;
  napi_value fn = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pn);
  napi_value fx = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &px);
  sail_guides_info n;
  const int rc = sail_guides(h->ctx, m, eye, depth, (float*)pn, (float*)px, &n);
  if (rc) return throwSail(env, "sail_guides", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "n", fn));
  NAPI_OK(napi_set_named_property(env, out, "x", fx));
  napi_set_named_property(env, out, "hitPixels", num(env, (double)n.hit_pixels));
  napi_set_named_property(env, out, "followedPixels", num(env, (double)n.followed_pixels));
  napi_set_named_property(env, out, "truncatedPixels", num(env, (double)n.truncated_pixels));
  napi_set_named_property(env, out, "depth", num(env, n.depth));
  napi_set_named_property(env, out, "maxDepth", num(env, n.max_depth));
  napi_set_named_property(env, out, "kernelMs", num(env, n.kernel_ms));
  return out;
}
// (ctx, n f32[W H 4], x f32[W H 4], mvp, eye): install a caller's guide maps for a view (sail_guides_load)
napi_value GuidesLoad(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  Handle* h;
  float *nm, *xm;
  size_t ln, lx;
  double* m;
  float* eye;
  if (!getHandle(env, a[0], &h) || !getArray(env, a[1], napi_float32_array, &nm, &ln) ||
      !getArray(env, a[2], napi_float32_array, &xm, &lx) || !viewArgs(env, a[3], a[4], &m, &eye))
    return nullptr;
  if (ln < (size_t)h->W * h->H * 4 || lx < (size_t)h->W * h->H * 4) {
    napi_throw_range_error(env, nullptr, "each map needs W * H * 4 floats");
    return nullptr;
  }
  const int rc = sail_guides_load(h->ctx, nm, xm, m, eye);
  if (rc) return throwSail(env, "sail_guides_load", rc, h->ctx);
  return undef(env);
}
// (ctx, which: 0 Ng, 1 Xg) -> Float32Array (4 per pixel): one of the context's guide maps (sail_guides_read)
napi_value GuidesRead(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  int which = 0;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &which)) return nullptr;
  void* pf = nullptr;
  napi_value f = makeTyped(env, napi_float32_array, (size_t)h->W * h->H * 4, 4, &pf);
  const int rc = sail_guides_read(h->ctx, which, (float*)pf);
  if (rc) return throwSail(env, "sail_guides_read", rc, h->ctx);
  return f;
}
// (ctx, on): the four filters read the guide maps in the AOVs' place (sail_use_guides)
napi_value UseGuides(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  bool on = false;
  if (!getHandle(env, a[0], &h)) return nullptr;
  if (napi_get_value_bool(env, a[1], &on) != napi_ok) {
    napi_throw_type_error(env, nullptr, "on must be a boolean");
    return nullptr;
  }
  const int rc = sail_use_guides(h->ctx, on ? 1 : 0);
  if (rc) return throwSail(env, "sail_use_guides", rc, h->ctx);
  return undef(env);
}
// (ctx, timeoutMs) -> whether the scene's run-time kernel is loaded (sail_kernel_ready; -1 waits for its build)
napi_value KernelReady(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!args(env, info, 2, a)) return nullptr;
  Handle* h;
  int ms = 0;
  if (!getHandle(env, a[0], &h) || !getInt(env, a[1], &ms)) return nullptr;
  int ready = 0;
  const int rc = sail_kernel_ready(h->ctx, ms, &ready);
  if (rc) return throwSail(env, "sail_kernel_ready", rc, h->ctx);
  napi_value out;
  NAPI_OK(napi_get_boolean(env, ready != 0, &out));
  return out;
}
// (ctx) -> {name, buildId, jitState, jitFromCache, jitCompileMs, jitError} (sail_get_kernel_info)
napi_value KernelInfo(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!args(env, info, 1, a)) return nullptr;
  Handle* h;
  if (!getHandle(env, a[0], &h)) return nullptr;
  sail_kernel_info k;
  const int rc = sail_get_kernel_info(h->ctx, &k);
  if (rc) return throwSail(env, "sail_get_kernel_info", rc, h->ctx);
  char id[17];
  snprintf(id, sizeof id, "%016llx", (unsigned long long)k.build_id);
  napi_value out, v;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_create_string_utf8(env, k.name, NAPI_AUTO_LENGTH, &v));
  napi_set_named_property(env, out, "name", v);
  NAPI_OK(napi_create_string_utf8(env, id, NAPI_AUTO_LENGTH, &v));
  napi_set_named_property(env, out, "buildId", v);
  static const char* const states[] = {"none", "pending", "ready", "failed"};
  NAPI_OK(napi_create_string_utf8(env, states[k.jit_state & 3], NAPI_AUTO_LENGTH, &v));
  napi_set_named_property(env, out, "jitState", v);
  napi_set_named_property(env, out, "jitFromCache", num(env, k.jit_from_cache));
  napi_set_named_property(env, out, "jitCompileMs", num(env, k.jit_compile_ms));
  NAPI_OK(napi_create_string_utf8(env, k.jit_error, NAPI_AUTO_LENGTH, &v));
  napi_set_named_property(env, out, "jitError", v);
  return out;
}
bool getVec(napi_env env, napi_value v, double* out, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    if (napi_get_element(env, v, i, &e) != napi_ok || napi_get_value_double(env, e, &out[i]) != napi_ok) {
      napi_throw_type_error(env, nullptr, "expected an array of numbers");
      return false;
    }
  }
  return true;
}
napi_value Camera(napi_env env, napi_callback_info info) {  // (eye, center, up, fovy, aspect, near, far) -> Float64Array(16)
  napi_value a[7];
  if (!args(env, info, 7, a)) return nullptr;
  double e[3], c[3], u[3], fovy, asp, zn, zf;
  if (!getVec(env, a[0], e, 3) || !getVec(env, a[1], c, 3) || !getVec(env, a[2], u, 3) || !getDouble(env, a[3], &fovy) ||
      !getDouble(env, a[4], &asp) || !getDouble(env, a[5], &zn) || !getDouble(env, a[6], &zf))
    return nullptr;
  void* p = nullptr;
  napi_value arr = makeTyped(env, napi_float64_array, 16, 8, &p);
  const int rc = sail_camera(e, c, u, fovy, asp, zn, zf, (double*)p);
  if (rc) return throwSail(env, "sail_camera", rc, nullptr);
  return arr;
}
napi_value JitterInverse(napi_env env, napi_callback_info info) {  // (mvp f64[16] row-major, jx, jy, W, H)
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  double* m;
  size_t nm;
  double jx, jy;
  int w, hh;
  if (!getArray(env, a[0], napi_float64_array, &m, &nm) || !getDouble(env, a[1], &jx) || !getDouble(env, a[2], &jy) ||
      !getInt(env, a[3], &w) || !getInt(env, a[4], &hh))
    return nullptr;
  if (nm < 16) { napi_throw_range_error(env, nullptr, "mvp needs 16 doubles"); return nullptr; }
  void* p = nullptr;
  napi_value arr = makeTyped(env, napi_float32_array, 16, 4, &p);
  const int rc = sail_jitter_inverse(m, jx, jy, w, hh, (float*)p);
  if (rc) return throwSail(env, "sail_jitter_inverse", rc, nullptr);
  return arr;
}
napi_value Schedule(napi_env env, napi_callback_info info) {  // (mvp, W, H, k0, spp) -> {inv, seeds}
  napi_value a[5];
  if (!args(env, info, 5, a)) return nullptr;
  double* m;
  size_t nm;
  int w, hh, k0, spp;
  if (!getArray(env, a[0], napi_float64_array, &m, &nm) || !getInt(env, a[1], &w) || !getInt(env, a[2], &hh) ||
      !getInt(env, a[3], &k0) || !getInt(env, a[4], &spp))
    return nullptr;
  if (nm < 16 || spp < 0) { napi_throw_range_error(env, nullptr, "bad schedule arguments"); return nullptr; }
  void *pi = nullptr, *ps = nullptr;
  napi_value inv = makeTyped(env, napi_float32_array, (size_t)spp * 16, 4, &pi);
  napi_value seeds = makeTyped(env, napi_float32_array, (size_t)spp, 4, &ps);
  const int rc = sail_schedule(m, w, hh, k0, spp, (float*)pi, (float*)ps);
  if (rc) return throwSail(env, "sail_schedule", rc, nullptr);
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "inv", inv));
  NAPI_OK(napi_set_named_property(env, out, "seeds", seeds));
  return out;
}
napi_value PartitionTiles(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!args(env, info, 4, a)) return nullptr;
  int w, hh, r, wo;
  if (!getInt(env, a[0], &w) || !getInt(env, a[1], &hh) || !getInt(env, a[2], &r) || !getInt(env, a[3], &wo)) return nullptr;
  const int n = sail_partition_tiles(w, hh, r, wo, nullptr, 0);
  if (n < 0) return throwSail(env, "sail_partition_tiles", n, nullptr);
  void* p = nullptr;
  napi_value arr = makeTyped(env, napi_int32_array, (size_t)n * 4, 4, &p);
  sail_partition_tiles(w, hh, r, wo, (int*)p, n);
  return arr;
}
napi_value MathProbe(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!args(env, info, 3, a)) return nullptr;
  int fn;
  float *x, *y;
  size_t nx, ny;
  if (!getInt(env, a[0], &fn) || !getArray(env, a[1], napi_float32_array, &x, &nx) ||
      !getArray(env, a[2], napi_float32_array, &y, &ny))
    return nullptr;
  if (ny < nx) { napi_throw_range_error(env, nullptr, "y shorter than x"); return nullptr; }
  void* p = nullptr;
  napi_value arr = makeTyped(env, napi_float32_array, nx, 4, &p);
  const int rc = sail_math_probe(fn, x, y, (float*)p, (int)nx);
  if (rc) return throwSail(env, "sail_math_probe", rc, nullptr);
  return arr;
}

napi_value Init(napi_env env, napi_value exports) {
  const napi_property_descriptor props[] = {
      {"deviceCount", 0, DeviceCount, 0, 0, 0, napi_enumerable, 0},
      {"abiVersion", 0, AbiVersion, 0, 0, 0, napi_enumerable, 0},
      {"create", 0, Create, 0, 0, 0, napi_enumerable, 0},
      {"createMulti", 0, CreateMulti, 0, 0, 0, napi_enumerable, 0},
      {"setDebug", 0, SetDebug, 0, 0, 0, napi_enumerable, 0},
      {"reduce", 0, Reduce, 0, 0, 0, napi_enumerable, 0},
      {"destroy", 0, Destroy, 0, 0, 0, napi_enumerable, 0},
      {"setScene", 0, SetScene, 0, 0, 0, napi_enumerable, 0},
      {"updateObjects", 0, UpdateObjects, 0, 0, 0, napi_enumerable, 0},
      {"moveObjects", 0, MoveObjects, 0, 0, 0, napi_enumerable, 0},
      {"setAccumMode", 0, SetAccumMode, 0, 0, 0, napi_enumerable, 0},
      {"setPartition", 0, SetPartition, 0, 0, 0, napi_enumerable, 0},
      {"setLaunchSamples", 0, SetLaunchSamples, 0, 0, 0, napi_enumerable, 0},
      {"render", 0, Render, 0, 0, 0, napi_enumerable, 0},
      {"renderSchedule", 0, RenderSchedule, 0, 0, 0, napi_enumerable, 0},
      {"reset", 0, Reset, 0, 0, 0, napi_enumerable, 0},
      {"sync", 0, Sync, 0, 0, 0, napi_enumerable, 0},
      {"readback", 0, Readback, 0, 0, 0, napi_enumerable, 0},
      {"readAccum", 0, ReadAccum, 0, 0, 0, napi_enumerable, 0},
      {"saveAccum", 0, SaveAccum, 0, 0, 0, napi_enumerable, 0},
      {"loadAccum", 0, LoadAccum, 0, 0, 0, napi_enumerable, 0},
      {"filter", 0, Filter, 0, 0, 0, napi_enumerable, 0},
      {"stats", 0, Stats, 0, 0, 0, napi_enumerable, 0},
      {"noiseMark", 0, NoiseMark, 0, 0, 0, napi_enumerable, 0},
      {"noise", 0, Noise, 0, 0, 0, napi_enumerable, 0},
      {"renderUntil", 0, RenderUntil, 0, 0, 0, napi_enumerable, 0},
      {"setActiveTiles", 0, SetActiveTiles, 0, 0, 0, napi_enumerable, 0},
      {"getActiveTiles", 0, GetActiveTiles, 0, 0, 0, napi_enumerable, 0},
      {"renderAdaptive", 0, RenderAdaptive, 0, 0, 0, napi_enumerable, 0},
      {"denoise", 0, Denoise, 0, 0, 0, napi_enumerable, 0},
      {"gbuffer", 0, Gbuffer, 0, 0, 0, napi_enumerable, 0},
      {"temporalBegin", 0, TemporalBegin, 0, 0, 0, napi_enumerable, 0},
      {"temporalResolve", 0, TemporalResolve, 0, 0, 0, napi_enumerable, 0},
      {"temporalRead", 0, TemporalRead, 0, 0, 0, napi_enumerable, 0},
      {"temporalLoadHistory", 0, TemporalLoadHistory, 0, 0, 0, napi_enumerable, 0},
      {"temporalMoments", 0, TemporalMoments, 0, 0, 0, napi_enumerable, 0},
      {"temporalLoadMoments", 0, TemporalLoadMoments, 0, 0, 0, napi_enumerable, 0},
      {"temporalReadMoments", 0, TemporalReadMoments, 0, 0, 0, napi_enumerable, 0},
      {"temporalFilterDefaults", 0, TemporalFilterDefaults, 0, 0, 0, napi_enumerable, 0},
      {"temporalFilter", 0, TemporalFilter, 0, 0, 0, napi_enumerable, 0},
      {"albedo", 0, Albedo, 0, 0, 0, napi_enumerable, 0},
      {"albedoLoad", 0, AlbedoLoad, 0, 0, 0, napi_enumerable, 0},
      {"albedoRead", 0, AlbedoRead, 0, 0, 0, napi_enumerable, 0},
      {"guides", 0, Guides, 0, 0, 0, napi_enumerable, 0},
      {"guidesLoad", 0, GuidesLoad, 0, 0, 0, napi_enumerable, 0},
      {"guidesRead", 0, GuidesRead, 0, 0, 0, napi_enumerable, 0},
      {"useGuides", 0, UseGuides, 0, 0, 0, napi_enumerable, 0},
      {"kernelReady", 0, KernelReady, 0, 0, 0, napi_enumerable, 0},
      {"kernelInfo", 0, KernelInfo, 0, 0, 0, napi_enumerable, 0},
      {"pick", 0, Pick, 0, 0, 0, napi_enumerable, 0},
      {"camera", 0, Camera, 0, 0, 0, napi_enumerable, 0},
      {"jitterInverse", 0, JitterInverse, 0, 0, 0, napi_enumerable, 0},
      {"schedule", 0, Schedule, 0, 0, 0, napi_enumerable, 0},
      {"partitionTiles", 0, PartitionTiles, 0, 0, 0, napi_enumerable, 0},
      {"mathProbe", 0, MathProbe, 0, 0, 0, napi_enumerable, 0},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
