"""The GPU parity scenes must reach every branch outcome of the CPU oracle's path code (CPU only, no GPU).

Every trace kernel form is held bit for bit to oracle/sail_oracle.cpp; that bar bites only where a scene drives a path
through a piece of code. tests/oracle_coverage.py measures (gcov) which outcome of which conditional each frame of
tests/parity_cases.py (what the GPU tests compare) and each directed scene of tests/golden/branch_scenes.json takes.

  * the gate: every outcome is taken at least 8 times within one single scene, or stands in
    tests/golden/unreachable_branches.json with a reason argued from the code; a listed `unreachable` outcome that is
    in fact taken fails the test, so the list can only shrink to the truth (`no_effect` entries are outcomes whose
    forcing cannot change a frame: they may be taken, and need no scene of their own);
  * the directed scenes are what their generator writes, take the outcomes they name, and agree between the C++ oracle
    and its JS twin (oracle/sail_soft.js), raw uint32;
  * each directed scene depends on each outcome it is there for: with that condition forced the other way in a copy of
    the oracle, at least one channel of the scene's frame (accumulator or AOV maps) or its exact segment count, which
    the GPU test compares too, changes.
tests/test_gpu_branch_scenes.py renders the same scenes on the GPU."""
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle
import oracle_coverage as oc
from sail_amd import capi
from test_fuzz_scenes import bit_equal  # raw uint32 but for the default NaN's sign (see its docstring)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOFT = os.path.join(ROOT, "oracle", "sail_soft.js")
NODE = shutil.which("node") or shutil.which("nodejs")
NEED = 8
LIMITS = (48, 32, 4, 8)  # a directed scene's largest width, height, samples, bounces

pytestmark = pytest.mark.skipif(not oc.AVAILABLE, reason="g++ or gcov not installed")

with open(os.path.join(GOLDEN, "branch_scenes.json")) as _f:
    SCENES = json.load(_f)
with open(os.path.join(GOLDEN, "unreachable_branches.json")) as _f:
    LISTED = {(e["function"], e["condition"], e["outcome"]): e for e in json.load(_f)}
NAMES = sorted(SCENES)


def directed_cases():
    return [("branch:" + n, SCENES[n], SCENES[n]["W"], SCENES[n]["H"], SCENES[n]["spp"], SCENES[n]["bounces"]) for n in NAMES]


@pytest.fixture(scope="module")
def coverage():
    import parity_cases
    reg = parity_cases.registry()
    cov = oc.measure(reg + directed_cases())
    cov.registry_ids = {c[0] for c in reg}
    return cov


# ---- the harness reads gcov right -------------------------------------------------------------------------------------
CALIBRATION = r"""
struct F { float v; F(float x) : v(x) {} };
static inline bool operator<(F a, F b) { return a.v < b.v; }
static inline bool operator>=(F a, F b) { return a.v >= b.v; }
static bool q(int x) { return x > 2; }
static int neg_float(float s) {
  if (!(s >= 0.0f)) return 0;
  return 1;
}
static int neg_bool(bool b) {
  if (!b) return 1;
  return 0;
}
static int both(F a, F b) {
  if (a < b && b >= F(3.0f)) return 1;
  return 0;
}
static int either(F a, F b) {
  if (a < b || b >= F(3.0f)) return 1;
  return 0;
}
static float tern(bool r) { return r ? -1.0f : 1.0f; }
static bool ret(F a) { return a >= F(1.0f) && a < F(2.0f); }
static int neg_call(int x) {
  if (!q(x)) return 5;
  return 6;
}
static int sw(int c) {
  switch (c) {
    case 1: return 4;
    case 2: return 5;
    case 7: return 9;
    default: break;
  }
  return 0;
}
static int loop(int n) {
  int s = 0;
  for (int i = 0; i < n; i++) s += i;
  return s;
}
static bool guard(int c, unsigned m) {
  if (!(c >= 0 && c < 32 && ((m >> c) & 1u))) return false;
  return true;
}
static int twice(int a) {
  if (a > 0) a -= 1;
  if (a > 0) a -= 1;
  return a;
}
extern "C" int run() {
  int s = 0;
  for (int i = 0; i < 3; i++) s += neg_float(1.0f);
  for (int i = 0; i < 5; i++) s += neg_bool(true);
  s += neg_bool(false);
  for (int i = 0; i < 7; i++) s += both(F(1), F(2));
  for (int i = 0; i < 2; i++) s += either(F(5), F(4));
  for (int i = 0; i < 4; i++) s += (int)tern(true);
  s += (int)tern(false);
  for (int i = 0; i < 6; i++) s += ret(F(1.5f));
  s += ret(F(0.5f));
  for (int i = 0; i < 3; i++) s += neg_call(5);
  s += neg_call(0);
  s += sw(1) + sw(1) + sw(2) + sw(9);
  s += loop(4);
  for (int i = 0; i < 9; i++) s += guard(3, 8u);
  s += guard(3, 0u) + guard(-1, 8u) + guard(-1, 8u);
  s += twice(1) + twice(2) + twice(2);
  return s;
}
"""
CALIBRATION_WANT = {
    ("neg_float", "!(s >= 0.0f)", "true"): 0, ("neg_float", "!(s >= 0.0f)", "false"): 3,
    ("neg_bool", "!b", "true"): 1, ("neg_bool", "!b", "false"): 5,
    ("both", "a < b", "true"): 7, ("both", "a < b", "false"): 0,
    ("both", "b >= F(3.0f)", "true"): 0, ("both", "b >= F(3.0f)", "false"): 7,
    ("both", "a < b && b >= F(3.0f)", "true"): 0, ("both", "a < b && b >= F(3.0f)", "false"): 7,
    ("either", "a < b", "true"): 0, ("either", "a < b", "false"): 2,
    ("either", "b >= F(3.0f)", "true"): 2, ("either", "b >= F(3.0f)", "false"): 0,
    ("either", "a < b || b >= F(3.0f)", "true"): 2, ("either", "a < b || b >= F(3.0f)", "false"): 0,
    ("tern", "r", "true"): 4, ("tern", "r", "false"): 1,
    ("ret", "a >= F(1.0f)", "true"): 6, ("ret", "a >= F(1.0f)", "false"): 1,
    ("ret", "a < F(2.0f)", "true"): 6, ("ret", "a < F(2.0f)", "false"): 0,
    ("neg_call", "!q(x)", "true"): 1, ("neg_call", "!q(x)", "false"): 3,
    ("sw", "switch", "case 1"): 2, ("sw", "switch", "case 2"): 1, ("sw", "switch", "case 7"): 0, ("sw", "switch", "default"): 1,
    ("loop", "i < n", "true"): 4, ("loop", "i < n", "false"): 1,
    ("guard", "c >= 0", "true"): 10, ("guard", "c >= 0", "false"): 2,
    ("guard", "c < 32", "true"): 10, ("guard", "c < 32", "false"): 0,
    ("guard", "(m >> c) & 1u", "true"): 9, ("guard", "(m >> c) & 1u", "false"): 1,
    ("twice", "a > 0  [1 of 2]", "true"): 3, ("twice", "a > 0  [1 of 2]", "false"): 0,
    ("twice", "a > 0  [2 of 2]", "true"): 2, ("twice", "a > 0  [2 of 2]", "false"): 1,
}


def test_harness_reads_a_program_with_known_counts(tmp_path):
    """every form of condition the oracle's path code uses (negations of floats, bools and calls, && and || over class
    operands with their temporary, ?:, a bool-valued return, a switch, a loop, the negated category guard, one text
    twice in a function), each with counts that tell its two outcomes apart"""
    src = tmp_path / "calibration.cpp"
    src.write_text(CALIBRATION)
    lib = oc.build(str(tmp_path), str(src), name="calibration")
    subprocess.run([sys.executable, "-c", "import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.run(); L.cov_flush()", lib],
                   check=True, timeout=60)
    got = oc.parse(str(tmp_path), str(src))
    assert got == CALIBRATION_WANT, {k: (got.get(k), CALIBRATION_WANT.get(k)) for k in set(got) | set(CALIBRATION_WANT)
                                     if got.get(k) != CALIBRATION_WANT.get(k)}


def test_no_condition_of_the_path_code_is_keyed_by_position(coverage):
    """the harness tells every condition of the path code apart by its text"""
    assert not {k[:2] for k in coverage.keys if k[2].startswith("arc ")}
    assert len(coverage.keys) > 400 and len({k[0] for k in coverage.keys}) >= 40


# ---- the fixture ------------------------------------------------------------------------------------------------------
def test_branch_fixture_is_what_the_generator_writes(tmp_path):
    out = tmp_path / "branch.json"
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_branch_scenes.py"), str(out)], check=True, timeout=120)
    assert json.loads(out.read_text()) == SCENES


def test_directed_scenes_are_small_and_some_are_cornell_set():
    cornell = 0
    for n, s in SCENES.items():
        assert (s["W"], s["H"]) <= LIMITS[:2] and s["W"] <= LIMITS[0] and s["H"] <= LIMITS[1], n
        assert s["spp"] <= LIMITS[2] and s["bounces"] <= LIMITS[3], n
        assert s["targets"] or s["also"], n
        p = s["plugins"]
        if (set(p["shape"]) <= {"cube", "sphere", "cornellbox"} and set(p["material"]) <= {"matte", "mirror"}
                and not p["texture"] and s["ln"] == 0 and s["n"] <= 3):
            cornell += 1
    assert cornell >= 4


# ---- the gate ---------------------------------------------------------------------------------------------------------
def test_every_outcome_is_taken_eight_times_in_one_scene_or_argued_unreachable(coverage):
    missing, taken_though_listed = [], []
    for k in sorted(coverage.keys):
        n, where = coverage.best(k)
        if k in LISTED:
            if LISTED[k]["kind"] == "unreachable" and coverage.total(k):
                taken_though_listed.append((k, coverage.total(k), where))
        elif n < NEED:
            missing.append((k, n, where))
    assert not taken_though_listed, f"listed as unreachable, but taken: {taken_though_listed}"
    assert not missing, "taken fewer than 8 times in every scene:\n" + "\n".join(map(str, missing))


def test_the_unreachable_list_names_real_outcomes_with_reasons(coverage):
    for k, e in LISTED.items():
        assert k in coverage.keys, f"no such outcome in the path code: {k}"
        assert e["kind"] in ("unreachable", "no_effect") and len(e["reason"]) > 40, k
    assert sum(e["kind"] == "unreachable" for e in LISTED.values()) == 13


def test_directed_scenes_take_what_they_name(coverage):
    for n in NAMES:
        for t in SCENES[n]["targets"] + SCENES[n]["also"]:
            got = coverage.per_case.get(tuple(t), {}).get("branch:" + n, 0)
            assert got >= NEED, f"{n}: {t} taken {got} times"
    # and they add something: each target was below 8 in every frame of the registry
    for n in NAMES:
        for t in SCENES[n]["targets"]:
            assert coverage.best(tuple(t), coverage.registry_ids)[0] < NEED, (n, t)


def test_hash_cannot_centre_a_disk_sample_eight_times():
    """concentricSampleDisk's (0, 0) return needs random2(seed) == (0.5, 0.5): every input a scene within LIMITS can
    present (pixel centre, the schedule's sample times, depth), through the oracle's own sin and fract"""
    f = np.float32
    w, h, spp, bounces = LIMITS
    _, times = capi.schedule(np.eye(4), w, h, 0, spp)

    def hash1(seed, fx, fy, a, b, c):
        d = ((fx + seed) * f(a) + (fy + seed) * f(b)) + (f(0.5) + seed) * f(c)
        return oracle.math(17, oracle.math(0, d) * f(43758.5453) + seed)

    xs, ys = np.meshgrid(np.arange(w, dtype=f) + f(0.5), np.arange(h, dtype=f) + f(0.5))
    both = 0
    for t in times:
        for depth in range(1, bounces + 1):
            seed = f(t) + f(depth)
            u = hash1(seed, xs.ravel(), ys.ravel(), 12.9898, 78.233, 151.7182)
            v = hash1(seed, xs.ravel(), ys.ravel(), 63.7264, 10.873, 623.6736)
            both += int(((u == f(0.5)) & (v == f(0.5))).sum())
    print("inputs with both hashes 0.5:", both)
    assert both < NEED


# ---- each directed scene depends on each outcome it is there for ---------------------------------------------------------
# (function, condition, outcome) -> (needle, replacement): the needle occurs exactly once in that function of
# sail_oracle.cpp, and the replacement forces the condition away from the named outcome. (texel's forced form sends the
# clamp to the other end of the texture instead of letting a negative index through: the mutant must stay in bounds.)
RET = "return BLACKv * F(0.001f);"
MUTANTS = {
    ("matte", "sameHemisphere(wo, wi)  [1 of 2]", "false"):
        ("// lambertian_r_sample_f bsdf.glsl:15-19\n    pdf = sameHemisphere(wo, wi) ?", "// forced\n    pdf = true ?"),
    ("matte", "sameHemisphere(wo, wi)  [2 of 2]", "false"):
        ("// orenNayar_sample_f bsdf.glsl:72-76\n    pdf = sameHemisphere(wo, wi) ?", "// forced\n    pdf = true ?"),
    ("intersectSphere", "hit.y == F(0.0f)", "false"): (" && hit.y == F(0.0f)) hit.x", " && true) hit.x"),
    ("intersectObjects", "(C.shapeMask >> category) & 1u", "false"):
        ("category < 32 && ((C.shapeMask >> category) & 1u)) {", "category < 32 && true) {"),
    ("texel", "!(s >= 0.0f)", "true"): ("if (!(s >= 0.0f)) return 0;", "if (!(s >= 0.0f)) return size - 1;"),
    ("veq", "a.z == b.z", "false"): ("a.y == b.y && a.z == b.z", "a.y == b.y && true"),
    ("intersectParaboloid", "hit.z < zMin  [2 of 2]", "true"):
        ("    if (hit.z < zMin || hit.z > zMax) return result;", "    if (false || hit.z > zMax) return result;"),
    ("trSampleWh", "!sameHemisphere(wo, wh)", "true"): ("if (!sameHemisphere(wo, wh)) wh = -wh;", "if (false) wh = -wh;"),
    ("microfacet_r_sample_f", "wo.z < F(kEps)", "true"): ("if (wo.z < F(kEps)) " + RET, "if (false) " + RET),
    ("microfacet_t_sample_f", "equalZero(wo.z)", "true"): ("if (equalZero(wo.z)) " + RET, "if (false) " + RET),
    ("microfacet_t_f", "sameHemisphere(wo, wi)", "true"): ("if (sameHemisphere(wo, wi)) " + RET, "if (false) " + RET),
    ("glass", "vr < F(kEps)", "false"): ("ur < F(kEps) && vr < F(kEps);", "ur < F(kEps) && true;"),
    ("trD", "t2 >= F(kInf)", "true"): ("if (t2 >= F(kInf)) return F(0.001f);", "if (false) return F(0.001f);"),
    ("sampleGeometry", "(C.shapeMask >> category) & 1u", "false"):
        ("category < 32 && ((C.shapeMask >> category) & 1u))) return result;", "category < 32 && true)) return result;"),
    ("getSurfaceColor", "!((C.texMask >> texCategory) & 1u)", "true"):
        ("if (!((C.texMask >> texCategory) & 1u)) return BLACKv;", "if (false) return BLACKv;"),
}


def mutate(text, function, needle, replacement):
    """`text` with `needle`, which must occur exactly once in `function`'s definition, replaced"""
    heads = [m for m in re.finditer(r"^static [^\n;(]*\b%s\([^\n;]*\{[^\n]*$" % re.escape(function), text, re.M)]
    assert len(heads) == 1, (function, len(heads))
    start = heads[0].start()
    end = text.index("\n}\n", start) if not heads[0].group(0).rstrip().endswith("}") else heads[0].end()
    body = text[start:end]
    assert body.count(needle) == 1, (function, needle, body.count(needle))
    return text[:start] + body.replace(needle, replacement) + text[end:]


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)


def test_every_target_has_a_mutant():
    targets = {tuple(t) for s in SCENES.values() for t in s["targets"]}
    assert targets == set(MUTANTS)


def test_each_directed_scene_depends_on_each_outcome_it_is_there_for(tmp_path):
    with open(oc.ORACLE_SRC) as f:
        text = f.read()
    cases = {c[0]: c for c in directed_cases()}
    jobs = {}  # mutant key -> the scenes that name it
    for n in NAMES:
        for t in SCENES[n]["targets"]:
            jobs.setdefault(tuple(t), []).append(cases["branch:" + n])

    def run(item):
        i, (key, todo) = item
        d = tmp_path / f"m{i}"
        d.mkdir()
        src = d / "sail_oracle.cpp"   # the same file name: the copy includes ref_math.h from oracle/ (-I)
        src.write_text(mutate(text, key[0], *MUTANTS[key]) if key else text)
        return key, oc.frames(todo, source=str(src), workdir=str(d))

    items = list(enumerate([(None, list(cases.values()))] + sorted(jobs.items())))
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        results = dict(pool.map(run, items))
    plain = results.pop(None)
    unmoved = []
    for key, frames in results.items():
        for cid, (acc, an, ap, segs) in frames.items():
            wacc, wan, wap, wsegs = plain[cid]
            changed = int((~same_bits(acc, wacc)).sum() + (~same_bits(an, wan)).sum() + (~same_bits(ap, wap)).sum())
            print(f"{cid}: {key}: {changed} channels change, {segs - wsegs:+d} segments")
            if not changed and segs == wsegs:
                unmoved.append((cid, key))
    assert not unmoved, f"forcing the condition changes no channel: {unmoved}"


# ---- the JS twin agrees on every directed scene --------------------------------------------------------------------------
@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("name", NAMES)
def test_branch_soft_js_equals_cpp_oracle(tmp_path, name):
    sc = SCENES[name]
    w, h, spp, b = sc["W"], sc["H"], sc["spp"], sc["bounces"]
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, spp)
    job = {"objects": sc["objects"], "n": sc["n"], "texparams": sc["texparams"], "tn": sc["tn"],
           "lights": sc["lights"], "ln": sc["ln"], "masks": list(capi.plugin_masks(sc["plugins"])), "W": w, "H": h,
           "inv": [float(v) for v in inv.reshape(-1)], "seeds": [float(v) for v in seeds], "eye": sc["eye"],
           "spp": spp, "maxBounces": b, "accumMode": 0, "aov": True}
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    out = subprocess.run([NODE, SOFT, str(jp), str(tmp_path / name)], capture_output=True, text=True, timeout=300,
                         check=True).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(tmp_path / f"{name}.accum.f32", dtype=np.float32).reshape(h, w, 4)
    gn = np.fromfile(tmp_path / f"{name}.aovn.f32", dtype=np.float32).reshape(h, w, 4)
    gp = np.fromfile(tmp_path / f"{name}.aovp.f32", dtype=np.float32).reshape(h, w, 4)
    oracle.reset_counters()
    want, wn, wp = oracle.render(sc, capi.plugin_masks(sc["plugins"]), w, h, inv, seeds, sc["eye"], b, aov=True)
    segs, _ = oracle.counters()
    same = bit_equal(got, want)
    assert same.all(), f"{name}: {int((~same).sum())} of {got.size} channels differ"
    assert bit_equal(gn, wn).all() and bit_equal(gp, wp).all()
    assert info["segments"] == segs
