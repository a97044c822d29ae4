"""The last bounce without its path sort and hit record (SailTraceArgs.lastQuietRows / lastSkipSort) vs the CPU oracle.
Needs an MI355X.

A path's last bounce only adds radiance. The host classifies every row (sail_plan_last_bounce): a hit on a quiet row
adds exactly +0 x throughput, so the path ends before the sort and builds no record, and where every other row is an
emitter the paths that are left are not sorted either (the Cornell and all-plugin forms; the room form, which the
light scenes and the run-time kernels of scenes outside the Cornell set take, runs its last bounce like the others and
is rendered here all the same). Every case here compares the accumulator with the oracle's render of the same schedule bit for bit:
the words themselves, NaN payloads included (no NaN tolerance).
"""
import numpy as np
import pytest

import oracle
from sail_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def words_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.view(np.uint32) == b.view(np.uint32)


def _why(got, want):
    same = words_equal(got, want)
    both_nan = np.isnan(got) & np.isnan(want) & ~same
    return f"{int((~same).sum())} of {same.size} words differ ({int(both_nan.sum())} of them NaN against NaN)"


_REFS = {}
_SEGS = {}


def _schedule(sc, W, H, spp):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), W, H, 0, spp)


def _want(key, sc, W, H, spp, B, mode=capi.ACCUM_SUM, aov=False):
    """the oracle's frame, rendered once per (scene variant, shape, schedule) and shared read-only"""
    k = (key, W, H, spp, B, mode, aov)
    if k not in _REFS:
        inv, seeds = _schedule(sc, W, H, spp)
        oracle.reset_counters()
        res = oracle.render(sc, capi.plugin_masks(sc["plugins"]), W, H, inv, seeds, sc["eye"], B, accum_mode=mode, aov=aov)
        _SEGS[k] = oracle.counters()[0]
        for a in (res if aov else (res,)):
            a.setflags(write=False)
        _REFS[k] = res
    return _REFS[k]


def _render(sc, W, H, spp, B, debug=None, mode=capi.ACCUM_SUM, aov=False, devices=None):
    inv, seeds = _schedule(sc, W, H, spp)
    ctx = capi.Context(W, H, flags=(capi.FLAG_AOV if aov else 0) | capi.FLAG_SEGMENT_COUNT, debug=debug, devices=devices)
    try:
        if mode != capi.ACCUM_SUM:
            ctx.set_accum_mode(mode)
        ctx.set_scene_dict(sc)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        got = ctx.read_accum()
        name = ctx.kernel_name()
        segs = ctx.stats().segments
        maps = ctx.readback(aov=True)[1:] if aov else None
    finally:
        ctx.close()
    return got, name, segs, maps


# kernel forms of a flat scene: the default run-time kernel, the precompiled kernel of the scene's set, and run-time
# kernels holding NS samples of each pixel in NT-thread workgroups
FORMS = {
    "default": {},
    "precompiled": {capi.DEBUG_JIT: 0},
    "ns16_nt512": {capi.DEBUG_JIT_NS: 16, capi.DEBUG_JIT_NT: 512},
    "ns4_nt128": {capi.DEBUG_JIT_NS: 4, capi.DEBUG_JIT_NT: 128},
    "ns1_nt512": {capi.DEBUG_JIT_NS: 1, capi.DEBUG_JIT_NT: 512},
}


def _expect_kernel(form, name):
    if form == "precompiled":
        assert "_jit" not in name, name
    else:
        assert "_jit" in name, name


# ---- C1: two quiet rows (walls, mirror sphere) and one emitter, so the last bounce runs unsorted ----------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("spp", [3, 17])   # 17 crosses a 16-in-flight step boundary
@pytest.mark.parametrize("B", [1, 2, 3, 6])
def test_c1_forms_and_launch_shapes(gpu, fixtures, B, spp, form):
    sc = fixtures["scenes"]["C1"]
    W, H = 37, 21  # ragged: partial pixel blocks of every form
    for groups in (1, 2):
        for mode in (capi.ACCUM_SUM, capi.ACCUM_MIX):
            got, name, segs, _ = _render(sc, W, H, spp, B, {**FORMS[form], capi.DEBUG_SAMPLE_GROUPS: groups}, mode)
            _expect_kernel(form, name)
            want = _want("C1", sc, W, H, spp, B, mode)
            assert words_equal(got, want).all(), (groups, mode, name, _why(got, want))
            assert segs == _SEGS[("C1", W, H, spp, B, mode, False)]  # the last bounce is still counted


@pytest.mark.parametrize("form", ["default", "precompiled", "ns16_nt512", "ns4_nt128"])
@pytest.mark.parametrize("B", [1, 3])
def test_c1_aovs(gpu, fixtures, B, form):
    """the AOVs come from the first bounce's record: with one bounce the quiet rows' lanes of the AOV sample build it"""
    sc = fixtures["scenes"]["C1"]
    W, H, spp = 40, 24, 3
    got, name, _, maps = _render(sc, W, H, spp, B, FORMS[form], aov=True)
    _expect_kernel(form, name)
    want, wn, wp = _want("C1", sc, W, H, spp, B, aov=True)
    assert words_equal(got, want).all(), _why(got, want)
    assert words_equal(maps[0], wn).all() and words_equal(maps[1], wp).all()


# ---- C1 with its rows edited ---------------------------------------------------------------------------------------
def _rows(sc):
    return np.array(sc["objects"], dtype=np.float32).reshape(sc["n"], 18)


def _tp(sc):
    return np.array(sc["texparams"], dtype=np.float32).reshape(sc["tn"], 16)


def _with(sc, rows=None, tp=None, plugins=None):
    out = dict(sc)
    if rows is not None:
        out["objects"] = rows.reshape(-1).tolist()
    if tp is not None:
        out["texparams"] = tp.reshape(-1).tolist()
    if plugins is not None:
        out["plugins"] = plugins
    return out


def v_sphere_emits(sc):
    rows = _rows(sc)
    rows[2, 8:11] = 8.0  # the sphere's emission
    return _with(sc, rows)


def v_all_emit(sc):
    """a Cornellbox's emission is forced black, so the walls become a reversed Cube of the same extent that emits: with
    the emitting sphere no quiet row remains and the unsorted last bounce has only emitters"""
    rows = _rows(sc)
    box = rows[1].copy()
    rows[1] = 0.0
    rows[1, 0] = 1.0
    rows[1, 1:7] = box[1:7]
    rows[1, 7] = 1.0               # reverseNormal
    rows[1, 8:10] = [box[7], 5.0]  # the walls' material row; texture row 5, a uniform white
    rows[1, 10:13] = 0.25
    rows[2, 8:11] = 8.0
    return _with(sc, rows)


def v_neg_zero(sc):
    rows = _rows(sc)
    rows[2, 8:11] = [0.0, -0.0, 0.0]
    return _with(sc, rows)


def v_nan_channel(sc):
    rows = _rows(sc)
    rows[2, 8:11] = [0.0, np.nan, 0.0]
    return _with(sc, rows)


def v_oren_nayar(sc):
    tp = _tp(sc)
    tp[:, 2:5] = np.where(tp[:, :1] == 1, [20.0, 0.6, 0.35], tp[:, 2:5])
    return _with(sc, tp=tp)


def v_inf_kd(sc):
    tp = _tp(sc)
    tp[0, 1] = np.inf
    return _with(sc, tp=tp)


def v_huge_kd(sc):
    tp = _tp(sc)
    tp[2, 1] = 3e38
    return _with(sc, tp=tp)


def v_textured_matte(sc):
    """the sphere a matte with a checkerboard: its colour is no per-scene constant"""
    tp = _tp(sc)
    tp[4] = 0.0
    tp[4, :2] = [1.0, 0.8]
    tp[5] = 0.0
    tp[5, :3] = [5.0, 0.1, 0.1]
    return _with(sc, tp=tp, plugins=dict(sc["plugins"], texture=["checkerboard"]))


# variant -> (edit, classes without a light plugin: quiet rows, skip_sort)
VARIANTS = {
    "sphere_emits": (v_sphere_emits, 0b010, 1),
    "all_emit": (v_all_emit, 0b000, 1),
    "neg_zero": (v_neg_zero, 0b010, 0),
    "nan_channel": (v_nan_channel, 0b010, 1),
    "oren_nayar": (v_oren_nayar, 0b100, 0),
    "inf_kd": (v_inf_kd, 0b100, 0),  # the walls share the light cube's material row: inf x 0 is NaN
    "huge_kd": (v_huge_kd, 0b110, 1),  # 3e38 x colour / pi is finite for every wall colour
    "textured_matte": (v_textured_matte, 0b010, 0),
}
# the forms each variant runs in: rows of other shape types or plugins have no shipped run-time kernel, so all_emit runs
# the precompiled Cornell kernel alone, and textured_matte (outside the Cornell set) its run-time kernel without a light
# plugin and the precompiled room kernel with them
VARIANT_FORMS = {"all_emit": ["precompiled"]}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("B", [1, 2, 3])
def test_c1_row_variants(gpu, fixtures, variant, B):
    sc = VARIANTS[variant][0](fixtures["scenes"]["C1"])
    W, H, spp = 24, 20, 3
    want = _want(variant, sc, W, H, spp, B)
    for form in VARIANT_FORMS.get(variant, ["default", "precompiled"]):
        got, name, _, _ = _render(sc, W, H, spp, B, FORMS[form])
        _expect_kernel(form, name)
        assert words_equal(got, want).all(), (form, name, _why(got, want))


# ---- light plugins: matte rows are full (the sort stays), the other rows are quiet -----------------------------------
@pytest.mark.parametrize("name", ["C3", "UI"])
@pytest.mark.parametrize("B", [1, 3])
def test_light_scenes(gpu, fixtures, name, B):
    sc = fixtures["scenes"][name]
    quiet, skip = capi.plan_last_bounce(sc, True)
    assert skip == 0 and quiet != 0
    W, H, spp = 40, 24, 5
    for form in ("default", "precompiled"):
        for groups in (1, 2):
            got, kname, _, _ = _render(sc, W, H, spp, B, {**FORMS[form], capi.DEBUG_SAMPLE_GROUPS: groups})
            _expect_kernel(form, kname)
            want = _want(name, sc, W, H, spp, B)
            assert words_equal(got, want).all(), (form, groups, kname, _why(got, want))


# ---- the remaining plugins (ALL) and an open scene (N1: paths leave it, so lanes are dead at the last bounce) ----------
@pytest.mark.parametrize("name", ["ALL", "N1"])
@pytest.mark.parametrize("B", [1, 4])
def test_remaining_plugins_and_open_scenes(gpu, fixtures, name, B):
    sc = fixtures["scenes"][name]
    W, H, spp = 33, 20, 3
    for form, dbg in (("default", {}), ("precompiled", {capi.DEBUG_JIT: 0}),
                      ("precompiled", {capi.DEBUG_JIT: 0, capi.DEBUG_FORCE_GENERIC: 1})):
        got, kname, _, _ = _render(sc, W, H, spp, B, dbg)
        _expect_kernel(form, kname)
        want = _want(name, sc, W, H, spp, B)
        assert words_equal(got, want).all(), (dbg, kname, _why(got, want))


# ---- a drag that toggles a row's emission changes the classes without a new kernel ------------------------------------
@pytest.mark.parametrize("form", ["default", "precompiled"])
def test_update_objects_toggles_emission(gpu, fixtures, form):
    base = fixtures["scenes"]["C1"]
    lit = v_sphere_emits(base)
    W, H, spp, B = 32, 20, 3, 3
    inv, seeds = _schedule(base, W, H, spp)
    ctx = capi.Context(W, H, debug=FORMS[form])
    try:
        ctx.set_scene_dict(base)
        ids = []
        for key, sc in (("C1", base), ("sphere_emits", lit), ("C1", base)):
            rows = np.array(sc["objects"], dtype=np.float32)
            assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]) == 0
            ctx.render_schedule(inv, seeds, sc["eye"], B)
            got = ctx.read_accum()
            ids.append(ctx.kernel_info()["build_id"])
            want = _want(key, sc, W, H, spp, B)
            assert words_equal(got, want).all(), (key, _why(got, want))
        assert ids[0] == ids[1] == ids[2], ids
    finally:
        ctx.close()


# ---- multi-device contexts: every sub-context derives the classes from the rows it is given -----------------------------
@pytest.mark.parametrize("devices", ["same", "two"])
def test_multi_device(gpu, fixtures, devices):
    if devices == "two" and capi.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    sc = fixtures["scenes"]["C1"]
    W, H, spp, B = 150, 70, 3, 3  # six 64x64 tiles, three per device
    got, name, _, _ = _render(sc, W, H, spp, B, devices=[0, 0] if devices == "same" else [0, 1])
    want = _want("C1", sc, W, H, spp, B)
    assert words_equal(got, want).all(), (name, _why(got, want))
