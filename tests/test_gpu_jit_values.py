"""The value kernel on the GPU: a flat-form run-time kernel with the scene's decoded rows and texParams table compiled in
(SAIL_JIT_ROWVALS in sail_geom.h), asked for once the rows have stood still for SAIL_DEBUG_JIT_VALUES_AFTER samples
(sail_capi.cpp refreshValues). Every frame is compared bit for bit with the CPU oracle, and every case sets the switch
explicitly; the value tier is told from the types tier by the build id, against the id obtained with the switch
negative. Scenes are C1 and variants of it: the value kernel exists for the flat form compiled for rows, which the
default switches give the Cornell plugin set only (no scene of tests/golden/fuzz_scenes.json gets one: checked below).
A variant no cache holds compiles with hipRTC in the background (seconds); the cases wait for it with kernel_ready.
Needs a GPU."""
import json
import os

import numpy as np
import pytest

import oracle
from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, B = 37, 21, 7, 6  # ragged blocks; 7 is no multiple of the 16 samples in flight
AFTER = capi.DEBUG_JIT_VALUES_AFTER
CUBE, SPHERE, CORNELL = 0, 2, 1  # C1's rows


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bit_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _variant(fixtures, rows=None, tp=None):
    """C1 with other object rows (n x 18) and / or texParams; float32 arrays keep NaN payloads and signed zeros"""
    sc = dict(fixtures["scenes"]["C1"])
    if rows is not None:
        rows = np.asarray(rows, np.float32)
        sc["n"] = int(rows.shape[0])
        sc["objects"] = rows.reshape(-1).copy()
    if tp is not None:
        sc["texparams"] = np.asarray(tp, np.float32).reshape(-1).copy()
    return sc


def _rows(fixtures):
    sc = fixtures["scenes"]["C1"]
    return np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18).copy()


def _tp(fixtures):
    sc = fixtures["scenes"]["C1"]
    return np.asarray(sc["texparams"], np.float32).reshape(sc["tn"], 16).copy()


def _f32(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def _schedule(sc, spp, w=W, h=H):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, spp)


def _want(sc, inv, seeds, mode=capi.ACCUM_SUM, aov=False, w=W, h=H, bounces=B):
    return oracle.render(sc, capi.plugin_masks(sc["plugins"]), w, h, inv, seeds, sc["eye"], bounces, accum_mode=mode, aov=aov)


def _render(sc, after, spp=SPP, mode=capi.ACCUM_SUM, aov=False, debug=None, devices=None):
    """(accumulator, AOVs or None, kernel info) of a context that waited for the best tier it asked for"""
    inv, seeds = _schedule(sc, spp)
    dbg = {AFTER: after, **(debug or {})}
    flags = capi.FLAG_AOV if aov else 0
    ctx = capi.Context(W, H, flags=flags, devices=devices, debug=dbg) if devices else capi.Context(W, H, flags=flags, debug=dbg)
    try:
        ctx.set_scene_dict(sc)
        if mode != capi.ACCUM_SUM:
            ctx.set_accum_mode(mode)
        ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        got = ctx.read_accum()
        aovs = ctx.readback(aov=True)[1:] if aov else None
        return got, aovs, ctx.kernel_info()
    finally:
        ctx.close()


def _update(ctx, sc):
    """Renderer.updateObjects: new object rows, same count"""
    rows = np.ascontiguousarray(np.asarray(sc["objects"], np.float32).reshape(-1))
    assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]) == 0


def _check_both_tiers(sc, **kw):
    """the value tier's frame equals the oracle's, under another build id than the types tier's"""
    inv, seeds = _schedule(sc, SPP)
    want = _want(sc, inv, seeds)
    got, _, info = _render(sc, 0, **kw)
    _, _, tinfo = _render(sc, -1, **kw)
    assert info["name"].startswith("sail_trace_kernel_jit") and tinfo["name"].startswith("sail_trace_kernel_jit"), (info, tinfo)
    assert info["build_id"] != tinfo["build_id"], "the launch ran the types kernel"
    assert info["build_id"] == info["jit_build_id"]
    assert bit_equal(got, want).all(), f"{int((~bit_equal(got, want)).sum())} channels differ"
    return info


# ---- 1. C1 itself: accumulation modes, AOVs, sample groups, samples in flight ----------------------------------------
_REF = {}


def _ref(fixtures, mode):
    if mode not in _REF:  # computed once per mode, shared, never written
        sc = fixtures["scenes"]["C1"]
        inv, seeds = _schedule(sc, SPP)
        _REF[mode] = _want(sc, inv, seeds, mode=mode, aov=True)
    return _REF[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [16, 1])
@pytest.mark.parametrize("groups", [0, 3])
@pytest.mark.parametrize("mode", [capi.ACCUM_SUM, capi.ACCUM_MIX, capi.ACCUM_COMPAT8])
def test_c1_value_kernel_bit_exact(gpu, fixtures, mode, groups, ns):
    sc = fixtures["scenes"]["C1"]
    dbg = {capi.DEBUG_SAMPLE_GROUPS: groups, capi.DEBUG_JIT_NS: ns}
    want, wn, wp = _ref(fixtures, mode)
    got, (gn, gp), info = _render(sc, 0, mode=mode, aov=True, debug=dbg)
    _, _, tinfo = _render(sc, -1, mode=mode, aov=True, debug=dbg)
    # one sample in flight splits this small frame's launch into sample groups by itself
    assert info["name"] == "sail_trace_kernel_jit" + ("_grouped" if groups or ns == 1 else ""), info
    assert info["build_id"] != tinfo["build_id"] and info["build_id"] == info["jit_build_id"], (info, tinfo)
    assert bit_equal(got, want).all()
    assert bit_equal(gn, wn).all() and bit_equal(gp, wp).all()


# ---- 2. / 3. row order and several rows per type ---------------------------------------------------------------------
def _more_rows(fixtures, spheres, cubes):
    """C1 with `spheres` spheres and `cubes` small cubes besides its light and box (the box stays row 1)"""
    r = _rows(fixtures)
    out = [r[CUBE], r[CORNELL]]
    for i in range(spheres):
        s = r[SPHERE].copy()
        s[1:5] = (1.0 + 1.3 * i, 0.8 + 0.9 * i, 1.5 + 1.1 * i, 0.7 - 0.12 * i)
        s[6] = 4.0 if i % 2 == 0 else 0.0  # mirror, matte
        out.append(s)
    for i in range(cubes):
        c = r[CUBE].copy()
        c[1:4] = (3.6 + 0.35 * i, 0.0, 0.4 + 1.2 * i)
        c[4:7] = (4.6 + 0.2 * i, 1.1 + 0.5 * i, 1.3 + 1.2 * i)
        c[10:13] = (0.0, 0.0, 0.0) if i % 2 == 0 else (0.5, 0.25, 2.0)
        out.append(c)
    return _variant(fixtures, rows=np.stack(out))


@pytest.mark.gpu
def test_row_order_differs_from_type_order(gpu, fixtures):
    r = _rows(fixtures)
    _check_both_tiers(_variant(fixtures, rows=r[[CORNELL, SPHERE, CUBE]]))


@pytest.mark.gpu
def test_two_spheres_in_three_rows(gpu, fixtures):
    """several rows of one type at the limit of a hit record per row (3 rows): the box and two spheres, one emitting"""
    r = _rows(fixtures)
    a, b = r[SPHERE].copy(), r[SPHERE].copy()
    a[1:5] = (1.6, 1.0, 2.2, 0.9)
    b[1:5] = (3.9, 3.6, 1.4, 0.8)
    b[6] = 0.0                      # matte
    b[8:11] = (6.0, 5.0, 4.0)       # the light
    _check_both_tiers(_variant(fixtures, rows=np.stack([a, r[CORNELL], b])))


@pytest.mark.gpu
@pytest.mark.parametrize("spheres,cubes", [(2, 0), (1, 2), (3, 3)])  # 4, 5 and 8 rows: above the limit, one generic record
def test_several_rows_per_type(gpu, fixtures, spheres, cubes):
    sc = _more_rows(fixtures, spheres, cubes)
    assert sc["n"] == 2 + spheres + cubes <= 8
    # 8 rows, the most a kernel is compiled for: the pre-cull path takes scenes from 8 rows on unless it is moved up
    _check_both_tiers(sc, debug={capi.DEBUG_CULL_MIN_PRIMS: 9} if sc["n"] == 8 else None)


# ---- 4. the fuzz scenes ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fuzz_scenes_with_a_value_kernel(gpu):
    """The value kernel is granted to flat-form kernels of the Cornell plugin set only (sail_capi.cpp valueSpecFor). No
    scene of the fuzz set is of that set, so none gets one under the default switches; and with SAIL_DEBUG_JIT without
    bit 8, which compiles their plugin sets (cones, rectangles, textures, lights) in the flat form for their rows, the
    switch 0 still leaves them on the types kernel: the same build id as with the switch negative, the oracle's frame."""
    with open(os.path.join(ROOT, "tests", "golden", "fuzz_scenes.json")) as f:
        scenes = json.load(f)
    scenes = {k: v for k, v in scenes.items() if isinstance(v, dict) and "objects" in v}
    assert len(scenes) >= 60
    assert [k for k, sc in scenes.items() if capi.jit_value_key(sc)[0] is not None] == []
    ran = 0
    for name in ("E02", "F01"):  # 4 rows with a light row, 3 rows with a light row
        sc = scenes[name]
        assert sc["n"] <= 7 and sc["ln"] >= 1
        flat = {capi.DEBUG_JIT: 19}  # 1 + 2 + 16: the plain flat form, compiled for the rows
        inv, seeds = _schedule(sc, 3)
        got, _, info = _render(sc, 0, spp=3, debug=flat)
        _, _, tinfo = _render(sc, -1, spp=3, debug=flat)
        assert info["name"].startswith("sail_trace_kernel_jit"), info
        assert info["build_id"] == tinfo["build_id"] == info["jit_build_id"], (name, info, tinfo)
        assert bit_equal(got, _want(sc, inv, seeds)).all(), name
        ran += 1
    assert ran == 2
    assert capi.jit_resident() == (0, 0)


# ---- 5. hostile rows ---------------------------------------------------------------------------------------------------
def _hostile(fixtures, which):
    r, tp = _rows(fixtures), _tp(fixtures)
    if which == "neg_zero_bound_zero_radius_kd0":
        r[CORNELL][1] = _f32(0x80000000)      # the box's min.x: -0.0
        r[SPHERE][4] = 0.0                    # radius 0
        r[CUBE][10] = _f32(0x80000000)        # emission.x: -0.0
        tp[0][1] = 0.0                        # kd 0
    elif which == "negative_radius_nan_emission_kd_inf":
        r[SPHERE][4] = -1.2
        r[SPHERE][8] = _f32(0x7fc01234)       # emission.x: a NaN with a payload
        tp[0][1] = np.inf
    elif which == "infinite_radius":
        r[SPHERE][4] = np.inf
    elif which == "nan_centre":
        r[SPHERE][1] = _f32(0xffc00001)
    elif which == "denormal_radius":
        r[SPHERE][4] = _f32(0x00012345)
    else:
        raise KeyError(which)
    return _variant(fixtures, rows=r, tp=tp)


HOSTILE = ["neg_zero_bound_zero_radius_kd0", "negative_radius_nan_emission_kd_inf", "infinite_radius", "nan_centre",
           "denormal_radius"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_rows(gpu, fixtures, which):
    _check_both_tiers(_hostile(fixtures, which))


# ---- 6. staleness ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_objects_returns_to_the_types_kernel(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    moved_rows = _rows(fixtures)
    moved_rows[SPHERE][1:4] += np.float32([0.5, 0.25, -0.4])
    moved = _variant(fixtures, rows=moved_rows)
    inv, seeds = _schedule(sc, 4)
    _, _, tinfo = _render(sc, -1, spp=1)
    types_id = tinfo["build_id"]
    ctx = capi.Context(W, H, debug={AFTER: 2})
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(inv[:2], seeds[:2], sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == types_id  # not settled yet when it was launched
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv[2:3], seeds[2:3], sc["eye"], B)
        first = ctx.kernel_info()["build_id"]
        assert first != types_id
        assert bit_equal(ctx.read_accum(), _want(sc, inv[:3], seeds[:3])).all()
        assert capi.jit_resident() == (1, 1)
        # the drag: the next launch runs the types kernel on the new rows, and the process keeps nothing of the old pose's
        # kernel (its object stays in the disk caches)
        _update(ctx, moved)
        assert capi.jit_resident() == (0, 0)
        ctx.render_schedule(inv[:1], seeds[:1], sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == types_id
        assert bit_equal(ctx.read_accum(), _want(moved, inv[:1], seeds[:1])).all()
        # three more samples: the new rows settle and get their own kernel
        ctx.render_schedule(inv[1:2], seeds[1:2], sc["eye"], B)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv[2:4], seeds[2:4], sc["eye"], B)
        second = ctx.kernel_info()["build_id"]
        assert second not in (types_id, first)
        assert capi.jit_resident() == (1, 1)
        assert bit_equal(ctx.read_accum(), _want(moved, inv, seeds)).all()
        # back to the first pose: its kernel again
        _update(ctx, sc)
        ctx.render_schedule(inv[:2], seeds[:2], sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == types_id
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv[2:3], seeds[2:3], sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == first
        assert bit_equal(ctx.read_accum(), _want(sc, inv[:3], seeds[:3])).all()
        # sail_reset does not restart the count: the value kernel stays
        ctx.reset()
        ctx.render_schedule(inv[:1], seeds[:1], sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == first
        assert capi.jit_resident() == (1, 1)  # three poses seen, one kept
    finally:
        ctx.close()
    assert capi.jit_resident() == (0, 0)


@pytest.mark.gpu
def test_masked_twin_of_the_value_kernel_goes_with_it(gpu, fixtures, tmp_path):
    """a launch under a tile mask runs the value kernel's masked twin, a module of its own (both specs carry the rows'
    words: two value objects, two modules); new rows and the context's end release both holds, the twin's with the value
    kernel's"""
    from test_gpu_adaptive import K, check_tiles, frame, masks_for, render, uniform
    sc = fixtures["scenes"]["C1"]
    w, h, bounces = 160, 96, 4  # 3 x 2 tiles, ragged right and top
    zero, first, both = uniform(fixtures, "C1", w, h, bounces)
    mask = masks_for(w, h)["checker"]
    assert mask.any() and not mask.all()
    capi.set_jit_cache(str(tmp_path / "jit"))
    try:
        ctx = capi.Context(w, h, flags=capi.FLAG_AOV, debug={AFTER: 0, capi.DEBUG_SAMPLE_GROUPS: 1})
        try:
            ctx.set_scene_dict(sc)
            render(ctx, sc, 0, K, bounces)
            assert ctx.kernel_ready(-1)
            ctx.set_active_tiles(mask)
            render(ctx, sc, K, K, bounces)
            name = ctx.kernel_name()
            assert "jit" in name and "_masked" in name, name
            check_tiles(frame(ctx), mask, both, first, "value kernel's masked twin")
            assert capi.jit_resident() == (2, 2)
            # The same rows: the value kernel and its twin go all the same. Under a threshold of 0 the update would ask for
            # the rows' value kernel again before it returns, and the cache would load it at once ((1, 1) here): the
            # threshold is out of reach while the rows change, so that the count shows what the update released.
            ctx.set_debug(AFTER, 1 << 20)
            _update(ctx, sc)
            assert capi.jit_resident() == (0, 0)
            ctx.set_debug(AFTER, 0)
            assert ctx.kernel_ready(-1)
            ctx.set_active_tiles(mask)  # the new rows' accumulation started without a mask
            render(ctx, sc, 0, K, bounces)
            name = ctx.kernel_name()
            assert "jit" in name and "_masked" in name, name
            check_tiles(frame(ctx), mask, first, zero, "masked twin after the update")
            assert capi.jit_resident() == (2, 2)
        finally:
            ctx.close()
        assert capi.jit_resident() == (0, 0)
    finally:
        capi.set_jit_cache(None)


@pytest.mark.gpu
def test_settle_count_restarts_with_the_scene_and_the_spec(gpu, fixtures):
    """the count of samples at rest (threshold 2 here) restarts at sail_set_scene and at a switch that changes the types
    spec, and a partition that leaves the spec alone leaves the value kernel: told by the build id of each launch"""
    sc = fixtures["scenes"]["C1"]
    inv, seeds = _schedule(sc, 3)
    one = (inv[:1], seeds[:1], sc["eye"], B)
    _, _, tinfo = _render(sc, -1, spp=1)
    _, _, tinfo16 = _render(sc, -1, spp=1, debug={capi.DEBUG_JIT_NS: 16})
    types_id, types16_id = tinfo["build_id"], tinfo16["build_id"]
    assert types_id != types16_id

    def settle(ctx, want_types):
        """two launches on the types kernel (the second crosses the threshold), then the value kernel"""
        for _ in range(2):
            ctx.render_schedule(*one)
            assert ctx.kernel_info()["build_id"] == want_types
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(*one)
        vid = ctx.kernel_info()["build_id"]
        assert vid not in (types_id, types16_id)
        return vid

    ctx = capi.Context(W, H, debug={AFTER: 2})
    try:
        ctx.set_scene_dict(sc)
        first = settle(ctx, types_id)
        ctx.set_scene_dict(sc)                    # the same rows again: the count restarts all the same
        assert settle(ctx, types_id) == first
        ctx.set_partition(0, 8, capi.PART_TILES)  # this frame is one tile: the spec stays, and so does the value kernel
        ctx.render_schedule(*one)
        assert ctx.kernel_info()["build_id"] == first
        ctx.set_partition(0, 1, capi.PART_TILES)
        ctx.set_debug(capi.DEBUG_JIT_NS, 16)      # another types spec: its own count, its own value kernel
        second = settle(ctx, types16_id)
        assert second != first
        ctx.reset()                               # not a change of the rows
        ctx.render_schedule(*one)
        assert ctx.kernel_info()["build_id"] == second
        assert capi.jit_resident() == (1, 1)
    finally:
        ctx.close()
    assert capi.jit_resident() == (0, 0)


# ---- 7. the default threshold keeps few-sample renders from compiling ---------------------------------------------------
@pytest.mark.gpu
def test_default_threshold_three_samples_compile_nothing_more(gpu, fixtures, tmp_path):
    r = _rows(fixtures)
    sc = _variant(fixtures, rows=r[[SPHERE, CUBE, CORNELL]])  # a row order no other test and no shipped cache has
    inv, seeds = _schedule(sc, 3)
    cache = str(tmp_path / "jit")
    capi.set_jit_cache(cache)
    try:
        ids = {}
        for after in (256, -1):
            ctx = capi.Context(W, H, debug={AFTER: after})
            try:
                ctx.set_scene_dict(sc)
                ctx.render_schedule(inv, seeds, sc["eye"], B)
                got = ctx.read_accum()
                # A value kernel asked for too early would still be compiling now, and its object would go to the
                # directory beside the cache: wait for the best tier asked for (were it the value kernel, this would
                # wait for its build and the object would exist), then look at what the next launch runs and at both
                # directories.
                assert ctx.kernel_ready(-1)
                ctx.render_schedule(inv[:1], seeds[:1], sc["eye"], B)
                ids[after] = ctx.kernel_info()
                assert capi.jit_resident() == (0, 0)
            finally:
                ctx.close()
            assert bit_equal(got, _want(sc, inv, seeds)).all()
    finally:
        capi.set_jit_cache(None)
    assert ids[256]["name"].startswith("sail_trace_kernel_jit"), ids
    assert ids[256]["build_id"] == ids[-1]["build_id"] == ids[256]["jit_build_id"], ids
    assert len(os.listdir(cache)) == 1, os.listdir(cache)
    values = str(tmp_path / "jit-values")
    assert not os.path.exists(values) or os.listdir(values) == [], os.listdir(values)


# ---- 8. a swap between two launches of one frame ------------------------------------------------------------------------
@pytest.mark.gpu
def test_swap_between_two_launches_of_one_frame(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    inv, seeds = _schedule(sc, 4)
    _, _, tinfo = _render(sc, -1, spp=1)
    ctx = capi.Context(W, H, debug={AFTER: 2})
    try:
        ctx.set_scene_dict(sc)
        ctx.set_launch_samples(2)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        info = ctx.kernel_info()
        st = ctx.stats()
        got = ctx.read_accum()
    finally:
        ctx.close()
    assert st.launches == 2
    assert info["build_id"] != tinfo["build_id"] and info["build_id"] == info["jit_build_id"], (info, tinfo)
    assert bit_equal(got, _want(sc, inv, seeds)).all()


# ---- 9. around the context ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scene_change_partition_and_multi_device(gpu, fixtures):
    sc, c3 = fixtures["scenes"]["C1"], fixtures["scenes"]["C3"]
    inv, seeds = _schedule(sc, 3)
    inv3, seeds3 = _schedule(c3, 3)
    want = _want(sc, inv, seeds)
    _, _, tinfo = _render(sc, -1, spp=1)
    ctx = capi.Context(W, H, debug={AFTER: 0})
    try:
        ctx.set_scene_dict(sc)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        first = ctx.kernel_info()["build_id"]
        assert first != tinfo["build_id"]
        assert bit_equal(ctx.read_accum(), want).all()
        # another scene (the room form: types-only) and back
        ctx.set_scene_dict(c3)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv3, seeds3, c3["eye"], B)
        assert bit_equal(ctx.read_accum(), _want(c3, inv3, seeds3)).all()
        ctx.set_scene_dict(sc)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == first
        assert bit_equal(ctx.read_accum(), want).all()
        # a rank of 8 and back (this frame is one tile: rank 0 owns it)
        ctx.set_partition(0, 8, capi.PART_TILES)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        assert ctx.kernel_info()["build_id"] != tinfo["build_id"]
        assert bit_equal(ctx.read_accum(), want).all()
        ctx.set_partition(0, 1, capi.PART_TILES)
        assert ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        assert ctx.kernel_info()["build_id"] == first
        assert bit_equal(ctx.read_accum(), want).all()
    finally:
        ctx.close()
    # one context over the same device twice: its sub-contexts derive their own value kernels
    got, _, info = _render(sc, 0, spp=3, devices=[0, 0])
    assert info["build_id"] == first, info
    assert bit_equal(got, want).all()
