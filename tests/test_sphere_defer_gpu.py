"""The deferred Sphere row on the GPU (SAIL_JIT_ROWDEFER in sail_geom.h / sail_trace.hip; SAIL_DEBUG_JIT bit 64 takes it
out). At the bounces that sort their paths and are not the last, the value kernel's sweep runs only the head of the
sphere's test; a ray whose discriminant is not negative (and that does not start outside the sphere moving away) is sorted
under the sphere's key with its winner among the other rows, and the sphere's waves run the root solve and the slab test
after the gather. Every frame here is compared bit for bit (raw uint32: a NaN equals only the same NaN) with the CPU
oracle and with the switch-off arm's frame, and the two arms' build ids differ wherever the scene has a sphere, so the new
code demonstrably ran. The shapes are those of tests/test_gpu_row_shading.py: 37 x 21 pixels (ragged blocks), 7 samples (no
multiple of the 16 in flight), 6 bounces (bounces 2..5 defer). C1's rows: 0 the light (a Cube), 1 the Cornellbox, 2 the
sphere (a mirror). Needs a GPU."""
import numpy as np
import pytest

import oracle
from sail_amd import capi

W, H, SPP, B = 37, 21, 7, 6
AFTER = capi.DEBUG_JIT_VALUES_AFTER
ON, OFF = 59, 59 | capi.JIT_NO_ROWDEFER
CUBE, CORNELL, SPHERE = 0, 1, 2  # C1's rows
MATROW_SPHERE, EMISSION_SPHERE = 6, slice(8, 11)  # where a sphere row keeps them (sail_capi.cpp decodePrims)


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.view(np.uint32) == b.view(np.uint32)


def _f32(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def _rows(fixtures):
    sc = fixtures["scenes"]["C1"]
    return np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18).copy()


def _variant(fixtures, rows):
    sc = dict(fixtures["scenes"]["C1"])
    rows = np.asarray(rows, np.float32)
    sc["n"] = int(rows.shape[0])
    sc["objects"] = rows.reshape(-1).copy()
    return sc


def _two_spheres(fixtures):
    r = _rows(fixtures)
    a, b = r[SPHERE].copy(), r[SPHERE].copy()
    a[1:5] = (1.6, 1.0, 2.2, 0.9)
    b[1:5] = (3.9, 3.6, 1.4, 0.8)
    b[MATROW_SPHERE] = 0.0                 # matte
    b[EMISSION_SPHERE] = (6.0, 5.0, 4.0)   # a light
    return r, a, b


def row_variant(fixtures, which):
    """the row variants of C1 that the tests below render (tests/parity_cases.py lists them by these names)"""
    r = _rows(fixtures)
    if which in ("sphere_row0", "sphere_row1"):
        return _variant(fixtures, r[[SPHERE, CUBE, CORNELL] if which == "sphere_row0" else [CUBE, SPHERE, CORNELL]])
    if which == "no_cornellbox":
        return _variant(fixtures, r[[CUBE, SPHERE]])
    if which == "around_the_eye_and_the_box":
        r[SPHERE][1:5] = (2.78, 2.73, 0.0, 40.0)
    elif which == "half_through_the_floor":
        r[SPHERE][2] = 0.0  # centre y: the floor
    elif which == "half_behind_the_light":  # the light is the slab x 2.13..3.43, y 5.487..5.488, z 2.27..3.32 under the ceiling
        r[SPHERE][1:5] = (2.78, 5.3, 2.8, 0.45)
    elif which in ("two_spheres_mirror", "two_spheres_emitter", "four_rows"):
        r, a, b = _two_spheres(fixtures)
        rows = {"two_spheres_mirror": [a, r[CORNELL], b], "two_spheres_emitter": [b, r[CORNELL], a],
                "four_rows": [r[CUBE], r[CORNELL], a, b]}[which]
        return _variant(fixtures, np.stack(rows))
    elif which == "radius_zero":
        r[SPHERE][4] = 0.0
    elif which == "radius_nan":
        r[SPHERE][4] = _f32(0x7fc00abc)
    elif which == "centre_inf":
        r[SPHERE][1] = np.inf
    else:
        raise KeyError(which)
    return _variant(fixtures, r)


ROW_VARIANTS = ["sphere_row0", "sphere_row1", "no_cornellbox", "around_the_eye_and_the_box", "half_through_the_floor",
                "half_behind_the_light", "two_spheres_mirror", "two_spheres_emitter", "four_rows", "radius_zero", "radius_nan",
                "centre_inf"]


def _schedule(sc, w=W, h=H):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, SPP)


def _want(sc, bounces=B, mode=capi.ACCUM_SUM, aov=False, w=W, h=H):
    inv, seeds = _schedule(sc, w, h)
    return oracle.render(sc, capi.plugin_masks(sc["plugins"]), w, h, inv, seeds, sc["eye"], bounces, accum_mode=mode, aov=aov)


def _render(sc, jit, bounces=B, mode=capi.ACCUM_SUM, aov=False, debug=None, w=W, h=H, mask=None):
    """(accumulator, AOVs or None, kernel info) of a context that waited for its value kernel"""
    inv, seeds = _schedule(sc, w, h)
    ctx = capi.Context(w, h, flags=capi.FLAG_AOV if aov else 0, debug={capi.DEBUG_JIT: jit, AFTER: 0, **(debug or {})})
    try:
        ctx.set_scene_dict(sc)
        if mode != capi.ACCUM_SUM:
            ctx.set_accum_mode(mode)
        if mask is not None:
            ctx.set_active_tiles(mask)
        ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], bounces)
        got = ctx.read_accum()
        aovs = ctx.readback(aov=True)[1:] if aov else None
        return got, aovs, ctx.kernel_info()
    finally:
        ctx.close()


def _defer(sc, jit=ON):
    _, defs = capi.jit_value_key(sc, jit=jit)
    return "#define SAIL_JIT_ROWDEFER" in defs


def _check_arms(sc, bounces=B, deferred=True, **kw):
    """both arms render the oracle's frame with their value kernels, which are two kernels exactly when a row is deferred"""
    assert _defer(sc) == deferred and not _defer(sc, OFF)
    want = _want(sc, bounces=bounces)
    on, _, ion = _render(sc, ON, bounces=bounces, **kw)
    off, _, ioff = _render(sc, OFF, bounces=bounces, **kw)
    for info in (ion, ioff):
        assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    assert (ion["build_id"] != ioff["build_id"]) == deferred, (ion, ioff)
    bad_on, bad_off = int((~same_bits(on, want)).sum()), int((~same_bits(off, want)).sum())
    print(f"channels differing from the oracle: on {bad_on}, off {bad_off}")
    assert bad_on == 0 and bad_off == 0
    assert same_bits(on, off).all()
    return on


# ---- 1. C1 as it is, with AOVs, in each accumulation mode ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [capi.ACCUM_SUM, capi.ACCUM_MIX, capi.ACCUM_COMPAT8])
def test_c1_with_aovs(gpu, fixtures, mode):
    sc = fixtures["scenes"]["C1"]
    assert _defer(sc)
    want, wn, wp = _want(sc, mode=mode, aov=True)
    on, (gn, gp), ion = _render(sc, ON, mode=mode, aov=True)
    off, (fn, fp), ioff = _render(sc, OFF, mode=mode, aov=True)
    assert ion["build_id"] != ioff["build_id"] and ion["build_id"] == ion["jit_build_id"], (ion, ioff)
    assert same_bits(on, want).all() and same_bits(gn, wn).all() and same_bits(gp, wp).all()
    assert same_bits(off, want).all() and same_bits(fn, wn).all() and same_bits(fp, wp).all()


# ---- 2. bounce counts: no bounce defers at 1 and 2; at 3 bounce 2 alone ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2, 3])
def test_bounce_counts(gpu, fixtures, bounces):
    _check_arms(fixtures["scenes"]["C1"], bounces=bounces)


# ---- 3. the sphere's row index: the tie rule (t == best and the lower row) from both sides -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sphere_row0", "sphere_row1"])
def test_row_order(gpu, fixtures, order):
    _check_arms(row_variant(fixtures, order))


# ---- 4. candidates whose provisional result is a miss --------------------------------------------------------------------
@pytest.mark.gpu
def test_no_cornellbox(gpu, fixtures):
    """the light cube and the sphere alone, seen from outside: a candidate that misses the sphere after all has no winner
    and ends after the gather; one that hits it goes on from a provisional miss"""
    on = _check_arms(row_variant(fixtures, "no_cornellbox"))
    assert (on[..., :3] != 0).any()  # the mirror shows the light


# ---- 5. candidates that resolve to the provisional row ------------------------------------------------------------------
@pytest.mark.gpu
def test_sphere_around_the_eye_and_the_box(gpu, fixtures):
    """every ray starts inside (cc < 0, t1 < kEps) and is a candidate; the box is nearer everywhere"""
    _check_arms(row_variant(fixtures, "around_the_eye_and_the_box"))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["half_through_the_floor", "half_behind_the_light"])
def test_sphere_partly_hidden(gpu, fixtures, where):
    _check_arms(row_variant(fixtures, where))


# ---- 6. more than one sphere: the first is deferred, the second tested in the sweep --------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["mirror", "emitter"])  # which of the two is deferred; the other is tested in the sweep
def test_two_spheres_with_the_box(gpu, fixtures, first):
    _check_arms(row_variant(fixtures, "two_spheres_" + first))


@pytest.mark.gpu
def test_four_rows(gpu, fixtures):
    """above kRowRecordMax: no row-shading form, one generic record; the deferral rides on the value kernel all the same"""
    sc = row_variant(fixtures, "four_rows")
    assert "SAIL_JIT_ROWSHADE" not in capi.jit_value_key(sc, jit=ON)[1]
    _check_arms(sc)


# ---- 7. degenerate sphere rows: the oracle decides what the frame is ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["radius_zero", "radius_nan", "centre_inf"])
def test_degenerate_sphere(gpu, fixtures, what):
    _check_arms(row_variant(fixtures, what))


# ---- 8. the other instances of the kernel --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("debug", [{capi.DEBUG_JIT_NS: 1}, {capi.DEBUG_SAMPLE_GROUPS: 3}, {capi.DEBUG_JIT_NS: 16}],
                         ids=["one_sample_in_flight", "sample_groups", "sixteen_in_flight"])
def test_other_instances(gpu, fixtures, debug):
    _check_arms(fixtures["scenes"]["C1"], debug=debug)


@pytest.mark.gpu
def test_under_a_tile_mask(gpu, fixtures):
    """the masked twin: 70 x 21 is two 64 x 64 tiles, the ragged second one alone traced"""
    sc = fixtures["scenes"]["C1"]
    w = 70
    mask = np.array([[0, 1]], np.uint8)
    want = _want(sc, w=w)
    on, _, ion = _render(sc, ON, w=w, mask=mask)
    off, _, ioff = _render(sc, OFF, w=w, mask=mask)
    # (build_id is the masked twin's, a module of its own; jit_build_id its unmasked base's)
    assert ion["name"].startswith("sail_trace_kernel_jit") and ioff["name"].startswith("sail_trace_kernel_jit"), (ion, ioff)
    assert ion["build_id"] != ioff["build_id"] and ion["jit_build_id"] != ioff["jit_build_id"], (ion, ioff)
    assert ion["build_id"] != ion["jit_build_id"], ion
    assert same_bits(on[:, 64:], want[:, 64:]).all() and same_bits(off, on).all()
    assert not on[:, :64].view(np.uint32).any()  # the frozen tile was not traced
