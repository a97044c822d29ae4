"""Row shading on the GPU (SAIL_JIT_ROWSHADE in sail_geom.h, SAIL_DEBUG_JIT bit 32): in the value kernel of a scene
of at most three rows, a wave whose paths all hit one quiet row runs the rest of the bounce in that row's branch of the
hit record, on the row's material constants, and neither loads nor stores the radiance. Every frame here is compared
bit for bit (raw uint32: a NaN equals only the same NaN) with the CPU oracle and with the switch-off arm's frame, and the
two arms' build ids differ wherever a row has a copy, so the new code demonstrably ran. The shapes are those of
tests/test_gpu_jit_values.py: 37 x 21 pixels (ragged blocks), 7 samples (no multiple of the 16 in flight), 6 bounces.
C1's rows: 0 the light (a Cube, matte, emitting: never quiet), 1 the Cornellbox (matte, quiet), 2 the sphere (mirror,
quiet): the shipped mask is 6. Needs a GPU."""
import json
import os
import re

import numpy as np
import pytest

import oracle
from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, B = 37, 21, 7, 6
AFTER = capi.DEBUG_JIT_VALUES_AFTER
ON, OFF = 59, 27  # SAIL_DEBUG_JIT with and without bit 32
CUBE, CORNELL, SPHERE = 0, 1, 2  # C1's rows
MATTE, MIRROR, METAL = 1.0, 2.0, 3.0  # material categories (texParams column 0)
# where a row of each shape keeps its material row and its emission (sail_capi.cpp decodePrims); the Cornellbox has no
# emission slot: the decoder gives it none
MATROW = {CUBE: 8, CORNELL: 7, SPHERE: 6}
EMISSION = {CUBE: slice(10, 13), SPHERE: slice(8, 11)}


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


def _tp(fixtures):
    sc = fixtures["scenes"]["C1"]
    return np.asarray(sc["texparams"], np.float32).reshape(sc["tn"], 16).copy()


def _variant(fixtures, rows=None, tp=None):
    sc = dict(fixtures["scenes"]["C1"])
    if rows is not None:
        rows = np.asarray(rows, np.float32)
        sc["n"] = int(rows.shape[0])
        sc["objects"] = rows.reshape(-1).copy()
    if tp is not None:
        sc["texparams"] = np.asarray(tp, np.float32).reshape(-1).copy()
    return sc


def _schedule(sc, spp=SPP):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), W, H, 0, spp)


def _want(sc, bounces=B, mode=capi.ACCUM_SUM, aov=False):
    inv, seeds = _schedule(sc)
    return oracle.render(sc, capi.plugin_masks(sc["plugins"]), W, H, inv, seeds, sc["eye"], bounces, accum_mode=mode, aov=aov)


def _render(sc, jit, after=0, bounces=B, mode=capi.ACCUM_SUM, aov=False, debug=None):
    """(accumulator, AOVs or None, kernel info) of a context that waited for the best tier it asked for"""
    inv, seeds = _schedule(sc)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV if aov else 0, debug={capi.DEBUG_JIT: jit, AFTER: after, **(debug or {})})
    try:
        ctx.set_scene_dict(sc)
        if mode != capi.ACCUM_SUM:
            ctx.set_accum_mode(mode)
        ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], bounces)
        got = ctx.read_accum()
        aovs = ctx.readback(aov=True)[1:] if aov else None
        return got, aovs, ctx.kernel_info()
    finally:
        ctx.close()


def _mask(sc, jit=ON):
    """(rows with a shading copy, quiet rows among them) of the value kernel's source prefix, None without the define"""
    _, defs = capi.jit_value_key(sc, jit=jit)
    m = re.search(r"#define SAIL_JIT_ROWSHADE (\d+)\n#define SAIL_JIT_ROWQUIET (\d+)\n", defs)
    return (int(m.group(1)), int(m.group(2))) if m else None


def _check_arms(sc, mask, bounces=B, **kw):
    """both arms render the oracle's frame; the arms are two kernels exactly when some row has a copy of its own"""
    assert _mask(sc) == (mask, mask) and _mask(sc, OFF) is None
    want = _want(sc, bounces=bounces)
    on, _, ion = _render(sc, ON, bounces=bounces, **kw)
    off, _, ioff = _render(sc, OFF, bounces=bounces, **kw)
    for info in (ion, ioff):
        assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    assert (ion["build_id"] != ioff["build_id"]) == (mask != 0), (mask, ion, ioff)
    bad_on, bad_off = int((~same_bits(on, want)).sum()), int((~same_bits(off, want)).sum())
    print(f"mask {mask}: channels differing from the oracle: on {bad_on}, off {bad_off}")
    assert bad_on == 0 and bad_off == 0
    assert same_bits(on, off).all()
    return ion, ioff


# ---- 1. C1 as shipped: samples in flight, sample groups, accumulation modes, with AOVs ---------------------------------
_REF = {}


def _ref(fixtures, mode):
    if mode not in _REF:  # computed once per mode, shared, never written
        _REF[mode] = _want(fixtures["scenes"]["C1"], mode=mode, aov=True)
    return _REF[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [16, 1])
@pytest.mark.parametrize("groups", [0, 3])
@pytest.mark.parametrize("mode", [capi.ACCUM_SUM, capi.ACCUM_MIX])
def test_c1_as_shipped(gpu, fixtures, mode, groups, ns):
    sc = fixtures["scenes"]["C1"]
    assert _mask(sc) == (6, 6)
    dbg = {capi.DEBUG_SAMPLE_GROUPS: groups, capi.DEBUG_JIT_NS: ns}
    want, wn, wp = _ref(fixtures, mode)
    on, (gn, gp), ion = _render(sc, ON, mode=mode, aov=True, debug=dbg)
    off, (fn, fp), ioff = _render(sc, OFF, mode=mode, aov=True, debug=dbg)
    _, _, itypes = _render(sc, ON, after=-1, mode=mode, aov=True, debug=dbg)
    assert ion["name"] == "sail_trace_kernel_jit" + ("_grouped" if groups or ns == 1 else ""), ion
    assert len({ion["build_id"], ioff["build_id"], itypes["build_id"]}) == 3, (ion, ioff, itypes)
    assert same_bits(on, want).all() and same_bits(gn, wn).all() and same_bits(gp, wp).all()
    assert same_bits(off, want).all() and same_bits(fn, wn).all() and same_bits(fp, wp).all()


# ---- 2. bounce counts: shadeLast, the quiet-row exit and lastSkipSort in a row's copy; the AOV sample at a last bounce ---
@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2, 3])
def test_bounce_counts(gpu, fixtures, bounces):
    sc = fixtures["scenes"]["C1"]
    want, wn, wp = _want(sc, bounces=bounces, aov=True)
    on, (gn, gp), ion = _render(sc, ON, bounces=bounces, aov=True)
    off, _, ioff = _render(sc, OFF, bounces=bounces, aov=True)
    assert ion["build_id"] != ioff["build_id"]
    assert same_bits(on, want).all() and same_bits(gn, wn).all() and same_bits(gp, wp).all()
    assert same_bits(off, want).all()


# ---- 3. per-row material edges, one row changed at a time ---------------------------------------------------------------
def _oren_nayar(tp, m, sigma=0.5):
    """texParams row m as a matte of roughness sigma (kd kept; A and B as bsdf.glsl's Oren-Nayar takes them)"""
    s2 = np.float32(sigma) * np.float32(sigma)
    tp[m][0] = MATTE
    tp[m][2] = sigma
    tp[m][3] = np.float32(1.0) - s2 / (np.float32(2.0) * (s2 + np.float32(0.33)))
    tp[m][4] = np.float32(0.45) * s2 / (s2 + np.float32(0.09))


def _edge(fixtures, row, what):
    """(scene, rows expected to keep a quiet copy)"""
    r, tp = _rows(fixtures), _tp(fixtures)
    # the light and the box share material row 0: the changed row gets a material row of its own (3, which no row of C1
    # uses: the box's slots 8 and 9 are not read, its material row is slot 7)
    m = 3
    assert not tp[m].any() and m not in [int(r[q][MATROW[q]]) for q in (CUBE, CORNELL, SPHERE)]
    tp[m] = tp[int(r[row][MATROW[row]])]
    r[row][MATROW[row]] = m
    quiet = {CORNELL, SPHERE}
    if what == "oren_nayar":
        _oren_nayar(tp, m)
        quiet.discard(row)  # f needs the sampled direction
    elif what == "kd_zero":       # the sphere's is its mirror's kr
        tp[m][1] = 0.0
    elif what == "kd_inf":
        tp[m][1] = np.inf
        if row == CORNELL:        # inf * the black wall's 0: f is not finite
            quiet.discard(row)
    elif what == "kd_nan":
        tp[m][1] = _f32(0x7fc00abc)
        if row == CORNELL:
            quiet.discard(row)
    elif what in ("emission_neg_zero", "emission_nan", "emission_nonzero"):
        v = {"emission_neg_zero": _f32(0x80000000), "emission_nan": _f32(0x7fc01234), "emission_nonzero": np.float32(3.0)}[what]
        if row == CORNELL:
            r[row][10:13] = v     # a Cube's emission slots: the decoder reads none for the box, the frame is C1's
        else:
            r[row][EMISSION[row]] = v
            quiet.discard(row)    # the words are not +0
    elif what == "absent_category":
        tp[m][0] = METAL          # not in C1's material plugins: material() returns 0
    else:
        raise KeyError(what)
    return _variant(fixtures, rows=r, tp=tp), sum(1 << q for q in quiet)


_EDGES = [(row, what) for row in (CORNELL, CUBE, SPHERE)
          for what in ("oren_nayar", "kd_zero", "kd_inf", "kd_nan", "emission_neg_zero", "emission_nan")]
_EDGES += [(CORNELL, "emission_nonzero"), (CORNELL, "absent_category"), (SPHERE, "absent_category")]


@pytest.mark.gpu
@pytest.mark.parametrize("row,what", _EDGES, ids=[f"{['cube', 'box', 'sphere'][r]}-{w}" for r, w in _EDGES])
def test_row_material_edges(gpu, fixtures, row, what):
    """(sphere-kd_zero is the mirror with kr = 0)"""
    sc, mask = _edge(fixtures, row, what)
    _check_arms(sc, mask)


def row_variant(fixtures, which):
    """the row variants of the three tests below (tests/parity_cases.py lists them by these names)"""
    r = _rows(fixtures)
    if which == "cube_reversed":
        r[CUBE][7] = 1.0  # rev
    elif which == "categories_swapped":
        r[SPHERE][MATROW[SPHERE]], r[CUBE][MATROW[CUBE]] = r[CUBE][MATROW[CUBE]], r[SPHERE][MATROW[SPHERE]]
    elif which == "two_spheres":
        a, b = r[SPHERE].copy(), r[SPHERE].copy()
        a[1:5] = (1.6, 1.0, 2.2, 0.9)
        b[1:5] = (3.9, 3.6, 1.4, 0.8)
        b[MATROW[SPHERE]] = 0.0              # matte
        b[EMISSION[SPHERE]] = (6.0, 5.0, 4.0)  # the light
        return _variant(fixtures, rows=np.stack([a, r[CORNELL], b]))
    else:
        raise KeyError(which)
    return _variant(fixtures, rows=r)


ROW_VARIANTS = ["cube_reversed", "categories_swapped", "two_spheres"]


@pytest.mark.gpu
def test_cube_reversed(gpu, fixtures):
    _check_arms(row_variant(fixtures, "cube_reversed"), 6)


@pytest.mark.gpu
def test_categories_swapped(gpu, fixtures):
    """the sphere a matte (the light's material row), the light cube a mirror (the sphere's)"""
    _check_arms(row_variant(fixtures, "categories_swapped"), 6)


# ---- 4. two rows of one type with different materials must not share a copy -------------------------------------------
@pytest.mark.gpu
def test_two_spheres_one_mirror_one_emitting_matte(gpu, fixtures):
    _check_arms(row_variant(fixtures, "two_spheres"), 3)


# ---- 5. above kRowRecordMax: no row-shading form, and the value tier still loads -----------------------------------------
def _more_rows(fixtures, spheres, cubes):
    r = _rows(fixtures)
    out = [r[CUBE], r[CORNELL]]
    for i in range(spheres):
        s = r[SPHERE].copy()
        s[1:5] = (1.0 + 1.3 * i, 0.8 + 0.9 * i, 1.5 + 1.1 * i, 0.7 - 0.12 * i)
        s[6] = 4.0 if i % 2 == 0 else 0.0
        out.append(s)
    for i in range(cubes):
        c = r[CUBE].copy()
        c[1:4] = (3.6 + 0.35 * i, 0.0, 0.4 + 1.2 * i)
        c[4:7] = (4.6 + 0.2 * i, 1.1 + 0.5 * i, 1.3 + 1.2 * i)
        c[10:13] = (0.0, 0.0, 0.0) if i % 2 == 0 else (0.5, 0.25, 2.0)
        out.append(c)
    return _variant(fixtures, rows=np.stack(out))


@pytest.mark.gpu
@pytest.mark.parametrize("spheres,cubes", [(2, 0), (1, 2)])  # 4 and 5 rows
def test_more_rows_than_records(gpu, fixtures, spheres, cubes):
    sc = _more_rows(fixtures, spheres, cubes)
    assert sc["n"] == 2 + spheres + cubes > 3
    assert _mask(sc) is None and capi.jit_value_key(sc, jit=ON) == capi.jit_value_key(sc, jit=OFF)
    want = _want(sc)
    on, _, ion = _render(sc, ON)
    _, _, ioff = _render(sc, OFF)
    _, _, itypes = _render(sc, ON, after=-1)
    assert ion["build_id"] == ioff["build_id"] == ion["jit_build_id"] != itypes["build_id"], (ion, ioff, itypes)
    assert same_bits(on, want).all()


# ---- 6. the quiet classification: a light plugin in the set (the word flips are cases of 3.) ----------------------------
@pytest.mark.gpu
def test_scene_with_a_light_plugin_has_no_quiet_rows(gpu):
    """A scene with a light plugin is outside the Cornell set: no value kernel, so no row-shading form, under either
    switch (its matte rows are lit: none could be quiet). 3 rows with a light row, compiled in the flat form for rows."""
    with open(os.path.join(ROOT, "tests", "golden", "fuzz_scenes.json")) as f:
        sc = json.load(f)["F01"]
    assert sc["n"] <= 3 and sc["ln"] >= 1
    flat = 1 + 2 + 16  # the plain flat form, compiled for the rows
    assert capi.jit_value_key(sc, jit=flat + 32)[0] is None
    inv, seeds = _schedule(sc, 3)
    want = oracle.render(sc, capi.plugin_masks(sc["plugins"]), W, H, inv, seeds, sc["eye"], B)
    ids = []
    for jit in (flat + 32, flat):
        ctx = capi.Context(W, H, debug={capi.DEBUG_JIT: jit, AFTER: 0})
        try:
            ctx.set_scene_dict(sc)
            ctx.kernel_ready(-1)
            ctx.render_schedule(inv, seeds, sc["eye"], B)
            assert same_bits(ctx.read_accum(), want).all(), jit
            ids.append(ctx.kernel_info()["build_id"])
        finally:
            ctx.close()
    assert ids[0] == ids[1]
