"""The directed branch scenes (tests/golden/branch_scenes.json) on the GPU. Each scene drives paths through outcomes of
the path code that no other parity scene takes (tests/test_oracle_branch_coverage.py measures that on the CPU and
shows that the scene's frame depends on them): the early returns where a BSDF hands back zero with pdf 0, half vectors
turned over, glass with one smooth axis, masked-out category words, the roots beyond MAX_DISTANCE, the sphere's pole.

Every frame is compared with the CPU oracle by raw uint32 (test_fuzz_scenes.bit_equal: a NaN equals only the same NaN,
but for the default NaN's sign): accumulator, normal and position AOV maps, and the exact segment count. Forms: the
precompiled kernels of test_fuzz_scenes.FORMS; the run-time kernel compiled for the scene's rows; for the Cornell-set
scenes the value kernel with row shading, with the sphere deferred and not; a masked launch; launches of 2 samples;
2 sample groups. Needs a GPU."""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from sail_amd import capi
from test_fuzz_scenes import FORMS, bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "branch_scenes.json")) as _f:
    SCENES = json.load(_f)
NAMES = sorted(SCENES)
AFTER = capi.DEBUG_JIT_VALUES_AFTER
VALUES_ON, VALUES_OFF = 59, 59 | capi.JIT_NO_ROWDEFER


def _cornell_set(s):
    p = s["plugins"]
    return (set(p["shape"]) <= {"cube", "sphere", "cornellbox"} and set(p["material"]) <= {"matte", "mirror"}
            and not p["texture"] and s["ln"] == 0)


CORNELL = [n for n in NAMES if _cornell_set(SCENES[n])]


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def _schedule(sc):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), sc["W"], sc["H"], 0, sc["spp"])


@functools.lru_cache(maxsize=None)
def want(name):
    """the oracle's frame, AOV maps and segment count: computed once per scene, shared, never written"""
    sc = SCENES[name]
    inv, seeds = _schedule(sc)
    oracle.reset_counters()
    acc, an, ap = oracle.render(sc, capi.plugin_masks(sc["plugins"]), sc["W"], sc["H"], inv, seeds, sc["eye"], sc["bounces"],
                                aov=True)
    segs, _ = oracle.counters()
    for a in (acc, an, ap):
        a.setflags(write=False)
    return acc, an, ap, segs


def render(name, debug, launch=3, wait=False, mask=None):
    sc = SCENES[name]
    inv, seeds = _schedule(sc)
    ctx = capi.Context(sc["W"], sc["H"], flags=capi.FLAG_AOV | capi.FLAG_SEGMENT_COUNT, debug=debug)
    try:
        ctx.set_scene_dict(sc)
        ctx.set_launch_samples(launch)
        if mask is not None:
            ctx.set_active_tiles(mask)
        if wait:
            ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], sc["bounces"])
        acc = ctx.read_accum()
        _, an, ap = ctx.readback(aov=True)
        return acc, an, ap, ctx.stats(), ctx.kernel_info()
    finally:
        ctx.close()


def check(name, got):
    acc, an, ap, st, info = got
    wacc, wn, wp, segs = want(name)
    bad = int((~bit_equal(acc, wacc)).sum())
    bad_n, bad_p = int((~bit_equal(an, wn)).sum()), int((~bit_equal(ap, wp)).sum())
    sign_only = sum(int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum())
                    for g, w in ((acc, wacc), (an, wn), (ap, wp))) - bad - bad_n - bad_p
    print(f"{name} ({info['name']}): channels differing from the oracle: accumulator {bad}, normal {bad_n}, position {bad_p} "
          f"(default NaNs of the other sign: {sign_only}); segments {st.segments} (oracle {segs})")
    assert bad == 0, f"{name} ({info['name']}): {bad} of {acc.size} channels differ"
    assert bad_n == 0 and bad_p == 0, info["name"]
    assert st.segments == segs, info["name"]


def test_some_scenes_are_cornell_set():
    """(cube + sphere + Cornellbox, matte and mirror, no light rows: the value kernel, row shading, the deferred sphere)"""
    assert len(CORNELL) >= 4 and sum(SCENES[n]["n"] <= 3 for n in CORNELL) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_precompiled_forms(gpu, name, form):
    got = render(name, FORMS[form])
    assert not got[4]["name"].startswith("sail_trace_kernel_jit") and "cull_jit" not in got[4]["name"], got[4]
    check(name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_run_time_kernel_for_the_rows(gpu, name):
    """the kernel hipRTC compiles for the scene's rows or, from 8 rows on, for its plugin set, in the flat form"""
    debug = {capi.DEBUG_JIT: 27}
    if SCENES[name]["n"] >= 8:  # the pre-cull form's threshold
        debug[capi.DEBUG_CULL_MIN_PRIMS] = 1000
    got = render(name, debug, wait=True)
    info = got[4]
    assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    check(name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [VALUES_ON, VALUES_OFF], ids=["deferred", "not_deferred"])
@pytest.mark.parametrize("name", CORNELL)
def test_value_kernel_with_row_shading(gpu, name, jit):
    got = render(name, {capi.DEBUG_JIT: jit, AFTER: 0}, wait=True)
    info = got[4]
    assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    check(name, got)


@pytest.mark.gpu
def test_value_kernel_arms_are_two_kernels(gpu):
    """where the scene has a sphere row, the deferred and the not deferred arm are different builds: both ran"""
    name = "graze_lambert"
    on = render(name, {capi.DEBUG_JIT: VALUES_ON, AFTER: 0}, wait=True)[4]
    off = render(name, {capi.DEBUG_JIT: VALUES_OFF, AFTER: 0}, wait=True)[4]
    assert on["build_id"] != off["build_id"], (on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["graze_oren_nayar", "metal_flip"])
def test_masked_launch(gpu, name):
    """under a tile mask (the frame is one 64 x 64 tile, active): the masked twin of the scene's kernel"""
    check(name, render(name, {}, mask=np.array([[1]], np.uint8), wait=True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_launches_of_two_samples(gpu, name):
    check(name, render(name, {}, launch=2, wait=True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_two_sample_groups(gpu, name):
    check(name, render(name, {capi.DEBUG_SAMPLE_GROUPS: 2}, wait=True))
