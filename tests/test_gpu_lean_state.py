"""Lanes past the live range after a path sort (traceTileCompact in sail_trace.hip). In the flat forms every lane reads
and unpacks the packed path state of its sorted slot after a sort, whether a path landed there or not: a lane with
li >= nAlive reads a slot nobody wrote this bounce, and nothing may depend on what it read. The path carries origin and
direction alone; the reciprocals of a direction are built where the segment is swept. The closed benchmark scenes keep
most paths alive for most bounces, so these scenes are open: with the room row taken out most paths leave at bounce 1
or 2, the live count falls far below the workgroup from the first sort on, and whole waves go dead. Every frame is
compared bit for bit (raw uint32: a NaN equals only the same NaN) with the CPU oracle. The shapes are those of
tests/test_sphere_defer_gpu.py: 37 x 21 pixels (ragged blocks), 7 samples (no multiple of the 16 in flight), 6 bounces.
Needs a GPU."""
import numpy as np
import pytest

import oracle
from sail_amd import capi

W, H, SPP, B = 37, 21, 7, 6
AFTER = capi.DEBUG_JIT_VALUES_AFTER
JIT = 59  # the default switches of a context (tests/test_sphere_defer_gpu.py ON)
AREA_LIGHT = 0  # a light row's type whose second word is the row of its object


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.view(np.uint32) == b.view(np.uint32)


def open_scene(fixtures, name):
    """scene `name` without its room row (C1: the Cornellbox, row 1; C3: the Cube around the scene, row 1; C4: the Cube
    around the scene, row 0), the area lights' object rows renumbered"""
    sc = dict(fixtures["scenes"][name])
    rows = np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18)
    room = {"C1": 1, "C3": 1, "C4": 0}[name]
    assert int(rows[room, 0]) in (1, 9)  # a Cube or a Cornellbox
    assert (np.abs(rows[room, 4:7] - rows[room, 1:4]) > 5.0).all()  # and the one that holds the scene
    sc["n"] = sc["n"] - 1
    sc["objects"] = np.delete(rows, room, axis=0).reshape(-1).copy()
    lights = np.asarray(sc["lights"], np.float32).reshape(sc["ln"], 18).copy()
    for l in lights:
        if int(l[0]) == AREA_LIGHT:
            assert int(l[1]) != room
            if int(l[1]) > room:
                l[1] -= 1.0
    sc["lights"] = lights.reshape(-1).copy()
    return sc


_WANT = {}


def _want(fixtures, name, w=W, h=H, spp=SPP, bounces=B, opened=True):
    """the oracle's frame: computed once per case, shared, never written"""
    k = (name, w, h, spp, bounces, opened)
    if k not in _WANT:
        sc = open_scene(fixtures, name) if opened else fixtures["scenes"][name]
        inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, spp)
        _WANT[k] = oracle.render(sc, capi.plugin_masks(sc["plugins"]), w, h, inv, seeds, sc["eye"], bounces)
        _WANT[k].setflags(write=False)
    return _WANT[k]


def _render(sc, w=W, h=H, spp=SPP, bounces=B, after=0, debug=None):
    """(accumulator, kernel info) of a context that waited for the best tier it asked for"""
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, spp)
    ctx = capi.Context(w, h, debug={capi.DEBUG_JIT: JIT, AFTER: after, **(debug or {})})
    try:
        ctx.set_scene_dict(sc)
        ctx.kernel_ready(-1)
        ctx.render_schedule(inv, seeds, sc["eye"], bounces)
        return ctx.read_accum(), ctx.kernel_info()
    finally:
        ctx.close()


def _check(got, want, what):
    bad = int((~same_bits(got, want)).sum())
    print(f"{what}: channels differing from the oracle: {bad}")
    assert bad == 0


# ---- 1. C1 without its Cornellbox: the light cube and the mirror sphere alone (the three-barrier sort) -----------------
@pytest.mark.gpu
@pytest.mark.parametrize("groups", [0, 3], ids=["plain", "sample_groups"])
@pytest.mark.parametrize("ns", [16, 4, 1])
@pytest.mark.parametrize("tier", ["types", "values"])
def test_open_cornell(gpu, fixtures, tier, ns, groups):
    """most rays miss both rows at the first bounce, so the first sort already leaves whole waves past the live range"""
    sc = open_scene(fixtures, "C1")
    want = _want(fixtures, "C1")
    assert (want[..., :3] != 0).any() and (want[..., :3] == 0).any()  # the light is seen, and so is the void
    dbg = {capi.DEBUG_SAMPLE_GROUPS: groups, capi.DEBUG_JIT_NS: ns}
    got, info = _render(sc, after=0 if tier == "values" else -1, debug=dbg)
    _, other = _render(sc, after=-1 if tier == "values" else 0, debug=dbg)
    assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    assert info["build_id"] != other["build_id"], (info, other)  # the two tiers are two kernels
    _check(got, want, f"{tier} ns {ns} groups {groups}")


# ---- 2. a room-set scene and a pre-cull scene without their rooms (the two-barrier sort; the compacted shadow rays) ------
@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 3], ids=["one_launch", "sample_groups"])
def test_open_room_set(gpu, fixtures, groups):
    sc = open_scene(fixtures, "C3")
    got, info = _render(sc, debug={capi.DEBUG_SAMPLE_GROUPS: groups})
    assert info["name"] == "sail_trace_kernel_jit" + ("_grouped" if groups > 1 else ""), info
    _check(got, _want(fixtures, "C3"), f"open C3, groups {groups}")


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 2], ids=["one_launch", "sample_groups"])
def test_open_pre_cull(gpu, fixtures, groups):
    sc = open_scene(fixtures, "C4")
    w, h, spp = 64, 40, 2
    got, info = _render(sc, w=w, h=h, spp=spp, debug={capi.DEBUG_SAMPLE_GROUPS: groups})
    assert info["name"] == "sail_trace_kernel_cull_jit" + ("_grouped" if groups > 1 else ""), info
    _check(got, _want(fixtures, "C4", w=w, h=h, spp=spp), f"open C4, groups {groups}")


# ---- 3. the closed scene at 1 and 2 bounces: no sorted bounce at all, or one that is also the last ----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["types", "values"])
@pytest.mark.parametrize("bounces", [1, 2])
def test_closed_cornell_short_paths(gpu, fixtures, bounces, tier):
    sc = fixtures["scenes"]["C1"]
    got, info = _render(sc, bounces=bounces, after=0 if tier == "values" else -1)
    assert info["name"].startswith("sail_trace_kernel_jit") and info["build_id"] == info["jit_build_id"], info
    _check(got, _want(fixtures, "C1", bounces=bounces, opened=False), f"C1, {bounces} bounce(s), {tier}")
