"""What a context still holds after the calls that restart its accumulation or change its rows: a table of
"call x what is left", each item asked for through the call that reports it (include/sail_hip.h). A state error with its
documented message counts as "gone". Needs a GPU.

    call                                         gone                                still there
    sail_reset, sail_set_accum_mode,             the mark, the mask, "resolved"      both views, nothing pending, the albedo
      sail_set_partition(0, 1, mode)                                                   map, the value kernel
    sail_set_scene, sail_update_objects          everything; the moment maps read    -
                                                   as zeros after the next begin
    sail_move_objects with a motion              the albedo map, the mark, the       both views; the motion is pending with
                                                   mask, "resolved", the value         the given cap
                                                   kernel
    sail_move_objects without temporal state     what sail_update_objects drops;     -
                                                   nothing pending

The value kernel's assertions hold only where the build has one for C1: they are made when <directory of the library>/
jit-values holds C1's object (then the context must have loaded it) or the context loaded one anyway, and are vacuous
otherwise, e.g. for a library in a directory without a shipped cache. The zeros of the moment maps are what the ABI
shows after the next begin; no call reads a moment map of a context without views before a begin has rewritten it.

The frame is C1 at 72x40: 2x1 tiles of 64 and 5x3 tiles of 16, ragged on both edges. On a multi-device context (one GPU
twice) device 0's sub-context holds the state; sail_update_objects and sail_move_objects are checked there."""
import os

import numpy as np
import pytest

import temporal_ref as tr
from sail_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
W, H, B = 72, 40, 5
SPHERE_ROW, SPHERE_MOVE, CAP = 2, (0.6, 0.1, -0.3), 8.0
STATE = -4  # SAIL_E_STATE


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


@pytest.fixture(scope="module")
def types_id(gpu, fixtures):
    """the build id of C1's types kernel, which a context reports while it has no loaded value kernel"""
    ctx = capi.Context(W, H, debug={capi.DEBUG_JIT_VALUES_AFTER: -1})
    try:
        ctx.set_scene_dict(fixtures["scenes"]["C1"])
        ctx.kernel_ready(-1)
        return ctx.kernel_info()["jit_build_id"]
    finally:
        ctx.close()


# the two views, built on first use: importing this module must not load the library (collection imports every test
# module, and the library has to come after torch's own HIP runtime where a later module imports torch)
def view_a():
    return tr.orbit(0)


def view_b():
    return tr.orbit(3)


def moved_scene(sc):
    rows = np.array(sc["objects"], F).reshape(sc["n"], 18)
    rows[SPHERE_ROW, 1:4] += np.array(SPHERE_MOVE, F)
    motion = np.zeros((sc["n"], 3), F)
    motion[SPHERE_ROW] = SPHERE_MOVE
    out = dict(sc)
    out["objects"] = rows.reshape(-1)
    return out, motion


def render(ctx, view, k0, spp):
    inv, seeds = capi.schedule(view[0], W, H, k0, spp)
    ctx.render_schedule(inv, seeds, view[1], B)


def gone(call, text):
    """the call refuses with the state error that says `text` (any other error is the test's failure); False: it succeeds"""
    try:
        call()
    except capi.SailError as e:
        assert ": %d: " % STATE in str(e) and text in str(e), str(e)
        return True
    return False


class Held:
    """what the context reports it holds, each item through its own call"""

    def __init__(self, ctx, types_id):
        self.ctx, self.types_id = ctx, types_id

    def mark(self):
        return not gone(self.ctx.noise_estimate, "no mark")

    def mask(self):
        return not self.ctx.get_active_tiles().all()

    def resolved(self):
        return not gone(self.ctx.temporal_filter, "not resolved")

    def view(self, which):
        return not gone(lambda: self.ctx.temporal_read(which), "needs a")

    def views(self):
        return self.view(capi.TEMPORAL_G_CUR), self.view(capi.TEMPORAL_G_PREV)

    def pending(self):
        return self.ctx.temporal_pending_motion()

    def albedo(self):
        return not gone(self.ctx.albedo_read, "no albedo map")

    def value_id(self):
        """the loaded value kernel's build id, or None while the types kernel (or none) is the scene's run-time kernel"""
        i = self.ctx.kernel_info()
        return i["jit_build_id"] if i["jit_state"] == capi.KERNEL_JIT_READY and i["jit_build_id"] != self.types_id else None


def full_state(sc, types_id, devices=None, temporal=True):
    """A context that holds everything: two samples with a mark between them, a tile mask with one tile off, a committed and
    a resolved current view with moment tracking on, the current view's albedo map, and C1's value kernel where the build
    has one. Returns the context, its reporter and the value kernel's id (None: the build has none)."""
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV, devices=devices, debug={capi.DEBUG_JIT_VALUES_AFTER: 0})
    ctx.set_scene_dict(sc)
    ctx.temporal_moments(True)
    ctx.kernel_ready(-1)
    held = Held(ctx, types_id)
    render(ctx, view_b(), 0, 1)
    ctx.noise_mark()
    render(ctx, view_b(), 1, 1)
    if temporal:
        ctx.temporal_begin(*view_a())
        ctx.temporal_resolve()
        ctx.temporal_begin(*view_b())
        ctx.temporal_resolve()
    ctx.albedo(*view_b())
    ctx.set_active_tiles([1, 0])
    value = held.value_id()
    shipped = os.path.join(os.path.dirname(capi.LIB_PATH), "jit-values", "%s.co" % capi.jit_value_key(sc)[0])
    assert value is not None or not os.path.exists(shipped), "the build ships C1's value kernel and the context did not load it"
    assert held.mark() and held.mask() and held.albedo()
    assert held.views() == (temporal, temporal) and held.pending()["pending"] == 0
    if temporal:
        assert held.resolved()
    return ctx, held, value


def assert_restarted(held):
    """what every restart of the accumulation drops (resetAccum)"""
    assert not held.mark() and not held.mask()


def assert_rows_dropped(ctx, held, value):
    """everything is gone; moment tracking stays on, over maps that read as zeros after the next begin"""
    assert_restarted(held)
    assert held.views() == (False, False)
    assert held.pending()["pending"] == 0 and held.pending()["hist_cap"] == np.inf
    assert not held.albedo()
    assert gone(ctx.temporal_filter, "no current view")
    if value is not None:
        assert held.value_id() != value, "the value kernel of the old rows is still the scene's"
    ctx.temporal_begin(*view_a())
    for which in (capi.TEMPORAL_M_R, capi.TEMPORAL_M_OUT):
        assert not ctx.temporal_read_moments(which).view(np.uint32).any()
    ctx.temporal_begin(*view_b())  # commits view A unresolved: its moments are the history now
    assert not ctx.temporal_read_moments(capi.TEMPORAL_M_HIST).view(np.uint32).any()


RESTARTS = {
    "reset": lambda ctx: ctx.reset(),
    "accum_mode": lambda ctx: ctx.set_accum_mode(capi.ACCUM_MIX),
    "partition": lambda ctx: ctx.set_partition(0, 1, capi.PART_TILES),
}


@pytest.mark.parametrize("call", sorted(RESTARTS))
def test_a_restart_keeps_views_albedo_and_value_kernel(gpu, fixtures, types_id, call):
    ctx, held, value = full_state(fixtures["scenes"]["C1"], types_id)
    try:
        RESTARTS[call](ctx)
        assert_restarted(held)
        assert not held.resolved()
        assert held.views() == (True, True)
        assert held.pending()["pending"] == 0
        assert held.albedo()
        assert held.value_id() == value
    finally:
        ctx.close()


def new_rows(ctx, sc, call):
    moved, _ = moved_scene(sc)
    if call == "set_scene":
        ctx.set_scene_dict(moved)
    else:
        rows = np.ascontiguousarray(moved["objects"], F)
        ctx._check(ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]), "sail_update_objects")


@pytest.mark.parametrize("call,devices", [("set_scene", None), ("update_objects", None), ("update_objects", [0, 0])],
                         ids=["set_scene", "update_objects", "update_objects-multi"])
def test_new_rows_drop_everything(gpu, fixtures, types_id, call, devices):
    sc = fixtures["scenes"]["C1"]
    ctx, held, value = full_state(sc, types_id, devices=devices)
    try:
        new_rows(ctx, sc, call)
        assert_rows_dropped(ctx, held, value)
    finally:
        ctx.close()


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one", "multi"])
def test_a_move_keeps_the_views_and_leaves_its_motion_pending(gpu, fixtures, types_id, devices):
    sc = fixtures["scenes"]["C1"]
    ctx, held, value = full_state(sc, types_id, devices=devices)
    try:
        moved, motion = moved_scene(sc)
        ctx.move_objects(moved["objects"], motion, hist_cap=CAP)
        assert_restarted(held)
        assert not held.resolved()
        assert not held.albedo()
        assert held.views() == (True, True)
        p = held.pending()
        assert p["pending"] == 1 and p["hist_cap"] == CAP
        assert np.array_equal(p["motion"].view(np.uint32), motion.view(np.uint32))
        if value is not None:
            assert held.value_id() != value, "the value kernel of the old rows is still the scene's"
    finally:
        ctx.close()


def test_a_move_without_temporal_state_is_an_update(gpu, fixtures, types_id):
    sc = fixtures["scenes"]["C1"]
    ctx, held, value = full_state(sc, types_id, temporal=False)
    try:
        moved, motion = moved_scene(sc)
        ctx.move_objects(moved["objects"], motion, hist_cap=CAP)
        assert_rows_dropped(ctx, held, value)
    finally:
        ctx.close()
