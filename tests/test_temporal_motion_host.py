"""CPU: the host-only side of the reprojection across an object move (include/sail_hip.h, sail_move_objects): the symbols
are bound, a NULL context is refused, the numpy reference (tests/temporal_motion_ref.py) with no motion and no cap is the
camera-motion reference bit for bit, with a motion it is not, and scene.objectMotion() of the JavaScript host reports a
Pickup drag in the right row without consuming it."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import temporal_filter_ref as tf
import temporal_motion_ref as tm
import temporal_ref as tr
from sail_amd import capi
from temporal_ref import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node") or shutil.which("nodejs")
F = np.float32

# the issue's cases: scene, {row: motion}, view of the history, the new view (None: the scene's fixture view)
CASES = {
    "C1-sphere": ("C1", {2: (0.6, 0.1, -0.3)}, 0, 0),
    "C1-sphere-orbit3": ("C1", {2: (0.6, 0.1, -0.3)}, 0, 3),
    "C1-light-and-sphere": ("C1", {0: (-0.5, 0.0, 0.4), 2: (0.3, 0.0, 0.2)}, 0, 0),
    "C3-two-spheres": ("C3", {3: (0.0, 0.5, 0.9), 5: (0.0, 0.6, 0.5)}, None, None),
}


def case_views(sc, a, b):
    fx = (np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F))
    return (fx if a is None else tr.orbit(a)), (fx if b is None else tr.orbit(b))


def test_symbols_are_bound():
    lib = capi.load()
    for name in ("sail_move_objects", "sail_temporal_pending_motion"):
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None
    for method in ("move_objects", "temporal_pending_motion"):
        assert callable(getattr(capi.Context, method))
    assert lib.sail_abi_version() == 4


def test_null_context_is_rejected():
    lib = capi.load()
    rows, motion = np.zeros(18, F), np.zeros(3, F)
    cap, pending = ctypes.c_float(), ctypes.c_int()
    assert lib.sail_move_objects(None, capi._ptr(rows), 1, capi._ptr(motion), 0.0) == -1
    assert lib.sail_move_objects(None, capi._ptr(rows), 1, None, 8.0) == -1
    assert lib.sail_temporal_pending_motion(None, capi._ptr(motion), ctypes.byref(cap), ctypes.byref(pending)) == -1


def test_moved_translates_the_right_words(fixtures):
    sc = fixtures["scenes"]["C1"]
    rows0 = np.array(sc["objects"], F).reshape(-1, 18)
    types = rows0[:, 0].astype(int).tolist()
    assert types[2] == 2 and any(t in tm.MINMAX_TYPES for t in types)
    box = next(r for r, t in enumerate(types) if t in tm.MINMAX_TYPES)
    d = np.array([0.6, 0.1, -0.3], F)
    rows1 = np.array(tm.moved(sc, {2: d, box: d})["objects"], F).reshape(-1, 18)
    assert np.array_equal(bits(rows1[2, 1:4]), bits(rows0[2, 1:4] + d)) and np.array_equal(bits(rows1[2, 4:]), bits(rows0[2, 4:]))
    assert np.array_equal(bits(rows1[box, 1:4]), bits(rows0[box, 1:4] + d))
    assert np.array_equal(bits(rows1[box, 4:7]), bits(rows0[box, 4:7] + d)) and np.array_equal(bits(rows1[box, 7:]), bits(rows0[box, 7:]))
    others = [r for r in range(len(types)) if r not in (2, box)]
    assert np.array_equal(bits(rows1[others]), bits(rows0[others]))
    assert np.array_equal(bits(np.array(sc["objects"], F).reshape(-1, 18)), bits(rows0))        # the fixture itself is not touched


@pytest.mark.parametrize("case", list(CASES))
def test_reference_without_motion_is_the_camera_reference(fixtures, case):
    """D = 0 and mc = inf: X - (+0) is X, min(m, inf) is m, so every bit is tests/temporal_ref.py's; with the motion the
    moved rows' pixels look elsewhere and more of them find a history"""
    name, moves, a, b = CASES[case]
    sc = fixtures["scenes"][name]
    W, H = 48, 32
    va, vb = case_views(sc, a, b)
    GA = tr.ref_gbuffer(sc, va[0], va[1], W, H)[0]
    GB = tr.ref_gbuffer(tm.moved(sc, moves), vb[0], vb[1], W, H)[0]
    rng = np.random.default_rng(11)
    hist = rng.random((H, W, 4), dtype=F) + F(1)
    mom = rng.random((H, W, 4), dtype=F) + F(1)
    zero = np.zeros((sc["n"], 3), F)
    R0, found0 = tr.ref_reproject(GB, GA, hist, va[0], va[1])
    R1, found1 = tm.ref_reproject_moved(GB, GA, hist, va[0], va[1], zero, np.inf)
    assert found0 == found1 and np.array_equal(bits(R0), bits(R1))
    M0 = tf.ref_moment_reproject(GB, GA, mom, va[0], va[1])
    M1 = tm.ref_moment_reproject_moved(GB, GA, mom, va[0], va[1], zero, np.inf)
    assert np.array_equal(bits(M0), bits(M1))
    D = tm.motion_table(sc["n"], moves)
    R2, found2 = tm.ref_reproject_moved(GB, GA, hist, va[0], va[1], D, np.inf)
    on_moved = np.isin(GB[..., 3], [F(r) for r in moves])
    with_motion = int(((R2[..., 3] > 0) & on_moved).sum())
    without = int(((R0[..., 3] > 0) & on_moved).sum())
    print(f"{case} {W}x{H}: history {found0} without motion, {found2} with; on the moved rows {without} -> {with_motion} "
          f"of {int(on_moved.sum())}; words differing {int((bits(R2) != bits(R0)).sum())}")
    assert (bits(R2) != bits(R0)).any() and with_motion > without
    # pixels off the moved rows are not touched by the table
    assert np.array_equal(bits(R2[~on_moved]), bits(R0[~on_moved]))
    # the cap clamps every count and nothing else
    R3, found3 = tm.ref_reproject_moved(GB, GA, hist * F(20), va[0], va[1], D, 8.0)
    R4, _ = tm.ref_reproject_moved(GB, GA, hist * F(20), va[0], va[1], D, np.inf)
    assert found3 == found2 and np.array_equal(bits(R3[..., :3]), bits(R4[..., :3]))
    assert np.array_equal(R3[..., 3], np.minimum(R4[..., 3], F(8))) and (R4[..., 3] > 8).any()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_object_motion_of_a_pickup_drag(fixtures):
    row = 5                                                  # C3's matte sphere
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "object_motion.js"), str(row)], cwd=ROOT,
                         capture_output=True, text=True, check=True, timeout=120).stdout
    js = json.loads(out.strip().splitlines()[-1])
    n = js["n"]
    assert n == fixtures["scenes"]["C3"]["n"] and js["began"] and js["moving"]
    assert len(js["before"]) == n * 3 and not any(js["before"]) and not any(js["after"])
    drag = np.array(js["drag1"], F).reshape(n, 3)
    assert js["again"] == js["drag1"]                        # reading does not consume it
    assert drag[row].any() and not drag[np.arange(n) != row].any()
    rows0, rows1 = (np.array(js[k], F).reshape(n, 18) for k in ("rows0", "rows1"))
    assert np.array_equal(bits(rows0), bits(np.array(fixtures["scenes"]["C3"]["objects"], F).reshape(n, 18)))
    # serializeObjects applied it: the sphere's centre moved by the motion to f32 rounding, nothing else changed
    assert np.abs((rows1[row, 1:4] - rows0[row, 1:4]) - drag[row]).max() <= 1e-6
    rows1[row, 1:4] = rows0[row, 1:4]
    assert np.array_equal(bits(rows0), bits(rows1))
