"""CPU: the host-only half of adaptive sampling. sail_plan_adaptive against tests/adaptive_ref.py's numpy restatement of
include/sail_hip.h's rule (random 16x16-tile error maps at ragged sizes, NaN entries, dilate 0 and 1), its monotonicity,
its refusals, the defaults, and the new names in the header and the binding."""
import math
import os
import re

import numpy as np
import pytest

import adaptive_ref as ar
from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (64, 64), (65, 3), (160, 96), (200, 136), (333, 257), (1920, 1080)]
NEW = ("sail_set_active_tiles", "sail_get_active_tiles", "sail_plan_adaptive", "sail_adaptive_defaults", "sail_render_adaptive")


def err_map(rng, W, H, nan=0.0):
    e = rng.random(((H + 15) // 16, (W + 15) // 16), dtype=np.float32)
    e[rng.random(e.shape) < nan] = np.nan
    return e


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("W,H", SIZES)
def test_plan_matches_the_numpy_rule(W, H, dilate):
    rng = np.random.default_rng(W * 1000 + H + dilate)
    tx, ty = ar.tiles64(W, H)
    for trial in range(6):
        e16 = err_map(rng, W, H, nan=0.1 if trial % 2 else 0.0)
        prev = None if trial < 2 else (rng.random((ty, tx)) < 0.7).astype(np.uint8)
        want_e = ar.e64(e16, W, H)
        finite = np.sort(want_e[np.isfinite(want_e)])
        # a target off every tile's value (a midpoint, or above / below all), so that a last-bit difference cannot decide
        target = 0.5 if finite.size < 2 else float((finite[finite.size // 2 - 1] + finite[finite.size // 2]) / 2)
        for tgt in (target, 0.0, math.inf, -1.0):
            want, _ = ar.plan(W, H, e16, tgt, dilate, prev)
            got, got_e, n = capi.plan_adaptive(W, H, e16, tgt, dilate, prev)
            assert np.array_equal(got, want), (W, H, dilate, trial, tgt)
            assert n == int(want.sum())
            assert np.array_equal(np.isnan(got_e), np.isnan(want_e))
            assert np.allclose(got_e, want_e, rtol=1e-14, atol=0, equal_nan=True)   # the same doubles in the same order
            if prev is not None:
                assert not (got & (1 - prev)).any(), "a frozen tile came back"


def test_nan_is_noisy_and_inf_target_is_not():
    W, H = 160, 96
    e16 = np.zeros(((H + 15) // 16, (W + 15) // 16), np.float32)
    e16[0, 0] = np.nan  # tile (0, 0)
    got, e, n = capi.plan_adaptive(W, H, e16, math.inf, 0)
    assert math.isnan(e[0, 0]) and got.tolist() == [[1, 0, 0], [0, 0, 0]] and n == 1
    got, _, n = capi.plan_adaptive(W, H, e16, math.inf, 1)
    assert got.tolist() == [[1, 1, 0], [1, 1, 0]] and n == 4
    e16[0, 0] = np.inf
    assert capi.plan_adaptive(W, H, e16, math.inf, 0)[2] == 0   # inf <= inf


def test_weights_are_in_frame_pixels():
    """65 x 3: tile 1 is one pixel wide, its single 16x16 tile holds 3 pixels; tile 0 weights four of 48 pixels each"""
    e16 = np.array([[1, 2, 3, 4, 100]], np.float32)
    _, e, _ = capi.plan_adaptive(65, 3, e16, 0.0, 0)
    assert e.tolist() == [[2.5, 100.0]]
    # 20 x 16: the second 16x16 tile holds 4 of its 16 columns
    _, e, _ = capi.plan_adaptive(20, 16, np.array([[1, 6]], np.float32), 0.0, 0)
    assert e[0, 0] == (1.0 * 256 + 6.0 * 64) / 320


@pytest.mark.parametrize("dilate", [0, 1])
def test_active_set_only_shrinks(dilate):
    W, H = 333, 257
    rng = np.random.default_rng(5)
    active = None
    counts = []
    for look in range(6):
        e16 = err_map(rng, W, H) * np.float32(0.8 ** look)
        nxt, _, n = capi.plan_adaptive(W, H, e16, 0.3, dilate, active)
        if active is not None:
            assert not (nxt & (1 - active)).any()
        active = nxt
        counts.append(n)
    assert counts == sorted(counts, reverse=True) and counts[-1] < counts[0]


def test_in_place_and_optional_outputs():
    lib = capi.load()
    W, H = 160, 96
    e16 = err_map(np.random.default_rng(1), W, H)
    prev = np.array([1, 1, 0, 1, 0, 1], np.uint8)
    want, _ = ar.plan(W, H, e16, 0.5, 1, prev)
    u8 = capi.ctypes.c_uint8
    buf = prev.copy()
    assert lib.sail_plan_adaptive(W, H, capi._ptr(e16), 0.5, 1, capi._ptr(buf, u8), capi._ptr(buf, u8), None, None) == 0
    assert np.array_equal(buf.reshape(2, 3), want)


def test_refusals():
    lib = capi.load()
    e16 = np.zeros(60, np.float32)
    out = np.zeros(6, np.uint8)
    u8 = capi.ctypes.c_uint8
    ok = (160, 96, capi._ptr(e16), 0.5, 1, None, capi._ptr(out, u8), None, None)
    assert lib.sail_plan_adaptive(*ok) == 0
    for i, bad in ((0, 0), (1, -1), (2, None), (3, math.nan), (4, 2), (4, -1), (6, None)):
        args = list(ok)
        args[i] = bad
        assert lib.sail_plan_adaptive(*args) == -1, (i, bad)
    assert lib.sail_adaptive_defaults(None) == -1
    with pytest.raises(capi.SailError):
        capi.plan_adaptive(160, 96, np.zeros(59, np.float32), 0.5)
    with pytest.raises(capi.SailError):
        capi.plan_adaptive(160, 96, e16, 0.5, 1, np.ones(5, np.uint8))


def test_defaults():
    assert capi.adaptive_defaults() == {"target": math.inf, "min_spp": 16, "max_spp": 1024, "dilate": 1}


def test_new_names_are_in_the_header_and_the_binding():
    with open(os.path.join(ROOT, "include", "sail_hip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|void|const char\*)\s+(sail_[a-z0-9_]+)\(", text, re.M))
    assert set(NEW) <= declared and set(NEW) <= set(capi.EXPORTS)
    assert declared == set(capi.EXPORTS)
    assert re.search(r"#define SAIL_ABI_VERSION 4\b", text)
    lib = capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
