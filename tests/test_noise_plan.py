"""CPU: the host-only side of the noise estimate (include/sail_hip.h): sail_plan_until's doubling schedule of looks, and
the device entry points refusing a null context."""
import ctypes

import pytest

from sail_amd import capi


def looks(k, mn, mx, count):
    out = []
    for _ in range(count):
        k = capi.plan_until(k, mn, mx)
        out.append(k)
    return out


def test_plan_until_doubles_from_min_to_max():
    assert looks(0, 4, 40, 6) == [4, 8, 16, 32, 40, 40]
    assert looks(0, 16, 65536, 14) == [16 << i for i in range(13)] + [65536]


def test_plan_until_from_inside_and_beyond_the_range():
    assert capi.plan_until(3, 4, 40) == 4
    assert capi.plan_until(5, 4, 40) == 10      # a resumed render doubles its own count
    assert capi.plan_until(20, 4, 40) == 40
    assert capi.plan_until(21, 4, 40) == 40
    assert capi.plan_until(40, 4, 40) == 40
    assert capi.plan_until(41, 4, 40) == 41     # past the cap: stay


def test_plan_until_min_equals_max():
    assert looks(0, 7, 7, 3) == [7, 7, 7]
    assert looks(0, 1, 1, 2) == [1, 1]


def test_plan_until_does_not_overflow():
    top = (1 << 64) - 1
    assert capi.plan_until(1 << 63, 1, top) == top
    assert capi.plan_until((1 << 63) - 1, 1, top) == top - 1
    assert capi.plan_until(top, 1, top) == top


def test_plan_until_rejects_bad_arguments():
    with pytest.raises(capi.SailError):
        capi.plan_until(0, 0, 40)      # min_spp < 1
    with pytest.raises(capi.SailError):
        capi.plan_until(0, 8, 4)       # max_spp < min_spp
    lib = capi.load()
    assert lib.sail_plan_until(0, 4, 40, None) == -1


def test_null_context_is_rejected():
    lib = capi.load()
    assert lib.sail_noise_mark(None) == -1
    info = capi.NoiseInfo()
    assert lib.sail_noise_estimate(None, ctypes.byref(info), None, None, 0) == -1
    mvp = (ctypes.c_double * 16)(*([0.0] * 16))
    eye = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    conv, n = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.sail_render_until(None, mvp, eye, 5, 0.0, 4, 40, ctypes.byref(info), ctypes.byref(conv), None, 0,
                                 ctypes.byref(n)) == -1
