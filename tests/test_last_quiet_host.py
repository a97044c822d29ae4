"""CPU: the host's last-bounce row classes (sail_plan_last_bounce, include/sail_hip.h) on the fixtures and on the row
edits tests/test_gpu_last_quiet.py renders: which rows add exactly +0 at a path's last bounce (no hit record), and
whether that bounce's path sort is skipped too."""
import numpy as np
import pytest

from sail_amd import capi
import test_gpu_last_quiet as q


def test_fixture_scenes(fixtures):
    sc = fixtures["scenes"]
    # C1: the walls (a Lambertian matte of constant colours) and the mirror sphere are quiet, the light cube emits
    assert capi.plan_last_bounce(sc["C1"], False) == (0b110, 1)
    # in a kernel with a light plugin a lit matte hit declines the shortcut: the walls are full, the sort stays
    assert capi.plan_last_bounce(sc["C1"], True) == (0b100, 0)
    for name in ("C3", "UI"):
        quiet, skip = capi.plan_last_bounce(sc[name], True)
        assert skip == 0 and quiet != 0 and not quiet & 1  # row 0, the rectangle light, emits
    # scenes of more than 32 rows are not classified
    assert sc["C4"]["n"] > 32 and capi.plan_last_bounce(sc["C4"], True) == (0, 0)


@pytest.mark.parametrize("variant", sorted(q.VARIANTS))
def test_row_edits(fixtures, variant):
    edit, quiet, skip = q.VARIANTS[variant]
    sc = edit(fixtures["scenes"]["C1"])
    assert capi.plan_last_bounce(sc, False) == (quiet, skip)
    # with a light plugin compiled in no matte row is quiet and, C1's rows being matte but the sphere, the sort stays
    ql, sl = capi.plan_last_bounce(sc, True)
    assert sl == 0 and ql & ~quiet == 0 and not ql & 0b011


def test_matte_plugin_absent_and_row_kinds(fixtures):
    c1 = fixtures["scenes"]["C1"]
    # without the matte plugin in the scene's mask material() leaves f at +0: sigma and the colour are never read
    sc = q.v_oren_nayar(c1)
    sc["plugins"] = dict(sc["plugins"], material=["mirror"])
    assert capi.plan_last_bounce(sc, False) == (0b110, 1)
    # a row whose shape plugin is absent is never hit and has no class: it neither is quiet nor keeps the sort
    sc = dict(c1, plugins=dict(c1["plugins"], shape=["cube", "cornellbox"]))
    assert capi.plan_last_bounce(sc, False) == (0b010, 1)
    # every channel counts, and so does the sign bit of each
    for ch in range(3):
        rows = q._rows(c1)
        rows[2, 8 + ch] = -0.0
        assert capi.plan_last_bounce(q._with(c1, rows), False) == (0b010, 0)
        rows[2, 8 + ch] = 1e-45  # a subnormal emitter is an emitter
        assert capi.plan_last_bounce(q._with(c1, rows), False) == (0b010, 1)


def test_bad_arguments():
    lib = capi.load()
    assert lib.sail_plan_last_bounce(None, 3, None, 1, None, 0, None, None) < 0
