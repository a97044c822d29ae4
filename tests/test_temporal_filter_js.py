"""Moment tracking and the temporal filter through the JavaScript host (Renderer({aov: true, temporal: {moments: true}}),
renderer.temporalFilter). Needs node and a GPU. tests/js/temporal_filter_check.js reports the views it rendered; the same
calls are made through capi, so the filter's outputs must be the same bytes."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node") or shutil.which("nodejs")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]
W, H, B = 48, 32, 5


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def js():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "temporal_filter_check.js"), str(W), str(H)],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_js_temporal_filter_equals_capi(fixtures, js):
    steps = js["steps"]
    assert [s["k"] for s in steps] == [4, 1] and steps[0]["mvp"] != steps[1]["mvp"]
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV | capi.FLAG_SEGMENT_COUNT)
    try:
        ctx.set_accum_mode(capi.ACCUM_MIX)                          # the renderer's default accumulation
        ctx.set_scene_dict(fixtures["scenes"]["C1"])
        ctx.temporal_moments(True)
        for s in steps:
            mvp, eye = np.array(s["mvp"], np.float64), np.array(s["eye"], np.float32)
            ctx.reset()
            ctx.temporal_begin(mvp, eye)
            ctx.render_schedule(*capi.schedule(mvp, W, H, 0, s["n"]), eye, B)
            assert fnv(ctx.temporal_resolve()["rgba"].tobytes()) == s["resolve"]
        assert fnv(ctx.temporal_read_moments(capi.TEMPORAL_M_OUT).tobytes()) == js["moments"]
        plain = ctx.temporal_filter()
        other = ctx.temporal_filter({"iterations": 2, "sigma_l": 1.5, "sigma_x": 0.1, "min_hist": 2.0,
                                     "display": capi.FILTER_GAMMA, "gamma_c": 1.8}, want_u8=True)
    finally:
        ctx.close()
    assert js["plain"]["rgba"] == fnv(plain["rgba"].tobytes()) and js["plain"]["has8"] is False
    assert js["other"]["rgba"] == fnv(other["rgba"].tobytes()) and js["other"]["rgba8"] == fnv(other["u8"].tobytes())
    assert js["plain"]["rgba"] != js["other"]["rgba"]
    for got, want in ((js["plain"]["info"], plain), (js["other"]["info"], other)):
        assert (got["k"], got["temporalPixels"], got["spatialPixels"], got["nonfinite"], got["iterations"]) == \
            (want["k"], want["temporal_pixels"], want["spatial_pixels"], want["nonfinite"], want["iterations"])
        assert len(got["passMs"]) == want["iterations"] + 1
    assert js["plain"]["info"]["temporalPixels"] > 0 and js["plain"]["info"]["k"] == 1
    assert js["other"]["info"]["temporalPixels"] >= js["plain"]["info"]["temporalPixels"]    # minHist 2 takes no fewer
    d, c = js["defaults"], capi.temporal_filter_defaults()
    assert (d["iterations"], d["sigmaL"], d["sigmaX"], d["minHist"], d["display"], d["gamma"]) == \
        (c["iterations"], c["sigma_l"], c["sigma_x"], c["min_hist"], c["display"], c["gamma_c"])


def test_js_temporal_filter_needs_aov_and_moments(js):
    assert "aov: true" in js["noAov"]
    assert "moments: true" in js["noMoments"] and "moments: true" in js["noTemporal"]
