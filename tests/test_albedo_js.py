"""The albedo map and the albedo-demodulated filters through the JavaScript host and the CLI (renderer.albedo,
renderer.denoise({albedo}), renderer.temporalFilter({albedo}), cli.js --denoise --albedo). Needs node and a GPU.
tests/js/albedo_check.js reports the view it rendered; the same calls are made through capi, so the outputs must be the
same bytes."""
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
W, H, SPP, B = 48, 32, 8, 5


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def js():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "albedo_check.js"), str(W), str(H), str(SPP)],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def through_capi(fixtures, js):
    """the materials demo (the frozen scene C3) at 48x32, 8 spp marked after 4, in the view the script reports"""
    sc = fixtures["scenes"]["C3"]
    mvp, eye = np.array(js["mvp"], np.float64), np.array(js["eye"], np.float32)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV | capi.FLAG_SEGMENT_COUNT)
    try:
        ctx.set_scene_dict(sc)
        ctx.temporal_moments(True)
        ctx.reset()
        ctx.temporal_begin(mvp, eye)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, SPP // 2), eye, B)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, SPP // 2, SPP - SPP // 2), eye, B)
        ctx.temporal_resolve()
        out = {"plain": ctx.denoise()}
        out["map2"] = ctx.albedo(mvp, eye, grid=2)
        out["one"] = ctx.denoise(albedo=capi.ALBEDO_AMIN_DEFAULT)
        out["tf"] = ctx.temporal_filter(albedo=capi.ALBEDO_AMIN_DEFAULT)
        out["map4"] = ctx.albedo(mvp, eye, grid=4)
        out["two"] = ctx.denoise({"iterations": 2, "sigma_l": 2.5, "sigma_x": 0.05, "display": capi.FILTER_GAMMA},
                                 want_u8=True, albedo=0.02)
        out["map1"] = ctx.albedo(mvp, eye, grid=1)
    finally:
        ctx.close()
    return out


def test_js_albedo_equals_capi(js, through_capi):
    c = through_capi
    assert js["early"] and "rendered view" in js["early"]
    assert js["unchanged"] is True
    for name in ("map1", "map2", "map4"):
        assert js[name] == fnv(c[name]["rgba"].tobytes()), name
    assert len({js["map1"], js["map2"], js["map4"]}) == 3             # the checkerboards: every grid gives another map
    a = js["albedo"]
    assert (a["hitPixels"], a["partialPixels"], a["grid"]) == (c["map1"]["hit_pixels"], c["map1"]["partial_pixels"], 1)
    assert js["plain"] == fnv(c["plain"]["rgba"].tobytes())
    assert js["one"] == fnv(c["one"]["rgba"].tobytes()) and js["one"] != js["plain"]
    assert js["tf"] == fnv(c["tf"]["rgba"].tobytes())
    assert js["two"] == fnv(c["two"]["rgba"].tobytes()) and js["twoU8"] == fnv(c["two"]["u8"].tobytes())
    assert js["again"] == js["one"]                                   # after new rows the renderer makes the map again
    i, t = js["oneInfo"], js["tfInfo"]
    assert (i["k"], i["kMark"], i["nonfinite"], i["iterations"]) == (8, 4, c["one"]["nonfinite"], 4)
    assert (t["k"], t["temporalPixels"], t["spatialPixels"]) == (8, c["tf"]["temporal_pixels"], c["tf"]["spatial_pixels"])


def test_cli_denoise_albedo_pfm(fixtures, tmp_path):
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    sc = fixtures["scenes"]["C3"]
    mvp = np.array(sc["mvp_rowmajor"])
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, SPP // 2), sc["eye"], B)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, SPP // 2, SPP - SPP // 2), sc["eye"], B)
        ctx.albedo(mvp, sc["eye"], grid=4)
        want = ctx.denoise(albedo=capi.ALBEDO_AMIN_DEFAULT)
    finally:
        ctx.close()
    pfm = tmp_path / "d.pfm"
    r = subprocess.run([NODE, "sail_amd/js/cli.js", "sail_amd/js/examples/materials.js", "--width", str(W), "--height", str(H),
                        "--spp", str(SPP), "--deterministic", "--denoise", "--albedo", "--albedo-grid", "4", "--pfm", str(pfm),
                        "--stats"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["spp"] == SPP and st["denoise_ms"] > 0 and st["albedo_ms"] > 0 and st["albedo_grid"] == 4
    raw = pfm.read_bytes()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want["rgba"][..., :3]).view(np.uint32))
    for bad in (["--albedo"], ["--denoise", "--albedo-grid", "2"], ["--denoise", "--albedo", "--albedo-grid", "5"]):
        r = subprocess.run([NODE, "sail_amd/js/cli.js", "sail_amd/js/examples/materials.js", *bad], cwd=ROOT,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--albedo" in r.stderr
