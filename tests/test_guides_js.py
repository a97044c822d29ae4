"""The guide maps and the guided filters through the JavaScript host and the CLI (renderer.guides, renderer.denoise({guides}),
renderer.temporalFilter({guides}), cli.js --denoise --guides). Needs node and a GPU. tests/js/guides_check.js reports the view
it rendered; the same calls are made through capi, so the outputs must be the same bytes."""
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
AMIN = capi.ALBEDO_AMIN_DEFAULT


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def js():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "guides_check.js"), str(W), str(H), str(SPP)],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def through_capi(fixtures, js):
    """the materials demo (the frozen scene C3) at 48x32, 8 spp marked after 4, in the view the script reports, on a context
    without AOV maps"""
    sc = fixtures["scenes"]["C3"]
    mvp, eye = np.array(js["mvp"], np.float64), np.array(js["eye"], np.float32)
    ctx = capi.Context(W, H, flags=capi.FLAG_SEGMENT_COUNT)
    try:
        ctx.set_scene_dict(sc)
        ctx.temporal_moments(True)
        ctx.reset()
        ctx.temporal_begin(mvp, eye)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, SPP // 2), eye, B)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, SPP // 2, SPP - SPP // 2), eye, B)
        ctx.temporal_resolve()
        ctx.use_guides(True)
        out = {"maps4": ctx.guides(mvp, eye, depth=4)}
        out["one"] = ctx.denoise()
        out["tf"] = ctx.temporal_filter()
        ctx.albedo(mvp, eye, grid=2)
        out["both"] = ctx.denoise(albedo=AMIN)
        out["maps1"] = ctx.guides(mvp, eye, depth=1)
        out["two"] = ctx.denoise({"iterations": 2, "sigma_l": 2.5, "sigma_x": 0.05, "display": capi.FILTER_GAMMA}, want_u8=True)
        out["maps0"] = ctx.guides(mvp, eye, depth=0)
    finally:
        ctx.close()
    return out


def test_js_guides_equal_capi(js, through_capi):
    c = through_capi
    assert js["early"] and "rendered view" in js["early"]
    assert js["noAov"] and "aov: true" in js["noAov"]
    assert js["unchanged"] is True
    for name in ("maps0", "maps1", "maps4"):
        assert js[name] == [fnv(c[name]["n"].tobytes()), fnv(c[name]["x"].tobytes())], name
    assert len({tuple(js["maps0"]), tuple(js["maps1"]), tuple(js["maps4"])}) == 3       # every depth gives other maps
    g, m0 = js["guides"], c["maps0"]
    assert (g["hitPixels"], g["followedPixels"], g["truncatedPixels"], g["depth"], g["maxDepth"]) == \
        (m0["hit_pixels"], 0, m0["truncated_pixels"], 0, 0)
    assert m0["truncated_pixels"] > 0 and c["maps4"]["followed_pixels"] > 0 and c["maps4"]["max_depth"] >= 2
    assert js["one"] == fnv(c["one"]["rgba"].tobytes())
    assert js["tf"] == fnv(c["tf"]["rgba"].tobytes())
    assert js["both"] == fnv(c["both"]["rgba"].tobytes()) and js["both"] != js["one"]
    assert js["two"] == fnv(c["two"]["rgba"].tobytes()) and js["twoU8"] == fnv(c["two"]["u8"].tobytes())
    assert js["again"] == js["one"]                                   # after new rows the renderer makes the maps again
    i, t = js["oneInfo"], js["tfInfo"]
    assert (i["k"], i["kMark"], i["nonfinite"], i["iterations"]) == (8, 4, c["one"]["nonfinite"], 4)
    assert (t["k"], t["temporalPixels"], t["spatialPixels"]) == (8, c["tf"]["temporal_pixels"], c["tf"]["spatial_pixels"])


def test_cli_denoise_guides_pfm(fixtures, tmp_path):
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    sc = fixtures["scenes"]["C3"]
    mvp = np.array(sc["mvp_rowmajor"])
    ctx = capi.Context(W, H)
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, SPP // 2), sc["eye"], B)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, SPP // 2, SPP - SPP // 2), sc["eye"], B)
        ctx.guides(mvp, sc["eye"], depth=2)
        ctx.use_guides(True)
        want = ctx.denoise()
    finally:
        ctx.close()
    pfm = tmp_path / "d.pfm"
    r = subprocess.run([NODE, "sail_amd/js/cli.js", "sail_amd/js/examples/materials.js", "--width", str(W), "--height", str(H),
                        "--spp", str(SPP), "--deterministic", "--denoise", "--guides", "--guide-depth", "2", "--pfm", str(pfm),
                        "--stats"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["spp"] == SPP and st["denoise_ms"] > 0 and st["guides_ms"] > 0 and st["guide_depth"] == 2
    raw = pfm.read_bytes()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want["rgba"][..., :3]).view(np.uint32))
    # bad flag combinations exit 1 before a device is touched
    for bad in (["--guides"], ["--denoise", "--guide-depth", "2"], ["--denoise", "--guides", "--guide-depth", "9"],
                ["--denoise", "--guides", "--guide-depth", "-1"]):
        r = subprocess.run([NODE, "sail_amd/js/cli.js", "sail_amd/js/examples/materials.js", *bad], cwd=ROOT,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--guide" in r.stderr
