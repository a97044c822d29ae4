"""The denoiser from the JavaScript host and the CLI (renderer.denoise, cli.js --denoise). Needs node; the rendering cases
need a GPU. The same frame is made through capi (renderSamples draws capi.schedule's samples), so the outputs must be
equal bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node") or shutil.which("nodejs")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")
CLI = ["sail_amd/js/cli.js", "sail_amd/js/examples/cornell.js"]
W, H, SPP, B = 48, 32, 8, 5


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def through_capi(fixtures):
    """the Cornell example (the frozen scene C1) at 48x32, 8 spp marked after 4: denoised with the defaults, and with
    the second parameter set of tests/js/denoise_check.js"""
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    sc = fixtures["scenes"]["C1"]
    mvp = np.array(sc["mvp_rowmajor"])
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, SPP // 2), sc["eye"], B)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, SPP // 2, SPP - SPP // 2), sc["eye"], B)
        one = ctx.denoise()
        two = ctx.denoise({"iterations": 2, "sigma_l": 2.5, "sigma_x": 0.05, "display": capi.FILTER_TONEMAPPING},
                          want_u8=True)
    finally:
        ctx.close()
    return one, two


@pytest.mark.gpu
def test_js_denoise_equals_capi(through_capi):
    one, two = through_capi
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "denoise_check.js"), str(W), str(H), str(SPP)],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r["noAov"] and "aov: true" in r["noAov"]
    assert r["early"] and "no mark" in r["early"]
    assert r["unchanged"] is True and r["hasU8"] is False
    assert r["hash"] == fnv(np.ascontiguousarray(one["rgba"][..., :3]).tobytes())
    assert r["hash2"] == fnv(two["rgba"].tobytes()) and r["hashU8"] == fnv(two["u8"].tobytes())
    i = r["info"]
    assert (i["k"], i["kMark"], i["nonfinite"], i["iterations"], len(i["passMs"])) == (8, 4, one["nonfinite"], 4, 5)
    assert r["info2"]["iterations"] == 2 and i["kernelMs"] > 0


@pytest.mark.gpu
def test_cli_denoise_pfm(through_capi, tmp_path):
    one, _ = through_capi
    pfm = tmp_path / "d.pfm"
    r = subprocess.run([NODE, *CLI, "--width", str(W), "--height", str(H), "--spp", str(SPP), "--deterministic", "--denoise",
                        "--pfm", str(pfm), "--stats"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["spp"] == SPP and st["denoise_ms"] > 0
    raw = pfm.read_bytes()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(one["rgba"][..., :3]).view(np.uint32))
