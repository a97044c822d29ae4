"""The noise estimate from the JavaScript host and the CLI (renderer.renderUntil / noiseMark / noise, cli.js --noise).
Needs node; the rendering cases need a GPU."""
import json
import os
import shutil
import subprocess

import pytest

from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node") or shutil.which("nodejs")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")
CLI = ["sail_amd/js/cli.js", "sail_amd/js/examples/cornell.js"]


def test_cli_noise_excludes_spp():
    """--noise with --spp is an error before any device is touched (so is --min-spp without --noise)"""
    r = subprocess.run([NODE, *CLI, "--noise", "0.01", "--spp", "4"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 1 and "--noise and --spp" in r.stderr
    r = subprocess.run([NODE, *CLI, "--min-spp", "4"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 1 and "needs --noise" in r.stderr


def test_cli_help_shows_the_whole_usage_header():
    out = subprocess.run([NODE, "sail_amd/js/cli.js", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--noise X" in out and "--stats" in out
    assert out.rstrip().endswith("unfiltered mean image.") and "require(" not in out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mix", "sum"])
def test_js_render_until(mode):
    """renderUntil to the cap on the Cornell example at 64x64: k = scene.sampleCount, and the frame is the one
    renderSamples(k) gives a second renderer; then noiseMark() / noise() by hand"""
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "noise_check.js"), "64", "64", "0", "4", "24", mode],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    res = r["res"]
    assert res["k"] == 24 and r["sampleCount"] == 24 and res["converged"] is False
    assert [s["k"] for s in res["history"]] == [4, 8, 16, 24]
    assert res["history"][0]["mean"] is None              # the first look only marks: +inf, null in JSON
    assert res["mean"] == res["history"][-1]["mean"] > 0 and res["maxTile"] >= res["mean"]
    assert r["same"] is True
    assert r["early"] and "no sample since the mark" in r["early"]
    n = r["noise"]
    assert (n["k"], n["kMark"], n["tilesX"], n["tilesY"], n["tiles"], n["nonfinite"]) == (48, 24, 4, 4, 16, 0)
    assert 0 < n["mean"] <= n["maxTile"]
    assert abs(n["tileMax"] - n["maxTile"]) <= 2.0 ** -23 * n["maxTile"]   # the tile map is the f32 of the same means


@pytest.mark.gpu
def test_cli_noise_stats():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    r = subprocess.run([NODE, *CLI, "--width", "40", "--height", "30", "--noise", "1e30", "--min-spp", "4", "--stats",
                        "--deterministic"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["spp"] == 8 and st["converged"] is True
    assert 0 < st["noise"] < 1e30
    assert st["segments"] == 40 * 30 * 8 * 5   # closed box: every path runs all bounces
