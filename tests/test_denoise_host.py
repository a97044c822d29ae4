"""CPU: the host-only side of the denoiser (include/sail_hip.h): sail_denoise_defaults, the null context, and the CLI's
--denoise options, which are checked before a device is touched."""
import ctypes
import os
import shutil
import subprocess

import pytest

from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node") or shutil.which("nodejs")
needs_node = pytest.mark.skipif(NODE is None, reason="node not installed")
CLI = ["sail_amd/js/cli.js", "sail_amd/js/examples/cornell.js"]


def test_defaults_are_the_documented_ones():
    d = capi.denoise_defaults()
    assert d["iterations"] == 4 and d["display"] == capi.FILTER_COLOR
    f32 = lambda v: ctypes.c_float(v).value
    assert (d["sigma_l"], d["sigma_x"], d["gamma_c"]) == (1.0, f32(0.2), f32(2.2))
    assert capi.load().sail_denoise_defaults(None) == -1


def test_null_context_is_rejected():
    lib = capi.load()
    info = capi.DenoiseInfo()
    assert lib.sail_denoise(None, None, None, None, None, ctypes.byref(info)) == -1


@needs_node
def test_cli_rejects_bad_denoise_options_before_a_device():
    for extra, text in ((["--denoise", "--spp", "1"], "--spp 2 or more"),
                        (["--denoise", "--spp", "8", "--denoise-iterations", "9"], "from 1 to 6"),
                        (["--spp", "8", "--denoise-iterations", "2"], "needs --denoise"),
                        (["--denoise", "--spp", "8", "--filter", "normal", "--png", "x.png"], "color, gamma or tonemapping")):
        r = subprocess.run([NODE, *CLI, *extra], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stderr)
        assert "HIP" not in r.stderr and "device" not in r.stderr


@needs_node
def test_cli_help_lists_denoise():
    out = subprocess.run([NODE, "sail_amd/js/cli.js", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--denoise" in out and "--denoise-iterations" in out and "--noise X" in out
    assert out.rstrip().endswith("unfiltered mean image.") and "require(" not in out
