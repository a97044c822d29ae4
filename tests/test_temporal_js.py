"""The temporal option of the JavaScript host (Renderer({temporal: true}), renderer.gbuffer / temporalBegin /
temporalResolve), orbited and zoomed by Sail.Control. Needs node and a GPU. tests/js/temporal_check.js reports every view it
rendered; the same calls are made through capi, so renderer.image() must give the same bytes. With the option off the
frames are today's: the display filter over the bare frame."""
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
KIND = {"color": capi.FILTER_COLOR, "tonemapping": capi.FILTER_TONEMAPPING}


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


def through_js(filter_name, temporal):
    """temporal: False, True, or "cap:posTol" for the option's object form"""
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "temporal_check.js"), str(W), str(H), filter_name,
                          temporal if isinstance(temporal, str) else ("1" if temporal else "0")],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def replay(fixtures, steps, kind, temporal, params=None):
    """the JS host's calls through capi: a step whose sample count restarted resets the frame and, with the option on,
    begins the view; the image is the resolve's RGBA8 (option on) or sail_filter's (off). The renderer's accumulation
    default is the running mean, its colour and tonemapping filters pass gamma 1."""
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV | capi.FLAG_SEGMENT_COUNT)
    hashes = []
    try:
        ctx.set_accum_mode(capi.ACCUM_MIX)
        ctx.set_scene_dict(fixtures["scenes"]["C1"])
        k = 0
        for s in steps:
            mvp, eye = np.array(s["mvp"], np.float64), np.array(s["eye"], np.float32)
            if s["k"] == s["n"]:                                   # the view changed: the frame restarted
                ctx.reset()
                k = 0
                if temporal:
                    ctx.temporal_begin(mvp, eye, params)
            ctx.render_schedule(*capi.schedule(mvp, W, H, k, s["n"]), eye, B)
            k += s["n"]
            assert k == s["k"]
            if temporal:
                u8 = ctx.temporal_resolve(dict(params or {}, display=kind, gamma_c=1.0), want_u8=True)["u8"]
            else:
                u8 = ctx.filter(kind, gamma_c=1.0, want_u8=True)[1]
            hashes.append(fnv(u8.tobytes()))
        last = None
        if temporal:
            mvp, eye = np.array(steps[-1]["mvp"], np.float64), np.array(steps[-1]["eye"], np.float32)
            g = ctx.gbuffer(mvp, eye)
            res = ctx.temporal_resolve(dict(params or {}, display=capi.FILTER_GAMMA, gamma_c=2.2), want_u8=True)
            last = {"id": fnv(g["id"].tobytes()), "t": fnv(g["t"].tobytes()), "xyz": fnv(g["xyz"].tobytes()),
                    "resolve": fnv(res["rgba"].tobytes()), "resolve8": fnv(res["u8"].tobytes()), "info": res}
    finally:
        ctx.close()
    return hashes, last


@pytest.mark.parametrize("filter_name", ["color", "tonemapping"])
def test_js_temporal_equals_capi(fixtures, filter_name):
    js = through_js(filter_name, True)
    steps = js["steps"]
    assert [s["k"] for s in steps] == [4, 1, 3, 1, 3]              # Control's moves restarted the frame three times
    assert steps[1]["mvp"] == steps[2]["mvp"] and steps[0]["mvp"] != steps[1]["mvp"] != steps[3]["mvp"] != steps[4]["mvp"]
    hashes, last = replay(fixtures, steps, KIND[filter_name], True)
    assert [s["hash"] for s in steps] == hashes
    assert len(set(hashes)) == len(hashes)
    gb = js["gb"]
    assert (gb["id"], gb["t"], gb["xyz"]) == (last["id"], last["t"], last["xyz"])
    assert (gb["resolve"], gb["resolve8"]) == (last["resolve"], last["resolve8"])
    info = last["info"]
    assert gb["info"]["historyPixels"] == info["history_pixels"] > 0 and gb["info"]["hitPixels"] == info["hit_pixels"]
    assert gb["info"]["k"] == 3 and len(gb["info"]["passMs"]) == 3
    # the option changes what image() shows after a move: not the bare frame's bytes
    plain, _ = replay(fixtures, steps, KIND[filter_name], False)
    assert plain[0] == hashes[0] and plain[1] != hashes[1]


def test_js_temporal_option_object(fixtures):
    """temporal: {cap, posTol} reaches the library: the bytes are those of capi with the same parameters, and they are not
    the defaults' bytes"""
    js = through_js("color", "4:0.01")
    hashes, last = replay(fixtures, js["steps"], capi.FILTER_COLOR, True, {"cap": 4.0, "pos_tol": 0.01})
    assert [s["hash"] for s in js["steps"]] == hashes
    assert (js["gb"]["resolve"], js["gb"]["resolve8"]) == (last["resolve"], last["resolve8"])
    assert js["gb"]["info"]["historyPixels"] == last["info"]["history_pixels"] > 0
    defaults, last_d = replay(fixtures, js["steps"], capi.FILTER_COLOR, True)
    assert defaults[0] == hashes[0] and defaults[1:] != hashes[1:]
    assert last_d["info"]["history_pixels"] > last["info"]["history_pixels"]      # the tighter tolerance finds less


def test_js_without_the_option_is_unchanged(fixtures):
    js = through_js("tonemapping", False)
    assert js["gb"] is None
    hashes, _ = replay(fixtures, js["steps"], capi.FILTER_TONEMAPPING, False)
    assert [s["hash"] for s in js["steps"]] == hashes
