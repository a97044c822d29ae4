"""The option temporal: {objects: true} of the JavaScript host: a Pickup drag of the materials demo's matte sphere keeps the
history (Renderer.updateObjects -> sail_move_objects). Needs node and a GPU. tests/js/motion_check.js reports the rows, the
motion and the view of every step; the same calls are made through capi, so renderer.image() must give the same bytes.
With temporal: true alone a drag drops the history at each move, as before."""
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
ROW = 5


def fnv(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


def through_js(objects):
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "motion_check.js"), str(W), str(H), "1" if objects else "0"],
                         cwd=ROOT, capture_output=True, text=True, check=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def replay(fixtures, steps, objects, hist_cap=8.0):
    """the JS host's calls through capi: a moved step hands the rows to sail_move_objects (option on) or
    sail_update_objects (off); a step whose sample count restarted resets the frame and begins the view; the image is the
    resolve's RGBA8. The renderer's accumulation default is the running mean, its colour filter passes gamma 1."""
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    sc = fixtures["scenes"]["C3"]
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV | capi.FLAG_SEGMENT_COUNT)
    hashes, infos = [], []
    try:
        ctx.set_accum_mode(capi.ACCUM_MIX)
        ctx.set_scene_dict(sc)
        k = 0
        for s in steps:
            mvp, eye = np.array(s["mvp"], np.float64), np.array(s["eye"], np.float32)
            if s["moved"]:
                rows = np.array(s["rows"], np.float32)
                if objects:
                    ctx.move_objects(rows, np.array(s["motion"], np.float32), hist_cap)
                else:
                    assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]) == 0
            if s["k"] == s["n"]:                                   # the frame restarted
                ctx.reset()
                k = 0
                infos.append(ctx.temporal_begin(mvp, eye))
            ctx.render_schedule(*capi.schedule(mvp, W, H, k, s["n"]), eye, B)
            k += s["n"]
            assert k == s["k"]
            u8 = ctx.temporal_resolve({"display": capi.FILTER_COLOR, "gamma_c": 1.0}, want_u8=True)["u8"]
            hashes.append(fnv(u8.tobytes()))
    finally:
        ctx.close()
    return hashes, infos


def check_steps(fixtures, js):
    steps = js["steps"]
    n = fixtures["scenes"]["C3"]["n"]
    assert js["selected"] == ROW and js["began"]
    assert [s["k"] for s in steps] == [4, 1, 1, 1, 3] and [s["moved"] for s in steps] == [False, True, True, True, False]
    assert all(s["mvp"] == steps[0]["mvp"] for s in steps)         # the camera stands still
    rows = np.array(fixtures["scenes"]["C3"]["objects"], np.float32).reshape(n, 18)
    for s in steps[1:4]:
        motion, new = np.array(s["motion"], np.float32).reshape(n, 3), np.array(s["rows"], np.float32).reshape(n, 18)
        assert motion[ROW].any() and not motion[np.arange(n) != ROW].any()
        assert np.abs((new[ROW, 1:4] - rows[ROW, 1:4]) - motion[ROW]).max() <= 1e-6
        rows = new


def test_js_drag_keeps_the_history(fixtures):
    js = through_js(True)
    check_steps(fixtures, js)
    assert js["histCap"] == 8
    hashes, infos = replay(fixtures, js["steps"], True)
    print(f"drag with the option: history pixels per begin {[i['history_pixels'] for i in infos]} of "
          f"{[i['hit_pixels'] for i in infos]}")
    assert [s["hash"] for s in js["steps"]] == hashes and len(set(hashes)) == len(hashes)
    assert infos[0]["history_pixels"] == 0 and all(i["history_pixels"] > 0.8 * i["hit_pixels"] for i in infos[1:])
    # the option changes what a drag shows: not the bytes of a history dropped at each move
    dropped, _ = replay(fixtures, js["steps"], False)
    assert dropped[0] == hashes[0] and all(a != b for a, b in zip(dropped[1:], hashes[1:]))
    # and the cap reaches the library: the counts here run 4, 5, 6, so the default 8 never binds and a cap of 2 does
    uncapped, _ = replay(fixtures, js["steps"], True, hist_cap=0.0)
    tight, _ = replay(fixtures, js["steps"], True, hist_cap=2.0)
    assert uncapped == hashes and tight[0] == hashes[0] and tight[1] != hashes[1]


def test_js_without_the_option_drops_the_history(fixtures):
    js = through_js(False)
    check_steps(fixtures, js)
    assert js["histCap"] is None
    hashes, infos = replay(fixtures, js["steps"], False)
    assert [s["hash"] for s in js["steps"]] == hashes
    assert all(i["history_pixels"] == 0 for i in infos)
