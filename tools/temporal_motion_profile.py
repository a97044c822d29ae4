#!/usr/bin/env python3
"""Device time of the reproject pass with an object motion pending (sail_move_objects, then sail_temporal_begin) at
1920x1080 on one MI355X, beside the plain reproject pass in the same run.

C2 (the README Cornell box, 8 bounces) from its own camera, which stands still. Two kinds of move alternate: a plain one
(the frame is reset and the same view begun again: sail_reproject_kernel) and a drag step (the mirror sphere, row 2, goes
back and forth by (0.3, 0, 0.2) through sail_move_objects with hist_cap 8, then the same view is begun:
sail_reproject_moved_kernel, which loads the row's translation from a table of n float4 per pixel). After every begin one
sample is rendered and the view resolved, so every reproject pass gathers a real history. After 5 warm-up moves of each
kind, 20 of each: HIP-event medians and min-max of the G-buffer pass and the reproject pass. The same again with moment
tracking on, where the reproject figure also holds the moment reproject (sail_moment_reproject_kernel /
sail_moment_reproject_moved_kernel). Run from the repository root; writes profiles/temporal_motion_1080p.json (or the path
given)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np

import bench
from sail_amd import capi

W, H = 1920, 1080
WARMUP, CALLS = 5, 20
ROW, STEP = 2, (0.3, 0.0, 0.2)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(moments, bounces=8):
    sc = bench.load_scene("C1")
    n = sc["n"]
    eye, center = np.array(sc["eye"], np.float64), np.array(sc["center"], np.float64)
    mvp, eye32 = capi.camera(eye, center, [0, 1, 0], 55.0, W / H, 1.0, 100.0).reshape(16), eye.astype(np.float32)
    home = np.array(sc["objects"], np.float32).reshape(n, 18)
    assert int(home[ROW, 0]) == 2                       # a sphere: words 1..3 are its centre
    away = home.copy()
    away[ROW, 1:4] = away[ROW, 1:4] + np.array(STEP, np.float32)
    ctx = capi.Context(W, H)
    ctx.set_scene_dict(sc)
    if moments:
        ctx.temporal_moments(True)
    ctx.kernel_ready(-1)
    runs = {"plain": [], "moved": []}
    at_home = True
    for i in range(2 * (WARMUP + CALLS)):
        kind = "moved" if i % 2 else "plain"
        if kind == "moved":
            motion = np.zeros((n, 3), np.float32)
            motion[ROW] = np.array(STEP, np.float32) * np.float32(1 if at_home else -1)
            ctx.move_objects(away if at_home else home, motion, 8.0)
            at_home = not at_home
            assert ctx.temporal_pending_motion()["pending"] == 1
        else:
            ctx.reset()
        begin = ctx.temporal_begin(mvp, eye32)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, 1), eye32, bounces)
        res = ctx.temporal_resolve()
        if i >= 2 * WARMUP:
            runs[kind].append({"gbuffer": begin["pass_ms"][0], "reproject": begin["pass_ms"][1],
                               "history": begin["history_pixels"] / max(1, begin["hit_pixels"]), "nonfinite": res["nonfinite"]})
    ctx.close()
    out = {}
    for kind, rs in runs.items():
        out[kind] = {"gbuffer_ms": spread([r["gbuffer"] for r in rs]), "reproject_ms": spread([r["reproject"] for r in rs]),
                     "history_share_of_hit_pixels": spread([r["history"] for r in rs]),
                     "nonfinite_max": max(r["nonfinite"] for r in rs), "moves": len(rs)}
    out["moved_over_plain_reproject"] = out["moved"]["reproject_ms"]["median"] / out["plain"]["reproject_ms"]["median"]
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "temporal_motion_1080p.json")
    res = {"what": __doc__, "width": W, "height": H, "samples": CALLS, "warmup": WARMUP,
           "colour_only": run(False), "with_moment_tracking": run(True)}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {kind: round(res[k][kind]["reproject_ms"]["median"], 4) for kind in ("plain", "moved")}
                      | {"ratio": round(res[k]["moved_over_plain_reproject"], 3)}
                      for k in ("colour_only", "with_moment_tracking")}))


if __name__ == "__main__":
    main()
