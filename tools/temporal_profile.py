#!/usr/bin/env python3
"""Device time of the camera-motion reprojection passes (sail_temporal_begin / sail_temporal_resolve) at 1920x1080 on one
MI355X, next to the 1-spp frame they have to fit beside.

C2 (the README Cornell box, 8 bounces): the camera swings between two views 3 degrees apart; at every move the frame is
reset, the new view begun (G-buffer pass + reproject pass), one sample rendered and the view resolved, so every reproject
pass gathers a real history. After 5 warm-up moves, 20 moves: HIP-event medians and min-max of the three passes and of the
1-spp trace launch of the same move (sail_get_stats kernel_ms, which a reset zeroes). The context waits for the scene's run-time kernel
before anything is timed, and the kernel each launch ran is recorded. A launch of one sample fills the device badly (the
Cornell form keeps 16 and more samples of a pixel in flight), so the per-sample cost of one 64-sample launch of the same
view is recorded beside it: an interactive frame pays the first figure, a batch render the second. The G-buffer pass is
also timed on C4 (67 rows: the sweep is one loop over all of them). For each pass the algorithmic bytes (every map counted once, though the reproject
gather touches G_prev and Hist up to four times per pixel) and their rate against the 8.0 TB/s HBM peak. The working set
(five float4 maps and the frame, about 200 MB) fits the 256 MB last-level cache, so the rates are effective ones. Run from
the repository root; writes profiles/temporal_1080p.json (or the path given)."""
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
HBM = 8.0e12
# bytes per pixel: the G-buffer pass writes G (16); reproject reads G_cur, G_prev and Hist (3 x 16) and writes R (16);
# resolve reads S and R (2 x 16) and writes Out (16) and the RGBA8 word (4)
GBUFFER_B, REPROJECT_B, RESOLVE_B = 16, 64, 52


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rate(ms, bytes_per_pixel):
    b = bytes_per_pixel * W * H
    return {"bytes_per_pixel": bytes_per_pixel, "bytes": b, "bytes_per_s": b / (ms * 1e-3),
            "hbm_peak_fraction": b / (ms * 1e-3) / HBM}


def views(sc, deg):
    """the scene's camera and the same camera swung `deg` degrees about the vertical axis through what it looks at"""
    eye, center = np.array(sc["eye"], np.float64), np.array(sc["center"], np.float64)
    out = []
    for a in (0.0, np.deg2rad(deg)):
        d = eye - center
        e = center + np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])
        out.append((capi.camera(e, center, [0, 1, 0], 55.0, W / H, 1.0, 100.0).reshape(16), e.astype(np.float32)))
    return out


def moves(name, bounces, deg=3.0):
    sc = bench.load_scene(name)
    vs = views(sc, deg)
    ctx = capi.Context(W, H)
    ctx.set_scene_dict(sc)
    ready = ctx.kernel_ready(-1)   # the scene's run-time kernel is loaded before anything is timed
    runs = []
    for i in range(WARMUP + CALLS):
        mvp, eye = vs[i % 2]
        ctx.reset()
        begin = ctx.temporal_begin(mvp, eye)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, 1), eye, bounces)
        frame_ms = ctx.stats().kernel_ms
        kernel = ctx.kernel_name()
        res = ctx.temporal_resolve(want_u8=True)
        if i >= WARMUP:
            runs.append({"gbuffer": begin["pass_ms"][0], "reproject": begin["pass_ms"][1], "resolve": res["pass_ms"][2],
                         "frame_1spp": frame_ms, "history": begin["history_pixels"] / max(1, begin["hit_pixels"]),
                         "nonfinite": res["nonfinite"], "kernel": kernel})
    # the same view in one 64-sample launch, per sample
    batch = []
    for i in range(WARMUP + CALLS):
        ctx.reset()
        ctx.set_launch_samples(64)
        ctx.render_schedule(*capi.schedule(vs[0][0], W, H, 0, 64), vs[0][1], bounces)
        if i >= WARMUP:
            batch.append(ctx.stats().kernel_ms / 64)
    info = {"jit_ready": bool(ready), "kernel_1spp": sorted({r["kernel"] for r in runs}), "kernel_64spp": ctx.kernel_name(),
            "per_sample_of_a_64spp_launch_ms": spread(batch)}
    ctx.close()
    return sc, runs, info


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "temporal_1080p.json")
    res = {"what": __doc__, "width": W, "height": H, "hbm_peak_bytes_per_s": HBM, "samples": CALLS, "warmup": WARMUP}
    sc2, c2, i2 = moves("C1", 8)
    sc4, c4, i4 = moves("C4", 12)
    col = lambda runs, f: [r[f] for r in runs]
    passes = {}
    for key, runs, f, bpp in (("gbuffer_C2", c2, "gbuffer", GBUFFER_B), ("gbuffer_C4", c4, "gbuffer", GBUFFER_B),
                              ("reproject_C2", c2, "reproject", REPROJECT_B), ("resolve_C2", c2, "resolve", RESOLVE_B)):
        ms = spread(col(runs, f))
        passes[key] = {"ms": ms, **rate(ms["median"], bpp)}
    res["passes"] = passes
    res["rows"] = {"C2": sc2["n"], "C4": sc4["n"]}
    res["frame_1spp_ms"] = {"C2 (8 bounces)": spread(col(c2, "frame_1spp")), "C4 (12 bounces)": spread(col(c4, "frame_1spp"))}
    res["trace_kernels"] = {"C2": i2, "C4": i4}
    res["history_share_of_hit_pixels"] = {"C2": spread(col(c2, "history")), "C4": spread(col(c4, "history"))}
    res["nonfinite_max"] = max(col(c2, "nonfinite") + col(c4, "nonfinite"))
    three = passes["gbuffer_C2"]["ms"]["median"] + passes["reproject_C2"]["ms"]["median"] + passes["resolve_C2"]["ms"]["median"]
    res["three_passes_C2_ms"] = three
    res["three_passes_vs_frame_1spp_C2"] = three / res["frame_1spp_ms"]["C2 (8 bounces)"]["median"]
    res["three_passes_vs_one_sample_of_a_64spp_launch_C2"] = three / i2["per_sample_of_a_64spp_launch_ms"]["median"]
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(v["ms"]["median"], 4), round(v["hbm_peak_fraction"], 3)) for k, v in passes.items()}
                     | {"frame_1spp_C2_ms": round(res["frame_1spp_ms"]["C2 (8 bounces)"]["median"], 4),
                        "three_vs_frame": round(res["three_passes_vs_frame_1spp_C2"], 3),
                        "per_sample_64spp_C2_ms": round(i2["per_sample_of_a_64spp_launch_ms"]["median"], 4),
                        "kernels_C2": i2["kernel_1spp"] + [i2["kernel_64spp"]]}))


if __name__ == "__main__":
    main()
