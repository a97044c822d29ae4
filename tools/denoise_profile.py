#!/usr/bin/env python3
"""Device time of the denoiser (sail_denoise) at 1920x1080 on one MI355X, next to the display filter it supersedes.

The C2 frame (the README Cornell box, 8 bounces) with 64 spp and the noise mark at 32. After 5 warm-up calls, 20 calls
of sail_denoise with the defaults: median and min-max of kernel_ms and of every pass (HIP events), the algorithmic
bytes each pass moves and their rate against the 8 TB/s HBM peak. The working set (about 130 MB) fits the 256 MB
last-level cache, so the rates are effective ones, not sustained HBM rates. In the same run: the same calls with the
variance and RGBA8 outputs, with 6 passes, and filter_ms() of one SAIL_FILTER_WAVELET pass (r = 2), the existing
denoiser. Run from the repository root; writes profiles/denoise_1080p.json (or the path given)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np

import bench
from sail_amd import capi

W, H, B, SPP, MARK = 1920, 1080, 8, 64, 32
WARMUP, CALLS = 5, 20
HBM = 8.0e12
# bytes per pixel: prepare reads S, P, N, X (4 x 16) and writes (c, v), the guides (16 + 16 + 8); a pass reads those 40
# and writes 16; the last pass may add the variance (4) and the RGBA8 word (4)
PREPARE_B, PASS_B = 64 + 40, 40 + 16


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rate(ms, bytes_per_pixel):
    b = bytes_per_pixel * W * H
    return {"bytes_per_pixel": bytes_per_pixel, "bytes": b, "bytes_per_s": b / (ms * 1e-3),
            "hbm_peak_fraction": b / (ms * 1e-3) / HBM}


def measure(ctx, params, extra):
    for _ in range(WARMUP):
        ctx.denoise(params, want_var=extra, want_u8=extra)
    runs = [ctx.denoise(params, want_var=extra, want_u8=extra) for _ in range(CALLS)]
    n = runs[0]["iterations"]
    out = {"iterations": n, "samples": CALLS, "kernel_ms": spread([r["kernel_ms"] for r in runs]), "passes": []}
    for i in range(n + 1):
        ms = spread([r["pass_ms"][i] for r in runs])
        bpp = PREPARE_B if i == 0 else PASS_B + (8 if extra and i == n else 0)
        taps_ms = None if i == 0 else ms["median"] / 25
        out["passes"].append({"pass": "prepare" if i == 0 else f"atrous step {1 << (i - 1)}", "ms": ms,
                              "ms_per_tap": taps_ms, **rate(ms["median"], bpp)})
    return out, runs[-1]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "denoise_1080p.json")
    sc = bench.load_scene("C1")
    mvp = capi.camera(sc["eye"], sc["center"], [0, 1, 0], 55.0, W / H, 1.0, 100.0)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    ctx.set_scene_dict(sc)
    ctx.render_schedule(*capi.schedule(mvp, W, H, 0, MARK), sc["eye"], B)
    ctx.noise_mark()
    ctx.render_schedule(*capi.schedule(mvp, W, H, MARK, SPP - MARK), sc["eye"], B)
    est = ctx.noise_estimate()
    res = {"what": __doc__, "width": W, "height": H, "scene": "C2 (README Cornell box, 8 bounces)", "spp": SPP, "mark": MARK,
           "hbm_peak_bytes_per_s": HBM, "noise_mean": est["mean"], "runs": {}}
    res["runs"]["defaults"], last = measure(ctx, None, False)
    res["runs"]["defaults_var_u8"], _ = measure(ctx, None, True)
    res["runs"]["six_passes"], _ = measure(ctx, {"iterations": 6}, False)
    res["nonfinite"] = last["nonfinite"]
    # what the passes change: mean luminance is kept, the estimated variance of the mean falls
    noisy = ctx.readback()[..., :3]
    res["mean_rgb_in"] = [float(v) for v in noisy.reshape(-1, 3).mean(axis=0, dtype=np.float64)]
    res["mean_rgb_out"] = [float(v) for v in last["rgba"][..., :3].reshape(-1, 3).mean(axis=0, dtype=np.float64)]
    ms = []
    for i in range(WARMUP + CALLS):
        ctx.filter(capi.FILTER_WAVELET, rx=2.0, ry=2.0)
        if i >= WARMUP:
            ms.append(ctx.filter_ms())
    taps = 25 + 13 + 7   # wavelet.glsl's three levels skip the taps whose kernel weight is 0
    res["wavelet_filter"] = {"what": "sail_filter SAIL_FILTER_WAVELET, r = (2, 2): one pass of three levels, 45 taps with a "
                             "non-zero weight, each two bilinear samples from global memory", "samples": CALLS,
                             "ms": spread(ms), "taps": taps, "ms_per_tap": statistics.median(ms) / taps}
    ctx.close()
    d = res["runs"]["defaults"]
    atrous = [p["ms_per_tap"] for p in d["passes"][1:]]
    res["atrous_ms_per_tap_median"] = statistics.median(atrous)
    res["atrous_vs_wavelet_per_tap"] = res["atrous_ms_per_tap_median"] / res["wavelet_filter"]["ms_per_tap"]
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"kernel_ms": d["kernel_ms"], "passes": [(p["pass"], round(p["ms"]["median"], 4),
                                                                round(p["hbm_peak_fraction"], 3)) for p in d["passes"]],
                      "wavelet_ms": res["wavelet_filter"]["ms"], "per_tap_ratio": res["atrous_vs_wavelet_per_tap"]}))


if __name__ == "__main__":
    main()
