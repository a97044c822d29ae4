#!/usr/bin/env python3
"""Device time of moment tracking and of sail_temporal_filter at 1920x1080 on one MI355X.

The moves of tools/temporal_profile.py: C2 (the README Cornell box, 8 bounces), the camera swings between two views 3
degrees apart; at every move the frame is reset, the new view begun, one sample rendered and the view resolved. Two contexts
make every move one after the other, one with moment tracking and one without, so begin and resolve are timed with tracking
on and off in the same run. After the resolve the tracking context is filtered three times: with the defaults, with
min_hist 1 (every pixel takes the variance of its moments) and with min_hist 1e9 (every pixel runs the 49-tap spatial
estimate), so the cost of the spatial path is known. After 5 warm-up moves, 20 moves: HIP-event medians and min-max. Then
sail_denoise's own passes on the same context (one sample, the mark, one sample), the same number of calls, for the a-trous
passes side by side. For the prepare pass the algorithmic bytes (every map counted once: Out, Mout, N and X read, the
count of S read, (c, v), g0 and g1 written; the halo's second reads come from cache) and their rate against the 8.0 TB/s
HBM peak. The working set fits the 256 MB last-level cache, so the rates are effective ones. Run from the repository
root; writes profiles/temporal_filter_1080p.json (or the path given)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))

import bench
from sail_amd import capi
from temporal_profile import views

W, H = 1920, 1080
WARMUP, CALLS = 5, 20
HBM = 8.0e12
BOUNCES = 8
# bytes per pixel of the prepare pass (SUM accumulation): Out, Mout, N, X (4 x 16) and S.w (4) read; cv, g0 (2 x 16), g1 (8) written
PREPARE_B = 4 * 16 + 4 + 2 * 16 + 8
FILTERS = {"defaults": None, "all_temporal": {"min_hist": 1.0}, "all_spatial": {"min_hist": 1e9}}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "temporal_filter_1080p.json")
    sc = bench.load_scene("C1")
    vs = views(sc, 3.0)
    ctxs = {}
    for name in ("tracking_off", "tracking_on"):
        ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
        ctx.set_scene_dict(sc)
        ctx.kernel_ready(-1)       # the scene's run-time kernel is loaded before anything is timed
        ctxs[name] = ctx
    ctxs["tracking_on"].temporal_moments(True)
    runs = {"tracking_off": [], "tracking_on": []}
    filt = {k: [] for k in FILTERS}
    for i in range(WARMUP + CALLS):
        mvp, eye = vs[i % 2]
        for name, ctx in ctxs.items():
            ctx.reset()
            begin = ctx.temporal_begin(mvp, eye)
            ctx.render_schedule(*capi.schedule(mvp, W, H, 0, 1), eye, BOUNCES)
            frame_ms = ctx.stats().kernel_ms
            res = ctx.temporal_resolve(want_u8=True)
            if i >= WARMUP:
                runs[name].append({"gbuffer": begin["pass_ms"][0], "reproject": begin["pass_ms"][1],
                                   "resolve": res["pass_ms"][2], "frame_1spp": frame_ms,
                                   "history": begin["history_pixels"] / max(1, begin["hit_pixels"])})
        for key, p in FILTERS.items():
            out = ctxs["tracking_on"].temporal_filter(p, want_u8=True)
            if i >= WARMUP:
                filt[key].append({"prepare": out["pass_ms"][0], "atrous": out["pass_ms"][1:], "total": out["kernel_ms"],
                                  "temporal_share": out["temporal_pixels"] / (W * H), "nonfinite": out["nonfinite"]})
    # sail_denoise on the same context and view: one sample, the mark, one sample
    ctx = ctxs["tracking_on"]
    mvp, eye = vs[0]
    ctx.reset()
    ctx.render_schedule(*capi.schedule(mvp, W, H, 0, 1), eye, BOUNCES)
    ctx.noise_mark()
    ctx.render_schedule(*capi.schedule(mvp, W, H, 1, 1), eye, BOUNCES)
    den = []
    for i in range(WARMUP + CALLS):
        out = ctx.denoise(want_u8=True)
        if i >= WARMUP:
            den.append({"prepare": out["pass_ms"][0], "atrous": out["pass_ms"][1:], "total": out["kernel_ms"]})
    for c in ctxs.values():
        c.close()

    col = lambda rows, f: [r[f] for r in rows]
    res = {"what": __doc__, "width": W, "height": H, "hbm_peak_bytes_per_s": HBM, "samples": CALLS, "warmup": WARMUP,
           "scene": "C2 (8 bounces)"}
    res["moves"] = {name: {f: spread(col(rows, f)) for f in ("gbuffer", "reproject", "resolve", "frame_1spp", "history")}
                    for name, rows in runs.items()}
    res["tracking_cost_ms"] = {f: res["moves"]["tracking_on"][f]["median"] - res["moves"]["tracking_off"][f]["median"]
                               for f in ("reproject", "resolve")}
    res["filter"] = {}
    for key, rows in filt.items():
        ms = spread(col(rows, "prepare"))
        b = PREPARE_B * W * H
        res["filter"][key] = {
            "prepare_ms": ms, "prepare_bytes_per_pixel": PREPARE_B, "prepare_bytes": b,
            "prepare_bytes_per_s": b / (ms["median"] * 1e-3), "prepare_hbm_peak_fraction": b / (ms["median"] * 1e-3) / HBM,
            "atrous_ms": [spread([r["atrous"][j] for r in rows]) for j in range(len(rows[0]["atrous"]))],
            "total_ms": spread(col(rows, "total")), "temporal_share": spread(col(rows, "temporal_share")),
            "nonfinite_max": max(col(rows, "nonfinite"))}
    res["denoise"] = {"prepare_ms": spread(col(den, "prepare")),
                      "atrous_ms": [spread([r["atrous"][j] for r in den]) for j in range(len(den[0]["atrous"]))],
                      "total_ms": spread(col(den, "total"))}
    res["spatial_path_cost_ms"] = (res["filter"]["all_spatial"]["prepare_ms"]["median"]
                                   - res["filter"]["all_temporal"]["prepare_ms"]["median"])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({
        "begin_reproject_off_on": [round(res["moves"][n]["reproject"]["median"], 4) for n in runs],
        "resolve_off_on": [round(res["moves"][n]["resolve"]["median"], 4) for n in runs],
        "prepare_ms": {k: round(v["prepare_ms"]["median"], 4) for k, v in res["filter"].items()},
        "prepare_hbm_fraction": {k: round(v["prepare_hbm_peak_fraction"], 3) for k, v in res["filter"].items()},
        "filter_total_ms": {k: round(v["total_ms"]["median"], 4) for k, v in res["filter"].items()},
        "denoise_total_ms": round(res["denoise"]["total_ms"]["median"], 4),
        "frame_1spp_ms": round(res["moves"]["tracking_on"]["frame_1spp"]["median"], 4)}))


if __name__ == "__main__":
    main()
