#!/usr/bin/env python3
"""Device time of the guide maps (sail_guides) and of the guided filters at 1920x1080 on one MI355X, what the AOV stores of
a launch cost, and the quality table of DESIGN.md.

Two frames: C3 (the materials demo: a mirror and a glass sphere, 5 bounces) and C2 (the README Cornell box with its mirror
sphere, 8 bounces), each 16 spp with the noise mark at 8, begun and resolved as one temporal view with moment tracking on.
After 5 warm-up calls, 20 calls each, HIP events, median and min-max:
  * sail_guides at depth 0 and 4 with its counts, next to sail_albedo at grid 1 (the same sweep and a slimmer record) in
    the same session, with the algorithmic bytes (two float4 stores per pixel; the rows come through the scalar cache);
  * sail_denoise and sail_temporal_filter with the AOVs and with the guide maps: kernel_ms and every pass.
Then, C2 only: 20 one-sample launches (after 5) on a context with SAIL_FLAG_AOV and on one without, the device time of each
launch from sail_get_stats: what the two float4 AOV stores per pixel per launch are worth.
Then the quality table at 96x64: relMSE of sail_denoise with the AOVs and with the guide maps (depth 4) against a separate
render from sample index 4096, over all pixels, the followed pixels (Ng.w > 0) and the others.
Run from the repository root; writes profiles/guides_1080p.json (or the path given)."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench
from sail_amd import capi

W, H, SPP, MARK = 1920, 1080, 16, 8
WARMUP, CALLS = 5, 20
HBM = 8.0e12
FRAMES = (("C3", "C3", 5, "C3 (materials demo, 5 bounces)"), ("C2", "C1", 8, "C2 (README Cornell box, 8 bounces)"))
QUALITY = (("C1", 16, 512), ("C3", 16, 512), ("C3", 64, 1024))      # scene, spp (marked at half), reference spp


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(call):
    for _ in range(WARMUP):
        call()
    return [call() for _ in range(CALLS)]


def filter_times(call):
    runs = timed(call)
    n = runs[0]["iterations"]
    return {"samples": CALLS, "kernel_ms": spread([r["kernel_ms"] for r in runs]),
            "pass_ms": [spread([r["pass_ms"][i] for r in runs]) for i in range(n + 1)]}


def view_of(sc, w, h):
    return capi.camera(sc["eye"], sc["center"], [0, 1, 0], 55.0, w / h, 1.0, 100.0).reshape(16), sc["eye"]


def frame(scene, bounces, label):
    sc = bench.load_scene(scene)
    mvp, eye = view_of(sc, W, H)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.temporal_moments(True)
        ctx.temporal_begin(mvp, eye)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, MARK), eye, bounces)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, MARK, SPP - MARK), eye, bounces)
        ctx.temporal_resolve()
        out = {"scene": label, "rows": sc["n"], "spp": SPP, "mark": MARK, "guides": {}}
        runs = timed(lambda: ctx.albedo(mvp, eye, grid=1))
        out["albedo_grid1"] = {"samples": CALLS, "kernel_ms": spread([r["kernel_ms"] for r in runs])}
        for d in (0, 4):
            runs = timed(lambda: ctx.guides(mvp, eye, depth=d))
            ms = spread([r["kernel_ms"] for r in runs])
            b = W * H * 32 + sc["n"] * 128
            last = runs[-1]
            out["guides"][f"depth{d}"] = {
                "samples": CALLS, "kernel_ms": ms, "hit_pixels": last["hit_pixels"], "followed_pixels": last["followed_pixels"],
                "truncated_pixels": last["truncated_pixels"], "max_depth": last["max_depth"], "algorithmic_bytes": b,
                "bytes_per_s": b / (ms["median"] * 1e-3), "hbm_peak_fraction": b / (ms["median"] * 1e-3) / HBM}
        out["denoise"] = filter_times(lambda: ctx.denoise())
        out["temporal_filter"] = filter_times(lambda: ctx.temporal_filter())
        ctx.use_guides(True)
        out["denoise_guided"] = filter_times(lambda: ctx.denoise())
        out["temporal_filter_guided"] = filter_times(lambda: ctx.temporal_filter())
        ctx.use_guides(False)
        out["denoise_again"] = filter_times(lambda: ctx.denoise())
    finally:
        ctx.close()
    return out


def aov_stores(scene, bounces):
    """device ms of a one-sample launch with and without the AOV maps, alternating contexts A B A B"""
    sc = bench.load_scene(scene)
    mvp, eye = view_of(sc, W, H)
    out = {}
    ctxs = {"aov": capi.Context(W, H, flags=capi.FLAG_AOV), "plain": capi.Context(W, H)}
    try:
        for c in ctxs.values():
            c.set_scene_dict(sc)
            c.kernel_ready(-1)
        ms = {k: [] for k in ctxs}
        for rnd in range(2):
            for key, c in ctxs.items():
                for i in range(WARMUP + CALLS // 2):
                    k = int(c.stats().samples)
                    c.render_schedule(*capi.schedule(mvp, W, H, k, 1), eye, bounces)
                    c.sync()
                    if i >= WARMUP:
                        ms[key].append(c.stats().last_launch_ms)
        for key in ctxs:
            out[key] = {"samples": len(ms[key]), "launch_ms": spread(ms[key])}
        out["aov_minus_plain_ms"] = out["aov"]["launch_ms"]["median"] - out["plain"]["launch_ms"]["median"]
        out["stored_bytes_per_launch"] = W * H * 32
    finally:
        for c in ctxs.values():
            c.close()
    return out


def rel_mse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


def quality(scene, spp, R, w=96, h=64, bounces=5):
    sc = bench.load_scene(scene)
    mvp, eye = view_of(sc, w, h)
    ref_ctx = capi.Context(w, h)
    try:
        ref_ctx.set_scene_dict(sc)
        ref_ctx.render_schedule(*capi.schedule(mvp, w, h, 4096, R), eye, bounces)
        ref = ref_ctx.readback()[..., :3]
    finally:
        ref_ctx.close()
    ctx = capi.Context(w, h, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(*capi.schedule(mvp, w, h, 0, spp // 2), eye, bounces)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, w, h, spp // 2, spp - spp // 2), eye, bounces)
        noisy = ctx.readback()[..., :3]
        plain = ctx.denoise()["rgba"][..., :3]
        g = ctx.guides(mvp, eye, depth=4)
        ctx.use_guides(True)
        guided = ctx.denoise()["rgba"][..., :3]
    finally:
        ctx.close()
    spec = g["n"][..., 3] > 0
    rows = {}
    for name, img in (("input", noisy), ("aov", plain), ("followed", guided)):
        rows[name] = {"all": rel_mse(img, ref), "spec": rel_mse(img[spec], ref[spec]), "other": rel_mse(img[~spec], ref[~spec])}
    depths = np.bincount(g["n"][..., 3].astype(int).ravel()).tolist()
    return {"scene": scene, "width": w, "height": h, "spp": spp, "reference_spp": R, "spec_pixels": int(spec.sum()),
            "depth_histogram": depths, "rel_mse": rows}


def main():
    args = sys.argv[1:]
    path = args[0] if args else os.path.join("profiles", "guides_1080p.json")
    res = {"what": __doc__, "width": W, "height": H, "hbm_peak_bytes_per_s": HBM, "frames": {}}
    for name, scene, bounces, label in FRAMES:
        res["frames"][name] = frame(scene, bounces, label)
    res["aov_stores_C2"] = aov_stores("C1", 8)
    res["quality"] = [quality(*q) for q in QUALITY]
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for name, fr in res["frames"].items():
        brief[name] = {k: round(v["kernel_ms"]["median"], 4) for k, v in fr.items() if isinstance(v, dict) and "kernel_ms" in v}
        for d, v in fr["guides"].items():
            brief[name][f"guides_{d}"] = round(v["kernel_ms"]["median"], 4)
    brief["aov_stores_C2"] = {k: (round(v["launch_ms"]["median"], 4) if isinstance(v, dict) else v)
                              for k, v in res["aov_stores_C2"].items()}
    brief["quality"] = [(q["scene"], q["spp"], {k: round(v["spec"], 4) for k, v in q["rel_mse"].items()}) for q in res["quality"]]
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
