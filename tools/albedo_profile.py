#!/usr/bin/env python3
"""Device time of the albedo map (sail_albedo) and of the albedo-demodulated filters at 1920x1080 on one MI355X.

Two frames: C3 (the materials demo: checkered room, checkered sphere, 5 bounces) and C2 (the README Cornell box, 8
bounces), each 16 spp with the noise mark at 8, begun and resolved as one temporal view with moment tracking on. After 5
warm-up calls, 20 calls each, HIP events, median and min-max:
  * sail_albedo at grid 1, 2 and 4, with the algorithmic bytes (one float4 store per pixel; the rows come through the
    scalar cache) and the time per sub-pixel ray;
  * sail_denoise next to sail_denoise_albedo and sail_temporal_filter next to sail_temporal_filter_albedo, in the same
    session: kernel_ms and every pass. The demodulated calls read the map twice more per pixel in prepare (and once per
    halo texel) and once in the last pass.
With --plain only the two plain calls are timed (the control of an A/B run against another build of the library: set
SAIL_HIP_LIB, or run a copy of this script in the other tree). Run from the repository root; writes
profiles/albedo_1080p.json (or the path given)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import bench
from sail_amd import capi

W, H, SPP, MARK = 1920, 1080, 16, 8
WARMUP, CALLS = 5, 20
HBM = 8.0e12
FRAMES = (("C3", "C3", 5, "C3 (materials demo, 5 bounces)"), ("C2", "C1", 8, "C2 (README Cornell box, 8 bounces)"))


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


def frame(name, scene, bounces, label, plain_only):
    sc = bench.load_scene(scene)
    mvp = capi.camera(sc["eye"], sc["center"], [0, 1, 0], 55.0, W / H, 1.0, 100.0).reshape(16)
    eye = sc["eye"]
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.temporal_moments(True)
        ctx.temporal_begin(mvp, eye)
        ctx.render_schedule(*capi.schedule(mvp, W, H, 0, MARK), eye, bounces)
        ctx.noise_mark()
        ctx.render_schedule(*capi.schedule(mvp, W, H, MARK, SPP - MARK), eye, bounces)
        ctx.temporal_resolve()
        out = {"scene": label, "rows": sc["n"], "spp": SPP, "mark": MARK}
        if not plain_only:
            out["albedo"] = {}
            for g in (1, 2, 4):
                runs = timed(lambda: ctx.albedo(mvp, eye, grid=g))
                ms = spread([r["kernel_ms"] for r in runs])
                b = W * H * 16 + sc["n"] * 128
                out["albedo"][f"grid{g}"] = {
                    "samples": CALLS, "kernel_ms": ms, "hit_pixels": runs[-1]["hit_pixels"],
                    "partial_pixels": runs[-1]["partial_pixels"], "algorithmic_bytes": b,
                    "bytes_per_s": b / (ms["median"] * 1e-3), "hbm_peak_fraction": b / (ms["median"] * 1e-3) / HBM,
                    "ns_per_ray": ms["median"] * 1e6 / (W * H * g * g)}
            ctx.albedo(mvp, eye, grid=2)
        # plain and demodulated in one session; the plain denoiser once more at the end, for the spread between runs
        out["denoise"] = filter_times(lambda: ctx.denoise())
        if not plain_only:
            out["denoise_albedo"] = filter_times(lambda: ctx.denoise(albedo=capi.ALBEDO_AMIN_DEFAULT))
        out["temporal_filter"] = filter_times(lambda: ctx.temporal_filter())
        if not plain_only:
            out["temporal_filter_albedo"] = filter_times(lambda: ctx.temporal_filter(albedo=capi.ALBEDO_AMIN_DEFAULT))
            out["denoise_again"] = filter_times(lambda: ctx.denoise())
            for a, b in (("denoise", "denoise_albedo"), ("temporal_filter", "temporal_filter_albedo")):
                out[f"{b}_minus_{a}_ms"] = out[b]["kernel_ms"]["median"] - out[a]["kernel_ms"]["median"]
    finally:
        ctx.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--plain"]
    plain_only = "--plain" in sys.argv[1:]
    path = args[0] if args else os.path.join("profiles", "albedo_1080p.json")
    res = {"what": __doc__, "width": W, "height": H, "hbm_peak_bytes_per_s": HBM, "plain_only": plain_only, "frames": {}}
    for name, scene, bounces, label in FRAMES:
        res["frames"][name] = frame(name, scene, bounces, label, plain_only)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for name, fr in res["frames"].items():
        brief[name] = {k: round(v["kernel_ms"]["median"], 4) for k, v in fr.items() if isinstance(v, dict) and "kernel_ms" in v}
        for g, v in fr.get("albedo", {}).items():
            brief[name][f"albedo_{g}"] = round(v["kernel_ms"]["median"], 4)
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
