#!/usr/bin/env python3
"""What adaptive sampling (sail_render_adaptive) saves on the README Cornell box at 1920x1080, 8 bounces, on one MI355X.

  1. `until`: sail_render_until with target 0 to 1,024 spp; its look at 1,024 gives the target T (the mean it reports
     there, so sail_render_until at T stops at exactly that look: this run is that run).
  2. `adaptive`: sail_render_adaptive at T, max_spp 4,096 (its criterion is stricter: every 64x64 tile <= T).
  3. `uniform_to_same_max_tile`: uniform looks (mark, estimate + remark) on sail_plan_until's schedule up to 4,096 spp
     until every 64x64 tile's error (sail_plan_adaptive's e64) is <= T: the uniform render of the adaptive criterion.
  Each with the traced pixel-samples, the trace kernel_ms (sail_stats) and the relMSE of the mean image against a
  65,536-spp render of the same view and bounce count (other sample indices: 100,000 on).
  4. `rate_by_active_tiles`: 1,024 spp under masks of 1 .. all tiles (spread over the frame): nominal segments / kernel
     time, which shows how well the sample groups keep the GPU full when a handful of tiles is left; and
     `rate_by_active_tiles_unsplit`, the same launches held to one workgroup per block (SAIL_DEBUG_SAMPLE_GROUPS 1), as
     the 16-sample Cornell form runs a full frame.
Run from the repository root; writes profiles/adaptive_1080p.json (or the path given)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench
from sail_amd import capi

W, H, B = 1920, 1080, 8
MIN_SPP, LOOK, CAP, REF_SPP, REF_K0 = 16, 1024, 4096, 65536, 100000


def rel_mse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


def mean_image(ctx):
    a = ctx.read_accum()
    return a[..., :3] / a[..., 3:4]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "adaptive_1080p.json")
    sc = bench.load_scene("C1")
    mvp = capi.camera(sc["eye"], sc["center"], [0, 1, 0], 55.0, W / H, 1.0, 100.0).reshape(16)
    eye = sc["eye"]
    res = {"what": __doc__, "width": W, "height": H, "bounces": B, "tiles": [(W + 63) // 64, (H + 63) // 64]}

    def context():
        ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
        ctx.set_scene_dict(sc)
        ctx.kernel_ready(-1)
        return ctx

    ctx = context()
    try:
        chunk = 4096
        for k in range(0, REF_SPP, chunk):
            ctx.render_schedule(*capi.schedule(mvp, W, H, REF_K0 + k, chunk), eye, B)
        ref = mean_image(ctx)
        res["reference"] = {"spp": REF_SPP, "first_sample": REF_K0, "kernel_ms": ctx.stats().kernel_ms}
        # 1. sail_render_until
        ctx.reset()
        u = ctx.render_until(mvp, eye, B, 0.0, MIN_SPP, LOOK)
        target = float(u["history"][-1]["mean"])
        st = ctx.stats()
        res["target"] = target
        res["until"] = {"k": u["k"], "history": u["history"], "mean": u["mean"], "max_tile16": u["max_tile"],
                        "pixel_samples": W * H * u["k"], "kernel_ms": st.kernel_ms, "rel_mse": rel_mse(mean_image(ctx), ref),
                        "max_e64": float(capi.plan_adaptive(W, H, ctx.noise_estimate(tiles=True)["tile_err"], target, 1)[1].max())}
        # 2. sail_render_adaptive at the same target
        ctx.reset()
        a = ctx.render_adaptive(mvp, eye, B, target=target, min_spp=MIN_SPP, max_spp=CAP, dilate=1)
        st = ctx.stats()
        ts = a["tile_samples"]
        res["adaptive"] = {"k": a["k"], "converged": a["converged"], "active_tiles": a["active_tiles"], "history": a["history"],
                           "pixel_samples": a["pixel_samples"], "frame_pixel_samples": a["frame_pixel_samples"],
                           "kernel_ms": a["trace_ms"], "nominal_segments": st.nominal_segments,
                           "rel_mse": rel_mse(mean_image(ctx), ref),
                           "tiles_by_samples": {str(int(v)): int((ts == v).sum()) for v in np.unique(ts)},
                           "max_e64": float(capi.plan_adaptive(W, H, ctx.noise_estimate(tiles=True)["tile_err"], target, 1)[1].max())}
        # 3. the uniform render that meets the adaptive criterion
        ctx.reset()
        k, looks = 0, []
        while True:
            nxt = capi.plan_until(k, MIN_SPP, CAP)
            if nxt == k:
                break
            ctx.render_schedule(*capi.schedule(mvp, W, H, k, nxt - k), eye, B)
            k = nxt
            if not looks:
                ctx.noise_mark()
                looks.append({"k": k})
                continue
            est = ctx.noise_estimate(tiles=True)
            mx = float(capi.plan_adaptive(W, H, est["tile_err"], target, 1)[1].max())
            looks.append({"k": k, "mean": est["mean"], "max_e64": mx})
            if mx <= target:
                break
            ctx.noise_mark()
        res["uniform_to_same_max_tile"] = {"k": k, "looks": looks, "pixel_samples": W * H * k, "kernel_ms": ctx.stats().kernel_ms,
                                           "rel_mse": rel_mse(mean_image(ctx), ref)}
        # 4. the rate under small masks
        tiles = res["tiles"][0] * res["tiles"][1]
        rates, unsplit = [], []
        for groups, rows in ((0, rates), (1, unsplit)):
            ctx.set_debug(capi.DEBUG_SAMPLE_GROUPS, groups)
            for n in (1, 2, 4, 8, 16, 64, 256, tiles):
                mask = np.zeros(tiles, np.uint8)
                mask[np.linspace(0, tiles - 1, n).round().astype(int)] = 1
                ctx.reset()
                ctx.set_active_tiles(mask)
                ctx.render_schedule(*capi.schedule(mvp, W, H, 0, LOOK), eye, B)   # warm-up of this shape
                ctx.reset()
                ctx.set_active_tiles(mask)
                ctx.render_schedule(*capi.schedule(mvp, W, H, 0, LOOK), eye, B)
                st = ctx.stats()
                rows.append({"active_tiles": int(mask.sum()), "spp": LOOK, "kernel_ms": st.kernel_ms, "launches": st.launches,
                              "kernel": ctx.kernel_name(), "gseg_per_s": st.nominal_segments / (st.kernel_ms * 1e-3) / 1e9})
        res["rate_by_active_tiles"] = rates
        res["rate_by_active_tiles_unsplit"] = unsplit
    finally:
        ctx.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"target": target, "until": {k: res["until"][k] for k in ("k", "pixel_samples", "kernel_ms", "rel_mse", "max_e64")},
                      "adaptive": {k: res["adaptive"][k] for k in ("k", "converged", "active_tiles", "pixel_samples", "kernel_ms", "rel_mse", "max_e64", "tiles_by_samples")},
                      "uniform": {k: res["uniform_to_same_max_tile"][k] for k in ("k", "pixel_samples", "kernel_ms", "rel_mse")},
                      "rates": [(r["active_tiles"], round(r["gseg_per_s"], 2)) for r in rates],
                      "unsplit": [(r["active_tiles"], round(r["gseg_per_s"], 2)) for r in unsplit]}))


if __name__ == "__main__":
    main()
