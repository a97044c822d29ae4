#!/usr/bin/env python3
"""The quality scenario of tests/test_gpu_temporal_filter.py on the CPU: tests/oracle.py renders and the numpy restatements
(tests/temporal_ref.py, tests/temporal_filter_ref.py), no device. The GPU equals these bit for bit, so the ratios printed
here are the ones the device gives; the test's bound and sail_temporal_filter's sigma_l default were fixed from this run
("sail_temporal_filter"). C1 at 96x64, 5 bounces: 64 spp at A resolved once with tracking on, a 5 degree
orbit, one sample at B, resolve, filter; reference = 512 spp of B over the sample indices 1..512. A second row: the same
after 16 further one-sample resolves at B (sample indices 600..615).

Usage: python tools/temporal_filter_quality.py [--json OUT]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import temporal_filter_ref as tf  # noqa: E402
import temporal_ref as tr  # noqa: E402
from sail_amd import capi  # noqa: E402

F = np.float32
W, H, B, ANGLE = 96, 64, 5, 5.0


def rel_mse(x, ref):
    """tests/test_gpu_denoise.py's definition"""
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


def render(sc, view, k0, spp, aov=False):
    inv, seeds = capi.schedule(view[0], W, H, k0, spp)
    return oracle.render(sc, capi.plugin_masks(sc["plugins"]), W, H, inv, seeds, view[1], B, k0=k0, aov=aov)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        sc = json.load(f)["scenes"]["C1"]
    va, vb = tr.orbit(0), tr.orbit(ANGLE)
    zero = np.zeros((H, W, 4), F)
    S = render(sc, vb, 1, 512)
    ref = (S[..., :3] / S[..., 3:4]).astype(F)
    GA, GB = tr.ref_gbuffer(sc, *va, W, H)[0], tr.ref_gbuffer(sc, *vb, W, H)[0]
    # A: 64 spp, one resolve (no history: Out = the mean, Mout = (l, l*l, 32))
    SA = render(sc, va, 0, 64)
    out_a = tr.ref_resolve(SA, zero)[0]
    mom_a = tf.ref_moment_resolve(SA, zero)
    # B: reproject, one sample, resolve
    r_b = tr.ref_reproject(GB, GA, out_a, *va)[0]
    mr_b = tf.ref_moment_reproject(GB, GA, mom_a, *va)
    SB, NB, XB = render(sc, vb, 0, 1, aov=True)
    noisy = (SB[..., :3] / SB[..., 3:4]).astype(F)
    out_b = tr.ref_resolve(SB, r_b)[0]
    mom_b = tf.ref_moment_resolve(SB, mr_b)
    hits = int((GB[..., 3] >= 0).sum())
    e_noisy, e_res = rel_mse(noisy, ref), rel_mse(out_b[..., :3], ref)
    rows = {"relmse_1spp": e_noisy, "relmse_resolved": e_res, "hit_pixels": hits, "sigma_l": {}}
    print(f"C1 {W}x{H}, {B} bounces, orbit {ANGLE}: relMSE 1-spp mean {e_noisy:.6g}, resolved {e_res:.6g} "
          f"(ratio {e_res / e_noisy:.4f}), hit pixels {hits}")
    for sl in (1.0, 2.0, 4.0):
        c, _, counts = tf.ref_filter(out_b, mom_b, SB, NB, XB, sigma_l=sl)
        e = rel_mse(c, ref)
        rows["sigma_l"][str(sl)] = {"relmse_filtered": e, "ratio": e / e_res, "temporal_pixels": counts["temporal"]}
        print(f"  sigma_l {sl}: filtered {e:.6g}, filtered / resolved {e / e_res:.4f}, temporal pixels "
              f"{counts['temporal']} ({counts['temporal'] / hits:.4f} of the hit pixels), nonfinite {counts['nonfinite']}")
    # 16 further one-sample resolves at B: begin(B) commits and reprojects onto the same view, reset, one sample, resolve
    out, mom = out_b, mom_b
    for i in range(16):
        r = tr.ref_reproject(GB, GB, out, *vb)[0]
        mr = tf.ref_moment_reproject(GB, GB, mom, *vb)
        Si, NB, XB = render(sc, vb, 600 + i, 1, aov=True)
        out = tr.ref_resolve(Si, r)[0]
        mom = tf.ref_moment_resolve(Si, mr)
    e_res16 = rel_mse(out[..., :3], ref)
    rows["after_16"] = {"relmse_resolved": e_res16, "sigma_l": {}}
    for sl in (1.0, 2.0, 4.0):
        c, _, counts = tf.ref_filter(out, mom, Si, NB, XB, sigma_l=sl)
        e = rel_mse(c, ref)
        rows["after_16"]["sigma_l"][str(sl)] = {"relmse_filtered": e, "ratio": e / e_res16,
                                                "temporal_pixels": counts["temporal"]}
        print(f"  after 16 more resolves, sigma_l {sl}: resolved {e_res16:.6g}, filtered {e:.6g}, ratio {e / e_res16:.4f}, "
              f"temporal pixels {counts['temporal']}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
