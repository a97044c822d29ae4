"""Writes tests/golden/post_ref_pins.npz: one 24x16 input of the post-processing references and what they give for it
(tests/test_post_ref_pins.py). Run it on the commit whose references are to be pinned:
    python tests/golden/make_post_ref_pins.py
The G-buffers are C1's from two views of an orbit with the sphere of row 2 moved in between (the case of
tests/test_temporal_motion_host.py); the histories and accumulators are random, with the texels that the gathers and the
filters must step over: counts of zero, a NaN colour, a miss, and pixels whose footprint crosses the frame's edge."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import temporal_motion_ref as tm  # noqa: E402
import temporal_ref as tr  # noqa: E402
import test_post_ref_pins as pins  # noqa: E402

F = np.float32
W, H = 24, 16


def inputs():
    with open(os.path.join(HERE, "fixtures.json")) as f:
        sc = json.load(f)["scenes"]["C1"]
    moves = {2: (0.6, 0.1, -0.3)}
    va, vb = tr.orbit(0), tr.orbit(3)
    rng = np.random.default_rng(20)
    i = {"Gprev": tr.ref_gbuffer(sc, va[0], va[1], W, H)[0], "Gcur": tr.ref_gbuffer(tm.moved(sc, moves), vb[0], vb[1], W, H)[0]}
    i["Gcur"][5, 7] = (0, 0, 0, -1)                        # a miss
    i["Hist"] = rng.random((H, W, 4), dtype=F) + F(1)
    i["Hist"][..., 3] = rng.integers(1, 20, (H, W)).astype(F)
    i["Hist"][2:5, 3:6, 3] = 0                             # no count
    i["Hist"][9, 12, 1] = np.nan
    i["Mhist"] = rng.random((H, W, 4), dtype=F)
    i["Mhist"][..., 2] = rng.integers(1, 20, (H, W)).astype(F)
    i["Mhist"][..., 3] = 0
    i["Mhist"][6:8, 14:17, 2] = 0
    i["Mhist"][11, 4, 0] = np.inf
    i["mvp_prev"], i["eye_prev"] = np.asarray(va[0], np.float64), np.asarray(va[1], F)
    i["D"], i["mc"] = tm.motion_table(sc["n"], moves), F(6)
    cnt = rng.integers(2, 9, (H, W)).astype(F)
    S = np.zeros((H, W, 4), F)
    S[..., :3] = rng.random((H, W, 3), dtype=F) * F(2) * cnt[..., None]
    S[..., 3] = cnt
    half = np.floor(cnt / F(2)).astype(F)
    P = np.zeros((H, W, 4), F)
    P[..., :3] = S[..., :3] * (half / cnt)[..., None] * (F(0.8) + F(0.4) * rng.random((H, W, 3), dtype=F))
    P[..., 3] = half
    S[3, 3, 3] = 0                                         # n = 0
    P[4, 9, 3] = 0                                         # h = 0
    S[10, 20, 0] = np.nan
    S[15, 23, 2] = np.inf
    i["S"], i["P"] = S, P
    n = rng.standard_normal((H, W, 3)).astype(F)
    n = (n / np.sqrt((n * n).sum(axis=-1, keepdims=True))).astype(F)
    i["N"] = np.concatenate([F(0.5) * n + F(0.5), np.zeros((H, W, 1), F)], axis=-1).astype(F)
    i["N"][:, :12, :3] = F(0.5) * np.array([0, 0, 1], F) + F(0.5)   # a flat half, so that the normal stop lets taps through
    v0 = (rng.random((H, W), dtype=F) * F(0.05)).astype(F)
    v0[0, 0], v0[7, 7], v0[15, 23] = np.nan, np.inf, np.nan
    i["v0"] = v0
    assert set(i) == set(pins.INPUTS)
    return i


if __name__ == "__main__":
    i = inputs()
    out = pins.outputs(i)
    np.savez_compressed(pins.PINS, **i, **out)
    print(pins.PINS, os.path.getsize(pins.PINS), "bytes;", ", ".join(sorted(out)))
