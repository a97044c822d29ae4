"""CPU: the numpy references of the post-processing kernels (tests/temporal_ref.py, tests/temporal_filter_ref.py,
tests/temporal_motion_ref.py, tests/atrous_ref.py and tests/test_gpu_denoise.py's ref_denoise) give, for one stored 24x16
input, the bits they gave before they were made to share one gather and one a-trous text. The device kernels are checked
against these references bit for bit, so a reference that drifted would let the kernels drift with it.
tests/golden/post_ref_pins.npz holds the inputs and the outputs (tests/golden/make_post_ref_pins.py wrote it); NaN is
compared as NaN, whatever its payload."""
import os

import numpy as np

import temporal_filter_ref as tf
import temporal_motion_ref as tm
import temporal_ref as tr
import test_gpu_denoise as dn

F = np.float32
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_ref_pins.npz")
INPUTS = ("Gcur", "Gprev", "Hist", "Mhist", "mvp_prev", "eye_prev", "D", "mc", "S", "P", "N", "v0")
ITER = 3


def outputs(i):
    """every pinned reference over the inputs `i`, as a dict of arrays"""
    mvp, eye, mc, X = i["mvp_prev"], i["eye_prev"], float(i["mc"]), i["Gcur"]
    o = {}
    o["R"], found = tr.ref_reproject(i["Gcur"], i["Gprev"], i["Hist"], mvp, eye)
    o["MR"] = tf.ref_moment_reproject(i["Gcur"], i["Gprev"], i["Mhist"], mvp, eye)
    o["R_moved"], found_moved = tm.ref_reproject_moved(i["Gcur"], i["Gprev"], i["Hist"], mvp, eye, i["D"], mc)
    o["MR_moved"] = tm.ref_moment_reproject_moved(i["Gcur"], i["Gprev"], i["Mhist"], mvp, eye, i["D"], mc)
    o["Out"], hist, bad = tr.ref_resolve(i["S"], o["R_moved"], cap=8.0)
    o["Mout"] = tf.ref_moment_resolve(i["S"], o["MR_moved"], cap=8.0)
    o["prefilter"] = tf.prefilter(i["v0"])
    nd = F(2) * i["N"][..., :3] - F(1)
    x = np.ascontiguousarray(X[..., :3])
    o["atrous_c"], o["atrous_v"] = tf.atrous(np.ascontiguousarray(o["Out"][..., :3]), o["prefilter"], nd, x, ITER, 2.5, 0.3)
    o["filter_c"], o["filter_v"], fc = tf.ref_filter(o["Out"], o["Mout"], i["S"], i["N"], X, iterations=ITER, min_hist=2.0)
    o["denoise_c"], o["denoise_v"], dbad = dn.ref_denoise(i["S"], i["P"], i["N"], X, iterations=ITER)
    o["counts"] = np.array([found, found_moved, hist, bad, fc["temporal"], fc["spatial"], fc["nonfinite"], dbad], np.int64)
    return o


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != F:
        return bool(np.array_equal(a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_the_stored_input_has_the_special_texels():
    with np.load(PINS) as z:
        i = {k: z[k] for k in INPUTS}
    assert i["Gcur"].shape == (16, 24, 4) and os.path.getsize(PINS) < 200 * 1024
    assert (i["Hist"][..., 3] == 0).any() and (i["Mhist"][..., 2] == 0).any()        # history texels without a count
    assert np.isnan(i["Hist"][..., :3]).sum() == 1                                   # one NaN colour
    assert (i["Gcur"][..., 3] < 0).sum() == 1                                        # one miss
    assert i["D"].any() and np.isfinite(i["mc"])
    # a pixel whose footprint crosses the frame's edge and that still finds a history
    u, v, valid = tr.project(tm.previous_position(i["Gcur"], i["D"]), tr.mp32(i["mvp_prev"]), 24, 16)
    iu, iv = np.floor(u), np.floor(v)
    with np.load(PINS) as z:
        found = z["R_moved"][..., 3] > 0
    assert (valid & found & ((iu == -1) | (iu == 23) | (iv == -1) | (iv == 15))).any()


def test_the_references_give_the_stored_bits():
    with np.load(PINS) as z:
        stored = {k: z[k] for k in z.files}
    got = outputs({k: stored[k] for k in INPUTS})
    assert set(got) | set(INPUTS) == set(stored)
    wrong = [k for k in sorted(got) if not same(got[k], stored[k])]
    print("pinned:", ", ".join(f"{k}{tuple(got[k].shape)}" for k in sorted(got)))
    assert not wrong, wrong
