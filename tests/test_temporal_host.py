"""CPU: the host-only side of the camera-motion reprojection (include/sail_hip.h, sail_temporal_*): the symbols are bound,
the defaults are the documented ones, every entry point fails loudly without a device, and the numpy reference of the
formula (tests/temporal_ref.py) is oriented the right way: a history at view A maps back onto itself at view A."""
import ctypes

import numpy as np
import pytest

import temporal_ref as tr
from sail_amd import capi

F = np.float32
ENTRY_POINTS = ("sail_temporal_defaults", "sail_gbuffer", "sail_temporal_begin", "sail_temporal_resolve",
                "sail_temporal_read", "sail_temporal_load_history")


def test_symbols_are_bound():
    lib = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None
    for method in ("gbuffer", "temporal_begin", "temporal_resolve", "temporal_read", "temporal_load_history"):
        assert callable(getattr(capi.Context, method))
    assert ctypes.sizeof(capi.TemporalParams) == 16
    assert ctypes.sizeof(capi.TemporalInfo) == 4 * 8 + 4 * 8
    assert (capi.TEMPORAL_G_CUR, capi.TEMPORAL_G_PREV, capi.TEMPORAL_HIST, capi.TEMPORAL_R, capi.TEMPORAL_OUT) == (0, 1, 2, 3, 4)


def test_defaults_are_the_documented_ones():
    d = capi.temporal_defaults()
    f32 = lambda v: ctypes.c_float(v).value
    assert (d["cap"], d["pos_tol"], d["display"], d["gamma_c"]) == (32.0, f32(0.05), capi.FILTER_COLOR, f32(2.2))
    assert capi.load().sail_temporal_defaults(None) == -1


def test_null_context_is_rejected():
    lib = capi.load()
    mvp, eye = tr.orbit(0)
    m, e = capi._ptr(np.ascontiguousarray(mvp), ctypes.c_double), capi._ptr(eye)
    buf = np.zeros(4, F)
    assert lib.sail_gbuffer(None, m, e, None, None, None, None) == -1
    assert lib.sail_temporal_begin(None, m, e, None, None) == -1
    assert lib.sail_temporal_resolve(None, None, None, None, None) == -1
    assert lib.sail_temporal_read(None, 0, capi._ptr(buf)) == -1
    assert lib.sail_temporal_load_history(None, capi._ptr(buf), capi._ptr(buf), m, e) == -1


def test_entry_points_fail_loudly_without_a_device():
    """no context can exist without a device, so none of the calls can quietly do nothing"""
    if capi.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(capi.SailError, match="no HIP device"):
        capi.Context(16, 16)
    with pytest.raises(capi.SailError, match="no HIP device"):
        capi.Context(16, 16, devices=[0, 0])


def test_unknown_parameters_are_rejected_on_the_host():
    with pytest.raises(capi.SailError, match="unknown parameters"):
        capi._temporal_params({"capp": 1.0}, "temporal_begin")
    assert capi._temporal_params(None, "temporal_begin") is None
    p = capi._temporal_params({"cap": 8, "display": capi.FILTER_GAMMA}, "temporal_resolve")
    assert (p.cap, p.display, p.pos_tol, p.gamma_c) == (8.0, 1, ctypes.c_float(0.05).value, ctypes.c_float(2.2).value)


def test_reference_maps_a_view_onto_itself(fixtures):
    """orientation of the formula, not the device: the first hits of view A, projected by A's own matrix, land within
    0.01 px of their pixel centres on C1, and reprojecting a history from A to A returns it"""
    sc = fixtures["scenes"]["C1"]
    W, H = 48, 32
    mvp, eye = np.array(sc["mvp_rowmajor"]).reshape(16), np.asarray(sc["eye"], F)
    G, rays, idx, t = tr.ref_gbuffer(sc, mvp, eye, W, H)
    assert (idx >= 0).all() and len(np.unique(idx)) == 3
    u, v, valid = tr.project(G, tr.mp32(mvp), W, H)
    assert valid.all()
    du = np.abs(u - np.arange(W, dtype=F)[None, :]).max()
    dv = np.abs(v - np.arange(H, dtype=F)[:, None]).max()
    print(f"C1 {W}x{H}: max |u - x| {du:.3g}, max |v - y| {dv:.3g}")
    assert du < 0.01 and dv < 0.01
    rng = np.random.default_rng(5)
    hist = rng.random((H, W, 4), dtype=F) + F(1)
    R, found = tr.ref_reproject(G, G, hist, mvp, eye)
    assert found == W * H
    # a bilinear gather a hundredth of a pixel off centre: the history's colours to a few parts in a hundred
    assert np.abs(R[..., :3] - hist[..., :3]).max() < 0.05
    # an orbit about the room's middle leaves the middle where it is and moves the far wall's pixels by whole pixels
    mb, eb = tr.orbit(5)
    ub, _, vb = tr.project(G, tr.mp32(mb), W, H)
    assert vb.all() and np.abs(ub - u).max() > 1.0


def test_reference_resolve_weights():
    """the history counts as at most cap samples and the output goes to the plain mean"""
    S = np.zeros((1, 4, 4), F)
    S[0, :, :3] = [[2, 2, 2], [10, 10, 10], [2000, 2000, 2000], [0, 0, 0]]
    S[0, :, 3] = [1, 5, 1000, 0]
    R = np.zeros((1, 4, 4), F)
    R[0, :, :3] = 1.0
    R[0, :, 3] = 32
    out, hist, bad = tr.ref_resolve(S, R, cap=32)
    assert (hist, bad) == (4, 0)
    want = [(32 * 1 + 1 * 2) / 33, (32 * 1 + 5 * 2) / 37, (32 * 1 + 1000 * 2) / 1032, 1.0]
    assert np.allclose(out[0, :, 0], want, rtol=1e-6)
    assert out[0, :, 3].tolist() == [32, 32, 32, 32]
    out, hist, bad = tr.ref_resolve(S, np.zeros_like(R), cap=8)
    assert hist == 0 and out[0, :, 0].tolist() == [2, 2, 2, 0] and out[0, :, 3].tolist() == [1, 5, 8, 0]
