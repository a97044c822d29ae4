"""CPU: the host side of moment tracking and sail_temporal_filter: the defaults, every SAIL_E_INVALID case of the new
parameter sets (the library checks them before it looks at the context, so a NULL context reaches them without a device),
and tests/temporal_filter_ref.py against values worked out by hand on 1x1 and 3x3 maps."""
import ctypes

import numpy as np
import pytest

import temporal_filter_ref as tf
from sail_amd import capi

F = np.float32
INVALID = -1


def test_defaults():
    d = capi.temporal_filter_defaults()
    assert d == {"iterations": 4, "sigma_l": 4.0, "sigma_x": pytest.approx(0.2), "min_hist": 4.0,
                 "display": capi.FILTER_COLOR, "gamma_c": pytest.approx(2.2)}
    assert F(d["sigma_x"]) == F(0.2) and F(d["gamma_c"]) == F(2.2)
    assert capi.load().sail_temporal_filter_defaults(None) == INVALID


def filter_null(**over):
    """sail_temporal_filter on a NULL context with the defaults and `over`: (return code, message)"""
    lib = capi.load()
    d = dict(capi.temporal_filter_defaults(), **over)
    p = capi.TfilterParams(int(d["iterations"]), float(d["sigma_l"]), float(d["sigma_x"]), float(d["min_hist"]),
                           int(d["display"]), float(d["gamma_c"]))
    rc = lib.sail_temporal_filter(None, ctypes.byref(p), None, None, None, None)
    return rc, lib.sail_last_error(None).decode()


BAD_FILTER = [{"iterations": 0}, {"iterations": 7}, {"iterations": -1},
              {"sigma_l": 0.0}, {"sigma_l": -1.0}, {"sigma_l": float("nan")}, {"sigma_l": float("inf")},
              {"sigma_x": 0.0}, {"sigma_x": -0.2}, {"sigma_x": float("nan")}, {"sigma_x": float("inf")},
              {"min_hist": 0.5}, {"min_hist": 0.0}, {"min_hist": -4.0}, {"min_hist": float("nan")},
              {"min_hist": float("inf")}, {"display": -1}, {"display": capi.FILTER_WINDOW}]


@pytest.mark.parametrize("bad", BAD_FILTER, ids=[f"{k}={v}" for b in BAD_FILTER for k, v in b.items()])
def test_filter_parameters_are_checked_before_the_context(bad):
    rc, msg = filter_null(**bad)
    assert rc == INVALID and "bad parameters" in msg, (rc, msg)


def test_good_parameters_reach_the_context_check():
    for good in ({}, {"iterations": 1}, {"iterations": 6}, {"min_hist": 1.0}, {"display": capi.FILTER_TONEMAPPING}):
        rc, msg = filter_null(**good)
        assert rc == INVALID and "a context is required" in msg, (good, rc, msg)
    lib = capi.load()
    assert lib.sail_temporal_filter(None, None, None, None, None, None) == INVALID      # NULL parameters: the defaults
    assert "a context is required" in lib.sail_last_error(None).decode()


def test_moment_calls_check_their_arguments_before_the_context():
    lib = capi.load()
    out = np.zeros(4, F)
    for on in (2, -1, 100):
        assert lib.sail_temporal_moments(None, on) == INVALID
        assert "on must be 0 or 1" in lib.sail_last_error(None).decode()
    for on in (0, 1):
        assert lib.sail_temporal_moments(None, on) == INVALID
        assert "a context is required" in lib.sail_last_error(None).decode()
    for which in (-1, 3, 5):
        assert lib.sail_temporal_read_moments(None, which, capi._ptr(out)) == INVALID
        assert "of 0..2" in lib.sail_last_error(None).decode()
    assert lib.sail_temporal_read_moments(None, 0, None) == INVALID
    assert "of 0..2" in lib.sail_last_error(None).decode()
    assert lib.sail_temporal_read_moments(None, 2, capi._ptr(out)) == INVALID
    assert "a context is required" in lib.sail_last_error(None).decode()
    assert lib.sail_temporal_load_moments(None, capi._ptr(out)) == INVALID


def test_python_binding_refuses_unknown_parameters_and_shapes():
    class Fake(capi.Context):
        def __init__(self):
            self.W, self.H, self.h, self.lib = 3, 2, None, capi.load()
    ctx = Fake()
    with pytest.raises(capi.SailError, match="unknown parameters"):
        ctx.temporal_filter({"sigma": 1.0})
    with pytest.raises(capi.SailError, match="shape"):
        ctx.temporal_load_moments(np.zeros((3, 2, 4), F))


# ---- the reference against values worked out by hand ----------------------------------------------------------------------------
def one(v):
    return np.array(v, F).reshape(1, 1, -1)


def test_moment_resolve_by_hand():
    # SUM, n = 2, sums (3, 6, 9): c0 = (1.5, 3, 4.5), l = 3; history mh = 6 with mu1 = 1, mu2 = 2:
    # ws = 8, mu1 = (6*1 + 2*3) / 8 = 1.5, mu2 = (6*2 + 2*9) / 8 = 3.75, mm = min(8, cap)
    S, MR = one([3, 6, 9, 2]), one([1, 2, 6, 0])
    assert tf.ref_moment_resolve(S, MR, cap=32.0).reshape(4).tolist() == [1.5, 3.75, 8.0, 0.0]
    assert tf.ref_moment_resolve(S, MR, cap=5.0).reshape(4).tolist() == [1.5, 3.75, 5.0, 0.0]
    # no history: (l, l*l, min(n, cap));  no sample: the history as it is;  neither: zero
    assert tf.ref_moment_resolve(S, one([7, 7, 0, 0])).reshape(4).tolist() == [3.0, 9.0, 2.0, 0.0]
    assert tf.ref_moment_resolve(one([0, 0, 0, 0]), MR).reshape(4).tolist() == [1.0, 2.0, 6.0, 0.0]
    assert tf.ref_moment_resolve(one([0, 0, 0, 0]), one([1, 2, 0, 0])).reshape(4).tolist() == [0.0, 0.0, 0.0, 0.0]
    # a colour that is not finite is no current sample
    assert tf.ref_moment_resolve(one([np.nan, 6, 9, 2]), MR).reshape(4).tolist() == [1.0, 2.0, 6.0, 0.0]
    # MIX: n = k, c0 = S.rgb
    assert tf.ref_moment_resolve(one([3, 3, 3, 1]), MR, mix=True, k=2).reshape(4).tolist() == [1.5, 3.75, 8.0, 0.0]


def test_variance_1x1_by_hand():
    Out, N, X = one([1, 2, 3, 9]), one([0.5, 0.5, 1.0, 0]), one([0, 0, 0, 0])
    n = np.array([[1]], F)
    # vt = (max(mu2 - mu1*mu1, 0) * nn) / mm = ((5 - 4) * 1) / 4;  the only spatial tap is the centre: vs = 0
    for mm, temporal in ((3, False), (4, True), (5, True)):
        v0, vt, vs, t = tf.ref_variance(Out, one([2, 5, mm, 0]), n, N, X, min_hist=4.0)
        assert vt[0, 0] == F(1) / F(mm) and vs[0, 0] == 0 and bool(t[0, 0]) is temporal
        assert v0[0, 0] == (F(1) / F(mm) if temporal else 0)
    # n samples per frame: the variance of the mean scales with nn; n = 0 counts as 1
    assert tf.ref_variance(Out, one([2, 5, 4, 0]), np.array([[3]], F), N, X)[1][0, 0] == F(0.75)
    assert tf.ref_variance(Out, one([2, 5, 4, 0]), np.array([[0]], F), N, X)[1][0, 0] == F(0.25)
    # mu2 < mu1*mu1 clamps to 0, and so does a NaN difference (max(a, b) = a > b ? a : b)
    v0, vt, _, t = tf.ref_variance(Out, one([2, 3, 8, 0]), n, N, X)
    assert vt[0, 0] == 0 and tf.bits(vt)[0, 0] == 0 and t[0, 0] and v0[0, 0] == 0
    v0, vt, _, t = tf.ref_variance(Out, one([np.nan, 3, 8, 0]), n, N, X)
    assert vt[0, 0] == 0 and t[0, 0]
    # mm = 0: 0 / 0 is not finite, and below min_hist anyway
    assert not tf.ref_variance(Out, one([2, 5, 0, 0]), n, N, X, min_hist=1.0)[3][0, 0]
    # an Inf second moment: vt is not finite, the spatial estimate stands in
    v0, vt, vs, t = tf.ref_variance(Out, one([2, np.inf, 8, 0]), n, N, X)
    assert np.isinf(vt[0, 0]) and not t[0, 0] and v0[0, 0] == 0


def test_variance_3x3_by_hand():
    # one flat wall: equal normals (d = 1) and equal positions (wx = 1), so every tap weighs 1 and vs is the plain variance
    # of the luminances inside the frame; the 7x7 window covers this frame from every pixel, corners included
    lums = np.array([[0, 3, 0], [3, 6, 3], [0, 3, 0]], F)
    Out = np.zeros((3, 3, 4), F)
    Out[..., :3] = lums[..., None]
    N = np.zeros((3, 3, 4), F)
    N[..., :3] = (0.5, 0.5, 1.0)
    X = np.zeros((3, 3, 4), F)
    Mout = np.zeros((3, 3, 4), F)
    Mout[..., :3] = (1, 3, 3)                      # vt = (3 - 1) / 3, young everywhere at min_hist 4
    Mout[1, 1, 2], Mout[0, 1, 2] = 4, 5            # ... but for the centre (mm 4) and one edge (mm 5)
    n = np.ones((3, 3), F)
    v0, vt, vs, t = tf.ref_variance(Out, Mout, n, N, X, min_hist=4.0)
    assert t.sum() == 2 and t[1, 1] and t[0, 1]
    assert v0[1, 1] == F(2) / F(4) and v0[0, 1] == F(2) / F(5)
    assert (vs == F(72) / F(9) - F(2) * F(2)).all() and vs[1, 1] == 4   # a1 = 18, a2 = 72 over 9 taps
    assert v0[0, 0] == 4 and v0[2, 1] == 4                              # the young pixels take it
    # a tap across a normal edge weighs nothing: turn the right column's normal away
    N2 = N.copy()
    N2[:, 2, :3] = (1.0, 0.5, 0.5)
    vs2 = tf.ref_variance(Out, Mout, n, N2, X)[2]
    assert vs2[1, 1] == F(63) / F(6) - F(2.5) * F(2.5) == 4.25          # the left two columns: 0, 3, 0, 3, 6, 3
    assert vs2[1, 2] == F(9) / F(3) - F(1) * F(1) == 2                  # the right column among itself: 0, 3, 0
    # a tap whose colour is not finite is skipped; a pixel that misses (NaN position) keeps only its centre tap
    Out3 = Out.copy()
    Out3[1, 1, 0] = np.inf
    assert tf.ref_variance(Out3, Mout, n, N, X)[2][0, 0] == F(36) / F(8) - F(1.5) * F(1.5) == 2.25
    X3 = X.copy()
    X3[0, 0, :3] = np.nan
    assert tf.ref_variance(Out, Mout, n, N, X3)[2][0, 0] == 0
    # the prefilter of a single spike spreads 1/4, 1/8, 1/16 renormalised at the border
    spike = np.zeros((3, 3), F)
    spike[1, 1] = 16
    pf = tf.prefilter(spike)
    assert pf[1, 1] == 4 and pf[0, 1] == F(2) / F(0.75) and pf[0, 0] == F(1) / F(0.5625)
    spike[0, 0] = np.nan                                                  # skipped, and the weights renormalised
    assert tf.prefilter(spike)[1, 1] == F(4) / F(0.9375)


def test_counts_and_nonfinite():
    Out = np.ones((3, 3, 4), F)
    Out[2, 2, 1] = np.nan
    N, X = np.full((3, 3, 4), 0.5, F), np.zeros((3, 3, 4), F)
    Mout = np.zeros((3, 3, 4), F)
    Mout[..., 2] = [[0, 0.5, 3], [4, 40, 4], [3.5, 1, 5]]
    S = np.ones((3, 3, 4), F)
    for min_hist, want in ((1.0, 7), (4.0, 4), (41.0, 0)):
        c, v, counts = tf.ref_filter(Out, Mout, S, N, X, min_hist=min_hist, iterations=1)
        assert counts == {"temporal": want, "spatial": 9 - want, "nonfinite": 1}
        assert np.isnan(c[2, 2, 1]) and c[2, 2, 0] == 1                   # stays as it is
        assert np.isfinite(np.delete(c.reshape(-1), 8 * 3 + 1)).all()      # and feeds nobody
