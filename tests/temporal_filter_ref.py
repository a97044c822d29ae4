"""The moment and temporal-filter formulas of include/sail_hip.h (sail_temporal_moments, sail_temporal_filter) in numpy
float32, one operation at a time, the tap loops in the stated order and vectorised over pixels: the reference of
tests/test_gpu_temporal_filter.py and tests/test_temporal_filter_host.py. Written from the header, not from the kernels.
Every operation of the formulas is an IEEE f32 one, so the device's maps must equal these bit for bit. The colour passes
and the gather are tests/temporal_ref.py's; the prefilter and the a-trous passes are sail_denoise's, tests/atrous_ref.py."""
import numpy as np

import temporal_ref as tr
from atrous_ref import atrous, lum, prefilter, shifted
from temporal_ref import bits, fmax, fmin  # noqa: F401  (bits is re-exported for the tests)

F = np.float32


# ---- moment reproject ---------------------------------------------------------------------------------------------------------
def ref_moment_reproject(Gcur, Gprev, Mhist, mvp_prev, eye_prev, pos_tol=0.05, D=None, mc=np.inf):
    """MR (H, W, 4): tests/temporal_ref.py's ref_reproject with Mhist in the place of Hist and .z as the count"""
    Mhist = np.asarray(Mhist, F)
    H, W = Mhist.shape[:2]
    a1, a2, wsum, m = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.full((H, W), np.inf, F)
    with np.errstate(all="ignore"):
        for w, ok, yi, xi in tr.gather(Gcur, Gprev, mvp_prev, eye_prev, pos_tol, D):
            h = Mhist[yi, xi]
            ok = ok & (h[..., 2] > F(0)) & np.isfinite(h[..., 0]) & np.isfinite(h[..., 1])
            a1 = np.where(ok, a1 + w * h[..., 0], a1)
            a2 = np.where(ok, a2 + w * h[..., 1], a2)
            wsum = np.where(ok, wsum + w, wsum)
            m = np.where(ok & (h[..., 2] < m), h[..., 2], m)
        found = wsum > F(0)
        MR = np.zeros((H, W, 4), F)
        MR[..., 0] = np.where(found, a1 / wsum, F(0))
        MR[..., 1] = np.where(found, a2 / wsum, F(0))
        MR[..., 2] = np.where(found, fmin(m, F(mc)), F(0))
    assert a1.dtype == F and wsum.dtype == F
    return MR


# ---- moment resolve -----------------------------------------------------------------------------------------------------------
def shown(S, mix, k):
    """(n, c0) of the shown accumulator as sail_temporal_resolve takes them"""
    S = np.asarray(S, F)
    n = np.full(S.shape[:2], F(k)) if mix else S[..., 3]
    with np.errstate(all="ignore"):
        c0 = S[..., :3].copy() if mix else np.where((n > F(0))[..., None], S[..., :3] / n[..., None], F(0)).astype(F)
    return n, c0


def ref_moment_resolve(S, MR, mix=False, k=0, cap=32.0):
    """Mout (H, W, 4)"""
    MR, cap = np.asarray(MR, F), F(cap)
    n, c0 = shown(S, mix, k)
    with np.errstate(all="ignore"):
        l = lum(c0)
        cur = (n > F(0)) & np.isfinite(c0).all(axis=-1)
        mh = MR[..., 2]
        hist = mh > F(0)
        ws = mh + n
        mu1 = ((mh * MR[..., 0]) + (n * l)) / ws
        mu2 = ((mh * MR[..., 1]) + (n * (l * l))) / ws
        both = np.stack([mu1, mu2, fmin(ws, cap), np.zeros_like(ws)], axis=-1)
        only = np.stack([l, l * l, fmin(n, cap), np.zeros_like(n)], axis=-1)
        Mout = np.where((hist & cur)[..., None], both,
                        np.where(hist[..., None], MR, np.where(cur[..., None], only, F(0)))).astype(F)
    assert mu1.dtype == F and Mout.dtype == F
    return Mout


# ---- the filter's prepare pass --------------------------------------------------------------------------------------------------
def ref_variance(Out, Mout, n, N, X, sigma_x=0.2, min_hist=4.0):
    """(v0 (H, W), vt, vs, mask of the pixels that took vt)"""
    Out, Mout, n = np.asarray(Out, F), np.asarray(Mout, F), np.asarray(n, F)
    c = Out[..., :3]
    nd = F(2) * np.asarray(N, F)[..., :3] - F(1)
    x = np.ascontiguousarray(np.asarray(X, F)[..., :3])
    shape = c.shape[:2]
    with np.errstate(all="ignore"):
        nn = np.where(n > F(0), n, F(1)).astype(F)
        vt = (fmax(Mout[..., 1] - Mout[..., 0] * Mout[..., 0], F(0)) * nn) / Mout[..., 2]
        sx0 = (F(sigma_x) * F(2)) * (F(sigma_x) * F(2))
        l = lum(c)
        fin = np.isfinite(c).all(axis=-1)
        a1, a2, ws = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                lq, inside = shifted(l, dy, dx, F(0))
                if not inside.any():
                    continue
                fq, _ = shifted(fin, dy, dx, False)
                if dy == 0 and dx == 0:
                    w = np.ones(shape, F)
                else:
                    nq, _ = shifted(nd, dy, dx, F(0))
                    xq, _ = shifted(x, dy, dx, F(0))
                    d = fmax((nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2], F(0))
                    for _ in range(6):
                        d = d * d
                    t = x - xq
                    dx2 = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
                    wx = F(1) / (F(1) + dx2 / sx0)
                    w = d * wx
                ok = inside & (w > F(0)) & fq
                a1 = np.where(ok, a1 + w * lq, a1)
                a2 = np.where(ok, a2 + w * (lq * lq), a2)
                ws = np.where(ok, ws + w, ws)
        m1 = a1 / ws
        vs = np.where(ws > F(0), fmax(a2 / ws - m1 * m1, F(0)), F(0)).astype(F)
        temporal = (Mout[..., 2] >= F(min_hist)) & np.isfinite(vt)
        v0 = np.where(temporal, vt, vs).astype(F)
    assert vt.dtype == F and vs.dtype == F and a1.dtype == F
    return v0, vt, vs, temporal


def ref_filter(Out, Mout, S, N, X, mix=False, k=0, iterations=4, sigma_l=4.0, sigma_x=0.2, min_hist=4.0):
    """(filtered rgb (H, W, 3), filtered variance (H, W), counts {"temporal", "spatial", "nonfinite"})"""
    Out = np.asarray(Out, F)
    n, _ = shown(S, mix, k)
    v0, _, _, temporal = ref_variance(Out, Mout, n, N, X, sigma_x, min_hist)
    c = np.ascontiguousarray(Out[..., :3])
    nd = F(2) * np.asarray(N, F)[..., :3] - F(1)
    x = np.ascontiguousarray(np.asarray(X, F)[..., :3])
    c1, v1 = atrous(c, prefilter(v0), nd, x, iterations, sigma_l, sigma_x)
    counts = {"temporal": int(temporal.sum()), "spatial": int((~temporal).sum()),
              "nonfinite": int((~np.isfinite(c).all(axis=-1)).sum())}
    return c1, v1, counts
