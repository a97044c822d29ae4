"""The reprojection across an object move (include/sail_hip.h, sail_move_objects and sail_temporal_begin with a motion
pending) in numpy float32, one operation at a time and vectorised over pixels: the reference of
tests/test_gpu_temporal_motion.py and tests/test_temporal_motion_host.py. Written from the header, not from the kernels.
Every operation of the formulas is an IEEE f32 one, so the device's maps must equal these bit for bit. With D = 0 and
mc = inf the functions here are tests/temporal_ref.py's ref_reproject and tests/temporal_filter_ref.py's
ref_moment_reproject."""
import copy

import numpy as np

import temporal_ref as tr
from temporal_ref import bits  # noqa: F401  (re-exported for the tests)

F = np.float32
MINMAX_TYPES = (1, 3, 9)     # the shapes whose row holds a min and a max corner: words 1..3 and 4..6


def moved(scene, moves):
    """a copy of the scene dict with the rows of `moves` ({row: (dx, dy, dz)}) translated: d is added in f32 to row words
    1..3, and to words 4..6 as well for the min/max shapes"""
    sc = copy.deepcopy(scene)
    rows = np.array(sc["objects"], F).reshape(-1, 18)
    for r, d in moves.items():
        d = np.asarray(d, F)
        rows[r, 1:4] = rows[r, 1:4] + d
        if int(rows[r, 0]) in MINMAX_TYPES:
            rows[r, 4:7] = rows[r, 4:7] + d
    sc["objects"] = rows.reshape(-1).tolist()
    return sc


def motion_table(n, moves):
    """(n, 3) f32: the motion argument of sail_move_objects for `moves`"""
    D = np.zeros((n, 3), F)
    for r, d in moves.items():
        D[r] = np.asarray(d, F)
    return D


def previous_position(Gcur, D):
    """(H, W, 4): (Xp, id) with Xp = X - D[(int)id] per component; pixels that miss keep X"""
    Gcur, D = np.asarray(Gcur, F), np.asarray(D, F).reshape(-1, 3)
    idf = Gcur[..., 3]
    hit = ~(idf < F(0))
    row = np.where(hit, idf, F(0)).astype(np.int64)
    d = np.where(hit[..., None], D[row], F(0)).astype(F)
    Gp = Gcur.copy()
    Gp[..., :3] = Gcur[..., :3] - d
    assert Gp.dtype == F
    return Gp


def _gather(Gcur, Gprev, mvp_prev, eye_prev, D, pos_tol):
    """the taps of the reproject with motion: yields (w, ok-so-far, flat tap index arrays) in the stated order"""
    Gcur, Gprev = np.asarray(Gcur, F), np.asarray(Gprev, F)
    H, W = Gcur.shape[:2]
    Mp, ep, tol = tr.mp32(mvp_prev), np.asarray(eye_prev, F), F(pos_tol)
    Gp = previous_position(Gcur, D)
    Xp, idf = Gp[..., :3], Gcur[..., 3]
    u, v, valid = tr.project(Gp, Mp, W, H)
    taps = []
    with np.errstate(all="ignore"):
        iu, iv = np.floor(u), np.floor(v)
        fu, fv = u - iu, v - iv
        r = Xp - ep
        r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        lim = (tol * tol) * r2
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = iu + F(a), iv + F(b)
                inside = valid & (qx >= F(0)) & (qx <= F(W - 1)) & (qy >= F(0)) & (qy <= F(H - 1))
                w = (fu if a else F(1) - fu) * (fv if b else F(1) - fv)
                xi = np.where(inside, qx, F(0)).astype(np.int64)
                yi = np.where(inside, qy, F(0)).astype(np.int64)
                gq = Gprev[yi, xi]
                e = Xp - gq[..., :3]
                e2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                ok = inside & (w > F(0)) & (gq[..., 3] == idf) & (e2 <= lim)
                assert w.dtype == F and e2.dtype == F
                taps.append((w, ok, yi, xi))
    return taps


def fmin(a, b):
    """the header's min(a, b) = a < b ? a : b"""
    return np.where(a < b, a, b).astype(F)


def ref_reproject_moved(Gcur, Gprev, Hist, mvp_prev, eye_prev, D, mc=np.inf, pos_tol=0.05):
    """(R (H, W, 4), the number of pixels that found a history)"""
    Hist = np.asarray(Hist, F)
    H, W = Hist.shape[:2]
    acc, wsum, m = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.full((H, W), np.inf, F)
    with np.errstate(all="ignore"):
        for w, ok, yi, xi in _gather(Gcur, Gprev, mvp_prev, eye_prev, D, pos_tol):
            h = Hist[yi, xi]
            ok = ok & (h[..., 3] > F(0)) & np.isfinite(h[..., :3]).all(axis=-1)
            acc = np.where(ok[..., None], acc + w[..., None] * h[..., :3], acc)
            wsum = np.where(ok, wsum + w, wsum)
            m = np.where(ok & (h[..., 3] < m), h[..., 3], m)
        found = wsum > F(0)
        R = np.zeros((H, W, 4), F)
        R[..., :3] = np.where(found[..., None], acc / wsum[..., None], F(0))
        R[..., 3] = np.where(found, fmin(m, F(mc)), F(0))
    assert acc.dtype == F and wsum.dtype == F
    return R, int(found.sum())


def ref_moment_reproject_moved(Gcur, Gprev, Mhist, mvp_prev, eye_prev, D, mc=np.inf, pos_tol=0.05):
    """MR (H, W, 4): the same gather over Mhist, MR.z = min(m, mc)"""
    Mhist = np.asarray(Mhist, F)
    H, W = Mhist.shape[:2]
    a1, a2, wsum, m = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.full((H, W), np.inf, F)
    with np.errstate(all="ignore"):
        for w, ok, yi, xi in _gather(Gcur, Gprev, mvp_prev, eye_prev, D, pos_tol):
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
