"""The camera-motion reprojection formulas of include/sail_hip.h (sail_gbuffer, sail_temporal_begin, sail_temporal_resolve)
in numpy float32, one operation at a time and vectorised over pixels: the reference of tests/test_gpu_temporal.py and
tests/test_temporal_host.py. Written from the header, not from the kernels. Every operation of the formulas is an IEEE
f32 one, so the device's maps must equal these bit for bit. The first hit itself (object row, distance) is not restated
here: it comes from oracle.pick, the shader's intersectObjects on the CPU."""
import numpy as np

import oracle
from sail_amd import capi

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- views --------------------------------------------------------------------------------------------------------------
CENTER = (2.78, 2.73, 2.8)          # the middle of the Cornell room the fixture cameras look into


def view(eye, center=CENTER):
    """(P*MV as 16 doubles row-major, eye as 3 f32) of the fixtures' camera model: fovy 55, aspect 1, near 1, far 100"""
    return capi.camera(eye, center).reshape(16), np.asarray(eye, F)


def orbit(deg, radius=8.8, center=CENTER, height=0.0):
    """the fixture camera (0 degrees: eye (2.78, 2.73, -6)) orbited about the vertical axis through `center`"""
    a = np.deg2rad(deg)
    eye = (center[0] + radius * np.sin(a), center[1] + height, center[2] - radius * np.cos(a))
    return view(eye, center)


INSIDE = ((2.0, 3.0, 0.6), (3.2, 1.8, 4.5))     # an eye inside the room and what it looks at


def mp32(mvp):
    """the view's matrix as the context keeps it: each double rounded to f32, row-major"""
    return np.asarray(mvp, np.float64).reshape(4, 4).astype(F)


# ---- G-buffer -----------------------------------------------------------------------------------------------------------
def corner_dirs(inv, eye):
    """the host's cornerDirs for one column-major f32 inverse: gdiv(a, b) = a * F(F(1) / b)"""
    M = np.asarray(inv, F).reshape(16)
    e = np.asarray(eye, F)
    out = np.zeros((4, 3), F)
    for c, (cx, cy) in enumerate(((-1, -1), (-1, 1), (1, -1), (1, 1))):
        q = [((M[r] * F(cx) + M[4 + r] * F(cy)) + M[8 + r] * F(0)) + M[12 + r] * F(1) for r in range(4)]
        rq = F(1) / q[3]
        w = [q[i] * rq - e[i] for i in range(3)]
        ln = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        rl = F(1) / ln
        out[c] = [w[i] * rl for i in range(3)]
    assert out.dtype == F
    return out


def ref_rays(mvp, eye, W, H):
    """(H, W, 6): origin and direction of every pixel's ray for a sample of zero jitter"""
    d = corner_dirs(capi.jitter_inverse(mvp, 0.0, 0.0, W, H), eye)
    s = np.broadcast_to(((np.arange(W, dtype=F) + F(0.5)) / F(W))[None, :], (H, W))
    t = np.broadcast_to(((np.arange(H, dtype=F) + F(0.5)) / F(H))[:, None], (H, W))
    tri0 = s + t <= F(1)
    out = np.zeros((H, W, 6), F)
    out[..., :3] = np.asarray(eye, F)
    for c in range(3):
        a = (d[0, c] + (d[2, c] - d[0, c]) * s) + (d[1, c] - d[0, c]) * t
        b = (d[3, c] + (d[1, c] - d[3, c]) * (F(1) - s)) + (d[2, c] - d[3, c]) * (F(1) - t)
        out[..., 3 + c] = np.where(tri0, a, b)
    return out


def ref_xyz(rays, idx, t):
    """o + d * t, a product and a sum per component; 0 on a miss"""
    X = rays[..., :3] + rays[..., 3:] * np.asarray(t, F)[..., None]
    return np.where((idx >= 0)[..., None], X, F(0)).astype(F)


def ref_gbuffer(sc, mvp, eye, W, H):
    """(G (H, W, 4), rays, id, t) with the first hit from oracle.pick"""
    rays = ref_rays(mvp, eye, W, H)
    idx, t = oracle.pick(sc, capi.plugin_masks(sc["plugins"])[0], rays.reshape(-1, 6))
    idx, t = idx.reshape(H, W), t.reshape(H, W)
    G = np.zeros((H, W, 4), F)
    G[..., :3] = ref_xyz(rays, idx, t)
    G[..., 3] = idx.astype(F)
    return G, rays, idx, t


# ---- reproject ----------------------------------------------------------------------------------------------------------
def project(G, Mp, W, H):
    """(u, v, valid): where each pixel's first hit lies in the view Mp, in that view's pixel coordinates"""
    X, idf = G[..., :3], G[..., 3]
    with np.errstate(all="ignore"):
        c = [((Mp[i, 0] * X[..., 0] + Mp[i, 1] * X[..., 1]) + Mp[i, 2] * X[..., 2]) + Mp[i, 3] for i in (0, 1, 3)]
        valid = ~(idf < F(0)) & (c[2] > F(0))
        u = ((c[0] / c[2]) * F(0.5) + F(0.5)) * F(W) - F(0.5)
        v = ((c[1] / c[2]) * F(0.5) + F(0.5)) * F(H) - F(0.5)
    valid &= np.isfinite(u) & np.isfinite(v)
    assert u.dtype == F and v.dtype == F
    return u, v, valid


def fmax(a, b):
    """the header's max(a, b) = a > b ? a : b"""
    return np.where(a > b, a, b).astype(F)


def fmin(a, b):
    """the header's min(a, b) = a < b ? a : b"""
    return np.where(a < b, a, b).astype(F)


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


def gather(Gcur, Gprev, mvp_prev, eye_prev, pos_tol, D=None):
    """the reproject passes' up to four taps per pixel, b then a: a list of (w, ok, yi, xi), ok = the tap lies inside the
    frame with a weight and shows the same object at the same place. With a motion table D (sail_move_objects) the point
    looked up is Xp = X - D[id]"""
    Gcur, Gprev = np.asarray(Gcur, F), np.asarray(Gprev, F)
    H, W = Gcur.shape[:2]
    Mp, ep, tol = mp32(mvp_prev), np.asarray(eye_prev, F), F(pos_tol)
    Gp = Gcur if D is None else previous_position(Gcur, D)
    Xp, idf = Gp[..., :3], Gcur[..., 3]
    u, v, valid = project(Gp, Mp, W, H)
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


def ref_reproject(Gcur, Gprev, Hist, mvp_prev, eye_prev, pos_tol=0.05, D=None, mc=np.inf):
    """(R (H, W, 4), the number of pixels that found a history); with D and mc, the pass after sail_move_objects"""
    Hist = np.asarray(Hist, F)
    H, W = Hist.shape[:2]
    acc, wsum, m = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.full((H, W), np.inf, F)
    with np.errstate(all="ignore"):
        for w, ok, yi, xi in gather(Gcur, Gprev, mvp_prev, eye_prev, pos_tol, D):
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


# ---- resolve ------------------------------------------------------------------------------------------------------------
def ref_resolve(S, R, mix=False, k=0, cap=32.0):
    """(Out (H, W, 4), pixels with a history, pixels whose current mean is not finite)"""
    S, R, cap = np.asarray(S, F), np.asarray(R, F), F(cap)
    n = np.full(S.shape[:2], F(k)) if mix else S[..., 3]
    with np.errstate(all="ignore"):
        if mix:
            c0 = S[..., :3].copy()
        else:
            c0 = np.where((n > F(0))[..., None], S[..., :3] / n[..., None], F(0)).astype(F)
        fin = np.isfinite(c0).all(axis=-1)
        m = R[..., 3]
        hist, cur = m > F(0), (n > F(0)) & fin
        ws = m + n
        both = ((m[..., None] * R[..., :3]) + (n[..., None] * c0)) / ws[..., None]
        Out = np.zeros(S.shape, F)
        Out[..., :3] = np.where((hist & cur)[..., None], both, np.where(hist[..., None], R[..., :3], c0))
        Out[..., 3] = np.where(hist & cur, np.where(ws < cap, ws, cap), np.where(hist, m, np.where(n < cap, n, cap)))
    assert both.dtype == F
    return Out, int(hist.sum()), int((~fin).sum())


def quantise(o):
    """the filter kernel's (uint8)(int)(clamp(o, 0, 1) * 255 + 0.5)"""
    return (oracle.math(12, o) * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)


def display(c, kind, gamma_c):
    """sail_filter's pointwise kinds 0..2 by the math spec's CPU restatement"""
    c = np.ascontiguousarray(c, F)
    if kind == capi.FILTER_COLOR:
        return c
    if kind == capi.FILTER_GAMMA:
        return oracle.math(5, c, oracle.math(14, np.full_like(c, F(gamma_c))))
    xx = oracle.math(10, np.zeros_like(c), c - F(0.004))
    return oracle.math(11, xx * (F(6.2) * xx + F(0.5)), xx * (F(6.2) * xx + F(1.7)) + F(0.06))
