"""The albedo map and the albedo-demodulated filters of include/sail_hip.h (sail_albedo, sail_denoise_albedo,
sail_temporal_filter_albedo) in numpy float32, one operation at a time: the reference of tests/test_gpu_albedo.py and
tests/test_albedo_host.py. Written from the header, not from the kernels. The first hit's surface colour comes from the CPU
oracle through tests/first_hit_oracle.cpp, a shim that includes the oracle's source and is built here on first use with
oracle/build.sh's flags; the sub-pixel rays are built from tests/temporal_ref.py's corner directions; the filters are the
plain references (tests/test_gpu_denoise.py's ref_denoise, tests/temporal_filter_ref.py) over the demodulated inputs."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_filter_ref as tf
import temporal_ref as tr
from atrous_ref import atrous, prefilter
from sail_amd import capi
from test_gpu_denoise import ref_denoise

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
# oracle/build.sh's flags
FLAGS = "-O2 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unused-function".split()
AMIN = capi.ALBEDO_AMIN_DEFAULT

_shim = None


def shim() -> ctypes.CDLL:
    global _shim
    if _shim is None:
        d = tempfile.mkdtemp(prefix="sail_first_hit_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libsail_first_hit.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, os.path.join(HERE, "first_hit_oracle.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        f32p, ci, u32 = ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_uint32
        L.oracle_first_hit.restype = ci
        L.oracle_first_hit.argtypes = [f32p, ci, f32p, ci, u32, u32, f32p, ci, ctypes.POINTER(ci), f32p]
        _shim = L
    return _shim


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F))


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def first_hit(sc, rays):
    """(index (count,) int32, surface colour (count, 3) f32) of the first hit of (count, 6) rays, with the scene's masks"""
    masks = capi.plugin_masks(sc["plugins"])
    r = _f(rays).reshape(-1, 6)
    o, t = _f(sc["objects"]), _f(sc["texparams"])
    idx = np.zeros(len(r), np.int32)
    col = np.zeros((len(r), 3), F)
    rc = shim().oracle_first_hit(_p(o), sc["n"], _p(t), sc["tn"], int(masks[0]), int(masks[2]), _p(r), len(r),
                                 idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _p(col))
    assert rc == 0
    return idx, col


def sub_rays(mvp, eye, W, H, g, i, j):
    """(H, W, 6): the ray of sub-pixel (i, j) of a g x g grid in every pixel"""
    d = tr.corner_dirs(capi.jitter_inverse(mvp, 0.0, 0.0, W, H), eye)
    s = np.broadcast_to(((np.arange(W, dtype=F) + (F(i) + F(0.5)) / F(g)) / F(W))[None, :], (H, W))
    t = np.broadcast_to(((np.arange(H, dtype=F) + (F(j) + F(0.5)) / F(g)) / F(H))[:, None], (H, W))
    tri0 = s + t <= F(1)
    out = np.zeros((H, W, 6), F)
    out[..., :3] = np.asarray(eye, F)
    for c in range(3):
        a = (d[0, c] + (d[2, c] - d[0, c]) * s) + (d[1, c] - d[0, c]) * t
        b = (d[3, c] + (d[1, c] - d[3, c]) * (F(1) - s)) + (d[2, c] - d[3, c]) * (F(1) - t)
        out[..., 3 + c] = np.where(tri0, a, b)
    assert out.dtype == F and s.dtype == F
    return out


def ref_albedo(sc, mvp, eye, W, H, g):
    """(A (H, W, 4), pixels with a hit, pixels where some but not all rays hit)"""
    total, cnt = np.zeros((H, W, 3), F), np.zeros((H, W), np.int32)
    for j in range(g):
        for i in range(g):
            idx, col = first_hit(sc, sub_rays(mvp, eye, W, H, g, i, j))
            hit = (idx >= 0).reshape(H, W)
            total = np.where(hit[..., None], total + col.reshape(H, W, 3), total)
            cnt = cnt + hit
    A = np.ones((H, W, 4), F)
    A[..., 3] = 0
    some = cnt > 0
    cf = cnt.astype(F)
    with np.errstate(all="ignore"):
        A[..., :3] = np.where(some[..., None], total / cf[..., None], F(1))
    A[..., 3] = cf
    assert total.dtype == F and A.dtype == F
    return A, int(some.sum()), int((some & (cnt < g * g)).sum())


# ---- demodulation ----------------------------------------------------------------------------------------------------------
def factor(A, amin=AMIN):
    """(f (H, W, 3), lf (H, W)): a channel of A that is finite and > amin, else 1"""
    a = np.asarray(A, F)[..., :3]
    with np.errstate(all="ignore"):
        f = np.where(np.isfinite(a) & (a > F(amin)), a, F(1)).astype(F)
    lf = ((f[..., 0] + f[..., 1]) + f[..., 2]) / F(3)
    assert lf.dtype == F
    return f, lf


def demodulated(S, f):
    out = np.array(S, F)
    with np.errstate(all="ignore"):
        out[..., :3] = out[..., :3] / f
    return out


def ref_denoise_albedo(S, P, N, X, A, amin=AMIN, **kw):
    """(rgb (H, W, 3), variance (H, W), pixels whose demodulated mean colour is not finite)"""
    f, lf = factor(A, amin)
    c, v, bad = ref_denoise(demodulated(S, f), demodulated(P, f), N, X, **kw)
    with np.errstate(all="ignore"):
        out, var = (c * f).astype(F), (v * (lf * lf)).astype(F)
    return out, var, bad


def ref_filter_albedo(Out, Mout, S, N, X, A, amin=AMIN, mix=False, k=0, iterations=4, sigma_l=4.0, sigma_x=0.2, min_hist=4.0):
    """(rgb (H, W, 3), variance (H, W), counts): tests/temporal_filter_ref.py's ref_filter with c = Out.rgb / f and
    vt / (lf * lf) in vt's place"""
    f, lf = factor(A, amin)
    OutD = demodulated(Out, f)
    Mout = np.asarray(Mout, F)
    n, _ = tf.shown(S, mix, k)
    _, vt, vs, _ = tf.ref_variance(OutD, Mout, n, N, X, sigma_x, min_hist)
    with np.errstate(all="ignore"):
        vtd = (vt / (lf * lf)).astype(F)
        temporal = (Mout[..., 2] >= F(min_hist)) & np.isfinite(vtd)
        v0 = np.where(temporal, vtd, vs).astype(F)
    c = np.ascontiguousarray(OutD[..., :3])
    nd = F(2) * np.asarray(N, F)[..., :3] - F(1)
    x = np.ascontiguousarray(np.asarray(X, F)[..., :3])
    c1, v1 = atrous(c, prefilter(v0), nd, x, iterations, sigma_l, sigma_x)
    with np.errstate(all="ignore"):
        out, var = (c1 * f).astype(F), (v1 * (lf * lf)).astype(F)
    counts = {"temporal": int(temporal.sum()), "spatial": int((~temporal).sum()),
              "nonfinite": int((~np.isfinite(c).all(axis=-1)).sum())}
    return out, var, counts


def rel_mse(x, ref):
    """tests/test_gpu_denoise.py's relMSE"""
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


# ---- the synthetic frame of the "texture survives" tests ---------------------------------------------------------------------
def synthetic_halves(A, seed=7):
    """For a map A (H, W, 4): the truth T = A.rgb * E with E = 0.5 + 0.25 x / W, and two halves of 8 samples each as SUM
    accumulators: the mark P (8 samples, mean T (1 + 0.5 e1)) and the frame S (16 samples: P plus 8 with mean
    T (1 + 0.5 e2)), e seeded uniform in (-1, 1)"""
    H, W = A.shape[:2]
    rng = np.random.default_rng(seed)
    E = (F(0.5) + F(0.25) * np.arange(W, dtype=F) / F(W))[None, :, None]
    T = (np.asarray(A, F)[..., :3] * E).astype(F)
    e1 = (rng.random((H, W, 1), dtype=F) * F(2) - F(1)).astype(F)
    e2 = (rng.random((H, W, 1), dtype=F) * F(2) - F(1)).astype(F)
    P = np.zeros((H, W, 4), F)
    P[..., :3] = T * (F(1) + F(0.5) * e1) * F(8)
    P[..., 3] = 8
    S = np.zeros((H, W, 4), F)
    S[..., :3] = P[..., :3] + T * (F(1) + F(0.5) * e2) * F(8)
    S[..., 3] = 16
    return T, P, S
