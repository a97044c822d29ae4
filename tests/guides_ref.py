"""The guide maps of include/sail_hip.h (sail_guides) from the CPU oracle: the reference of tests/test_gpu_guides.py and
tests/test_guides_host.py. The walk is tests/follow_oracle.cpp, a shim that includes the oracle's source and is built here on
first use with oracle/build.sh's flags; the rays are tests/temporal_ref.py's G-buffer rays. The guided filters are the plain
numpy references (tests/test_gpu_denoise.py's ref_denoise, tests/albedo_ref.py, tests/temporal_filter_ref.py) with Ng, Xg in
the place of N, X: they are not restated here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_ref as tr
from albedo_ref import FLAGS
from sail_amd import capi

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MISS_N = np.array([0.5, 0.5, 0.5, 0.0], F)

_shim = None


def shim() -> ctypes.CDLL:
    global _shim
    if _shim is None:
        d = tempfile.mkdtemp(prefix="sail_follow_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libsail_follow.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, os.path.join(HERE, "follow_oracle.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        f32p, ci, u32 = ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_uint32
        L.oracle_follow.restype = ci
        L.oracle_follow.argtypes = [f32p, ci, f32p, ci, u32, u32, u32, f32p, ci, ci, f32p, f32p,
                                    ctypes.POINTER(ctypes.c_ulonglong)]
        _shim = L
    return _shim


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F))


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def ref_guides(sc, mvp, eye, W, H, D):
    """(Ng (H, W, 4), Xg (H, W, 4), {"hit", "followed", "truncated"}) of the view with follow depth D"""
    masks = capi.plugin_masks(sc["plugins"])
    rays = _f(tr.ref_rays(mvp, eye, W, H)).reshape(-1, 6)
    o, t = _f(sc["objects"]), _f(sc["texparams"])
    Ng, Xg = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    counts = (ctypes.c_ulonglong * 3)()
    rc = shim().oracle_follow(_p(o), sc["n"], _p(t), sc["tn"], int(masks[0]), int(masks[1]), int(masks[2]), _p(rays),
                              len(rays), int(D), _p(Ng), _p(Xg), counts)
    assert rc == 0
    return Ng, Xg, {"hit": int(counts[0]), "followed": int(counts[1]), "truncated": int(counts[2])}


def same_maps(a, b):
    """bit for bit, a NaN (a missed pixel's position) matching any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((tr.bits(a) == tr.bits(b)) | (np.isnan(a) & np.isnan(b))).all())
