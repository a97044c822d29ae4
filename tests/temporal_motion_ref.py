"""The reprojection across an object move (include/sail_hip.h, sail_move_objects and sail_temporal_begin with a motion
pending) in numpy float32, one operation at a time and vectorised over pixels: the reference of
tests/test_gpu_temporal_motion.py and tests/test_temporal_motion_host.py. Written from the header, not from the kernels.
Every operation of the formulas is an IEEE f32 one, so the device's maps must equal these bit for bit. The gather is
tests/temporal_ref.py's, with the motion table D; the two functions at the end only name the moved passes."""
import copy

import numpy as np

import temporal_filter_ref as tf
import temporal_ref as tr
from temporal_ref import bits, previous_position  # noqa: F401  (re-exported for the tests)

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


def ref_reproject_moved(Gcur, Gprev, Hist, mvp_prev, eye_prev, D, mc=np.inf, pos_tol=0.05):
    """(R (H, W, 4), the number of pixels that found a history)"""
    return tr.ref_reproject(Gcur, Gprev, Hist, mvp_prev, eye_prev, pos_tol, D, mc)


def ref_moment_reproject_moved(Gcur, Gprev, Mhist, mvp_prev, eye_prev, D, mc=np.inf, pos_tol=0.05):
    """MR (H, W, 4): the same gather over Mhist, MR.z = min(m, mc)"""
    return tf.ref_moment_reproject(Gcur, Gprev, Mhist, mvp_prev, eye_prev, pos_tol, D, mc)
