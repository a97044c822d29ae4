"""CPU: the host side of the albedo map and the albedo-demodulated filters: the argument checks that come before the
context, the first-hit shim (tests/first_hit_oracle.cpp) against oracle.pick, the numpy references of tests/albedo_ref.py
against the plain references for a map of ones, and the "texture survives" inequality of tests/test_gpu_albedo.py evaluated
entirely on the CPU (AOVs from oracle.render, the map from the shim, the filters from the numpy references)."""
import ctypes

import numpy as np
import pytest

import albedo_ref as ar
import oracle
import temporal_filter_ref as tf
import temporal_ref as tr
from sail_amd import capi
from temporal_ref import bits
from test_gpu_denoise import ref_denoise

F = np.float32
INVALID = -1


def scene_view(sc):
    return np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 5, -1, 100])
def test_grid_is_checked_before_the_context(grid):
    lib = capi.load()
    assert lib.sail_albedo(None, None, None, grid, None, None) == INVALID
    assert "grid" in lib.sail_last_error(None).decode()


def test_a_good_grid_reaches_the_context_check():
    lib = capi.load()
    for grid in (1, 2, 3, 4):
        assert lib.sail_albedo(None, None, None, grid, None, None) == INVALID
        assert "a context is required" in lib.sail_last_error(None).decode()


@pytest.mark.parametrize("amin", [0.0, -0.01, float("nan"), float("inf"), -float("inf")])
def test_amin_is_checked_before_the_context(amin):
    lib = capi.load()
    assert lib.sail_temporal_filter_albedo(None, None, amin, None, None, None, None) == INVALID
    assert "amin" in lib.sail_last_error(None).decode()
    assert lib.sail_denoise_albedo(None, None, amin, None, None, None, None) == INVALID


def test_what_the_plain_calls_refuse_is_refused():
    lib = capi.load()
    p = capi.TfilterParams(0, 4.0, 0.2, 4.0, 0, 2.2)
    assert lib.sail_temporal_filter_albedo(None, ctypes.byref(p), 0.01, None, None, None, None) == INVALID
    assert "bad parameters" in lib.sail_last_error(None).decode()
    assert lib.sail_temporal_filter_albedo(None, None, 0.01, None, None, None, None) == INVALID
    assert "a context is required" in lib.sail_last_error(None).decode()
    for fn in (lib.sail_albedo_read, ):
        assert fn(None, None) == INVALID
    assert lib.sail_albedo_load(None, None, None, None) == INVALID
    assert capi.ALBEDO_AMIN_DEFAULT == 0.01


# ---- the shim ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C3", "C4", "ALL", "BILERP"])
def test_shim_index_equals_oracle_pick(fixtures, name):
    sc = fixtures["scenes"][name]
    mvp, eye = scene_view(sc)
    W, H = 33, 17
    rays = tr.ref_rays(mvp, eye, W, H)
    idx, _ = oracle.pick(sc, capi.plugin_masks(sc["plugins"])[0], rays.reshape(-1, 6))
    got, col = ar.first_hit(sc, rays)
    assert np.array_equal(got, idx) and (idx >= 0).any()
    assert np.isfinite(col).all() and not col[idx < 0].any()
    # the grid-1 sub-ray is the G-buffer's ray bit for bit
    assert np.array_equal(bits(ar.sub_rays(mvp, eye, W, H, 1, 0, 0)), bits(rays))


def test_map_of_a_textured_scene_has_texture(fixtures):
    """C3 at 33x17, grid 2: the checkerboards give values other than one flat colour per object, and pixels whose
    sub-samples disagree"""
    sc = fixtures["scenes"]["C3"]
    mvp, eye = scene_view(sc)
    A, hit, partial = ar.ref_albedo(sc, mvp, eye, 33, 17, 2)
    assert hit == 33 * 17 and partial == 0 and (A[..., 3] == 4).all()
    A1, _, _ = ar.ref_albedo(sc, mvp, eye, 33, 17, 1)
    assert len(np.unique(bits(A[..., 0]))) > len(np.unique(bits(A1[..., 0])))


# ---- a map of ones changes nothing ---------------------------------------------------------------------------------------------
def random_frame(W, H, seed):
    rng = np.random.default_rng(seed)
    P = np.zeros((H, W, 4), F)
    P[..., 3] = rng.integers(1, 5, (H, W))
    P[..., :3] = rng.random((H, W, 3), dtype=F) * P[..., 3:4]
    S = P.copy()
    add = rng.integers(1, 5, (H, W)).astype(F)
    S[..., :3] += rng.random((H, W, 3), dtype=F) * add[..., None]
    S[..., 3] += add
    N = np.zeros((H, W, 4), F)
    n = rng.standard_normal((H, W, 3)).astype(F)
    N[..., :3] = F(0.5) * (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F) + F(0.5)
    X = np.zeros((H, W, 4), F)
    X[..., :3] = rng.random((H, W, 3), dtype=F)
    return S, P, N, X


@pytest.mark.parametrize("w", [0.0, 1.0, 16.0])
def test_ones_map_gives_the_plain_references(w):
    W, H = 21, 13
    S, P, N, X = random_frame(W, H, 5)
    A = np.ones((H, W, 4), F)
    A[..., 3] = w
    c, v, bad = ref_denoise(S, P, N, X)
    ca, va, bada = ar.ref_denoise_albedo(S, P, N, X, A)
    assert np.array_equal(bits(c), bits(ca)) and np.array_equal(bits(v), bits(va)) and bad == bada
    rng = np.random.default_rng(9)
    Out = np.zeros((H, W, 4), F)
    Out[..., :3] = rng.random((H, W, 3), dtype=F)
    Out[..., 3] = 3
    Mout = np.zeros((H, W, 4), F)
    Mout[..., 0] = rng.random((H, W), dtype=F)
    Mout[..., 1] = Mout[..., 0] ** 2 + rng.random((H, W), dtype=F) * F(0.1)
    Mout[..., 2] = rng.choice(np.array([1, 3, 4, 9], F), (H, W))          # both sides of min_hist
    c, v, counts = tf.ref_filter(Out, Mout, S, N, X)
    ca, va, countsa = ar.ref_filter_albedo(Out, Mout, S, N, X, A)
    assert np.array_equal(bits(c), bits(ca)) and np.array_equal(bits(v), bits(va)) and counts == countsa
    assert 0 < counts["temporal"] < W * H


def test_factor_guards():
    """channels that are 0, -0, below, at and just above amin, negative, NaN, Inf and large"""
    amin = F(0.01)
    vals = np.array([0.0, -0.0, 0.005, amin, np.nextafter(amin, F(1)), -0.5, np.nan, np.inf, -np.inf, 2.0 ** 20, 0.5], F)
    A = np.zeros((1, len(vals), 4), F)
    A[0, :, 0] = vals
    A[0, :, 1:3] = 1
    f, lf = ar.factor(A, amin)
    want = np.array([1, 1, 1, 1, np.nextafter(amin, F(1)), 1, 1, 1, 1, 2.0 ** 20, 0.5], F)
    assert np.array_equal(bits(f[0, :, 0]), bits(want))
    assert np.array_equal(bits(lf[0]), bits(((want + F(1)) + F(1)) / F(3)))


# ---- texture survives: the inequality of the GPU test, on the CPU ---------------------------------------------------------------
def test_texture_survives_on_the_cpu(fixtures):
    sc = fixtures["scenes"]["C3"]
    mvp, eye = scene_view(sc)
    W, H = 96, 64
    A, hit, _ = ar.ref_albedo(sc, mvp, eye, W, H, 4)
    assert hit == W * H
    T, P, S = ar.synthetic_halves(A)
    inv, seeds = capi.schedule(mvp, W, H, 0, 1)
    _, N, X = oracle.render(sc, capi.plugin_masks(sc["plugins"]), W, H, inv, seeds, sc["eye"], 3, aov=True)
    plain, _, bad = ref_denoise(S, P, N, X)
    demod, _, bada = ar.ref_denoise_albedo(S, P, N, X, A)
    noisy = S[..., :3] / S[..., 3:4]
    e_in, e_plain, e_demod = ar.rel_mse(noisy, T), ar.rel_mse(plain, T), ar.rel_mse(demod, T)
    print(f"texture survives (CPU) C3 {W}x{H}: relMSE input {e_in:.6g}, plain {e_plain:.6g}, albedo {e_demod:.6g}")
    assert bad == 0 and bada == 0
    assert e_demod < e_plain
