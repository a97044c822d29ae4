"""CPU: the host side of the guide maps (sail_guides): the argument checks that come before the context, the walk's shim
(tests/follow_oracle.cpp) against oracle.pick and the oracle's own AOVs at depth 0, what the fixture scenes give the walk to
follow, and the quality inequality of tests/test_gpu_guides.py evaluated entirely on the CPU (frames and AOVs from
oracle.render, the maps from the shim, the denoiser from the numpy reference)."""
import json
import os

import numpy as np
import pytest

import guides_ref as gr
import oracle
import temporal_ref as tr
from albedo_ref import rel_mse
from sail_amd import capi
from temporal_ref import bits
from test_gpu_denoise import ref_denoise

F = np.float32
INVALID = -1
W, H = 96, 64


def scene_view(sc):
    return np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [-1, 9, 100, -2 ** 31])
def test_depth_is_checked_before_the_context(depth):
    lib = capi.load()
    assert lib.sail_guides(None, None, None, depth, None, None, None) == INVALID
    assert "depth" in lib.sail_last_error(None).decode()


def test_a_good_depth_reaches_the_context_check():
    lib = capi.load()
    for depth in range(9):
        assert lib.sail_guides(None, None, None, depth, None, None, None) == INVALID
        assert "a context is required" in lib.sail_last_error(None).decode()


def test_the_other_calls_check_their_arguments_first():
    lib = capi.load()
    for on in (-1, 2):
        assert lib.sail_use_guides(None, on) == INVALID
        assert "on must be 0 or 1" in lib.sail_last_error(None).decode()
    assert lib.sail_use_guides(None, 1) == INVALID
    assert "a context is required" in lib.sail_last_error(None).decode()
    assert lib.sail_guides_load(None, None, None, None, None) == INVALID
    assert lib.sail_guides_read(None, 0, None) == INVALID
    assert (capi.GUIDE_N, capi.GUIDE_X) == (0, 1)
    assert lib.sail_abi_version() == 4


# ---- the shim ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C3", "C4", "ALL"])
def test_depth_0_is_the_first_hit_and_its_aovs(fixtures, name):
    """D = 0: the row is oracle.pick's, and the xyz of both maps are the AOVs of a one-sample render without jitter"""
    sc = fixtures["scenes"][name]
    mvp, eye = scene_view(sc)
    w, h = 33, 17
    masks = capi.plugin_masks(sc["plugins"])
    Ng, Xg, counts = gr.ref_guides(sc, mvp, eye, w, h, 0)
    idx, _ = oracle.pick(sc, masks[0], tr.ref_rays(mvp, eye, w, h).reshape(-1, 6))
    assert np.array_equal(Xg[..., 3].astype(np.int32).ravel(), idx) and (idx >= 0).any()
    hit = Xg[..., 3] >= 0
    assert counts["hit"] == int(hit.sum()) and counts["followed"] == 0 and not Ng[..., 3].any()
    _, seeds = capi.schedule(mvp, w, h, 0, 1)
    _, N, X = oracle.render(sc, masks, w, h, capi.jitter_inverse(mvp, 0.0, 0.0, w, h), seeds, sc["eye"], 1, aov=True)
    assert np.array_equal(bits(Ng[hit][:, :3]), bits(N[hit][:, :3]))
    assert np.array_equal(bits(Xg[hit][:, :3]), bits(X[hit][:, :3]))
    assert gr.same_maps(Ng[~hit], np.broadcast_to(gr.MISS_N, Ng[~hit].shape)) and np.isnan(Xg[~hit][:, :3]).all()


def test_the_fixture_scenes_give_the_walk_something_to_follow(fixtures):
    """96x64, D = 4: C1's mirror sphere (350 pixels, all depth 1); C3's mirror and glass reach depth 2 and more; C3 at D = 1
    is truncated (221 pixels); a larger D never shortens a walk"""
    c1, c3 = fixtures["scenes"]["C1"], fixtures["scenes"]["C3"]
    Ng, Xg, counts = gr.ref_guides(c1, *scene_view(c1), W, H, 4)
    assert counts["followed"] > 0 and counts["truncated"] == 0 and Ng[..., 3].max() == 1
    print(f"C1 {W}x{H} D 4: {counts}")
    followed = Ng[..., 3] > 0
    first = gr.ref_guides(c1, *scene_view(c1), W, H, 0)[1]
    assert (Xg[followed][:, 3] != first[followed][:, 3]).all()           # the surface behind is another row
    assert gr.same_maps(Xg[~followed], first[~followed])
    Ng3, _, counts3 = gr.ref_guides(c3, *scene_view(c3), W, H, 4)
    print(f"C3 {W}x{H} D 4: {counts3}, depths {np.bincount(Ng3[..., 3].astype(int).ravel())}")
    assert counts3["followed"] > 0 and (Ng3[..., 3] >= 2).any()
    _, _, counts1 = gr.ref_guides(c3, *scene_view(c3), W, H, 1)
    print(f"C3 {W}x{H} D 1: {counts1}")
    assert counts1["truncated"] > 0 and counts1["followed"] == counts3["followed"]
    Ng8 = gr.ref_guides(c3, *scene_view(c3), W, H, 8)[0]
    assert (Ng8[..., 3] >= Ng3[..., 3]).all() and Ng8[..., 3].max() <= 8


def test_rough_glass_is_not_followed():
    """glass_from_below of tests/golden/branch_scenes.json: its glass has ur = vr = 3, the microfacet branch, which scatters:
    the walk stops on it at every depth and the maps are the first hit's"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "branch_scenes.json")) as f:
        sc = json.load(f)["glass_from_below"]
    Ng0, Xg0, counts0 = gr.ref_guides(sc, *scene_view(sc), 33, 17, 0)
    Ng, Xg, counts = gr.ref_guides(sc, *scene_view(sc), 33, 17, 8)
    glass = capi.plugin_masks(sc["plugins"])[1] >> 4 & 1
    assert glass and counts == counts0 and counts["hit"] > 0 and (counts["followed"], counts["truncated"]) == (0, 0)
    assert gr.same_maps(Ng, Ng0) and gr.same_maps(Xg, Xg0)


# ---- quality: the inequality of the GPU test, on the CPU ------------------------------------------------------------------------
def test_guided_denoise_is_better_on_the_mirror_on_the_cpu(fixtures):
    """C1 at 96x64, 16 spp marked at 8, 5 bounces, against 512 spp from sample index 4096: relMSE over the pixels the walk
    follows, sail_denoise's reference with the guide maps against the same with the AOVs"""
    sc = fixtures["scenes"]["C1"]
    mvp, eye = scene_view(sc)
    masks = capi.plugin_masks(sc["plugins"])
    inv, seeds = capi.schedule(mvp, W, H, 0, 16)
    P = oracle.render(sc, masks, W, H, inv[:8], seeds[:8], sc["eye"], 5)
    S, N, X = oracle.render(sc, masks, W, H, inv[8:], seeds[8:], sc["eye"], 5, k0=8, accum=P.copy(), aov=True)
    inv_r, seeds_r = capi.schedule(mvp, W, H, 4096, 512)
    R = oracle.render(sc, masks, W, H, inv_r, seeds_r, sc["eye"], 5, k0=4096)
    ref = R[..., :3] / R[..., 3:4]
    Ng, Xg, counts = gr.ref_guides(sc, mvp, eye, W, H, 4)
    spec = Ng[..., 3] > 0
    plain, _, bad = ref_denoise(S, P, N, X)
    guided, _, badg = ref_denoise(S, P, Ng, Xg)
    e_plain, e_guided = rel_mse(plain[spec], ref[spec]), rel_mse(guided[spec], ref[spec])
    print(f"guided denoise (CPU) C1 {W}x{H}, {int(spec.sum())} followed pixels: relMSE plain {e_plain:.6g}, guided "
          f"{e_guided:.6g}; all pixels plain {rel_mse(plain, ref):.6g}, guided {rel_mse(guided, ref):.6g}")
    assert bad == 0 and badg == 0 and counts["followed"] == int(spec.sum()) > 0
    assert e_guided < e_plain
