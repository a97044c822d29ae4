"""Adaptive sampling on the GPU: the tile mask (sail_set_active_tiles: the tile table every trace kernel walks, the masked
mark of sail_noise.hip) and sail_render_adaptive. Needs a GPU.

Every comparison is bit for bit, as raw uint32, against *uniform* renders (render_schedule over samples 0..k-1 on a
context that never saw a mask), which tests/test_gpu_parity.py proves against the CPU oracle for every kernel form: sample
k has one seed and one jitter whatever the mask, so a tile traced for samples 0..k-1 and then left alone must hold the
uniform k-sample frame's bits, accumulator and AOVs. The driver's outcome (which tile freezes at which look) is computed in
numpy (tests/adaptive_ref.py) from the uniform run's own tile_err maps; the target is taken from those maps, halfway
between two adjacent distinct per-tile errors, so that no rounding can flip a decision."""
import math

import numpy as np
import pytest

import adaptive_ref as ar
from sail_amd import capi
from test_gpu_denoise import ref_denoise, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
K = 3  # samples per half of the explicit-mask renders
SIZES = [(160, 96), (64, 64), (65, 3)]  # 3 x 2 tiles ragged right and top; one tile; a one-pixel-wide tile


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def sched(sc, W, H, k0, spp):
    return capi.schedule(np.array(sc["mvp_rowmajor"]), W, H, k0, spp)


def render(ctx, sc, k0, spp, B):
    inv, seeds = sched(sc, ctx.W, ctx.H, k0, spp)
    ctx.render_schedule(inv, seeds, sc["eye"], B)


def frame(ctx):
    """(accumulator, normal map, position map) as the device holds them"""
    _, n, p = ctx.readback(aov=True)
    return ctx.read_accum(), n, p


_UNIFORM = {}


def uniform(fixtures, name, W, H, B):
    """the uniform K- and 2K-sample frames and the zero frame, rendered once per case on a context of its own"""
    key = (name, W, H, B)
    if key not in _UNIFORM:
        sc = fixtures["scenes"][name]
        ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
        try:
            ctx.set_scene_dict(sc)
            zero = frame(ctx)
            render(ctx, sc, 0, K, B)
            first = frame(ctx)
            render(ctx, sc, K, K, B)
            _UNIFORM[key] = (zero, first, frame(ctx))
        finally:
            ctx.close()
    return _UNIFORM[key]


def masks_for(W, H):
    tx, ty = ar.tiles64(W, H)
    i, j = np.meshgrid(np.arange(tx), np.arange(ty))
    ragged = ((i == tx - 1) & (W % 64 != 0)) | ((j == ty - 1) & (H % 64 != 0))
    one = np.zeros((ty, tx), bool)
    one[ty - 1, tx - 1] = True  # the last tile: the corner one, ragged both ways where the frame is
    cands = {"one": one, "checker": (i + j) % 2 == 0, "ragged": ragged, "empty": np.zeros((ty, tx), bool),
             "ones": np.ones((ty, tx), bool)}
    out, seen = {}, set()
    for name, m in cands.items():
        if name in ("empty", "ones") or m.tobytes() not in seen:
            out[name] = m.astype(np.uint8)
        seen.add(m.tobytes())
    return out


def check_tiles(got, mask, inside, outside, what):
    """active tiles hold `inside`'s texels, inactive ones `outside`'s: accumulator and both AOV maps"""
    H, W = got[0].shape[:2]
    wrong = []
    for t, ys, xs in ar.tile_slices(W, H):
        want = inside if mask.reshape(-1)[t] else outside
        for g, w, label in zip(got, want, ("accum", "normal", "position")):
            d = int((bits(g[ys, xs]) != bits(w[ys, xs])).sum())
            if d:
                wrong.append((t, label, d))
    assert not wrong, f"{what}: (tile, map, channels differing) {wrong}"


ONE = {capi.DEBUG_SAMPLE_GROUPS: 1}  # a small frame would otherwise split its samples into groups by itself
GROUPS = {capi.DEBUG_SAMPLE_GROUPS: 3}  # the stage and sail_accum_kernel
FORMS = {
    "cornell": ("C1", 4, ONE),
    "cornell_groups": ("C1", 4, GROUPS),
    "cornell_ns4": ("C1", 4, {capi.DEBUG_JIT_NS: 4, **ONE}),
    "cornell_ns16": ("C1", 4, {capi.DEBUG_JIT_NS: 16, **ONE}),
    "cornell_ns16_groups": ("C1", 4, {capi.DEBUG_JIT_NS: 16, **GROUPS}),  # what a masked launch of few tiles picks at 1080p
    "cornell_ns4_groups": ("C1", 4, {capi.DEBUG_JIT_NS: 4, **GROUPS}),
    "cornell_values": ("C1", 4, {capi.DEBUG_JIT_VALUES_AFTER: 0, **ONE}),
    "cornell_values_groups": ("C1", 4, {capi.DEBUG_JIT_VALUES_AFTER: 0, **GROUPS}),
    "room": ("C3", 4, ONE),
    "room_groups": ("C3", 4, GROUPS),  # the room form's first group accumulates at home
    "cull": ("C4", 3, ONE),  # 67 primitives: the pre-cull form
    "cull_groups": ("C4", 3, GROUPS),
    "wavefront": ("C4", 3, {capi.DEBUG_WAVEFRONT: 1}),
    "precompiled_cornell": ("C1", 4, {capi.DEBUG_JIT: 0, **ONE}),
    "precompiled_cornell_groups": ("C1", 4, {capi.DEBUG_JIT: 0, **GROUPS}),
    "precompiled_room": ("C3", 4, {capi.DEBUG_JIT: 0, **ONE}),
    "precompiled_room_groups": ("C3", 4, {capi.DEBUG_JIT: 0, **GROUPS}),
    "precompiled_cull": ("C4", 3, {capi.DEBUG_JIT: 0, **ONE}),
    "precompiled_generic": ("ALL", 4, {capi.DEBUG_JIT: 0, **ONE}),
}


# ---- 1. explicit masks, every kernel form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_explicit_masks(gpu, fixtures, form):
    """K samples unmasked, the mask, K more: active tiles hold the uniform 2K-sample frame, the others still the K-sample
    one; and from a fresh accumulator: the K-sample frame and zeros. An empty mask launches nothing and advances the sample
    index; an all-ones mask is the uniform frame through the table path."""
    name, B, dbg = FORMS[form]
    sc = fixtures["scenes"][name]
    for W, H in SIZES:
        zero, first, both = uniform(fixtures, name, W, H, B)
        ctx = capi.Context(W, H, flags=capi.FLAG_AOV, debug=dbg)
        try:
            ctx.set_scene_dict(sc)
            ctx.kernel_ready(-1)
            for label, mask in masks_for(W, H).items():
                what = f"{form} {W}x{H} {label}"
                ctx.reset()                                  # also removes the mask of the round before
                assert ctx.get_active_tiles().all()
                ctx.set_active_tiles(mask)
                assert np.array_equal(ctx.get_active_tiles(), mask)
                launches = ctx.stats().launches
                render(ctx, sc, 0, K, B)
                st = ctx.stats()
                assert st.samples == K
                assert st.nominal_segments == int(ar.tile_pixels(W, H)[mask != 0].sum()) * K * B, what
                assert (st.launches == launches) == (not mask.any()), what
                check_tiles(frame(ctx), mask, first, zero, what + " from zero")
                ctx.reset()
                render(ctx, sc, 0, K, B)
                ctx.set_active_tiles(mask)
                render(ctx, sc, K, K, B)
                assert ctx.stats().samples == 2 * K
                check_tiles(frame(ctx), mask, both, first, what + " after an unmasked render")
            name_ran = ctx.kernel_name()
            print(form, W, H, name_ran)
            if dbg.get(capi.DEBUG_SAMPLE_GROUPS, 0) > 1:
                assert "grouped" in name_ran, name_ran
            if dbg.get(capi.DEBUG_JIT, 1) == 0:
                assert "jit" not in name_ran, name_ran
        finally:
            ctx.close()


# ---- 2. the driver -----------------------------------------------------------------------------------------------------------------
LOOKS = [4, 8, 16, 32]  # sail_plan_until(4, 32)
DRIVER = {"C1": ("C1", 200, 136, 4), "AREA": ("AREA", 200, 136, 4)}  # 4 x 3 tiles, ragged right and top
_RUNS = {}


def uniform_run(fixtures, case):
    """one uniform context rendered look by look: per look the frame, and from the second look on the estimate against the
    look before (tile_err and per-pixel maps), with the mark moved every look"""
    if case not in _RUNS:
        name, W, H, B = DRIVER[case]
        sc = fixtures["scenes"][name]
        assert [capi.plan_until(k, 4, 32) for k in [0] + LOOKS[:-1]] == LOOKS
        ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
        try:
            ctx.set_scene_dict(sc)
            frames, tile_err, pixel_err, k = [], [None], [None], 0
            for j, kj in enumerate(LOOKS):
                render(ctx, sc, k, kj - k, B)
                k = kj
                frames.append(frame(ctx))
                if j == 0:
                    ctx.noise_mark()
                else:
                    est = ctx.noise_estimate(tiles=True, pixels=True, remark=True)
                    assert est["nonfinite"] == 0
                    tile_err.append(est["tile_err"])
                    pixel_err.append(est["pixel_err"])
            _RUNS[case] = (frames, tile_err, pixel_err)
        finally:
            ctx.close()
    return _RUNS[case]


def both_ways(frozen, last):
    return (frozen < last).any() and (frozen == last).any()


def pick_target(W, H, tile_err, dilate):
    """The midpoint of two adjacent distinct per-tile errors of the second look, the pair nearest the median for which
    (by the numpy rule, on the uniform run's maps) a tile freezes before the last look and another stays active to it."""
    v = np.unique(ar.e64(tile_err[1], W, H).ravel())
    mids = [(float(v[i]) + float(v[i + 1])) / 2 for i in range(len(v) - 1)]
    order = sorted(range(len(mids)), key=lambda i: abs(i - (len(mids) - 1) / 2))
    for i in order:
        frozen, _, _ = ar.freeze_schedule(W, H, LOOKS, tile_err, mids[i], dilate)
        if both_ways(frozen, len(LOOKS) - 1):
            return mids[i]
    return None


def adaptive(fixtures, case, target, dilate, debug=None):
    name, W, H, B = DRIVER[case]
    sc = fixtures["scenes"][name]
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV, debug=debug)
    ctx.set_scene_dict(sc)
    res = ctx.render_adaptive(np.array(sc["mvp_rowmajor"]), sc["eye"], B, target=target, min_spp=4, max_spp=32, dilate=dilate)
    return ctx, res


def check_driver(ctx, res, case, fixtures, target, dilate):
    """the adaptive frame against the uniform run and the numpy schedule; returns the composed (S, P, N, X)"""
    name, W, H, B = DRIVER[case]
    frames, tile_err, pixel_err = uniform_run(fixtures, case)
    frozen, active, pixel_samples = ar.freeze_schedule(W, H, LOOKS, tile_err, target, dilate)
    last = int(frozen.max())
    print(f"{case} target {target} dilate {dilate}: freezing looks\n{frozen}\nactive\n{active}\ntile_samples\n{res['tile_samples']}")
    assert np.array_equal(res["tile_samples"], np.asarray(LOOKS)[frozen])
    assert np.array_equal(ctx.get_active_tiles(), active)
    assert res["active_tiles"] == int(active.sum()) and res["converged"] == (not active.any())
    assert res["pixel_samples"] == pixel_samples and res["frame_pixel_samples"] == W * H * LOOKS[last]
    assert [s["k"] for s in res["history"]] == LOOKS[:last + 1] and res["history"][0]["mean"] == math.inf
    assert ctx.stats().samples == LOOKS[last] and ctx.stats().nominal_segments == pixel_samples * B
    got = frame(ctx)
    err = ctx.noise_estimate(pixels=True)["pixel_err"]  # of each tile's own (P, S) pair
    S, P = np.zeros_like(got[0]), np.zeros_like(got[0])
    wrong = []
    for t, ys, xs in ar.tile_slices(W, H):
        j = int(frozen.reshape(-1)[t])
        for g, w, label in zip(got, frames[j], ("accum", "normal", "position")):
            if (bits(g[ys, xs]) != bits(w[ys, xs])).any():
                wrong.append((t, label))
        if (bits(err[ys, xs]) != bits(pixel_err[j][ys, xs])).any():
            wrong.append((t, "pixel_err"))
        S[ys, xs], P[ys, xs] = frames[j][0][ys, xs], frames[j - 1][0][ys, xs]
    assert not wrong, f"(tile, map) differing from the uniform frame at the tile's freezing look: {wrong}"
    return S, P, got[1], got[2]


@pytest.mark.parametrize("case,dilate", [("C1", 0), ("C1", 1), ("AREA", 0)])
def test_driver_freezes_tiles_at_their_looks(gpu, fixtures, case, dilate):
    name, W, H, B = DRIVER[case]
    _, tile_err, _ = uniform_run(fixtures, case)
    target = pick_target(W, H, tile_err, dilate)
    assert target is not None, "no target freezes one tile early and keeps another to max_spp: pick another fixture"
    ctx, res = adaptive(fixtures, case, target, dilate)
    try:
        check_driver(ctx, res, case, fixtures, target, dilate)
        assert res["pixel_samples"] < res["frame_pixel_samples"]
    finally:
        ctx.close()


def test_driver_infinite_target_freezes_everything_at_the_second_look(gpu, fixtures):
    ctx, res = adaptive(fixtures, "C1", math.inf, 1)
    try:
        assert res["converged"] and res["k"] == 8 and res["k_mark"] == 4 and (res["tile_samples"] == 8).all()
        check_driver(ctx, res, "C1", fixtures, math.inf, 1)
    finally:
        ctx.close()


def test_driver_zero_target_freezes_only_error_free_tiles(gpu, fixtures):
    """C1 at this size has a tile whose second look reads no error at all; only such tiles freeze at target 0"""
    name, W, H, B = DRIVER["C1"]
    _, tile_err, _ = uniform_run(fixtures, "C1")
    frozen, active, _ = ar.freeze_schedule(W, H, LOOKS, tile_err, 0.0, 0)
    assert both_ways(frozen, len(LOOKS) - 1), "the fixture has no error-free tile any more"
    ctx, res = adaptive(fixtures, "C1", 0.0, 0)
    try:
        assert not res["converged"] and res["k"] == 32
        check_driver(ctx, res, "C1", fixtures, 0.0, 0)
    finally:
        ctx.close()


def test_driver_resumes_under_its_mask(gpu, fixtures):
    """a second call at max_spp renders nothing and keeps everything; rejected arguments render nothing"""
    name, W, H, B = DRIVER["C1"]
    sc = fixtures["scenes"][name]
    _, tile_err, _ = uniform_run(fixtures, "C1")
    target = pick_target(W, H, tile_err, 0)
    ctx, res = adaptive(fixtures, "C1", target, 0)
    try:
        before, mask = frame(ctx), ctx.get_active_tiles()
        mvp = np.array(sc["mvp_rowmajor"])
        again = ctx.render_adaptive(mvp, sc["eye"], B, target=target, min_spp=4, max_spp=32, dilate=0)
        assert again["history"] == [] and again["pixel_samples"] == 0 and again["frame_pixel_samples"] == 0
        assert np.array_equal(again["tile_samples"], res["tile_samples"]) and np.array_equal(ctx.get_active_tiles(), mask)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame(ctx), before))
        for kw in ({"target": math.nan}, {"min_spp": 0}, {"min_spp": 8, "max_spp": 4}, {"dilate": 2}):
            with pytest.raises(capi.SailError, match="-1"):
                ctx.render_adaptive(mvp, sc["eye"], B, **{"target": 1.0, "min_spp": 4, "max_spp": 64, "dilate": 1, **kw})
        assert ctx.stats().samples == 32
        # more samples under the mask: only its tiles move, frozen ones stay frozen
        more = ctx.render_adaptive(mvp, sc["eye"], B, target=0.0, min_spp=4, max_spp=40, dilate=0)
        assert [s["k"] for s in more["history"]] == [40] and more["pixel_samples"] == int(ar.tile_pixels(W, H)[mask != 0].sum()) * 8
        after = frame(ctx)
        for t, ys, xs in ar.tile_slices(W, H):
            same = all(np.array_equal(bits(a[ys, xs]), bits(b[ys, xs])) for a, b in zip(after, before))
            assert same == (not mask.reshape(-1)[t]), t
        assert (after[0][..., 3] == np.repeat(np.repeat(more["tile_samples"], 64, 0), 64, 1)[:H, :W]).all()
    finally:
        ctx.close()


# ---- 3. downstream: heterogeneous counts pass through the denoiser ----------------------------------------------------------
def test_denoise_after_an_adaptive_run(gpu, fixtures):
    name, W, H, B = DRIVER["C1"]
    _, tile_err, _ = uniform_run(fixtures, "C1")
    target = pick_target(W, H, tile_err, 0)
    ctx, res = adaptive(fixtures, "C1", target, 0)
    try:
        S, P, N, X = check_driver(ctx, res, "C1", fixtures, target, 0)
        assert len(np.unique(S[..., 3])) > 1, "the frame's tiles hold one sample count: nothing heterogeneous to pass through"
        c, v, bad = ref_denoise(S, P, N, X)
        out = ctx.denoise(None, want_var=True)
        assert out["nonfinite"] == bad
        same_bits(out, c, v, "denoise after render_adaptive")
    finally:
        ctx.close()


def test_temporal_resolve_after_an_adaptive_run(gpu, fixtures):
    """a history for the frame's own view (every pixel that hits finds it), then the resolve: the formula of
    tests/temporal_ref.py fed with the adaptive S, whose tiles hold different counts, and the R the context read back"""
    import temporal_ref as tr
    name, W, H, B = DRIVER["C1"]
    sc = fixtures["scenes"][name]
    mvp, eye = np.array(sc["mvp_rowmajor"], np.float64), np.array(sc["eye"], F)
    _, tile_err, _ = uniform_run(fixtures, "C1")
    ctx, res = adaptive(fixtures, "C1", pick_target(W, H, tile_err, 0), 0)
    try:
        S = ctx.read_accum()
        assert len(np.unique(S[..., 3])) > 1
        g = ctx.gbuffer(mvp, eye)
        G = np.concatenate([g["xyz"], g["id"].astype(F)[..., None]], axis=-1).astype(F)
        rng = np.random.default_rng(7)
        hist = np.zeros((H, W, 4), F)
        hist[..., :3] = rng.random((H, W, 3), dtype=F) * F(2)
        hist[..., 3] = rng.integers(1, 41, (H, W)).astype(F)
        ctx.temporal_load_history(hist, G, mvp, eye)
        info = ctx.temporal_begin(mvp, eye)
        R = ctx.temporal_read(capi.TEMPORAL_R)
        assert info["history_pixels"] > W * H // 2
        assert np.array_equal(bits(ctx.read_accum()), bits(S)), "the begin of a view changed the frame"
        for cap in (8.0, 32.0):
            out = ctx.temporal_resolve({"cap": cap, "display": capi.FILTER_COLOR, "gamma_c": 1.0})
            want, nhist, bad = tr.ref_resolve(S, R, cap=cap)
            assert not np.isnan(want).any() and bad == 0
            assert np.array_equal(bits(out["rgba"]), bits(want)) and out["history_pixels"] == nhist
    finally:
        ctx.close()


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------------
def test_clearing_calls_and_refusals(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H, B = 160, 96, 3
    mask = masks_for(W, H)["checker"]
    rows = capi._f32(sc["objects"])
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        render(ctx, sc, 0, 2, B)
        saved = ctx.save()
        clearing = {
            "sail_reset": ctx.reset,
            "sail_set_scene": lambda: ctx.set_scene_dict(sc),
            "sail_update_objects": lambda: ctx._check(ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]), "update"),
            "sail_move_objects": lambda: ctx._check(ctx.lib.sail_move_objects(ctx.h, capi._ptr(rows), sc["n"], None, 0.0), "move"),
            "sail_set_accum_mode": lambda: ctx.set_accum_mode(capi.ACCUM_SUM),
            "sail_set_partition": lambda: ctx.set_partition(0, 1, capi.PART_TILES),
            "sail_load_accum": lambda: ctx.load(saved),
        }
        for what, call in clearing.items():
            ctx.set_active_tiles(mask)
            assert np.array_equal(ctx.get_active_tiles(), mask), what
            call()
            assert ctx.get_active_tiles().all(), f"{what} kept the mask"
        # a wrong count: SAIL_E_INVALID, and the mask that is set stays
        ctx.set_active_tiles(mask)
        for count in (0, mask.size - 1, mask.size + 1):
            a = np.ones(mask.size + 1, np.uint8)
            assert ctx.lib.sail_set_active_tiles(ctx.h, capi._ptr(a, capi.ctypes.c_uint8), count) == -1
        assert ctx.lib.sail_set_active_tiles(ctx.h, None, mask.size) == -1
        assert ctx.lib.sail_get_active_tiles(ctx.h, capi._ptr(a, capi.ctypes.c_uint8), mask.size + 1, None) == -1
        assert np.array_equal(ctx.get_active_tiles(), mask)
        ctx.set_active_tiles(None)
        assert ctx.get_active_tiles().all()
        # the modes without a per-pixel count: SAIL_E_STATE from the mask and from the driver, nothing rendered
        for mode in (capi.ACCUM_MIX, capi.ACCUM_COMPAT8):
            ctx.set_accum_mode(mode)
            with pytest.raises(capi.SailError, match="-4"):
                ctx.set_active_tiles(mask)
            with pytest.raises(capi.SailError, match="-4"):
                ctx.render_adaptive(np.array(sc["mvp_rowmajor"]), sc["eye"], B, target=1.0, min_spp=4, max_spp=8)
            assert ctx.get_active_tiles().all() and ctx.stats().samples == 0
    finally:
        ctx.close()


def test_masked_remark_leaves_frozen_tiles_their_mark(gpu, fixtures):
    """sail_noise_estimate's remark under a mask: the estimate reads no mask, the remark store writes P in active tiles
    only. Uniform run: mark at 2, looks at 4 (error map E1, remark) and 8 (E2). Masked run: the same up to 4, the mask
    before the remarking estimate, then 4 masked samples: the next estimate reads E2 in active tiles and still E1 in
    frozen ones (a remark that had written their P would leave n == h there, error 0)."""
    sc = fixtures["scenes"]["C1"]
    W, H, B = 160, 96, 3
    mask = masks_for(W, H)["checker"]

    def run(masked):
        ctx = capi.Context(W, H)
        try:
            ctx.set_scene_dict(sc)
            render(ctx, sc, 0, 2, B)
            ctx.noise_mark()
            render(ctx, sc, 2, 2, B)
            if masked:
                ctx.set_active_tiles(mask)
            e1 = ctx.noise_estimate(pixels=True, remark=True)["pixel_err"]
            render(ctx, sc, 4, 4, B)
            return e1, ctx.noise_estimate(pixels=True)["pixel_err"]
        finally:
            ctx.close()
    u1, u2 = run(False)
    m1, m2 = run(True)
    assert np.array_equal(bits(m1), bits(u1))
    for t, ys, xs in ar.tile_slices(W, H):
        want = u2 if mask.reshape(-1)[t] else u1
        assert np.array_equal(bits(m2[ys, xs]), bits(want[ys, xs])), (t, int(mask.reshape(-1)[t]))
        assert u1[ys, xs].any() and not np.array_equal(bits(u1[ys, xs]), bits(u2[ys, xs])), "the tile cannot tell the marks apart"


def test_a_rank_without_an_active_tile_launches_nothing(gpu, fixtures):
    """one rank of a three-rank tile partition (tiles 1 and 4 of 160 x 96), as each process of a sail_comm_init group runs
    it: under a mask that holds none of its tiles it launches nothing, its frame stays, and the sample index advances"""
    sc = fixtures["scenes"]["C3"]
    W, H, B = 160, 96, 4
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        ctx.set_scene_dict(sc)
        ctx.set_partition(1, 3, capi.PART_TILES)
        render(ctx, sc, 0, K, B)
        before, st0 = frame(ctx), ctx.stats()
        ctx.set_active_tiles(np.array([[1, 0, 1], [1, 0, 1]], np.uint8))
        render(ctx, sc, K, K, B)
        st = ctx.stats()
        assert (st.launches, st.nominal_segments, st.kernel_ms) == (st0.launches, st0.nominal_segments, st0.kernel_ms)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame(ctx), before))
        ctx.set_active_tiles(np.array([[1, 1, 0], [0, 0, 1]], np.uint8))   # tile 1 of its two
        render(ctx, sc, 2 * K, K, B)
        st = ctx.stats()
        assert st.launches > st0.launches and st.nominal_segments - st0.nominal_segments == 64 * 64 * K * B
    finally:
        ctx.close()


def test_half_loaded_checkpoint_refuses_the_mask(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H, B = 160, 96, 3
    mask = masks_for(W, H)["checker"]
    ctx = capi.Context(W, H, devices=[0, 0])
    try:
        ctx.set_scene_dict(sc)
        ctx.set_active_tiles(mask)
        a = np.ones((H, W, 4), F)
        half = capi.plan_keep(W, H, 0, 2, capi.PART_TILES, a)
        assert ctx.lib.sail_load_accum(ctx.h, 0, capi._ptr(half), 5) == 0
        with pytest.raises(capi.SailError, match="parts not loaded"):
            ctx.set_active_tiles(mask)
        with pytest.raises(capi.SailError, match="parts not loaded"):
            ctx.render_adaptive(np.array(sc["mvp_rowmajor"]), sc["eye"], B, target=1.0, min_spp=4, max_spp=8)
        assert ctx.get_active_tiles().all(), "the load of a part keeps the mask on some device"
        ctx.reset()                                            # abandons the half-loaded checkpoint
        ctx.set_active_tiles(mask)
        assert np.array_equal(ctx.get_active_tiles(), mask)
    finally:
        ctx.close()


# ---- 5. multi-device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,mode,dbg", [([0, 0, 0], capi.PART_TILES, None), ([0, 0], capi.PART_SAMPLES, None),
                                              ([0], capi.PART_TILES, {capi.DEBUG_FORCE_RCCL: 1})],
                         ids=["tiles3", "samples2", "rccl1"])
def test_multi_device_masks(gpu, fixtures, devices, mode, dbg):
    """the masked frame of a partitioned context against the uniform frames, as tests/test_gpu_multi.py compares each
    partition: tile partitions bit for bit, AOVs included; a sample partition of two to the rounding of the ranks' sum.
    Mask `own0` leaves ranks 1 and 2 of the three-device tile partition without an active tile: they launch nothing (the
    nominal segments are the active pixels' alone)."""
    name, W, H, B = "C3", 160, 96, 4
    sc = fixtures["scenes"][name]
    zero, first, both = uniform(fixtures, name, W, H, B)
    masks = dict(masks_for(W, H), own0=np.array([[1, 0, 0], [1, 0, 0]], np.uint8))
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV, devices=devices)
    try:
        for opt, val in (dbg or {}).items():
            ctx.set_debug(opt, val)
        ctx.set_scene_dict(sc)
        ctx.set_partition(0, 1, mode)
        exact = mode == capi.PART_TILES or len(devices) == 1
        for label, mask in masks.items():
            ctx.reset()
            render(ctx, sc, 0, K, B)
            ctx.set_active_tiles(mask)
            assert np.array_equal(ctx.get_active_tiles(), mask)
            seg = ctx.stats().nominal_segments
            render(ctx, sc, K, K, B)
            assert ctx.stats().nominal_segments - seg == int(ar.tile_pixels(W, H)[mask != 0].sum()) * K * B, label
            got = frame(ctx)
            if exact:
                check_tiles(got, mask, both, first, f"{devices} {label}")
            else:
                for t, ys, xs in ar.tile_slices(W, H):
                    want = both if mask.reshape(-1)[t] else first
                    assert np.allclose(got[0][ys, xs], want[0][ys, xs], rtol=1e-5, atol=1e-5), (label, t)
                    assert (got[0][ys, xs, 3] == want[0][ys, xs, 3]).all(), (label, t)
    finally:
        ctx.close()
