"""The albedo map of a view and the albedo-demodulated denoiser and temporal filter (sail_albedo_kernel behind sail_albedo;
the DEMOD instances of the prepare kernels and the remodulating last a-trous pass behind sail_denoise_albedo and
sail_temporal_filter_albedo). Needs a GPU.

The references are tests/albedo_ref.py's: the map from the CPU oracle's first hit (tests/first_hit_oracle.cpp), summed and
divided in numpy float32 in the header's order; the filters from the plain numpy references over the demodulated inputs.
Every operation is an IEEE f32 one, so the device must equal them bit for bit: raw uint32 bits are compared. The quality
test compares with a separate, far longer render over other sample indices, never with the code under test."""
import numpy as np
import pytest

import albedo_ref as ar
import temporal_ref as tr
import test_gpu_denoise as dn
import test_gpu_temporal_filter as tft
from sail_amd import capi
from temporal_ref import bits

pytestmark = pytest.mark.gpu

F = np.float32
AMIN = capi.ALBEDO_AMIN_DEFAULT
SIZES = dn.SIZES                                  # (1, 1), (16, 16), (33, 17), (150, 70)
OUT, M_OUT = capi.TEMPORAL_OUT, capi.TEMPORAL_M_OUT


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def scene_view(sc):
    return np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F)


def hostile_map(A, amin=AMIN):
    """A with channels that are 0, -0, below, at and just above amin, negative, NaN, +Inf and 2^20 spread over its first
    pixels, and a channel below amin in the last pixel (33x17: the single pixel of the ragged corner tile)"""
    A = np.array(A, F)
    flat = A.reshape(-1, 4)
    a = F(amin)
    vals = [0.0, -0.0, a * F(0.5), a, np.nextafter(a, F(1)), -0.5, np.nan, np.inf, 2.0 ** 20]
    for j, v in enumerate(vals):
        flat[(j * 7) % len(flat), j % 3] = v
    flat[-1, 1] = a * F(0.5)
    if len(flat) > 1:
        flat[-1, 2] = np.nan
    return A


# ---- 1. the map against the oracle shim ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["C1", "C3", "C4", "ALL", "BILERP", "AREA"])
def test_map_equals_the_oracle(gpu, fixtures, name, W, H):
    sc = fixtures["scenes"][name]
    mvp, eye = scene_view(sc)
    ctx = capi.Context(W, H)
    try:
        ctx.set_scene_dict(sc)
        for g in (1, 2, 4):
            want, hit, partial = ar.ref_albedo(sc, mvp, eye, W, H, g)
            got = ctx.albedo(mvp, eye, grid=g)
            print(f"map {name} {W}x{H} grid {g}: hit {got['hit_pixels']} (ref {hit}), partial {got['partial_pixels']} (ref "
                  f"{partial}), channels differing {differing(got['rgba'], want)}")
            assert not np.isnan(want).any()
            assert same(got["rgba"], want) and same(ctx.albedo_read(), want)
            assert (got["hit_pixels"], got["partial_pixels"], got["grid"]) == (hit, partial, g)
            if g == 1:
                assert np.array_equal(got["rgba"][..., 3] > 0, ctx.gbuffer(mvp, eye)["id"] >= 0)
    finally:
        ctx.close()


def test_map_of_a_silhouette_and_of_an_empty_scene(gpu, fixtures):
    """N1S: one sphere, most pixels miss and the silhouette is partial. N0: no rows, every pixel (1, 1, 1, 0)"""
    W, H = 33, 17
    sc = fixtures["scenes"]["N1S"]
    mvp, eye = scene_view(sc)
    ctx = capi.Context(W, H)
    try:
        ctx.set_scene_dict(sc)
        for g in (1, 2, 4):
            want, hit, partial = ar.ref_albedo(sc, mvp, eye, W, H, g)
            got = ctx.albedo(mvp, eye, grid=g)
            assert same(got["rgba"], want) and (got["hit_pixels"], got["partial_pixels"]) == (hit, partial)
            assert 0 < hit < W * H // 2 and (g == 1 or partial > 0)
            miss = want[..., 3] == 0
            assert same(got["rgba"][miss], np.broadcast_to(np.array([1, 1, 1, 0], F), got["rgba"][miss].shape))
            if g == 1:
                assert np.array_equal(got["rgba"][..., 3] > 0, ctx.gbuffer(mvp, eye)["id"] >= 0)
        empty = fixtures["scenes"]["N0"]
        ctx.set_scene_dict(empty)
        got = ctx.albedo(*scene_view(empty), grid=2)
        assert (got["hit_pixels"], got["partial_pixels"]) == (0, 0)
        assert same(got["rgba"], np.broadcast_to(np.array([1, 1, 1, 0], F), (H, W, 4)))
    finally:
        ctx.close()


# ---- 2. sail_denoise_albedo against the numpy reference -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_inputs(gpu, fixtures):
    """tests/test_gpu_denoise.py's C3 inputs (3 bounces, 8 spp marked after 3) per size and accumulation mode: the context
    (kept open), what it holds, and its own map of the fixture view at grid 2"""
    made = {}

    def get(W, H, mix=False):
        if (W, H, mix) not in made:
            sc = fixtures["scenes"]["C3"]
            ctx = dn.aov_context(sc, W, H)
            if mix:
                ctx.set_accum_mode(capi.ACCUM_MIX)
            maps = dn.marked_render(ctx, sc, 3, 3, 8)
            view = scene_view(sc)
            A = ctx.albedo(*view, grid=2)["rgba"]
            for a in (*maps, A):
                a.setflags(write=False)
            made[(W, H, mix)] = (ctx, maps, A, view)
        return made[(W, H, mix)]
    yield get
    for ctx, *_ in made.values():
        ctx.close()


@pytest.mark.parametrize("mix", [False, True], ids=["sum", "mix"])
@pytest.mark.parametrize("W,H", SIZES)
def test_denoise_matches_the_f32_reference(c3_inputs, W, H, mix):
    ctx, (S, P, N, X), own, view = c3_inputs(W, H, mix)
    try:
        for what, A in (("own", own), ("hostile", hostile_map(own))):
            if what == "hostile":
                ctx.albedo_load(A, *view)
            assert same(ctx.albedo_read(), A)
            for iterations in (1, 4):
                for params in ({}, dn.OTHER):
                    p = dict(params, iterations=iterations)
                    c, v, bad = ar.ref_denoise_albedo(S, P, N, X, A, AMIN, mix=mix, k=8, h=3, **p)
                    out = ctx.denoise(p, want_var=True, albedo=AMIN)
                    dc, dv = differing(out["rgba"][..., :3], c), differing(out["var"], v)
                    print(f"denoise_albedo C3 {W}x{H} mix {mix} {what} map, it {iterations} {params}: colour channels "
                          f"differing {dc}, variance texels differing {dv}")
                    assert not np.isnan(c).any() and not np.isnan(v).any()
                    assert dc == 0 and dv == 0
                    assert (bits(out["rgba"][..., 3]) == bits(F(1))).all()
                    assert (out["k"], out["k_mark"], out["iterations"], out["nonfinite"]) == (8, 3, iterations, bad)
        if W * H > 1:
            plain = ctx.denoise(want_var=True)
            assert not same(plain["rgba"], ctx.denoise(want_var=True, albedo=AMIN)["rgba"])   # the map does something
    finally:
        ctx.albedo_load(own, *view)


@pytest.mark.parametrize("mix", [False, True], ids=["sum", "mix"])
def test_denoise_of_chosen_accumulators(gpu, fixtures, mix):
    """tests/test_gpu_denoise.py's recipe (h = 0, n = h, NaN, Inf, -0, the 2^40 tile) at 33x17, with the device's map"""
    sc = fixtures["scenes"]["C3"]
    W, H = 33, 17
    Pa, Sa = dn.make_chain(W, H, seed=W * 91 + H, mix=mix)
    ctx = dn.aov_context(sc, W, H)
    try:
        if mix:
            ctx.set_accum_mode(capi.ACCUM_MIX)
        dn.render(ctx, sc, 0, 2, 3)
        ctx.load({"k": 3, "parts": [Pa]})
        ctx.noise_mark()
        ctx.load({"k": 7, "parts": [Sa]})
        _, N, X = ctx.readback(aov=True)
        A = ctx.albedo(*scene_view(sc), grid=2)["rgba"]
        for p in ({}, dict(dn.OTHER, iterations=6)):
            out = ctx.denoise(p, want_var=True, albedo=AMIN)
            c, v, bad = ar.ref_denoise_albedo(Sa, Pa, N, X, A, AMIN, mix=mix, k=7, h=3, **p)
            ok = (bits(out["rgba"][..., :3]) == bits(c)) | (np.isnan(out["rgba"][..., :3]) & np.isnan(c))
            ok_v = (bits(out["var"]) == bits(v)) | (np.isnan(out["var"]) & np.isnan(v))
            print(f"chosen {W}x{H} mix {mix} {p}: nonfinite {out['nonfinite']} (ref {bad}), differing "
                  f"{int((~ok).sum())} colour channels, {int((~ok_v).sum())} variance texels")
            assert ok.all() and ok_v.all()
            assert out["nonfinite"] == bad == 2
    finally:
        ctx.close()


# ---- 3. sail_temporal_filter_albedo against the numpy reference -----------------------------------------------------------------
@pytest.fixture(scope="module")
def filter_inputs(gpu, fixtures):
    """tests/test_gpu_temporal_filter.py's setup: C1 per size, a loaded history with chosen moments seen from A, one sample
    at B, that accumulator loaded again with a NaN and an Inf texel, a second sample, resolved; and the map of B at grid 2"""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            sc = fixtures["scenes"]["C1"]
            va, vb = (f() for f in tft.VIEWS["C1"])
            hist, gprev, mom = tft.chosen_history(tft.ref_g(fixtures, "C1", W, H, "A", va), seed=W * 5 + H)
            GB = tft.ref_g(fixtures, "C1", W, H, "B", vb)
            free = np.argwhere((tr.ref_reproject(GB, gprev, hist, va[0], va[1])[0][..., 3] == 0) & (GB[..., 3] >= 0))
            ctx = tft.context(sc, W, H)
            ctx.temporal_load_history(hist, gprev, va[0], va[1])
            ctx.temporal_load_moments(mom)
            ctx.temporal_begin(vb[0], vb[1])
            tft.render(ctx, vb, 0, 1, 3)
            S = ctx.read_accum()
            if len(free) >= 2:
                S[free[0][0], free[0][1], 1] = np.nan
                S[free[len(free) // 2][0], free[len(free) // 2][1], 0] = np.inf
                ctx.load({"k": 1, "parts": [S]})
                tft.render(ctx, vb, 1, 1, 3)
            ctx.temporal_resolve()
            _, N, X = ctx.readback(aov=True)
            maps = dict(Out=ctx.temporal_read(OUT), Mout=ctx.temporal_read_moments(M_OUT), S=ctx.read_accum(), N=N, X=X,
                        A=ctx.albedo(vb[0], vb[1], grid=2)["rgba"])
            for a in maps.values():
                a.setflags(write=False)
            maps["k"] = ctx.save()["k"]
            maps["view"] = vb
            made[(W, H)] = (ctx, maps)
        return made[(W, H)]
    yield get
    for ctx, _ in made.values():
        ctx.close()


TF_CASES = {"defaults": {}, "it1": {"iterations": 1}, "hist1": {"min_hist": 1.0}, "all-spatial": {"min_hist": 1000.0},
            "other-sigmas": {"sigma_l": 1.0, "sigma_x": 0.05}}


@pytest.mark.parametrize("W,H", tft.SIZES)
def test_temporal_filter_matches_the_f32_reference(filter_inputs, W, H):
    ctx, m = filter_inputs(W, H)
    try:
        for what, A in (("own", m["A"]), ("hostile", hostile_map(m["A"]))):
            ctx.albedo_load(A, *m["view"])
            for case, p in TF_CASES.items():
                c, v, counts = ar.ref_filter_albedo(m["Out"], m["Mout"], m["S"], m["N"], m["X"], A, AMIN, k=m["k"], **p)
                out = ctx.temporal_filter(p, want_var=True, want_u8=True, albedo=AMIN)
                nan_c, nan_v = np.isnan(c), np.isnan(v)
                dc = int((bits(out["rgba"][..., :3]) != bits(c))[~nan_c].sum())
                dv = int((bits(out["var"]) != bits(v))[~nan_v].sum())
                print(f"filter_albedo {W}x{H} {what} map {case}: temporal {out['temporal_pixels']} (ref {counts['temporal']}), "
                      f"nonfinite {out['nonfinite']} (ref {counts['nonfinite']}); colour channels differing {dc}, variance "
                      f"texels differing {dv}")
                assert dc == 0 and dv == 0
                assert np.array_equal(np.isnan(out["rgba"][..., :3]), nan_c) and np.array_equal(np.isnan(out["var"]), nan_v)
                assert int(nan_c.any(axis=-1).sum()) <= 1 and not nan_v.any()
                assert (out["temporal_pixels"], out["spatial_pixels"], out["nonfinite"]) == \
                    (counts["temporal"], counts["spatial"], counts["nonfinite"])
                u8 = tr.quantise(np.where(nan_c, F(0), c))
                ok = ~nan_c.any(axis=-1)
                assert np.array_equal(out["u8"][..., :3][ok], u8[ok]) and (out["u8"][..., 3] == 255).all()
                if W * H >= 33 * 18:
                    assert counts["nonfinite"] == 2
                    if case == "all-spatial":
                        assert counts["temporal"] == 0
                    else:
                        assert 0 < counts["temporal"] < W * H          # pixels on both sides of min_hist
        if W * H >= 33 * 18:
            assert not same(np.nan_to_num(ctx.temporal_filter()["rgba"]),
                            np.nan_to_num(ctx.temporal_filter(albedo=AMIN)["rgba"]))
    finally:
        ctx.albedo_load(m["A"], *m["view"])


# ---- 4. a map of ones ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, 4.0])
def test_ones_map_gives_the_plain_calls(c3_inputs, filter_inputs, w):
    for W, H in ((33, 17), (150, 70)):
        ctx, _, own, view = c3_inputs(W, H)
        ones = np.ones((H, W, 4), F)
        ones[..., 3] = w
        try:
            ctx.albedo_load(ones, *view)
            for p in (None, dict(dn.OTHER, iterations=2, display=capi.FILTER_GAMMA)):
                a = ctx.denoise(p, want_var=True, want_u8=True)
                b = ctx.denoise(p, want_var=True, want_u8=True, albedo=AMIN)
                assert same(a["rgba"], b["rgba"]) and same(a["var"], b["var"]) and np.array_equal(a["u8"], b["u8"])
                assert a["nonfinite"] == b["nonfinite"]
        finally:
            ctx.albedo_load(own, *view)
    for W, H in tft.SIZES[2:]:
        ctx, m = filter_inputs(W, H)
        ones = np.ones((H, W, 4), F)
        ones[..., 3] = w
        try:
            ctx.albedo_load(ones, *m["view"])
            for p in (None, {"min_hist": 1.0, "iterations": 2, "display": capi.FILTER_TONEMAPPING}):
                a = ctx.temporal_filter(p, want_var=True, want_u8=True)
                b = ctx.temporal_filter(p, want_var=True, want_u8=True, albedo=AMIN)
                assert same(a["rgba"], b["rgba"]) and same(a["var"], b["var"]) and np.array_equal(a["u8"], b["u8"])
                assert (a["temporal_pixels"], a["nonfinite"]) == (b["temporal_pixels"], b["nonfinite"])
        finally:
            ctx.albedo_load(m["A"], *m["view"])


# ---- 5. state rules --------------------------------------------------------------------------------------------------------------
NO_MAP = ": -4: .*no albedo map"


def test_state_rules(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H, B = 16, 16, 3
    va, vb = tr.orbit(0), tr.orbit(3)
    ones = np.ones((H, W, 4), F)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    try:
        with pytest.raises(capi.SailError, match=": -4: .*no scene"):
            ctx.albedo(*va)
        ctx.set_scene_dict(sc)
        ctx.temporal_moments(True)
        for grid in (0, 5, -3):
            with pytest.raises(capi.SailError, match=": -1: .*grid"):
                ctx.albedo(*va, grid=grid)
        with pytest.raises(capi.SailError, match=": -1: .*singular"):
            ctx.albedo(np.zeros(16), va[1])
        with pytest.raises(capi.SailError, match=NO_MAP):
            ctx.albedo_read()
        # the plain calls' own refusals come as they do there: no mark, no sample since the mark, no current view
        tft.render(ctx, va, 0, 2, B)
        with pytest.raises(capi.SailError, match=": -4: .*no mark"):
            ctx.denoise(albedo=AMIN)
        ctx.noise_mark()
        with pytest.raises(capi.SailError, match=": -4: .*no sample since the mark"):
            ctx.denoise(albedo=AMIN)
        tft.render(ctx, va, 2, 2, B)
        with pytest.raises(capi.SailError, match=NO_MAP):
            ctx.denoise(albedo=AMIN)
        with pytest.raises(capi.SailError, match=": -4: .*no current view"):
            ctx.temporal_filter(albedo=AMIN)
        assert ctx.albedo(*va)["grid"] == 2                          # the default grid
        assert ctx.denoise(albedo=AMIN)["k"] == 4
        for amin in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(capi.SailError, match=": -1: .*amin"):
                ctx.denoise(albedo=amin)
            with pytest.raises(capi.SailError, match=": -1: .*amin"):
                ctx.temporal_filter(albedo=amin)
        for bad in ({"iterations": 0}, {"sigma_l": float("nan")}, {"display": capi.FILTER_WINDOW}):
            with pytest.raises(capi.SailError, match=": -1: .*bad parameters"):
                ctx.denoise(bad, albedo=AMIN)
            with pytest.raises(capi.SailError, match=": -1: .*bad parameters"):
                ctx.temporal_filter(bad, albedo=AMIN)

        # the temporal filter wants the map of the current temporal view, bit for bit
        ctx.reset()
        ctx.temporal_begin(*vb)
        tft.render(ctx, vb, 0, 1, B)
        with pytest.raises(capi.SailError, match=": -4: .*not resolved"):
            ctx.temporal_filter(albedo=AMIN)
        ctx.temporal_resolve()
        with pytest.raises(capi.SailError, match=": -4: .*another view"):
            ctx.temporal_filter(albedo=AMIN)                          # the map is va's
        ctx.temporal_filter()                                         # the plain call does not care
        ctx.albedo(*vb)
        assert ctx.temporal_filter(albedo=AMIN)["k"] == 1
        ctx.albedo_load(ones, vb[0], vb[1] + F(1e-6))
        with pytest.raises(capi.SailError, match=": -4: .*another view"):
            ctx.temporal_filter(albedo=AMIN)
        ctx.albedo_load(ones, *vb)
        assert ctx.temporal_filter(albedo=AMIN)["k"] == 1

        # what keeps the map: reset, load_accum, set_accum_mode, set_partition and the temporal calls
        kept = ctx.albedo(*vb)["rgba"]
        for op in (lambda: ctx.reset(), lambda: ctx.load({"k": 2, "parts": [ones]}),
                   lambda: ctx.set_accum_mode(capi.ACCUM_MIX), lambda: ctx.set_accum_mode(capi.ACCUM_SUM),
                   lambda: ctx.set_partition(0, 1, capi.PART_TILES), lambda: ctx.temporal_begin(*va),
                   lambda: ctx.temporal_resolve(), lambda: ctx.temporal_load_history(ones, ones, *va),
                   lambda: ctx.temporal_moments(False), lambda: ctx.temporal_moments(True)):
            op()
            assert same(ctx.albedo_read(), kept)
        # COMPAT8 is refused as in the plain calls
        ctx.reset()
        ctx.temporal_begin(*vb)
        tft.render(ctx, vb, 0, 1, B)
        ctx.noise_mark()
        tft.render(ctx, vb, 1, 1, B)
        ctx.temporal_resolve()
        assert ctx.temporal_filter(albedo=AMIN)["k"] == 2 and ctx.denoise(albedo=AMIN)["k"] == 2
        ctx.set_accum_mode(capi.ACCUM_COMPAT8)
        with pytest.raises(capi.SailError, match=": -4: .*COMPAT8"):
            ctx.denoise(albedo=AMIN)
        with pytest.raises(capi.SailError, match=": -4: .*COMPAT8"):
            ctx.temporal_filter(albedo=AMIN)
        ctx.set_accum_mode(capi.ACCUM_SUM)
        assert same(ctx.albedo_read(), kept)

        # what invalidates it: new rows by any of the three calls
        rows = capi._f32(sc["objects"])
        for drop in (lambda: ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows), sc["n"]),
                     lambda: ctx.move_objects(rows), lambda: ctx.set_scene_dict(sc)):
            ctx.albedo(*vb)
            assert ctx.albedo_read().any()
            assert not drop()
            with pytest.raises(capi.SailError, match=NO_MAP):
                ctx.albedo_read()
            tft.render(ctx, vb, 0, 1, B)
            ctx.noise_mark()
            tft.render(ctx, vb, 1, 1, B)
            with pytest.raises(capi.SailError, match=NO_MAP):
                ctx.denoise(albedo=AMIN)
        # moved rows keep the temporal state and still drop the map
        ctx.temporal_begin(*vb)
        tft.render(ctx, vb, 0, 1, B)
        ctx.temporal_resolve()
        ctx.albedo(*vb)
        ctx.move_objects(rows)
        ctx.temporal_begin(*vb)
        tft.render(ctx, vb, 0, 1, B)
        ctx.temporal_resolve()
        with pytest.raises(capi.SailError, match=NO_MAP):
            ctx.temporal_filter(albedo=AMIN)
        ctx.albedo_load(ones, *vb)                                    # a loaded map serves like a computed one
        assert ctx.temporal_filter(albedo=AMIN)["k"] == 1
    finally:
        ctx.close()
    plain = capi.Context(W, H)                                        # no AOV maps
    try:
        plain.set_scene_dict(sc)
        plain.temporal_moments(True)
        plain.temporal_begin(*va)
        tft.render(plain, va, 0, 1, B)
        plain.noise_mark()
        tft.render(plain, va, 1, 1, B)
        plain.temporal_resolve()
        assert plain.albedo(*va)["hit_pixels"] > 0                    # the map itself needs no AOV
        with pytest.raises(capi.SailError, match=": -4: .*SAIL_FLAG_AOV"):
            plain.denoise(albedo=AMIN)
        with pytest.raises(capi.SailError, match=": -4: .*SAIL_FLAG_AOV"):
            plain.temporal_filter(albedo=AMIN)
    finally:
        plain.close()
    multi = tft.context(sc, W, H, devices=[0, 0])
    try:
        multi.temporal_begin(*va)
        tft.render(multi, va, 0, 1, B)
        multi.noise_mark()
        tft.render(multi, va, 1, 1, B)
        multi.temporal_resolve()
        multi.albedo(*va)
        assert multi.denoise(albedo=AMIN)["k"] == 2 and multi.temporal_filter(albedo=AMIN)["k"] == 2
        half = capi.plan_keep(W, H, 0, 2, capi.PART_TILES, multi.read_accum())
        assert multi.lib.sail_load_accum(multi.h, 0, capi._ptr(half), 5) == 0      # a half-loaded checkpoint
        with pytest.raises(capi.SailError, match=": -4: .*parts not loaded"):
            multi.denoise(albedo=AMIN)
        with pytest.raises(capi.SailError, match=": -4: .*parts not loaded"):
            multi.temporal_filter(albedo=AMIN)
    finally:
        multi.close()


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------
def test_changes_nothing(gpu, fixtures):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 33, 18, 3
    va, vb = tr.orbit(0), tr.orbit(4)
    ctx = tft.context(sc, W, H)
    try:
        ctx.temporal_begin(*va)
        tft.render(ctx, va, 0, 3, B)
        ctx.temporal_resolve()
        ctx.reset()
        ctx.temporal_begin(*vb)
        tft.render(ctx, vb, 0, 1, B)
        ctx.noise_mark()
        tft.render(ctx, vb, 1, 1, B)
        ctx.temporal_resolve()

        def state():
            noise = ctx.noise_estimate(pixels=True)
            g = ctx.gbuffer(*vb, rays=True)
            return ([ctx.read_accum(), *ctx.readback(aov=True), *(ctx.temporal_read(w) for w in range(5)),
                     *(ctx.temporal_read_moments(w) for w in range(3)), noise["pixel_err"], g["t"], g["xyz"], g["rays"],
                     g["id"].astype(F)],
                    (int(ctx.stats().samples), int(ctx.stats().launches), ctx.save()["k"],
                     *(noise[f] for f in ("mean", "max_tile", "k", "k_mark", "nonfinite"))))

        def plain_calls():
            return ctx.denoise(want_var=True, want_u8=True), ctx.temporal_filter(want_var=True, want_u8=True)
        before, plain0 = state(), plain_calls()
        ctx.albedo(*vb, grid=4)
        ctx.albedo(*vb)
        a = ctx.denoise(want_var=True, want_u8=True, albedo=AMIN)
        b = ctx.temporal_filter(want_var=True, want_u8=True, albedo=AMIN)
        ctx.albedo_load(ctx.albedo_read(), *vb)
        after, plain1 = state(), plain_calls()
        for x, y in zip(before[0], after[0]):
            assert same(x, y)
        assert before[1] == after[1] and before[1][2] == 2
        for p0, p1 in zip(plain0, plain1):
            assert same(np.nan_to_num(p0["rgba"]), np.nan_to_num(p1["rgba"])) and same(p0["var"], p1["var"])
            assert np.array_equal(p0["u8"], p1["u8"])
        # and the demodulated calls give the same again after the plain ones (they share the work buffers)
        a2 = ctx.denoise(want_var=True, want_u8=True, albedo=AMIN)
        b2 = ctx.temporal_filter(want_var=True, want_u8=True, albedo=AMIN)
        for x, y in ((a, a2), (b, b2)):
            assert same(x["rgba"], y["rgba"]) and same(x["var"], y["var"]) and np.array_equal(x["u8"], y["u8"])
        assert not same(a["rgba"], plain0[0]["rgba"]) and not same(b["rgba"], plain0[1]["rgba"])
        tft.render(ctx, vb, 2, 2, B)
        got = ctx.read_accum()
    finally:
        ctx.close()
    fresh = tft.context(sc, W, H, moments=False)
    try:
        tft.render(fresh, vb, 0, 4, B)
        assert same(got, fresh.read_accum())                          # the render goes on as if nothing had been called
    finally:
        fresh.close()


# ---- 7. multi-device --------------------------------------------------------------------------------------------------------------
def test_multi_device_equals_one_device(gpu, fixtures):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 70, 40, 3
    va, vb = tr.orbit(0), tr.orbit(5)
    got = {}
    for devices in (None, [0, 0]):
        ctx = tft.context(sc, W, H, devices=devices)
        try:
            ctx.temporal_begin(*va)
            tft.render(ctx, va, 0, 4, B)
            ctx.temporal_resolve()
            ctx.reset()
            ctx.temporal_begin(*vb)
            tft.render(ctx, vb, 0, 1, B)
            ctx.noise_mark()
            tft.render(ctx, vb, 1, 1, B)
            ctx.temporal_resolve()
            A = ctx.albedo(*vb, grid=4)
            got[devices is None] = (A, ctx.albedo_read(), ctx.denoise(want_var=True, want_u8=True, albedo=AMIN),
                                    ctx.temporal_filter(want_var=True, want_u8=True, albedo=AMIN))
        finally:
            ctx.close()
    (A1, r1, d1, f1), (A2, r2, d2, f2) = got[True], got[False]
    assert same(A1["rgba"], A2["rgba"]) and same(r1, r2) and same(A1["rgba"], r1)
    assert (A1["hit_pixels"], A1["partial_pixels"]) == (A2["hit_pixels"], A2["partial_pixels"])
    for a, b in ((d1, d2), (f1, f2)):
        assert same(a["rgba"], b["rgba"]) and same(a["var"], b["var"]) and np.array_equal(a["u8"], b["u8"])
        assert (a["k"], a["nonfinite"], a["iterations"]) == (b["k"], b["nonfinite"], b["iterations"])
    assert f1["temporal_pixels"] == f2["temporal_pixels"]


# ---- 8. texture survives (deterministic) ---------------------------------------------------------------------------------------------
def test_texture_survives(gpu, fixtures):
    """C3's view at 96x64: the truth is the device's grid-4 map times a horizontal ramp, the two halves are that truth with
    seeded multiplicative noise, the guides come from a one-sample render. tests/test_albedo_host.py shows the same
    inequality for the numpy references first (CPU: relMSE input 0.117755, plain 0.0487572, albedo 0.0285457)."""
    sc = fixtures["scenes"]["C3"]
    mvp, eye = scene_view(sc)
    W, H = 96, 64
    ctx = dn.aov_context(sc, W, H)
    try:
        A = ctx.albedo(mvp, eye, grid=4)["rgba"]
        T, P, S = ar.synthetic_halves(A)
        # A load clears the AOV maps and only a rendered sample writes them, so the frame's sixteenth sample is a rendered
        # one: its sums are taken off the synthetic frame before the load and the render puts them back (to rounding).
        dn.render(ctx, sc, 15, 1, 3)
        last = ctx.read_accum()
        assert (last[..., 3] == 1).all()
        ctx.load({"k": 8, "parts": [P]})
        ctx.noise_mark()
        ctx.load({"k": 15, "parts": [(S - last).astype(F)]})
        dn.render(ctx, sc, 15, 1, 3)
        S = ctx.read_accum()
        _, N, X = ctx.readback(aov=True)
        plain = ctx.denoise()
        demod = ctx.denoise(albedo=AMIN)
    finally:
        ctx.close()
    assert (plain["k"], plain["k_mark"]) == (16, 8) and (S[..., 3] == 16).all()
    assert plain["nonfinite"] == 0 and demod["nonfinite"] == 0 and np.isfinite(N).all() and np.isfinite(X).all()
    noisy = S[..., :3] / S[..., 3:4]
    e_in, e_plain, e_demod = ar.rel_mse(noisy, T), ar.rel_mse(plain["rgba"][..., :3], T), ar.rel_mse(demod["rgba"][..., :3], T)
    print(f"texture survives C3 {W}x{H}: relMSE input {e_in:.6g}, plain {e_plain:.6g}, albedo {e_demod:.6g}")
    assert e_demod < e_plain


# ---- 9. quality on a real render ------------------------------------------------------------------------------------------------------
def quality(fixtures, name, W, H, spp, B, R, grid=4):
    """(relMSE of the noisy frame, of sail_denoise, of sail_denoise_albedo) against R samples of other indices"""
    sc = fixtures["scenes"][name]
    ref_ctx = capi.Context(W, H)
    try:
        ref_ctx.set_scene_dict(sc)
        dn.render(ref_ctx, sc, spp, R, B)
        ref = ref_ctx.readback()[..., :3]
    finally:
        ref_ctx.close()
    ctx = dn.aov_context(sc, W, H)
    try:
        dn.marked_render(ctx, sc, B, spp // 2, spp)
        noisy = ctx.readback()[..., :3]
        plain = ctx.denoise()
        ctx.albedo(*scene_view(sc), grid=grid)
        demod = ctx.denoise(albedo=AMIN)
    finally:
        ctx.close()
    assert np.isfinite(ref).all() and np.isfinite(noisy).all() and plain["nonfinite"] == 0 and demod["nonfinite"] == 0
    return ar.rel_mse(noisy, ref), ar.rel_mse(plain["rgba"][..., :3], ref), ar.rel_mse(demod["rgba"][..., :3], ref)


def test_quality_on_a_real_render(gpu, fixtures):
    """C3 at 192x128, 5 bounces, 16 spp marked at 8, grid 4, defaults, against 1024 samples of other indices: the
    demodulated denoiser must be no worse than the plain one. Also printed, not asserted: C3 at 96x64 / 64 spp (the row of
    DESIGN.md's table) and the untextured C1."""
    e_in, e_plain, e_demod = quality(fixtures, "C3", 192, 128, 16, 5, 1024)
    print(f"quality C3 192x128 16 spp, reference 1024 spp: relMSE in {e_in:.6g}, plain {e_plain:.6g} (ratio "
          f"{e_plain / e_in:.4f}), albedo {e_demod:.6g} (ratio {e_demod / e_in:.4f})")
    for name, spp, B, R in (("C3", 64, 5, 1024), ("C1", 16, 5, 512)):
        i, p, d = quality(fixtures, name, 96, 64, spp, B, R)
        print(f"  reported: {name} 96x64 {spp} spp, reference {R} spp: relMSE in {i:.6g}, plain {p:.6g} (ratio {p / i:.4f}), "
              f"albedo {d:.6g} (ratio {d / i:.4f})")
    assert e_demod <= e_plain
