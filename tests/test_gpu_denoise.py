"""The variance-guided a-trous denoiser (sail_denoise_prepare_kernel and sail_denoise_atrous_kernel behind sail_denoise).
Needs a GPU.

`ref_denoise` is the formula of include/sail_hip.h in numpy float32, one operation at a time, the tap loops in the stated
order and vectorised over pixels (the prefilter and the a-trous passes are tests/atrous_ref.py's). Every operation of the
formula is an IEEE f32 one (the weights are rational, no exp), so the device's colour and variance maps must equal it bit
for bit. The quality tests compare with a separate, far longer render of the same scene over other sample indices, never
with the code under test."""
import numpy as np
import pytest

import oracle
from atrous_ref import atrous, lum, prefilter
from sail_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (16, 16), (33, 17), (150, 70)]
OTHER = {"sigma_l": 2.5, "sigma_x": 0.05}


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the reference: include/sail_hip.h's formula, every operation rounded to f32 ---------------------------------------
def ref_prepare(S, P, mix=False, k=0, h=0):
    """(c0, v, mask of the pixels whose mean colour is not finite)"""
    S, P = np.asarray(S, F), np.asarray(P, F)
    shape = S.shape[:2]
    n = np.full(shape, F(k)) if mix else S[..., 3]
    hh = np.full(shape, F(h)) if mix else P[..., 3]
    with np.errstate(all="ignore"):
        if mix:
            c0 = S[..., :3].copy()
        else:
            c0 = np.where((n > F(0))[..., None], S[..., :3] / n[..., None], F(0)).astype(F)
        halves = (hh > F(0)) & (n > hh)
        dn = n - hh
        if mix:
            a = P[..., :3]
            b = ((n[..., None] * S[..., :3]) - (hh[..., None] * a)) / dn[..., None]
        else:
            a = P[..., :3] / hh[..., None]
            b = (S[..., :3] - P[..., :3]) / dn[..., None]
        dl = lum(a) - lum(b)
        v0 = np.where(halves, (dl * dl) * ((hh * dn) / (n * n)), F(0)).astype(F)
    v = prefilter(v0)
    assert c0.dtype == F and v.dtype == F
    return c0, v, ~np.isfinite(c0).all(axis=-1)


def ref_denoise(S, P, N, X, mix=False, k=0, h=0, iterations=4, sigma_l=1.0, sigma_x=0.2):
    """(denoised rgb (H, W, 3), filtered variance (H, W), number of pixels whose mean colour is not finite)"""
    c, v, bad = ref_prepare(S, P, mix, k, h)
    nd = F(2) * np.asarray(N, F)[..., :3] - F(1)
    x = np.ascontiguousarray(np.asarray(X, F)[..., :3])
    c, v = atrous(c, v, nd, x, iterations, sigma_l, sigma_x)
    return c, v, int(bad.sum())


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_chain(W, H, seed, steps=2, mix=False):
    """tests/test_gpu_noise.py's accumulators: `steps` accumulators of one progressive render, each holding more samples
    than the one before: random non-negative sums with per-pixel counts (or, mix, running means), plus the special pixels
    where the frame has room for them"""
    rng = np.random.default_rng(seed)
    out = []
    cnt = np.zeros((H, W), F)
    rgb = np.zeros((H, W, 3), F)
    scale = np.ones((H, W, 1), F)
    if W >= 32:  # one tile (1, 0) whose values span about 2^40 in magnitude
        scale[0:16, 16:32, 0] = np.exp2(rng.integers(-20, 21, (min(H, 16), 16))).astype(F)
    for _ in range(steps):
        add = rng.integers(1, 9, (H, W)).astype(F)
        rgb = (rgb + rng.random((H, W, 3), dtype=F) * F(2) * add[..., None] * scale).astype(F)
        cnt = cnt + add
        a = np.zeros((H, W, 4), F)
        a[..., :3] = rgb / cnt[..., None] if mix else rgb
        a[..., 3] = F(1) if mix else cnt
        out.append(a)
    if W * H >= 256:
        flat = [a.reshape(-1, 4) for a in out]
        last = W * H - 1                      # 33x17: the single pixel of the ragged corner tile
        flat[0][3, 3] = 0.0                   # h = 0: no samples at the mark
        flat[0][5, 3] = 0.0
        for f in flat[1:]:
            f[5, 3] = 0.0                     # n = 0 too
        for f in flat[1:]:
            f[7, 3] = flat[0][7, 3]           # n = h: none since the mark
        for f in flat[1:]:
            f[last, 1] = np.nan               # a NaN channel
            f[W + 2, 0] = np.inf              # an Inf channel
        for f in flat:
            f[9, 2] = -0.0                    # a -0 channel in both
        flat[-1][11, 0] = -0.0                # ... and in the newest only
    return out


def aov_context(sc, W, H, **kw):
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV, **kw)
    ctx.set_scene_dict(sc)
    return ctx


def render(ctx, sc, k0, spp, B):
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), ctx.W, ctx.H, k0, spp)
    ctx.render_schedule(inv, seeds, sc["eye"], B)


def marked_render(ctx, sc, B, mark, spp):
    """`mark` samples, the mark, the rest up to `spp`; returns (S, P, N, X) as the device holds them"""
    render(ctx, sc, 0, mark, B)
    P = ctx.read_accum()
    ctx.noise_mark()
    render(ctx, sc, mark, spp - mark, B)
    S = ctx.read_accum()
    _, N, X = ctx.readback(aov=True)
    return S, P, N, X


def same_bits(out, c, v, what):
    dc = int((bits(out["rgba"][..., :3]) != bits(c)).sum())
    dv = int((bits(out["var"]) != bits(v)).sum())
    print(f"{what}: colour channels differing {dc}, variance texels differing {dv}")
    assert dc == 0 and dv == 0
    assert (bits(out["rgba"][..., 3]) == bits(F(1))).all()


@pytest.fixture(scope="module")
def c3_inputs(gpu, fixtures):
    """C3, 3 bounces, 8 spp marked after 3, per size: the context (kept open) and what it holds"""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            ctx = aov_context(fixtures["scenes"]["C3"], W, H)
            made[(W, H)] = (ctx, marked_render(ctx, fixtures["scenes"]["C3"], 3, 3, 8))
        return made[(W, H)]
    yield get
    for ctx, _ in made.values():
        ctx.close()


# ---- 1. bit-exact against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [{}, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("iterations", [1, 4, 6])
@pytest.mark.parametrize("W,H", SIZES)
def test_matches_the_f32_reference(c3_inputs, W, H, iterations, params):
    ctx, (S, P, N, X) = c3_inputs(W, H)
    p = dict(params, iterations=iterations)
    c, v, bad = ref_denoise(S, P, N, X, **p)
    assert not np.isnan(c).any() and not np.isnan(v).any()     # so that raw bits can be compared
    out = ctx.denoise(p, want_var=True)
    assert (out["k"], out["k_mark"], out["iterations"], out["nonfinite"]) == (8, 3, iterations, bad)
    assert len(out["pass_ms"]) == iterations + 1
    same_bits(out, c, v, f"C3 {W}x{H} it {iterations} {params}")
    if not params and iterations == 4:                          # NULL parameters are the defaults
        again = ctx.denoise(None, want_var=True)
        assert np.array_equal(bits(again["rgba"]), bits(out["rgba"])) and np.array_equal(bits(again["var"]), bits(out["var"]))


# ---- 2. non-finite guides ---------------------------------------------------------------------------------------------------
def test_missed_pixels_stay(gpu, fixtures):
    """N1S at 33x17: most pixels miss the scene and carry a NaN position; they take no neighbours and keep their mean"""
    sc = fixtures["scenes"]["N1S"]
    ctx = aov_context(sc, 33, 17)
    try:
        S, P, N, X = marked_render(ctx, sc, 3, 3, 8)
        out = ctx.denoise(want_var=True)
    finally:
        ctx.close()
    miss = ~np.isfinite(X[..., :3]).all(axis=-1)
    print("N1S 33x17: texels with a non-finite position:", int(miss.sum()), "of", miss.size)
    assert miss.any() and not miss.all()
    c, v, bad = ref_denoise(S, P, N, X)
    assert np.array_equal(bits(out["rgba"][..., :3]), bits(c)) and np.array_equal(bits(out["var"]), bits(v))
    assert out["nonfinite"] == bad
    c0, _, _ = ref_prepare(S, P)
    assert np.array_equal(bits(out["rgba"][..., :3])[miss], bits(c0)[miss])


# ---- 3. chosen accumulators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [False, True], ids=["sum", "mix"])
@pytest.mark.parametrize("W,H", [(33, 17), (150, 70)])
def test_chosen_accumulators(gpu, fixtures, W, H, mix):
    """h = 0, n = h, NaN, Inf, -0 and the 2^40 tile, loaded as a checkpoint for the mark and for the frame"""
    sc = fixtures["scenes"]["C3"]
    Pa, Sa = make_chain(W, H, seed=W * 91 + H, mix=mix)
    ctx = aov_context(sc, W, H)
    try:
        if mix:
            ctx.set_accum_mode(capi.ACCUM_MIX)
        render(ctx, sc, 0, 2, 3)
        ctx.load({"k": 3, "parts": [Pa]})
        ctx.noise_mark()
        ctx.load({"k": 7, "parts": [Sa]})
        _, N, X = ctx.readback(aov=True)        # whatever the device holds after the load
        for p in ({}, dict(OTHER, iterations=6)):
            out = ctx.denoise(p, want_var=True)
            c, v, bad = ref_denoise(Sa, Pa, N, X, mix=mix, k=7, h=3, **p)
            same = (bits(out["rgba"][..., :3]) == bits(c)) | (np.isnan(out["rgba"][..., :3]) & np.isnan(c))
            same_v = (bits(out["var"]) == bits(v)) | (np.isnan(out["var"]) & np.isnan(v))
            print(f"chosen {W}x{H} mix {mix} {p}: nonfinite {out['nonfinite']} (ref {bad}), differing "
                  f"{int((~same).sum())} colour channels, {int((~same_v).sum())} variance texels")
            # the reference's NaNs are quiet NaNs made by the same operations: compare raw bits wherever either is no NaN
            assert same.all() and same_v.all()
            assert out["nonfinite"] == bad == 2
    finally:
        ctx.close()


# ---- 4. display and RGBA8 -----------------------------------------------------------------------------------------------------
def quantise(o):
    """the filter kernel's (uint8)(int)(clamp(o, 0, 1) * 255 + 0.5)"""
    return (oracle.math(12, o) * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)


def display(c, kind, gamma_c):
    c = np.ascontiguousarray(c, F)
    if kind == capi.FILTER_COLOR:
        return c
    if kind == capi.FILTER_GAMMA:
        return oracle.math(5, c, oracle.math(14, np.full_like(c, F(gamma_c))))
    xx = oracle.math(10, np.zeros_like(c), c - F(0.004))
    return oracle.math(11, xx * (F(6.2) * xx + F(0.5)), xx * (F(6.2) * xx + F(1.7)) + F(0.06))


@pytest.mark.parametrize("kind,gamma_c", [(capi.FILTER_COLOR, 2.2), (capi.FILTER_GAMMA, 2.2), (capi.FILTER_GAMMA, 1.8),
                                          (capi.FILTER_TONEMAPPING, 2.2)])
def test_display_and_rgba8(c3_inputs, kind, gamma_c):
    ctx, _ = c3_inputs(150, 70)
    out = ctx.denoise({"display": kind, "gamma_c": gamma_c}, want_u8=True)
    rgb = out["rgba"][..., :3]
    want = quantise(display(rgb, kind, gamma_c))
    assert np.array_equal(out["u8"][..., :3], want) and (out["u8"][..., 3] == 255).all()
    assert len(np.unique(want)) > 16                               # a real image, not a constant
    if kind == capi.FILTER_COLOR:
        assert np.array_equal(out["u8"][..., :3], quantise(rgb))


# ---- 5. no side effects -------------------------------------------------------------------------------------------------------
def test_changes_nothing(gpu, fixtures):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 33, 17, 3
    ctx = aov_context(sc, W, H)
    try:
        marked_render(ctx, sc, B, 3, 8)
        before = (ctx.read_accum(), ctx.save()["k"], ctx.noise_estimate(pixels=True), ctx.readback(aov=True))
        one = ctx.denoise(want_var=True, want_u8=True)
        after = (ctx.read_accum(), ctx.save()["k"], ctx.noise_estimate(pixels=True), ctx.readback(aov=True))
        two = ctx.denoise(want_var=True, want_u8=True)
        assert np.array_equal(bits(before[0]), bits(after[0])) and before[1] == after[1] == 8
        for f in ("mean", "max_tile", "k", "k_mark", "nonfinite"):
            assert before[2][f] == after[2][f]
        assert np.array_equal(bits(before[2]["pixel_err"]), bits(after[2]["pixel_err"]))
        for a, b in zip(before[3], after[3]):
            assert np.array_equal(bits(a), bits(b))
        for f in ("rgba", "var"):
            assert np.array_equal(bits(one[f]), bits(two[f]))
        assert np.array_equal(one["u8"], two["u8"])
        render(ctx, sc, 8, 4, B)
        got = ctx.read_accum()
    finally:
        ctx.close()
    plain = aov_context(sc, W, H)
    try:
        render(plain, sc, 0, 12, B)
        assert np.array_equal(bits(got), bits(plain.read_accum()))
    finally:
        plain.close()


# ---- 6. multi-device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,dbg", [([0, 0, 0], None), ([0], {capi.DEBUG_FORCE_RCCL: 1})])
def test_multi_device_equals_one_device(c3_inputs, fixtures, devices, dbg):
    W, H = 150, 70
    one, _ = c3_inputs(W, H)
    want = one.denoise(want_var=True, want_u8=True)
    sc = fixtures["scenes"]["C3"]
    ctx = aov_context(sc, W, H, devices=devices)
    try:
        for opt, val in (dbg or {}).items():
            ctx.set_debug(opt, val)
        marked_render(ctx, sc, 3, 3, 8)
        got = ctx.denoise(want_var=True, want_u8=True)
    finally:
        ctx.close()
    for f in ("rgba", "var"):
        assert np.array_equal(bits(got[f]), bits(want[f]))
    assert np.array_equal(got["u8"], want["u8"])
    assert (got["k"], got["k_mark"], got["nonfinite"]) == (want["k"], want["k_mark"], want["nonfinite"])


# ---- 7. state rules -----------------------------------------------------------------------------------------------------------
def test_state_rules(gpu, fixtures):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 16, 16, 3
    plain = capi.Context(W, H)
    try:
        plain.set_scene_dict(sc)
        render(plain, sc, 0, 2, B)
        plain.noise_mark()
        render(plain, sc, 2, 2, B)
        with pytest.raises(capi.SailError, match="-4.*SAIL_FLAG_AOV"):
            plain.denoise()
    finally:
        plain.close()
    ctx = aov_context(sc, W, H)
    try:
        render(ctx, sc, 0, 2, B)
        with pytest.raises(capi.SailError, match="-4.*no mark"):
            ctx.denoise()
        ctx.noise_mark()
        with pytest.raises(capi.SailError, match="-4.*no sample since the mark"):
            ctx.denoise()
        render(ctx, sc, 2, 2, B)
        assert ctx.denoise()["k_mark"] == 2
        for bad in ({"iterations": 0}, {"iterations": 7}, {"sigma_l": 0.0}, {"sigma_l": float("nan")},
                    {"sigma_x": float("inf")}, {"display": capi.FILTER_WINDOW}):
            with pytest.raises(capi.SailError, match="-1.*bad parameters"):
                ctx.denoise(bad)
        ctx.set_accum_mode(capi.ACCUM_COMPAT8)
        with pytest.raises(capi.SailError, match="-4.*COMPAT8"):
            ctx.denoise()
    finally:
        ctx.close()
    multi = aov_context(sc, W, H, devices=[0, 0])
    try:
        marked_render(multi, sc, B, 2, 4)
        assert multi.denoise()["k"] == 4
        half = capi.plan_keep(W, H, 0, 2, capi.PART_TILES, multi.read_accum())
        assert multi.lib.sail_load_accum(multi.h, 0, capi._ptr(half), 5) == 0      # a half-loaded checkpoint
        with pytest.raises(capi.SailError, match="-4.*parts not loaded"):
            multi.denoise()
    finally:
        multi.close()


# ---- 8. quality ---------------------------------------------------------------------------------------------------------------
def rel_mse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


@pytest.mark.parametrize("name,spp,B,R,bound", [("C1", 16, 5, 512, 0.5), ("C4", 16, 4, 512, 0.6), ("C3", 64, 5, 1024, 1.0)])
def test_quality_against_a_reference_render(gpu, fixtures, name, spp, B, R, bound):
    """denoised relMSE / input relMSE against R samples of other indices (spp .. spp + R - 1), defaults, 96x64"""
    sc = fixtures["scenes"][name]
    W, H = 96, 64
    ref_ctx = capi.Context(W, H)
    try:
        ref_ctx.set_scene_dict(sc)
        render(ref_ctx, sc, spp, R, B)
        ref = ref_ctx.readback()[..., :3]
    finally:
        ref_ctx.close()
    ctx = aov_context(sc, W, H)
    try:
        marked_render(ctx, sc, B, spp // 2, spp)
        noisy = ctx.readback()[..., :3]
        out = ctx.denoise()
    finally:
        ctx.close()
    assert np.isfinite(ref).all() and np.isfinite(noisy).all() and out["nonfinite"] == 0
    e_in, e_out = rel_mse(noisy, ref), rel_mse(out["rgba"][..., :3], ref)
    print(f"quality {name} {spp} spp, {B} bounces, reference {R} spp: relMSE in {e_in:.6g}, out {e_out:.6g}, "
          f"ratio {e_out / e_in:.4f} (required <= {bound})")
    assert e_out / e_in <= bound
