"""The device-side noise estimate (sail_noise_kernel behind sail_noise_mark / sail_noise_estimate) and
render-until-converged (sail_render_until). Needs a GPU.

Kernel tests render nothing: a checkpoint load keeps the mark, so chosen accumulators P (the mark) and S go in through
Context.load and the estimate is compared with `ref_error`, the formula of include/sail_hip.h in numpy float32, one
operation at a time. The per-pixel map must equal it bit for bit. Sums: a tile adds at most 256 non-negative f32 terms,
so whatever the order its f32 sum lies within GAMMA = 255 u / (1 - 255 u), u = 2^-24, of the exact sum (Higham, Accuracy
and Stability of Numerical Algorithms, eq. 4.4); the kernel's tree has depth 8 and the tile map rounds the tile's mean
to f32 once more, 9 roundings in all, so the bound also holds for tile_err * pixels. The host adds the tiles in double.

Driver tests: the frame of render_until must equal render_schedule over the same sample indices bit for bit, and the
stopping rule is checked against targets taken from a run's own history (no noise level is guessed in advance)."""
import math

import numpy as np
import pytest

from sail_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
GAMMA = 255 * 2.0 ** -24 / (1 - 255 * 2.0 ** -24)
SIZES = [(1, 1), (16, 16), (33, 17), (150, 70)]


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the reference: include/sail_hip.h's formula, every operation rounded to f32 ---------------------------------------
def ref_error(S, P, mix=False, k=0, h=0):
    """(per-pixel error with 0 where it is not finite, mask of the non-finite ones)"""
    S, P = np.asarray(S, F), np.asarray(P, F)
    shape = S.shape[:2]
    n = np.full(shape, F(k)) if mix else S[..., 3]
    hh = np.full(shape, F(h)) if mix else P[..., 3]
    with np.errstate(all="ignore"):
        valid = (hh > F(0)) & (n > hh)
        dn = (n - hh)[..., None]
        if mix:
            a, m = P[..., :3], S[..., :3]
            b = ((n[..., None] * m) - (hh[..., None] * a)) / dn
        else:
            a = P[..., :3] / hh[..., None]
            b = (S[..., :3] - P[..., :3]) / dn
            m = S[..., :3] / n[..., None]
        ad = np.abs(a - b)
        d = (ad[..., 0] + ad[..., 1]) + ad[..., 2]
        l = (m[..., 0] + m[..., 1]) + m[..., 2]
        e = (F(0.5) * d) / (F(1e-4) + np.sqrt(np.maximum(l, F(0)) / F(3)))
    assert e.dtype == F
    e = np.where(valid, e, F(0))
    bad = ~np.isfinite(e)
    return np.where(bad, F(0), e).astype(F), bad


def tile_sums(e):
    """float64 sum of the f32 per-pixel values of each 16x16 tile, and each tile's in-frame pixel count"""
    H, W = e.shape
    ty, tx = (H + 15) // 16, (W + 15) // 16
    sums, npix = np.zeros((ty, tx)), np.zeros((ty, tx))
    for j in range(ty):
        for i in range(tx):
            t = e[j * 16:(j + 1) * 16, i * 16:(i + 1) * 16].astype(np.float64)
            sums[j, i], npix[j, i] = t.sum(), t.size
    return sums, npix


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_chain(W, H, seed, steps=2, mix=False):
    """`steps` accumulators of one progressive render, each holding more samples than the one before: random non-negative
    sums with per-pixel counts (or, mix, running means), plus the special pixels where the frame has room for them"""
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


# ---- running and checking ---------------------------------------------------------------------------------------------------
def parts_of(a, W, H, nd):
    return [a] if nd == 1 else [capi.plan_keep(W, H, i, nd, capi.PART_TILES, a) for i in range(nd)]


def load(ctx, a, k, nd=1):
    ctx.load({"k": k, "parts": parts_of(a, ctx.W, ctx.H, nd)})


def check(out, S, P, mix=False, k=0, h=0, what=""):
    e, bad = ref_error(S, P, mix, k, h)
    H, W = e.shape
    sums, npix = tile_sums(e)
    tol = GAMMA * sums
    got_sums = out["tile_err"].astype(np.float64) * npix
    ref_mean, ref_max = sums.sum() / (W * H), (sums / npix).max()
    rel = np.abs(got_sums - sums)[sums > 0] / sums[sums > 0]
    print(f"{what} {W}x{H}: nonfinite {out['nonfinite']} (ref {int(bad.sum())}), pixel mismatches "
          f"{int((bits(out['pixel_err']) != bits(e)).sum())}, worst tile rel err {rel.max() if rel.size else 0.0:.3g} (bound {GAMMA:.3g}), "
          f"mean {out['mean']:.9g} (ref {ref_mean:.9g}), max_tile {out['max_tile']:.9g} (ref {ref_max:.9g})")
    assert (out["tiles_x"], out["tiles_y"]) == (sums.shape[1], sums.shape[0])
    assert np.array_equal(bits(out["pixel_err"]), bits(e))     # raw uint32: the map holds no NaN (reported as counts)
    assert out["nonfinite"] == int(bad.sum())
    assert (np.abs(got_sums - sums) <= tol).all()
    assert abs(out["mean"] - ref_mean) <= GAMMA * ref_mean
    assert abs(out["max_tile"] - ref_max) <= GAMMA * ref_max
    return e, bad


def same_estimate(a, b):
    return (all(a[f] == b[f] for f in ("mean", "max_tile", "k", "k_mark", "nonfinite", "tiles_x", "tiles_y"))
            and np.array_equal(bits(a["tile_err"]), bits(b["tile_err"]))
            and np.array_equal(bits(a["pixel_err"]), bits(b["pixel_err"])))


def run_chain(ctx, chain, ks, mix, nd=1, what=""):
    """mark on chain[0]; estimate chain[1] (twice: determinism), re-marking with the last one; estimate chain[2] against
    chain[1]. Returns the estimates."""
    load(ctx, chain[0], ks[0], nd)
    ctx.noise_mark()
    load(ctx, chain[1], ks[1], nd)     # a loaded checkpoint keeps the mark
    o1 = ctx.noise_estimate(tiles=True, pixels=True)
    assert (o1["k"], o1["k_mark"]) == (ks[1], ks[0])
    check(o1, chain[1], chain[0], mix, ks[1], ks[0], what)
    o2 = ctx.noise_estimate(tiles=True, pixels=True, remark=True)
    assert same_estimate(o1, o2)
    outs = [o1]
    if len(chain) > 2:
        load(ctx, chain[2], ks[2], nd)
        o3 = ctx.noise_estimate(tiles=True, pixels=True)
        assert (o3["k"], o3["k_mark"]) == (ks[2], ks[1])
        check(o3, chain[2], chain[1], mix, ks[2], ks[1], what + " after remark")
        outs.append(o3)
    return outs


@pytest.mark.parametrize("W,H", SIZES)
def test_kernel_matches_the_f32_reference(gpu, W, H):
    chain = make_chain(W, H, seed=W * 1000 + H, steps=3)
    if W * H >= 256:   # the special pixels are what they are meant to be
        e, bad = ref_error(chain[1], chain[0])
        assert int(bad.sum()) == 2 and e.reshape(-1)[[3, 5, 7]].tolist() == [0.0, 0.0, 0.0]
    ctx = capi.Context(W, H)
    try:
        run_chain(ctx, chain, (3, 7, 12), False, what="sum")
    finally:
        ctx.close()


@pytest.mark.parametrize("W,H", [(1, 1), (33, 17), (150, 70)])
def test_kernel_mix_mode(gpu, W, H):
    """running means: the halves are weighed by the context's sample index now and at the mark"""
    chain = make_chain(W, H, seed=W * 77 + H, steps=3, mix=True)
    ctx = capi.Context(W, H)
    try:
        ctx.set_accum_mode(capi.ACCUM_MIX)
        run_chain(ctx, chain, (3, 7, 12), True, what="mix")
    finally:
        ctx.close()


def test_compat8_is_refused(gpu):
    ctx = capi.Context(16, 16)
    try:
        ctx.set_accum_mode(capi.ACCUM_COMPAT8)
        with pytest.raises(capi.SailError, match="COMPAT8"):
            ctx.noise_mark()
        with pytest.raises(capi.SailError, match="COMPAT8"):
            ctx.noise_estimate()
    finally:
        ctx.close()


def test_until_refuses_before_rendering(gpu, fixtures):
    """what the looks would refuse (no scene, COMPAT8) is refused before a sample is rendered"""
    sc = fixtures["scenes"]["C1"]
    mvp = np.array(sc["mvp_rowmajor"])
    ctx = capi.Context(24, 16)
    try:
        with pytest.raises(capi.SailError, match="-4.*before sail_set_scene"):
            ctx.render_until(mvp, sc["eye"], 3, 0.0, 4, 8)
        ctx.set_scene_dict(sc)
        ctx.set_accum_mode(capi.ACCUM_COMPAT8)
        with pytest.raises(capi.SailError, match="-4.*COMPAT8"):
            ctx.render_until(mvp, sc["eye"], 3, 0.0, 4, 8)
        assert ctx.stats().samples == 0 and ctx.save()["k"] == 0
    finally:
        ctx.close()


def test_state_rules(gpu, fixtures):
    W, H = 16, 16
    P, S = make_chain(W, H, seed=5)
    ctx = capi.Context(W, H)
    try:
        with pytest.raises(capi.SailError, match="no mark"):
            ctx.noise_estimate()                       # before any mark
        load(ctx, P, 4)
        ctx.noise_mark()
        with pytest.raises(capi.SailError, match="no sample since the mark"):
            ctx.noise_estimate()                       # k == k_mark
        load(ctx, S, 4)
        with pytest.raises(capi.SailError, match="no sample since the mark"):
            ctx.noise_estimate()                       # other sums, but still k == k_mark
        load(ctx, S, 8)
        assert ctx.noise_estimate()["k_mark"] == 4
        # everything that restarts the accumulation drops the mark
        drops = [ctx.reset, lambda: ctx.set_accum_mode(capi.ACCUM_MIX), lambda: ctx.set_accum_mode(capi.ACCUM_SUM),
                 lambda: ctx.set_partition(0, 1, capi.PART_TILES), lambda: ctx.set_scene_dict(fixtures["scenes"]["C1"])]
        for drop in drops:
            load(ctx, P, 4)
            ctx.noise_mark()
            drop()
            load(ctx, S, 8)
            with pytest.raises(capi.SailError, match="no mark"):
                ctx.noise_estimate()
        sc = fixtures["scenes"]["C1"]
        load(ctx, P, 4)
        ctx.noise_mark()
        assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(capi._f32(sc["objects"])), sc["n"]) == 0
        load(ctx, S, 8)
        with pytest.raises(capi.SailError, match="no mark"):
            ctx.noise_estimate()
    finally:
        ctx.close()


@pytest.mark.parametrize("devices,dbg", [([0, 0, 0], None), ([0], {capi.DEBUG_FORCE_RCCL: 1})])
def test_multi_device_equals_one_device(gpu, devices, dbg):
    """a multi-device context reduces first and estimates device 0's frame: the parts of the same P and S (plan_keep)
    give every output the one-device run gives, bit for bit"""
    W, H = 150, 70
    chain = make_chain(W, H, seed=31, steps=3)
    one = capi.Context(W, H)
    try:
        want = run_chain(one, chain, (3, 7, 12), False, what="one device")
    finally:
        one.close()
    ctx = capi.Context(W, H, devices=devices)
    try:
        for opt, val in (dbg or {}).items():
            ctx.set_debug(opt, val)
        got = run_chain(ctx, chain, (3, 7, 12), False, nd=len(devices), what=f"devices {devices}")
        load(ctx, chain[0], 20, len(devices))
        half = capi.plan_keep(W, H, 0, max(len(devices), 2), capi.PART_TILES, chain[0])
        if len(devices) > 1:   # a half-loaded checkpoint
            assert ctx.lib.sail_load_accum(ctx.h, 0, capi._ptr(half), 21) == 0
            with pytest.raises(capi.SailError, match="parts not loaded"):
                ctx.noise_mark()
            with pytest.raises(capi.SailError, match="parts not loaded"):
                ctx.noise_estimate()
    finally:
        ctx.close()
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert same_estimate(g, w)


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def scheduled_frame(sc, W, H, B, spp):
    """a fresh context's render_schedule over samples 0 .. spp-1"""
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), W, H, 0, spp)
    ctx = capi.Context(W, H)
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        return ctx.read_accum()
    finally:
        ctx.close()


def until(sc, W, H, B, target, mn, mx, debug=None):
    ctx = capi.Context(W, H, debug=debug)
    try:
        ctx.set_scene_dict(sc)
        res = ctx.render_until(np.array(sc["mvp_rowmajor"]), sc["eye"], B, target, mn, mx)
        return res, ctx.read_accum(), ctx.kernel_name()
    finally:
        ctx.close()


C3 = ("C3", 150, 70, 5)


@pytest.fixture(scope="module")
def c3_frames(gpu, fixtures):
    """render_schedule's frames of C3 by sample count, each rendered once"""
    name, W, H, B = C3
    cache = {}

    def get(spp):
        if spp not in cache:
            cache[spp] = scheduled_frame(fixtures["scenes"][name], W, H, B, spp)
        return cache[spp]
    return get


@pytest.fixture(scope="module")
def c3_to_cap(gpu, fixtures):
    name, W, H, B = C3
    res, frame, _ = until(fixtures["scenes"][name], W, H, B, 0.0, 4, 40)
    print("C3 150x70 looks:", [(s["k"], s["mean"], s["max_tile"]) for s in res["history"]])
    return res, frame


def test_until_runs_to_the_cap(c3_to_cap, c3_frames):
    res, frame = c3_to_cap
    assert res["k"] == 40 and res["converged"] is False
    assert [s["k"] for s in res["history"]] == [4, 8, 16, 32, 40]
    assert res["history"][0]["mean"] == math.inf                # the first look only marks
    assert all(0 < s["mean"] <= s["max_tile"] < math.inf for s in res["history"][1:])
    assert (res["k_mark"], res["mean"], res["nonfinite"]) == (32, res["history"][-1]["mean"], 0)
    assert np.array_equal(bits(frame), bits(c3_frames(40)))


@pytest.mark.parametrize("first", [1, 2])
def test_until_stops_at_a_look(fixtures, c3_to_cap, c3_frames, first):
    """target = the mean of the first look j >= `first` that is below every earlier look's (look 0 only marks: +inf): a
    fresh render_until must stop there, converged, with render_schedule's frame. first = 1 is the rule as stated;
    first = 2 also passes over at least one estimate above the target."""
    name, W, H, B = C3
    hist = c3_to_cap[0]["history"]
    js = [j for j in range(first, len(hist)) if all(hist[j]["mean"] < hist[i]["mean"] for i in range(j))]
    assert js, f"no look from {first} on improves on all its predecessors: {hist}"
    j = js[0]
    res, frame, _ = until(fixtures["scenes"][name], W, H, B, hist[j]["mean"], 4, 40)
    assert res["converged"] is True and res["k"] == hist[j]["k"]
    assert res["history"] == hist[:j + 1]
    assert np.array_equal(bits(frame), bits(c3_frames(hist[j]["k"])))


def test_until_largest_target_stops_at_the_second_look(fixtures, c3_to_cap, c3_frames):
    name, W, H, B = C3
    res, frame, _ = until(fixtures["scenes"][name], W, H, B, 1e30, 4, 40)
    assert res["converged"] is True and res["k"] == 8 and res["k_mark"] == 4
    assert res["history"] == c3_to_cap[0]["history"][:2]
    assert np.array_equal(bits(frame), bits(c3_frames(8)))


def test_until_noise_falls(c3_to_cap):
    """loose sanity: 32 -> 40 samples is estimated less noisy than 4 -> 8"""
    hist = c3_to_cap[0]["history"]
    assert hist[-1]["mean"] < hist[1]["mean"]


def test_until_cornell_form(gpu, fixtures):
    """C1 at 64x48 with the Cornell form holding 16 samples in flight: the look boundaries (4, 8, 16, 32, 40) split its
    steps, bit for bit"""
    sc = fixtures["scenes"]["C1"]
    res, frame, kernel = until(sc, 64, 48, 5, 0.0, 4, 40, debug={capi.DEBUG_JIT_NS: 16})
    assert kernel.startswith("sail_trace_kernel_jit"), kernel
    assert res["k"] == 40 and [s["k"] for s in res["history"]] == [4, 8, 16, 32, 40]
    assert np.array_equal(bits(frame), bits(scheduled_frame(sc, 64, 48, 5, 40)))


def test_until_continues_and_rejects(gpu, fixtures):
    """render_until starts at the context's sample index; bad arguments are SAIL_E_INVALID and render nothing"""
    sc = fixtures["scenes"]["C1"]
    W, H, B = 24, 16, 3
    mvp = np.array(sc["mvp_rowmajor"])
    ctx = capi.Context(W, H)
    try:
        ctx.set_scene_dict(sc)
        for target, mn, mx in ((0.0, 0, 8), (0.0, 8, 4), (math.nan, 4, 8)):
            with pytest.raises(capi.SailError, match="-1"):
                ctx.render_until(mvp, sc["eye"], B, target, mn, mx)
        assert ctx.stats().samples == 0
        inv, seeds = capi.schedule(mvp, W, H, 0, 5)
        ctx.render_schedule(inv, seeds, sc["eye"], B)
        res = ctx.render_until(mvp, sc["eye"], B, 0.0, 4, 12)
        assert [s["k"] for s in res["history"]] == [10, 12] and res["k"] == 12 and res["k_mark"] == 10
        again = ctx.render_until(mvp, sc["eye"], B, 0.0, 4, 12)    # already at the cap: nothing to render
        assert again["history"] == [] and again["k"] == 12 and again["converged"] is False
        assert np.array_equal(bits(ctx.read_accum()), bits(scheduled_frame(sc, W, H, B, 12)))
    finally:
        ctx.close()
