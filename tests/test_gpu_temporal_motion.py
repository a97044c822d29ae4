"""Keeping the temporal history across an object drag (sail_move_objects, sail_temporal_pending_motion and the motion
variants of the two reproject kernels behind sail_temporal_begin). Needs a GPU.

The reference is tests/temporal_motion_ref.py: the formulas of include/sail_hip.h in numpy float32, one operation at a time,
with the first hits from oracle.pick. Every operation is an IEEE f32 one, so the device's maps must equal it bit for bit: raw
uint32 bits are compared, with no NaN-equals-NaN shortcut. The quality test compares with a separate, far longer render of
the moved scene over other sample indices, never with the code under test."""
import numpy as np
import pytest

import temporal_filter_ref as tf
import temporal_motion_ref as tm
import temporal_ref as tr
from sail_amd import capi
from temporal_ref import bits

pytestmark = pytest.mark.gpu

F = np.float32
G_CUR, G_PREV, HIST, R_MAP, OUT = (capi.TEMPORAL_G_CUR, capi.TEMPORAL_G_PREV, capi.TEMPORAL_HIST, capi.TEMPORAL_R,
                                   capi.TEMPORAL_OUT)
M_HIST, M_R, M_OUT = capi.TEMPORAL_M_HIST, capi.TEMPORAL_M_R, capi.TEMPORAL_M_OUT
SPHERE = (0.6, 0.1, -0.3)

# name: (scene, {row: motion}, the history's view, the new view); a view is an orbit angle or None for the scene's own
CASES = {
    "C1-sphere": ("C1", {2: SPHERE}, 0, 0),
    "C1-sphere-orbit3": ("C1", {2: SPHERE}, 0, 3),
    "C1-light-and-sphere": ("C1", {0: (-0.5, 0.0, 0.4), 2: (0.3, 0.0, 0.2)}, 0, 0),
    "C3-two-spheres": ("C3", {3: (0.0, 0.5, 0.9), 5: (0.0, 0.6, 0.5)}, None, None),
}
# words of R that differ between the reference with the motion and the one without, all-ones history, 96x64 (the issue's
# figures, from the CPU reference)
DISCRIMINATION = {"C1-sphere": 920, "C1-sphere-orbit3": 948, "C1-light-and-sphere": 396, "C3-two-spheres": 632}


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def context(sc, W, H, flags=0, moments=False, **kw):
    ctx = capi.Context(W, H, flags=flags, **kw)
    ctx.set_scene_dict(sc)
    if moments:
        ctx.temporal_moments(True)
    return ctx


def render(ctx, view, k0, spp, B):
    inv, seeds = capi.schedule(view[0], ctx.W, ctx.H, k0, spp)
    ctx.render_schedule(inv, seeds, view[1], B)


def fixture_view(sc):
    return np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F)


def case_views(sc, a, b):
    return (fixture_view(sc) if a is None else tr.orbit(a)), (fixture_view(sc) if b is None else tr.orbit(b))


def rows_of(sc):
    return np.array(sc["objects"], F)


# the reference's G-buffers (oracle.pick), computed once per (label of the rows, size, view) and never changed
_G = {}


def ref_g(sc, label, W, H, key, view):
    k = (label, W, H, key)
    if k not in _G:
        _G[k] = tr.ref_gbuffer(sc, view[0], view[1], W, H)[0]
        _G[k].setflags(write=False)
    return _G[k]


def chosen_history(G, seed):
    """tests/test_gpu_temporal.py's recipe. A history for the G-buffer G of some view: random colours with some NaN and Inf,
    integer counts in [0, 40] with zeros, and a G-buffer whose ids are overwritten here and there (another row, a miss, a
    row that does not exist)"""
    H, W = G.shape[:2]
    rng = np.random.default_rng(seed)
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = rng.random((H, W, 3), dtype=F) * F(3)
    hist[..., 3] = rng.integers(0, 41, (H, W)).astype(F)
    flat = hist.reshape(-1, 4)
    n = flat.shape[0]
    flat[rng.integers(0, n, max(2, n // 23)), 3] = 0.0
    flat[rng.integers(0, n, max(2, n // 31)), rng.integers(0, 3)] = np.nan
    flat[rng.integers(0, n, max(2, n // 37)), rng.integers(0, 3)] = np.inf
    flat[rng.integers(0, n, max(1, n // 41)), 1] = -np.inf
    g = np.array(G, F)
    gf = g.reshape(-1, 4)
    gf[rng.integers(0, n, max(2, n // 19)), 3] = 1.0
    gf[rng.integers(0, n, max(2, n // 29)), 3] = -1.0
    gf[rng.integers(0, n, max(2, n // 43)), 3] = 7.0
    return hist, g


def chosen_moments(W, H, seed):
    """moments for a history: random first and second moments, counts from {0, 0.5, 3, 4, 40} in blocks, some NaN and Inf"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    levels = np.array([0, 0.5, 3, 4, 40], F)
    mom = np.zeros((H, W, 4), F)
    mom[..., 0] = rng.random((H, W), dtype=F) * F(2)
    mom[..., 1] = mom[..., 0] * mom[..., 0] + rng.random((H, W), dtype=F) * F(0.5)
    mom[..., 2] = levels[((xx // 5) + 2 * (yy // 3)) % 5]
    mf = mom.reshape(-1, 4)
    n = W * H
    mf[rng.integers(0, n, max(2, n // 31)), 0] = np.nan
    mf[rng.integers(0, n, max(2, n // 37)), 1] = np.inf
    return mom


def footprint_ids_differ(GB, GA, D, view_a):
    """mask of the hit pixels of GB none of whose four taps in GA (inside the frame) carries the pixel's row"""
    H, W = GB.shape[:2]
    Gp = tm.previous_position(GB, D)
    u, v, valid = tr.project(Gp, tr.mp32(view_a[0]), W, H)
    with np.errstate(all="ignore"):
        iu, iv = np.floor(u), np.floor(v)
    any_same = np.zeros((H, W), bool)
    for b in (0, 1):
        for a in (0, 1):
            qx, qy = iu + F(a), iv + F(b)
            inside = valid & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
            xi, yi = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
            any_same |= inside & (GA[yi, xi, 3] == GB[..., 3])
    return (GB[..., 3] >= 0) & ~any_same


# ---- 1. reproject with motion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("W,H", [(33, 17), (96, 64)])
def test_reproject_with_motion(gpu, fixtures, W, H, case):
    name, moves, a, b = CASES[case]
    sc = fixtures["scenes"][name]
    sc2 = tm.moved(sc, moves)
    va, vb = case_views(sc, a, b)
    D = tm.motion_table(sc["n"], moves)
    zero = np.zeros_like(D)
    ctx = context(sc, W, H)
    try:
        ga = ctx.gbuffer(va[0], va[1])                    # G_prev from a real G-buffer of view A over the old rows
        GA = np.concatenate([ga["xyz"], ga["id"].astype(F)[..., None]], axis=-1)
        assert same(GA, ref_g(sc, name, W, H, f"v{a}", va))
        GB = ref_g(sc2, case, W, H, f"v{b}", vb)
        on_moved = np.isin(GB[..., 3], [F(r) for r in moves])
        hits = int((GB[..., 3] >= 0).sum())

        hist, gprev = chosen_history(GA, seed=W * 7 + H)  # the hostile history
        ctx.temporal_load_history(hist, gprev, va[0], va[1])
        ctx.move_objects(sc2["objects"], D)
        assert ctx.temporal_pending_motion()["pending"] == 1
        info = ctx.temporal_begin(vb[0], vb[1])
        Rref, found = tm.ref_reproject_moved(GB, gprev, hist, va[0], va[1], D)
        Rstill, found_still = tm.ref_reproject_moved(GB, gprev, hist, va[0], va[1], zero)
        R = ctx.temporal_read(R_MAP)
        print(f"moved reproject {case} {W}x{H}: hit {info['hit_pixels']} (ref {hits}), history {info['history_pixels']} "
              f"(ref {found}; without the motion {found_still}), R words differing {differing(R, Rref)}; the reference "
              f"without the motion differs in {differing(Rref, Rstill)} words")
        assert not np.isnan(Rref).any()                   # every counted tap is finite: raw bits can be compared
        assert same(ctx.temporal_read(G_CUR), GB)         # G_cur is the new rows'
        assert same(ctx.temporal_read(G_PREV), gprev) and same(ctx.temporal_read(HIST), hist)
        assert same(R, Rref) and same(ctx.temporal_read(OUT), Rref)
        assert (info["hit_pixels"], info["history_pixels"], info["nonfinite"], info["k"]) == (hits, found, 0, 0)
        assert differing(Rref, Rstill) > 0 and 0 < found < hits

        # an all-ones history over the true G-buffer: what the motion finds that a still reprojection does not
        ones = np.ones((H, W, 4), F)
        ctx.set_scene_dict(sc)
        ctx.temporal_load_history(ones, GA, va[0], va[1])
        ctx.move_objects(sc2["objects"], D)
        info = ctx.temporal_begin(vb[0], vb[1])
        R1ref, found1 = tm.ref_reproject_moved(GB, GA, ones, va[0], va[1], D)
        R0ref, found0 = tm.ref_reproject_moved(GB, GA, ones, va[0], va[1], zero)
        R1 = ctx.temporal_read(R_MAP)
        assert same(R1, R1ref) and info["history_pixels"] == found1
        words = differing(R1ref, R0ref)
        print(f"  all-ones history: found {found1} with the motion, {found0} without; {words} words differ")
        if (W, H) == (96, 64):
            assert words == DISCRIMINATION[case]
            if case == "C1-sphere":
                assert (found1, found0, hits) == (6054, 5824, 6144)
        for r in moves:                                   # on every moved row more pixels find a history with the motion
            row = GB[..., 3] == F(r)
            with_motion, without = int((R1[..., 3] > 0)[row].sum()), int((R0ref[..., 3] > 0)[row].sum())
            print(f"  row {r}: {with_motion} of {int(row.sum())} pixels find a history, {without} without the motion")
            assert with_motion > without
            if (W, H, case) == (96, 64, "C1-sphere"):
                assert (with_motion, without, int(row.sum())) == (377, 147, 377)
        assert same(R1[~on_moved], R0ref[~on_moved])      # rows that did not move reproject as they always did
        # what the move uncovered: a pixel that now shows a row that did not move, and whose footprint in the old view
        # shows other rows only (the moved object hid it), finds nothing. (Read per pixel instead of per footprint the
        # statement does not hold in the formulas themselves: at the rim of the uncovered region a neighbouring tap of the
        # right row counts with a small weight, 9 of 99 pixels for C1-sphere at 96x64.)
        if a == b:
            uncovered = footprint_ids_differ(GB, GA, D, va) & ~on_moved
            print(f"  uncovered pixels on rows that did not move: {int(uncovered.sum())}")
            assert uncovered.sum() > 0 and not (R1[..., 3] > 0)[uncovered].any() and not R1[uncovered].any()
    finally:
        ctx.close()


# ---- 2. accumulation and clearing -------------------------------------------------------------------------------------------------
def test_two_moves_equal_their_f32_sum(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H = 33, 17
    va = tr.orbit(0)
    d1, d2 = np.array([0.35, 0.1, -0.2], F), np.array([0.25, 0.0, -0.1000001], F)
    total = d1 + d2                                       # the f32 sum, per component
    step1 = tm.moved(sc, {2: d1})
    step2 = tm.moved(step1, {2: d2})
    n = sc["n"]
    GA = ref_g(sc, "C1", W, H, "v0", va)
    hist, gprev = chosen_history(GA, seed=5)
    ctx = context(sc, W, H)
    try:
        idle = ctx.temporal_pending_motion()
        assert idle["pending"] == 0 and idle["hist_cap"] == np.inf and not bits(idle["motion"]).any()
        ctx.temporal_load_history(hist, gprev, *va)
        ctx.move_objects(step1["objects"], tm.motion_table(n, {2: d1}), 8.0)
        p = ctx.temporal_pending_motion()
        assert p["pending"] == 1 and p["hist_cap"] == 8.0 and same(p["motion"], tm.motion_table(n, {2: d1}))
        ctx.move_objects(step2["objects"], tm.motion_table(n, {2: d2}), 3.0)
        ctx.move_objects(step2["objects"], None, 0.0)     # nothing moved, no cap: the sum and the cap stay
        ctx.move_objects(step2["objects"], np.zeros((n, 3), F), 5.0)
        p = ctx.temporal_pending_motion()
        assert p["pending"] == 1 and p["hist_cap"] == 3.0 and same(p["motion"], tm.motion_table(n, {2: total}))
        info = ctx.temporal_begin(*va)
        twice = ctx.temporal_read(R_MAP)
        after = ctx.temporal_pending_motion()
        assert after["pending"] == 0 and after["hist_cap"] == np.inf and not bits(after["motion"]).any()   # +0, not -0

        ctx.set_scene_dict(sc)
        ctx.temporal_load_history(hist, gprev, *va)
        ctx.move_objects(step2["objects"], tm.motion_table(n, {2: total}), 3.0)
        info_once = ctx.temporal_begin(*va)
        once = ctx.temporal_read(R_MAP)
        GB = ref_g(step2, "C1-two-steps", W, H, "v0", va)
        Rref, found = tm.ref_reproject_moved(GB, gprev, hist, va[0], va[1], tm.motion_table(n, {2: total}), 3.0)
        print(f"two moves: history {info['history_pixels']} / one move {info_once['history_pixels']} (ref {found}), words "
              f"differing from the reference {differing(twice, Rref)}")
        assert same(twice, once) and same(twice, Rref) and info["history_pixels"] == info_once["history_pixels"] == found > 0
        assert twice[..., 3].max() == 3.0
    finally:
        ctx.close()


# ---- 3. hist_cap, 5. moments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hist_cap", [0.0, 1.0, 8.0])
def test_hist_cap_and_moments(gpu, fixtures, hist_cap):
    """R.w and MR.z are min(m, mc); hist_cap = 0 leaves m as it is. With tracking on MR and Mout are the reference's bits, and
    after a render and a resolve sail_temporal_filter equals the reference filter over the maps read back"""
    sc = fixtures["scenes"]["C1"]
    W, H, B = 33, 17, 3
    va = tr.orbit(0)
    moves = {2: SPHERE}
    sc2 = tm.moved(sc, moves)
    D = tm.motion_table(sc["n"], moves)
    GA, GB = ref_g(sc, "C1", W, H, "v0", va), ref_g(sc2, "C1-sphere", W, H, "v0", va)
    hist, gprev = chosen_history(GA, seed=W * 7 + H)
    mom = chosen_moments(W, H, seed=3)
    mc = np.inf if hist_cap == 0.0 else hist_cap
    ctx = context(sc, W, H, flags=capi.FLAG_AOV, moments=True)
    try:
        ctx.temporal_load_history(hist, gprev, *va)
        ctx.temporal_load_moments(mom)
        ctx.move_objects(sc2["objects"], D, hist_cap)
        assert same(ctx.temporal_read_moments(M_HIST), mom)          # the move keeps the moment maps
        info = ctx.temporal_begin(*va)
        Rfree, found = tm.ref_reproject_moved(GB, gprev, hist, va[0], va[1], D)
        MRfree = tm.ref_moment_reproject_moved(GB, gprev, mom, va[0], va[1], D)
        Rref, _ = tm.ref_reproject_moved(GB, gprev, hist, va[0], va[1], D, mc)
        MRref = tm.ref_moment_reproject_moved(GB, gprev, mom, va[0], va[1], D, mc)
        R, MR = ctx.temporal_read(R_MAP), ctx.temporal_read_moments(M_R)
        print(f"hist_cap {hist_cap}: history {info['history_pixels']} (ref {found}), moment history "
              f"{int((MRref[..., 2] > 0).sum())}; R words differing {differing(R, Rref)}, MR {differing(MR, MRref)}; counts "
              f"above the cap before it {int((Rfree[..., 3] > mc).sum())} / {int((MRfree[..., 2] > mc).sum())}")
        assert not np.isnan(Rref).any() and not np.isnan(MRref).any()
        assert same(R, Rref) and same(MR, MRref) and same(ctx.temporal_read_moments(M_OUT), MRref)
        assert info["history_pixels"] == found
        assert same(R[..., :3], Rfree[..., :3]) and same(MR[..., :2], MRfree[..., :2])
        assert np.array_equal(R[..., 3], np.minimum(Rfree[..., 3], F(mc)))
        assert np.array_equal(MR[..., 2], np.minimum(MRfree[..., 2], F(mc)))
        assert (Rfree[..., 3] > 8).any() and (MRfree[..., 2] > 8).any() and (MRfree[..., 2] == 0.5).any()
        if hist_cap == 0.0:
            assert same(R, Rfree) and same(MR, MRfree)
        else:
            assert R[..., 3].max() == hist_cap and MR[..., 2].max() == hist_cap
        # the filter over the resolved frame
        with pytest.raises(capi.SailError, match=": -4: .*not resolved"):
            ctx.temporal_filter()
        render(ctx, va, 0, 2, B)
        out = ctx.temporal_resolve()
        S, (_, N, X) = ctx.read_accum(), ctx.readback(aov=True)
        assert same(out["rgba"], tr.ref_resolve(S, Rref)[0])
        Mout = ctx.temporal_read_moments(M_OUT)
        assert same(Mout, tf.ref_moment_resolve(S, MRref))
        c, v, counts = tf.ref_filter(out["rgba"], Mout, S, N, X, k=2)
        got = ctx.temporal_filter(want_var=True)
        print(f"  filter: temporal {got['temporal_pixels']} (ref {counts['temporal']}); colour words differing "
              f"{differing(got['rgba'][..., :3], c)}, variance {differing(got['var'], v)}")
        assert not np.isnan(c).any() and not np.isnan(v).any()
        assert same(got["rgba"][..., :3], c) and same(got["var"], v)
        assert (got["temporal_pixels"], got["spatial_pixels"], got["nonfinite"]) == (counts["temporal"], counts["spatial"], 0)
    finally:
        ctx.close()


# ---- 4. no motion, unchanged rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["null", "zero"])
@pytest.mark.parametrize("W,H", [(33, 17), (96, 64)])
def test_no_motion_is_the_camera_reprojection(gpu, fixtures, W, H, motion):
    sc = fixtures["scenes"]["C1"]
    va, vb = tr.orbit(0), tr.orbit(3)
    GA, GB = ref_g(sc, "C1", W, H, "v0", va), ref_g(sc, "C1", W, H, "v3", vb)
    hist, gprev = chosen_history(GA, seed=W * 7 + H)
    ctx = context(sc, W, H)
    try:
        ctx.temporal_load_history(hist, gprev, *va)
        ctx.move_objects(sc["objects"], None if motion == "null" else np.zeros((sc["n"], 3), F))
        assert ctx.temporal_pending_motion()["pending"] == 1          # the motion kernels run, over a table of +0
        info = ctx.temporal_begin(*vb)
        Rref, found = tr.ref_reproject(GB, gprev, hist, va[0], va[1])
        R = ctx.temporal_read(R_MAP)
        print(f"no motion ({motion}) {W}x{H}: history {info['history_pixels']} (ref {found}), words differing {differing(R, Rref)}")
        assert same(R, Rref) and same(ctx.temporal_read(G_CUR), GB) and info["history_pixels"] == found
    finally:
        ctx.close()


# ---- 6. the frame -----------------------------------------------------------------------------------------------------------------
def test_the_frame_is_update_objects(gpu, fixtures):
    """after move_objects(rows) k samples give the accumulator and AOVs of a context that took sail_update_objects(rows), bit
    for bit, and the noise mark is dropped"""
    sc = fixtures["scenes"]["C3"]
    W, H, B = 33, 17, 3
    va = fixture_view(sc)
    moves = {3: (0.0, 0.5, 0.9), 5: (0.0, 0.6, 0.5)}
    sc2 = tm.moved(sc, moves)

    def run(move):
        ctx = context(sc, W, H, flags=capi.FLAG_AOV)
        try:
            ctx.temporal_begin(*va)
            render(ctx, va, 0, 3, B)
            ctx.noise_mark()
            render(ctx, va, 3, 1, B)
            ctx.temporal_resolve()
            assert ctx.noise_estimate()["k_mark"] == 3
            if move:
                ctx.move_objects(sc2["objects"], tm.motion_table(sc["n"], moves), 8.0)
            else:
                assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(rows_of(sc2)), sc["n"]) == 0
            with pytest.raises(capi.SailError, match="no mark"):
                ctx.noise_estimate()
            assert ctx.save()["k"] == 0 and not ctx.read_accum().any()
            render(ctx, va, 0, 3, B)
            return ctx.read_accum(), ctx.readback(aov=True), int(ctx.stats().samples), ctx.gbuffer(*va)
        finally:
            ctx.close()

    acc0, aov0, samples0, g0 = run(False)
    acc1, aov1, samples1, g1 = run(True)
    assert same(acc0, acc1) and samples0 == samples1 == 3 and acc0.any()
    for x, y in zip(aov0, aov1):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(g0["id"], g1["id"]) and same(g0["xyz"], g1["xyz"])
    assert same(np.concatenate([g1["xyz"], g1["id"].astype(F)[..., None]], axis=-1), ref_g(sc2, "C3-two-spheres", W, H, "vNone", va))


# ---- 7. state rules ---------------------------------------------------------------------------------------------------------------
def test_state_rules(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H, B = 16, 16, 3
    va = tr.orbit(0)
    n = sc["n"]
    moves = {2: SPHERE}
    sc2 = tm.moved(sc, moves)
    D = tm.motion_table(n, moves)
    bare = capi.Context(W, H)
    try:
        with pytest.raises(capi.SailError, match=": -4: .*before sail_set_scene"):
            bare.move_objects(sc2["objects"], D)
    finally:
        bare.close()
    ctx = context(sc, W, H, flags=capi.FLAG_AOV, moments=True)
    try:
        # no temporal state at all: exactly sail_update_objects
        ctx.move_objects(sc2["objects"], D, 8.0)
        assert ctx.temporal_pending_motion()["pending"] == 0
        assert ctx.temporal_begin(*va)["history_pixels"] == 0
        ctx.set_scene_dict(sc)

        ctx.temporal_begin(*va)
        render(ctx, va, 0, 2, B)
        out = ctx.temporal_resolve()["rgba"]
        acc = ctx.read_accum()
        g_old = ctx.gbuffer(*va)

        def bad_motion(v):
            m = D.copy()
            m[1, 2] = v
            return m
        refused = [(sc2["objects"], bad_motion(np.nan), 0.0), (sc2["objects"], bad_motion(np.inf), 0.0),
                   (sc2["objects"], bad_motion(-np.inf), 8.0), (sc2["objects"], D, 0.5), (sc2["objects"], D, float("nan")),
                   (sc2["objects"], D, float("inf")), (sc2["objects"], D, -1.0)]
        for rows, motion, cap in refused:
            with pytest.raises(capi.SailError, match=": -1: .*sail_move_objects"):
                ctx.move_objects(rows, motion, cap)
        r2 = rows_of(sc2)
        assert ctx.lib.sail_move_objects(ctx.h, capi._ptr(r2), n - 1, capi._ptr(D), 0.0) == -1      # a wrong n
        assert ctx.lib.sail_move_objects(ctx.h, None, n, capi._ptr(D), 0.0) == -1
        # a refused call leaves the rows, the accumulator and the temporal state as they were
        g_now = ctx.gbuffer(*va)
        assert np.array_equal(g_now["id"], g_old["id"]) and same(g_now["xyz"], g_old["xyz"])
        assert same(ctx.read_accum(), acc) and ctx.save()["k"] == 2
        assert same(ctx.temporal_read(OUT), out) and ctx.temporal_pending_motion()["pending"] == 0
        ctx.temporal_filter()                              # still resolved

        def pending():
            return ctx.temporal_pending_motion()["pending"]

        def establish():
            """a current view over the old rows, then a move: something is pending"""
            ctx.set_scene_dict(sc)
            ctx.temporal_begin(*va)
            render(ctx, va, 0, 1, B)
            ctx.temporal_resolve()
            ctx.move_objects(sc2["objects"], D, 8.0)
            assert pending() == 1

        # the move restarts the accumulator: the view is no longer resolved for the filter, but it is still current
        establish()
        assert ctx.save()["k"] == 0
        with pytest.raises(capi.SailError, match=": -4: .*not resolved"):
            ctx.temporal_filter()
        assert ctx.temporal_read(OUT)[..., 3].max() == 1.0 and ctx.temporal_read_moments(M_OUT).any()
        # reset, load_accum, set_accum_mode and set_partition keep what is pending
        keep = [lambda: ctx.reset(), lambda: ctx.load({"k": 2, "parts": [np.ones((H, W, 4), F)]}),
                lambda: ctx.set_accum_mode(capi.ACCUM_MIX), lambda: ctx.set_accum_mode(capi.ACCUM_SUM),
                lambda: ctx.set_partition(0, 1, capi.PART_TILES)]
        for op in keep:
            op()
            assert pending() == 1
        # a begin that fails keeps it; one that succeeds consumes it
        with pytest.raises(capi.SailError, match=": -1: .*singular"):
            ctx.temporal_begin(np.zeros(16), va[1])
        assert pending() == 1
        assert ctx.temporal_begin(*va)["history_pixels"] > 0
        assert pending() == 0
        # set_scene, update_objects and load_history clear it
        establish()
        ctx.set_scene_dict(sc)
        assert pending() == 0
        establish()
        assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(r2), n) == 0
        assert pending() == 0 and ctx.temporal_begin(*va)["history_pixels"] == 0
        establish()
        ctx.temporal_load_history(np.ones((H, W, 4), F), np.zeros((H, W, 4), F), *va)
        assert pending() == 0
    finally:
        ctx.close()


# ---- 8. a drag chain --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 17), (48, 32)])
def test_drag_chain(gpu, fixtures, W, H):
    """begin(A), 4 spp, resolve; three times: move, begin(A), 1 spp, resolve. Every map along the way equals the reference
    pipeline fed with the accumulators read back; the counts grow 4, 5, 6, 7 where a history is found (hist_cap 0)"""
    sc = fixtures["scenes"]["C1"]
    B = 3
    va = tr.orbit(0)
    n = sc["n"]
    steps = [(0.2, 0.0, -0.1), (0.25, 0.05, -0.1), (0.15, 0.05, -0.1)]
    zero = np.zeros((H, W, 4), F)
    ctx = context(sc, W, H)
    try:
        ctx.temporal_begin(*va)
        render(ctx, va, 0, 4, B)
        prev_out, _, _ = tr.ref_resolve(ctx.read_accum(), zero)
        assert same(ctx.temporal_resolve()["rgba"], prev_out)
        prev_g, cur = ref_g(sc, "C1", W, H, "v0", va), sc
        for i, d in enumerate(steps):
            cur = tm.moved(cur, {2: d})
            D = tm.motion_table(n, {2: d})
            ctx.move_objects(cur["objects"], D)
            info = ctx.temporal_begin(*va)
            G = ref_g(cur, f"C1-chain{i}", W, H, "v0", va)
            Rref, found = tm.ref_reproject_moved(G, prev_g, prev_out, va[0], va[1], D)
            assert same(ctx.temporal_read(HIST), prev_out) and same(ctx.temporal_read(G_PREV), prev_g)
            assert same(ctx.temporal_read(G_CUR), G) and same(ctx.temporal_read(R_MAP), Rref)
            assert info["history_pixels"] == found > 0 and info["k"] == 0
            sphere = G[..., 3] == F(2)
            assert (Rref[..., 3] > 0)[sphere].sum() > 0.9 * sphere.sum()      # the dragged sphere keeps its history
            render(ctx, va, 0, 1, B)
            out, nhist, bad = tr.ref_resolve(ctx.read_accum(), Rref)
            got = ctx.temporal_resolve()
            print(f"drag chain {W}x{H} step {i}: history {found}, on the sphere {int((Rref[..., 3] > 0)[sphere].sum())} of "
                  f"{int(sphere.sum())}; resolved words differing {differing(got['rgba'], out)}, largest count {out[..., 3].max()}")
            assert same(got["rgba"], out) and (got["history_pixels"], got["nonfinite"]) == (nhist, bad)
            assert out[..., 3].max() == 4 + (i + 1) and out[..., 3].min() >= 1
            assert out[..., 3][sphere].max() == 4 + (i + 1)
            prev_out, prev_g = out, G
    finally:
        ctx.close()


# ---- 9. multi-device --------------------------------------------------------------------------------------------------------------
def moved_views(ctx, sc, sc2, D, va, B):
    """begin(A), 4 spp, resolve, move, begin(A), 1 spp, resolve; every map and count on the way"""
    seen = [ctx.temporal_begin(*va)]
    render(ctx, va, 0, 4, B)
    seen.append(ctx.temporal_resolve(want_u8=True))
    ctx.move_objects(sc2["objects"], D, 8.0)
    pend = ctx.temporal_pending_motion()
    seen.append(ctx.temporal_begin(*va))
    maps = [ctx.temporal_read(w) for w in (G_CUR, G_PREV, HIST, R_MAP, OUT)] + [pend["motion"]]
    render(ctx, va, 0, 1, B)
    seen.append(ctx.temporal_resolve(want_u8=True))
    maps.append(ctx.temporal_read(OUT))
    return seen, maps, pend


@pytest.mark.parametrize("devices,dbg", [([0, 0, 0], None), ([0], {capi.DEBUG_FORCE_RCCL: 1})])
def test_multi_device_equals_one_device(gpu, fixtures, devices, dbg):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 150, 70, 3
    va = fixture_view(sc)
    moves = {3: (0.0, 0.5, 0.9), 5: (0.0, 0.6, 0.5)}
    sc2 = tm.moved(sc, moves)
    D = tm.motion_table(sc["n"], moves)
    one = context(sc, W, H)
    try:
        want, want_maps, _ = moved_views(one, sc, sc2, D, va, B)
    finally:
        one.close()
    ctx = context(sc, W, H, devices=devices)
    try:
        for opt, val in (dbg or {}).items():
            ctx.set_debug(opt, val)
        got, got_maps, pend = moved_views(ctx, sc, sc2, D, va, B)
        after = ctx.temporal_pending_motion()
    finally:
        ctx.close()
    assert (pend["pending"], pend["hist_cap"]) == (1, 8.0) and same(pend["motion"], D) and after["pending"] == 0
    for x, y in zip(got_maps, want_maps):
        assert same(x, y)
    for x, y in zip(got, want):
        for f in ("k", "hit_pixels", "history_pixels", "nonfinite"):
            assert x[f] == y[f]
        if "rgba" in x:
            assert same(x["rgba"], y["rgba"]) and np.array_equal(x["u8"], y["u8"])
    assert want[2]["history_pixels"] > 0 and want_maps[3][..., 3].max() == 4.0      # min(4 spp, hist_cap 8)


# ---- 10. quality ------------------------------------------------------------------------------------------------------------------
def rel_mse(x, ref):
    """tests/test_gpu_temporal.py's definition"""
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


# 1.5 x the ratio measured on an MI355X, 0.1004 ("Keeping the history across a drag"): the margin covers
# sample-index sensitivity, as for the camera-motion bound; never above 0.5
QUALITY_BOUND = min(1.5 * 0.1004, 0.5)


def test_quality_after_a_drag(gpu, fixtures):
    """C3 at 96x64 with 5 bounces from its fixture view: 64 spp resolved, the matte sphere (row 5) dragged by (0, 0.6, 0.5)
    with hist_cap 8, 1 spp, resolved: relMSE against 512 spp of the moved scene over other sample indices, as a ratio to the
    bare 1-spp mean's, which is what a drag shows without the motion. Measured on an MI355X: relMSE 0.915242 for the 1-spp
    mean, 0.0918623 resolved, ratio 0.1004; 6078 of the 6144 hit pixels find a history."""
    sc = fixtures["scenes"]["C3"]
    W, H, B = 96, 64, 5
    va = fixture_view(sc)
    moves = {5: (0.0, 0.6, 0.5)}
    sc2 = tm.moved(sc, moves)
    D = tm.motion_table(sc["n"], moves)
    ref_ctx = context(sc2, W, H)
    try:
        render(ref_ctx, va, 1, 512, B)
        ref = ref_ctx.readback()[..., :3]
    finally:
        ref_ctx.close()
    ctx = context(sc, W, H)
    try:
        ctx.temporal_begin(*va)
        render(ctx, va, 0, 64, B)
        ctx.temporal_resolve()
        ctx.move_objects(sc2["objects"], D, 8.0)
        info = ctx.temporal_begin(*va)
        render(ctx, va, 0, 1, B)
        noisy = ctx.readback()[..., :3]
        out = ctx.temporal_resolve()
    finally:
        ctx.close()
    # the conditions on the input: the reprojection finds most of the picture, on the device as in the reference
    GA, GB = ref_g(sc, "C3", W, H, "vNone", va), ref_g(sc2, "C3-matte", W, H, "vNone", va)
    found = tm.ref_reproject_moved(GB, GA, np.ones((H, W, 4), F), va[0], va[1], D)[1]
    share = info["history_pixels"] / info["hit_pixels"]
    print(f"quality: history {info['history_pixels']} of {info['hit_pixels']} hit pixels ({share:.4f}; reference {found})")
    assert info["history_pixels"] == found and share >= 0.8
    assert (found, info["hit_pixels"]) == (6078, 6144)
    assert np.isfinite(ref).all() and np.isfinite(noisy).all() and out["nonfinite"] == 0
    assert out["rgba"][..., 3].max() == 8.0 + 1.0          # hist_cap 8 and the new sample
    e_in, e_out = rel_mse(noisy, ref), rel_mse(out["rgba"][..., :3], ref)
    print(f"quality C3 {W}x{H}, {B} bounces, row 5 dragged by {moves[5]}, reference 512 spp: relMSE of the 1-spp mean "
          f"{e_in:.6g}, resolved {e_out:.6g}, ratio {e_out / e_in:.4f} (required <= {QUALITY_BOUND})")
    assert e_out / e_in <= QUALITY_BOUND
