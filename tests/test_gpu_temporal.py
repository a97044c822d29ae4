"""Camera-motion reprojection (sail_gbuffer_kernel, sail_reproject_kernel and sail_temporal_resolve_kernel behind
sail_gbuffer / sail_temporal_begin / sail_temporal_resolve). Needs a GPU.

The reference is tests/temporal_ref.py: the formulas of include/sail_hip.h in numpy float32, one operation at a time, with
the first hits from oracle.pick. Every operation is an IEEE f32 one, so the device's maps must equal it bit for bit: raw
uint32 bits are compared, with no NaN-equals-NaN shortcut. The quality test compares with a separate, far longer render of
the same view over other sample indices, never with the code under test."""
import numpy as np
import pytest

import oracle
import temporal_ref as tr
from sail_amd import capi
from temporal_ref import bits

pytestmark = pytest.mark.gpu

F = np.float32
G_CUR, G_PREV, HIST, R_MAP, OUT = (capi.TEMPORAL_G_CUR, capi.TEMPORAL_G_PREV, capi.TEMPORAL_HIST, capi.TEMPORAL_R,
                                   capi.TEMPORAL_OUT)
DISPLAYS = [(capi.FILTER_COLOR, 2.2), (capi.FILTER_GAMMA, 2.2), (capi.FILTER_GAMMA, 1.8), (capi.FILTER_TONEMAPPING, 2.2)]


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def context(sc, W, H, flags=0, **kw):
    ctx = capi.Context(W, H, flags=flags, **kw)
    ctx.set_scene_dict(sc)
    return ctx


def render(ctx, view, k0, spp, B):
    inv, seeds = capi.schedule(view[0], ctx.W, ctx.H, k0, spp)
    ctx.render_schedule(inv, seeds, view[1], B)


def fixture_view(sc):
    return np.array(sc["mvp_rowmajor"], np.float64).reshape(16), np.asarray(sc["eye"], F)


# the reference's G-buffers (oracle.pick), computed once per (scene, size, view) and never changed
_G = {}


def ref_g(fixtures, name, W, H, key, view):
    k = (name, W, H, key)
    if k not in _G:
        _G[k] = tr.ref_gbuffer(fixtures["scenes"][name], view[0], view[1], W, H)
        for a in _G[k]:
            a.setflags(write=False)
    return _G[k]


# ---- 1. G-buffer ------------------------------------------------------------------------------------------------------------
def gbuffer_views(sc, name):
    if name == "C4":   # an open scene: its own camera and a second eye among the objects
        return {"fixture": fixture_view(sc), "inside": tr.view((4.0, 5.5, 1.0), (5.5, 4.5, 6.0))}
    # the room scenes: their camera, an eye inside the room, and an orbit far enough round that some pixels miss
    return {"fixture": fixture_view(sc), "inside": tr.view(*tr.INSIDE), "orbit25": tr.orbit(25)}


def check_gbuffer(fixtures, name, W, H):
    sc = fixtures["scenes"][name]
    ctx = context(sc, W, H, flags=capi.FLAG_AOV)
    try:
        for key, view in gbuffer_views(sc, name).items():
            G, rays, idx, t = ref_g(fixtures, name, W, H, key, view)
            got = ctx.gbuffer(view[0], view[1], rays=True)
            pid, pt = ctx.pick(got["rays"].reshape(-1, 6))
            print(f"{name} {W}x{H} {key}: hits {int((idx >= 0).sum())} of {idx.size}, rows {np.unique(idx).tolist()[:8]}, "
                  f"rays differing {differing(got['rays'], rays)}, t differing {differing(got['t'], t)}")
            assert same(got["rays"], rays)
            assert np.array_equal(got["id"], idx) and same(got["t"], t)                       # oracle.pick
            assert np.array_equal(got["id"].reshape(-1), pid) and same(got["t"].reshape(-1), pt)  # sail_pick
            assert same(got["xyz"], tr.ref_xyz(rays, idx, t)) and same(got["xyz"], G[..., :3])
            assert (got["t"][idx < 0] == F(1e5)).all()
            # one sample without jitter: the pixels that miss are exactly those whose position AOV is NaN
            ctx.reset()
            inv = capi.jitter_inverse(view[0], 0.0, 0.0, W, H)
            ctx.render_schedule(inv[None, :], np.array([0.25], F), view[1], 2)
            _, _, X = ctx.readback(aov=True)
            assert np.array_equal(np.isnan(X[..., :3]).any(axis=-1), got["id"] < 0)
        if name != "C4" and (W, H) != (1, 1):
            miss = int((ref_g(fixtures, name, W, H, "orbit25", None)[2] < 0).sum())
            assert 0 < miss < W * H
    finally:
        ctx.close()


@pytest.mark.parametrize("W,H", [(33, 17), (48, 32)])
@pytest.mark.parametrize("name", ["C1", "C3", "C4"])
def test_gbuffer(gpu, fixtures, name, W, H):
    check_gbuffer(fixtures, name, W, H)


def test_gbuffer_of_one_pixel(gpu, fixtures):
    check_gbuffer(fixtures, "C1", 1, 1)


# ---- 2. reproject -----------------------------------------------------------------------------------------------------------
def chosen_history(G, seed):
    """a history for the G-buffer G of some view: random colours with some NaN and Inf, integer counts in [0, 40] with
    zeros, and a G-buffer whose ids are overwritten here and there (another row, a miss, a row that does not exist)"""
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


REPROJECT_CASES = {
    # name: (view A of the history, the new view)
    "orbit3": (lambda: tr.orbit(0), lambda: tr.orbit(3)),
    "orbit25": (lambda: tr.orbit(0), lambda: tr.orbit(25)),
    # the history was seen from inside the room: from outside, the room's front lies behind that camera and most of the
    # rest outside its frame
    "behind": (lambda: tr.view(*tr.INSIDE), lambda: tr.orbit(0)),
}


@pytest.mark.parametrize("pos_tol", [None, 0.005], ids=["tol-default", "tol-0.005"])
@pytest.mark.parametrize("case", list(REPROJECT_CASES))
@pytest.mark.parametrize("W,H", [(33, 17), (96, 64)])
def test_reproject(gpu, fixtures, W, H, case, pos_tol):
    sc = fixtures["scenes"]["C1"]
    va, vb = (f() for f in REPROJECT_CASES[case])
    ctx = context(sc, W, H)
    try:
        ga = ctx.gbuffer(va[0], va[1])                    # G_prev from a real G-buffer of view A
        GA = np.concatenate([ga["xyz"], ga["id"].astype(F)[..., None]], axis=-1)
        assert same(GA, ref_g(fixtures, "C1", W, H, case + "A", va)[0])
        hist, gprev = chosen_history(GA, seed=W * 7 + H)
        ctx.temporal_load_history(hist, gprev, va[0], va[1])
        assert same(ctx.temporal_read(HIST), hist) and same(ctx.temporal_read(G_PREV), gprev)
        info = ctx.temporal_begin(vb[0], vb[1], None if pos_tol is None else {"pos_tol": pos_tol})
        GB = ref_g(fixtures, "C1", W, H, case + "B", vb)[0]
        Rref, found = tr.ref_reproject(GB, gprev, hist, va[0], va[1], 0.05 if pos_tol is None else pos_tol)
        R = ctx.temporal_read(R_MAP)
        hits = int((GB[..., 3] >= 0).sum())
        print(f"reproject {case} {W}x{H} tol {pos_tol}: hit {info['hit_pixels']} (ref {hits}), history "
              f"{info['history_pixels']} (ref {found}), R channels differing {differing(R, Rref)}")
        assert not np.isnan(Rref).any()                   # every counted tap is finite: raw bits can be compared
        assert same(ctx.temporal_read(G_CUR), GB)
        assert same(R, Rref) and same(ctx.temporal_read(OUT), Rref)
        assert (info["hit_pixels"], info["history_pixels"], info["nonfinite"], info["k"]) == (hits, found, 0, 0)
        assert 0 < found < hits                           # some pixels find a history and some do not
        if case == "behind":
            u, v, valid = tr.project(GB, tr.mp32(va[0]), W, H)
            behind = int(((GB[..., 3] >= 0) & ~valid).sum())
            outside = int((valid & ((u < -1) | (u > W) | (v < -1) | (v > H))).sum())
            print(f"  behind the previous camera {behind}, outside its frame {outside}")
            assert behind > 0 and outside > 0
    finally:
        ctx.close()


def test_tighter_tolerance_finds_less(gpu, fixtures):
    """the two tolerances are different cases, not one: at a 25 degree orbit the tight one rejects taps the default takes"""
    sc = fixtures["scenes"]["C1"]
    W, H = 96, 64
    va, vb = tr.orbit(0), tr.orbit(25)
    GA, GB = ref_g(fixtures, "C1", W, H, "orbit25A", va)[0], ref_g(fixtures, "C1", W, H, "orbit25B", vb)[0]
    hist = np.ones((H, W, 4), F)
    wide = tr.ref_reproject(GB, GA, hist, va[0], va[1], 0.05)[1]
    tight = tr.ref_reproject(GB, GA, hist, va[0], va[1], 0.005)[1]
    ctx = context(sc, W, H)
    try:
        ctx.temporal_load_history(hist, GA, va[0], va[1])
        got_wide = ctx.temporal_begin(vb[0], vb[1])["history_pixels"]
        ctx.temporal_load_history(hist, GA, va[0], va[1])
        got_tight = ctx.temporal_begin(vb[0], vb[1], {"pos_tol": 0.005})["history_pixels"]
    finally:
        ctx.close()
    print(f"history pixels at 25 degrees: tol 0.05 {got_wide}, tol 0.005 {got_tight}")
    assert (got_wide, got_tight) == (wide, tight) and tight < wide


# ---- 3. resolve -------------------------------------------------------------------------------------------------------------
def chosen_accum(W, H, mix, seed):
    """an accumulator to load: SUM: sums with per-pixel counts from {0, 1, 5, 1000}; MIX: running means. One NaN pixel, one
    Inf pixel."""
    rng = np.random.default_rng(seed)
    S = np.zeros((H, W, 4), F)
    mean = rng.random((H, W, 3), dtype=F) * F(2)
    if mix:
        S[..., :3] = mean
        S[..., 3] = 1.0
    else:
        cnt = rng.choice(np.array([0, 1, 5, 1000], F), (H, W))
        S[..., :3] = mean * cnt[..., None]
        S[..., 3] = cnt
    flat = S.reshape(-1, 4)
    flat[5, 1] = np.nan
    flat[W + 3, 0] = np.inf
    if not mix:
        flat[5, 3] = 5.0
        flat[W + 3, 3] = 1.0
    return S


@pytest.mark.parametrize("mix,k", [(False, 1000), (True, 0), (True, 1), (True, 5), (True, 1000)],
                         ids=["sum", "mix-0", "mix-1", "mix-5", "mix-1000"])
def test_resolve(gpu, fixtures, mix, k):
    sc = fixtures["scenes"]["C1"]
    W, H = 33, 17
    va = tr.orbit(0)
    GA = ref_g(fixtures, "C1", W, H, "orbit3A", va)[0]
    hist, gprev = chosen_history(GA, seed=99)
    hist[0:2, 4:7, 3] = 0.0                               # no history round the NaN pixel: its NaN goes straight through
    S = chosen_accum(W, H, mix, seed=k + 3)
    ctx = context(sc, W, H)
    try:
        if mix:
            ctx.set_accum_mode(capi.ACCUM_MIX)
        ctx.temporal_load_history(hist, gprev, va[0], va[1])
        ctx.temporal_begin(va[0], va[1])                  # the same view: R is the history where it is usable
        R = ctx.temporal_read(R_MAP)
        assert same(R, tr.ref_reproject(GA, gprev, hist, va[0], va[1])[0])
        ctx.load({"k": k, "parts": [S]})
        assert same(ctx.read_accum(), S)
        for cap in (1.0, 8.0, 32.0):
            for kind, gamma_c in DISPLAYS:
                out = ctx.temporal_resolve({"cap": cap, "display": kind, "gamma_c": gamma_c}, want_u8=True)
                want, nhist, bad = tr.ref_resolve(S, R, mix=mix, k=k, cap=cap)
                nan = np.isnan(want)
                if cap == 32.0 and kind == capi.FILTER_COLOR:
                    print(f"resolve mix {mix} k {k}: history {out['history_pixels']} (ref {nhist}), nonfinite "
                          f"{out['nonfinite']} (ref {bad}), NaN channels in the reference {int(nan.sum())}, channels "
                          f"differing {differing(out['rgba'], want)}")
                # raw bits everywhere, the NaN pixel included: its NaN is the accumulator's quiet NaN copied (MIX) or
                # divided by its count (SUM), and an IEEE divide hands a quiet NaN operand through as it is
                assert nan.sum() == 1 and (bits(want)[nan] == 0x7FC00000).all()
                assert same(out["rgba"], want)
                assert same(ctx.temporal_read(OUT), out["rgba"])
                assert (out["history_pixels"], out["nonfinite"], out["k"]) == (nhist, bad, k)
                assert bad == 2 and 0 < nhist < W * H
                u8 = tr.quantise(tr.display(want[..., :3], kind, gamma_c))
                assert np.array_equal(out["u8"][..., :3], u8) and (out["u8"][..., 3] == 255).all()
        assert same(ctx.temporal_read(R_MAP), R)          # resolving again blends from the same R
    finally:
        ctx.close()


@pytest.mark.parametrize("W,H", [(33, 17), (64, 32)])
def test_resolve_without_history_is_the_display_filter(gpu, fixtures, W, H):
    sc = fixtures["scenes"]["C1"]
    va = tr.orbit(0)
    ctx = context(sc, W, H)
    try:
        info = ctx.temporal_begin(va[0], va[1])
        assert info["history_pixels"] == 0 and not ctx.temporal_read(R_MAP).any()
        render(ctx, va, 0, 4, 3)
        S = ctx.read_accum()
        for kind, gamma_c in DISPLAYS:
            out = ctx.temporal_resolve({"display": kind, "gamma_c": gamma_c}, want_u8=True)
            _, f8 = ctx.filter(kind, gamma_c=gamma_c, want_u8=True)
            print(f"no history {W}x{H} kind {kind} gamma {gamma_c}: bytes differing from sail_filter "
                  f"{int((out['u8'] != f8).sum())}")
            assert np.array_equal(out["u8"], f8)
            assert same(out["rgba"], tr.ref_resolve(S, np.zeros_like(S))[0]) and out["history_pixels"] == 0
    finally:
        ctx.close()


# ---- 4. a chain of views ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 17), (48, 32)])
def test_chain(gpu, fixtures, W, H):
    """begin(A), 4 spp, resolve, reset, begin(B), 1 spp, resolve, begin(C) with no resolve, begin(D), 1 spp, resolve:
    every map along the way equals the reference pipeline fed with the accumulators read back"""
    sc = fixtures["scenes"]["C1"]
    views = {"A": tr.orbit(0), "B": tr.orbit(3), "C": tr.orbit(10), "D": tr.orbit(6, height=0.4)}
    G = {n: ref_g(fixtures, "C1", W, H, "chain" + n, v)[0] for n, v in views.items()}
    zero = np.zeros((H, W, 4), F)
    ctx = context(sc, W, H)
    try:
        a = ctx.temporal_begin(*views["A"])
        assert (a["hit_pixels"], a["history_pixels"]) == (int((G["A"][..., 3] >= 0).sum()), 0)
        assert same(ctx.temporal_read(G_CUR), G["A"]) and same(ctx.temporal_read(R_MAP), zero)
        assert same(ctx.temporal_read(OUT), zero)
        render(ctx, views["A"], 0, 4, 3)
        out_a, _, _ = tr.ref_resolve(ctx.read_accum(), zero)
        assert same(ctx.temporal_resolve()["rgba"], out_a)

        ctx.reset()
        b = ctx.temporal_begin(*views["B"])
        r_b, found_b = tr.ref_reproject(G["B"], G["A"], out_a, *views["A"])
        assert same(ctx.temporal_read(HIST), out_a) and same(ctx.temporal_read(G_PREV), G["A"])
        assert same(ctx.temporal_read(G_CUR), G["B"]) and same(ctx.temporal_read(R_MAP), r_b)
        assert b["history_pixels"] == found_b > 0
        render(ctx, views["B"], 0, 1, 3)
        out_b, _, _ = tr.ref_resolve(ctx.read_accum(), r_b)
        got_b = ctx.temporal_resolve()
        assert same(got_b["rgba"], out_b) and got_b["history_pixels"] == found_b

        ctx.reset()
        c = ctx.temporal_begin(*views["C"])              # B is committed, C is never resolved
        r_c, found_c = tr.ref_reproject(G["C"], G["B"], out_b, *views["B"])
        assert same(ctx.temporal_read(HIST), out_b) and same(ctx.temporal_read(G_PREV), G["B"])
        assert same(ctx.temporal_read(R_MAP), r_c) and same(ctx.temporal_read(OUT), r_c)
        assert c["history_pixels"] == found_c > 0

        d = ctx.temporal_begin(*views["D"])              # C hands the history through: Hist = R_C
        r_d, found_d = tr.ref_reproject(G["D"], G["C"], r_c, *views["C"])
        assert same(ctx.temporal_read(HIST), r_c) and same(ctx.temporal_read(G_PREV), G["C"])
        assert same(ctx.temporal_read(G_CUR), G["D"]) and same(ctx.temporal_read(R_MAP), r_d)
        assert d["history_pixels"] == found_d > 0
        render(ctx, views["D"], 0, 1, 3)
        out_d, nhist, bad = tr.ref_resolve(ctx.read_accum(), r_d)
        got_d = ctx.temporal_resolve(want_u8=True)
        print(f"chain {W}x{H}: history pixels B {found_b}, C {found_c}, D {found_d}; final channels differing "
              f"{differing(got_d['rgba'], out_d)}")
        assert same(got_d["rgba"], out_d) and (got_d["history_pixels"], got_d["nonfinite"]) == (nhist, bad)
        assert np.array_equal(got_d["u8"][..., :3], tr.quantise(out_d[..., :3]))
        # the counts grow along the chain where the history was found, capped at 32
        assert out_d[..., 3].max() == 4 + 1 + 1 and out_d[..., 3].min() >= 1
    finally:
        ctx.close()


# ---- 5. no side effects -----------------------------------------------------------------------------------------------------
def test_changes_nothing(gpu, fixtures):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 33, 17, 3
    va, vb = fixture_view(sc), tr.orbit(4)

    def run(temporal):
        ctx = context(sc, W, H, flags=capi.FLAG_AOV)
        try:
            if temporal:
                ctx.temporal_begin(*va)
            render(ctx, va, 0, 3, B)
            ctx.noise_mark()
            if temporal:
                ctx.temporal_resolve(want_u8=True)
                ctx.gbuffer(*vb, rays=True)
            render(ctx, va, 3, 2, B)
            if temporal:
                ctx.temporal_begin(*vb)
                ctx.temporal_resolve()
                ctx.temporal_read(OUT)
                ctx.temporal_load_history(np.ones((H, W, 4), F), np.zeros((H, W, 4), F), *va)
                ctx.temporal_begin(*va)
            seen = (ctx.read_accum(), ctx.readback(aov=True), ctx.noise_estimate(pixels=True), int(ctx.stats().samples),
                    ctx.save()["k"])
            render(ctx, va, 5, 4, B)
            return seen, ctx.read_accum()
        finally:
            ctx.close()

    (acc0, aov0, noise0, samples0, k0), next0 = run(False)
    (acc1, aov1, noise1, samples1, k1), next1 = run(True)
    assert same(acc0, acc1) and same(next0, next1)
    for a, b in zip(aov0, aov1):
        assert np.array_equal(bits(a), bits(b))
    for f in ("mean", "max_tile", "k", "k_mark", "nonfinite"):
        assert noise0[f] == noise1[f]
    assert same(noise0["pixel_err"], noise1["pixel_err"])
    assert samples0 == samples1 == 5 and k0 == k1 == 5


# ---- 6. state rules ---------------------------------------------------------------------------------------------------------
BAD_PARAMS = [{"cap": float("nan")}, {"cap": float("inf")}, {"cap": 0.5}, {"pos_tol": 0.0}, {"pos_tol": -1.0},
              {"pos_tol": float("nan")}, {"pos_tol": float("inf")}, {"display": capi.FILTER_WINDOW}, {"display": -1}]


def test_state_rules(gpu, fixtures):
    sc = fixtures["scenes"]["C1"]
    W, H, B = 16, 16, 3
    va, vb = tr.orbit(0), tr.orbit(3)
    bare = capi.Context(W, H)
    try:
        for bad in BAD_PARAMS:                            # bad parameters are refused before anything else
            with pytest.raises(capi.SailError, match=": -1: .*bad parameters"):
                bare.temporal_begin(*va, bad)
            with pytest.raises(capi.SailError, match=": -1: .*bad parameters"):
                bare.temporal_resolve(bad)
        for call in (lambda: bare.temporal_begin(*va), lambda: bare.temporal_resolve(), lambda: bare.gbuffer(*va)):
            with pytest.raises(capi.SailError, match=": -4: .*no scene"):
                call()
        with pytest.raises(capi.SailError, match=": -4: "):
            bare.temporal_read(R_MAP)
    finally:
        bare.close()
    ctx = context(sc, W, H)
    try:
        with pytest.raises(capi.SailError, match=": -4: .*no current view"):
            ctx.temporal_resolve()
        with pytest.raises(capi.SailError, match=": -1: .*singular"):
            ctx.temporal_begin(np.zeros(16), va[1])
        assert ctx.temporal_begin(*va)["history_pixels"] == 0
        with pytest.raises(capi.SailError, match=": -4: .*committed"):
            ctx.temporal_read(HIST)
        render(ctx, va, 0, 2, B)
        ctx.temporal_resolve()

        # reset, load_accum, set_accum_mode and set_partition keep the history
        keep = [lambda: ctx.reset(), lambda: ctx.load({"k": 2, "parts": [np.ones((H, W, 4), F)]}),
                lambda: ctx.set_accum_mode(capi.ACCUM_MIX), lambda: ctx.set_partition(0, 1, capi.PART_TILES)]
        for i, op in enumerate(keep):
            op()
            info = ctx.temporal_begin(*(vb if i % 2 == 0 else va))
            assert info["history_pixels"] > 0, i
            render(ctx, vb if i % 2 == 0 else va, 0, 1, B)
            ctx.temporal_resolve()
        ctx.set_accum_mode(capi.ACCUM_SUM)

        # update_objects and set_scene drop it
        assert ctx.lib.sail_update_objects(ctx.h, capi._ptr(capi._f32(sc["objects"])), sc["n"]) == 0
        with pytest.raises(capi.SailError, match=": -4: .*no current view"):
            ctx.temporal_resolve()
        assert ctx.temporal_begin(*vb)["history_pixels"] == 0
        render(ctx, vb, 0, 1, B)
        ctx.temporal_resolve()
        assert ctx.temporal_begin(*va)["history_pixels"] > 0
        ctx.set_scene_dict(sc)
        with pytest.raises(capi.SailError, match=": -4: .*no current view"):
            ctx.temporal_resolve()
        with pytest.raises(capi.SailError, match=": -4: "):
            ctx.temporal_read(G_CUR)
        assert ctx.temporal_begin(*vb)["history_pixels"] == 0

        for bad in BAD_PARAMS:
            with pytest.raises(capi.SailError, match=": -1: .*bad parameters"):
                ctx.temporal_resolve(bad)
        with pytest.raises(capi.SailError, match=": -1: "):
            ctx.temporal_read(5)
        ctx.set_accum_mode(capi.ACCUM_COMPAT8)
        with pytest.raises(capi.SailError, match=": -4: .*COMPAT8"):
            ctx.temporal_begin(*va)
        with pytest.raises(capi.SailError, match=": -4: .*COMPAT8"):
            ctx.temporal_resolve()
    finally:
        ctx.close()
    multi = context(sc, W, H, devices=[0, 0])
    try:
        multi.temporal_begin(*va)
        render(multi, va, 0, 2, B)
        assert multi.temporal_resolve()["k"] == 2
        half = capi.plan_keep(W, H, 0, 2, capi.PART_TILES, multi.read_accum())
        assert multi.lib.sail_load_accum(multi.h, 0, capi._ptr(half), 5) == 0      # a half-loaded checkpoint
        with pytest.raises(capi.SailError, match=": -4: .*parts not loaded"):
            multi.temporal_resolve()
        with pytest.raises(capi.SailError, match=": -4: .*parts not loaded"):
            multi.temporal_begin(*vb)
    finally:
        multi.close()


# ---- 7. multi-device --------------------------------------------------------------------------------------------------------
def two_views(ctx, va, vb, B):
    """begin(A), 4 spp, resolve, reset, begin(B), 1 spp, resolve; every map and count on the way"""
    seen = [ctx.temporal_begin(*va)]
    render(ctx, va, 0, 4, B)
    seen.append(ctx.temporal_resolve(want_u8=True))
    ctx.reset()
    seen.append(ctx.temporal_begin(*vb))
    maps = [ctx.temporal_read(w) for w in (G_CUR, G_PREV, HIST, R_MAP, OUT)]
    render(ctx, vb, 0, 1, B)
    seen.append(ctx.temporal_resolve(want_u8=True))
    maps.append(ctx.temporal_read(OUT))
    return seen, maps


@pytest.mark.parametrize("devices,dbg", [([0, 0, 0], None), ([0], {capi.DEBUG_FORCE_RCCL: 1})])
def test_multi_device_equals_one_device(gpu, fixtures, devices, dbg):
    sc = fixtures["scenes"]["C3"]
    W, H, B = 150, 70, 3
    va, vb = fixture_view(sc), tr.orbit(5)
    one = context(sc, W, H)
    try:
        want, want_maps = two_views(one, va, vb, B)
    finally:
        one.close()
    ctx = context(sc, W, H, devices=devices)
    try:
        for opt, val in (dbg or {}).items():
            ctx.set_debug(opt, val)
        got, got_maps = two_views(ctx, va, vb, B)
    finally:
        ctx.close()
    for a, b in zip(got_maps, want_maps):
        assert same(a, b)
    for a, b in zip(got, want):
        for f in ("k", "hit_pixels", "history_pixels", "nonfinite"):
            assert a[f] == b[f]
        if "rgba" in a:
            assert same(a["rgba"], b["rgba"]) and np.array_equal(a["u8"], b["u8"])
    assert want[2]["history_pixels"] > 0


# ---- 8. quality -------------------------------------------------------------------------------------------------------------
def rel_mse(x, ref):
    """tests/test_gpu_denoise.py's definition"""
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    l = ref.sum(axis=-1) / 3.0
    return float((((x - ref) ** 2).sum(axis=-1) / (l * l + 1e-2)).mean())


QUALITY_ANGLE = 5.0     # degrees; on the CPU (the reference with oracle.pick) 0.963 of B's hit pixels find A's history
# 1.5 x the ratio measured on an MI355X, 0.0565 (the camera-motion reprojection kernels' section); never above 0.5
QUALITY_BOUND = min(1.5 * 0.0565, 0.5)


def test_quality_after_an_orbit(gpu, fixtures):
    """C1 at 96x64 with 5 bounces: 64 spp at A resolved, orbit to B, 1 spp, resolved: relMSE against 512 spp of B over other
    sample indices, as a ratio to the 1-spp mean's. Measured on an MI355X: relMSE 38.98 for the 1-spp mean, 2.202 resolved,
    ratio 0.0565; where the history is valid the new sample weighs 1/33."""
    sc = fixtures["scenes"]["C1"]
    W, H, B = 96, 64, 5
    va, vb = tr.orbit(0), tr.orbit(QUALITY_ANGLE)
    ref_ctx = context(sc, W, H)
    try:
        render(ref_ctx, vb, 1, 512, B)
        ref = ref_ctx.readback()[..., :3]
    finally:
        ref_ctx.close()
    ctx = context(sc, W, H)
    try:
        ctx.temporal_begin(*va)
        render(ctx, va, 0, 64, B)
        ctx.temporal_resolve()
        ctx.reset()
        info = ctx.temporal_begin(*vb)
        render(ctx, vb, 0, 1, B)
        noisy = ctx.readback()[..., :3]
        out = ctx.temporal_resolve()
    finally:
        ctx.close()
    # the condition on the input: the reprojection finds most of the picture, on the device as in the reference
    GA, GB = ref_g(fixtures, "C1", W, H, "qualA", va)[0], ref_g(fixtures, "C1", W, H, "qualB", vb)[0]
    found = tr.ref_reproject(GB, GA, np.ones((H, W, 4), F), *va)[1]
    share = info["history_pixels"] / info["hit_pixels"]
    print(f"quality: history {info['history_pixels']} of {info['hit_pixels']} hit pixels ({share:.4f}; reference {found})")
    assert info["history_pixels"] == found and share >= 0.8
    assert np.isfinite(ref).all() and np.isfinite(noisy).all() and out["nonfinite"] == 0
    e_in, e_out = rel_mse(noisy, ref), rel_mse(out["rgba"][..., :3], ref)
    print(f"quality C1 {W}x{H}, {B} bounces, orbit {QUALITY_ANGLE} degrees, reference 512 spp: relMSE of the 1-spp mean "
          f"{e_in:.6g}, resolved {e_out:.6g}, ratio {e_out / e_in:.4f} (required <= {QUALITY_BOUND})")
    assert e_out / e_in <= QUALITY_BOUND
