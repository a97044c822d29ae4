"""CPU: the deferred Sphere row's spec and keys (sail_capi.cpp valueSpecFor, sail_jit.cpp), and the arithmetic behind the
deferring sweep's moving-away reject (sail_geom.h sweepRowsDefer). A value kernel carries SAIL_JIT_ROWDEFER = the index of
the scene's first Sphere row unless SAIL_DEBUG_JIT bit 64 is set (the sense is inverted: the default, 59, defers). The define
is part of the source prefix, so of the cache key; the types kernel's prefix and key do not know the switch."""
import re

import numpy as np

from sail_amd import capi

ON, ON_PLAIN, OFF = 59, 27, 59 | capi.JIT_NO_ROWDEFER  # 123


def _rows(fixtures):
    sc = fixtures["scenes"]["C1"]
    return np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18).copy()


def _c1(fixtures, rows=None):
    sc = dict(fixtures["scenes"]["C1"])
    if rows is not None:
        sc["n"] = int(rows.shape[0])
        sc["objects"] = np.asarray(rows, np.float32).reshape(-1).copy()
    return sc


def _defer(defs):
    m = re.findall(r"#define SAIL_JIT_ROWDEFER (-?\d+)\n", defs)
    assert len(m) <= 1
    return int(m[0]) if m else None


def test_the_define_follows_the_switch(fixtures):
    sc = _c1(fixtures)
    assert OFF == 123
    kon, don = capi.jit_value_key(sc, jit=ON)
    kpl, dpl = capi.jit_value_key(sc, jit=ON_PLAIN)
    koff, doff = capi.jit_value_key(sc, jit=OFF)
    assert None not in (kon, kpl, koff) and len({kon, kpl, koff}) == 3
    assert _defer(don) == 2 and _defer(dpl) == 2  # C1's rows: the light cube, the box, the sphere
    assert _defer(doff) is None and "ROWDEFER" not in doff
    assert _defer(capi.jit_value_key(sc, jit=ON_PLAIN | capi.JIT_NO_ROWDEFER)[1]) is None
    # the switch takes one line out of the value lines and nothing else; the line stands behind the row-shading pair
    line = "#define SAIL_JIT_ROWDEFER 2\n"
    assert don.replace(line, "") == doff
    assert don.startswith("#define SAIL_JIT_ROWSHADE 6\n#define SAIL_JIT_ROWQUIET 6\n" + line)
    assert dpl.startswith(line)
    # the product's default defers
    assert capi.jit_value_key(sc) == (kon, don)
    # the types kernel knows neither the define nor the switch
    ton = capi.jit_value_key(sc, jit=ON, value=False)
    assert ton[0] is not None and ton == capi.jit_value_key(sc, jit=OFF, value=False)
    assert "ROWDEFER" not in ton[1]
    for d in (don, dpl, doff):
        assert d.endswith(ton[1])


def test_which_row_is_deferred(fixtures):
    r = _rows(fixtures)
    # no sphere: the light cube and the box alone
    kon, don = capi.jit_value_key(_c1(fixtures, rows=r[[0, 1]]), jit=ON)
    assert kon is not None and _defer(don) is None
    assert (kon, don) == capi.jit_value_key(_c1(fixtures, rows=r[[0, 1]]), jit=OFF)
    # the sphere in another place
    assert _defer(capi.jit_value_key(_c1(fixtures, rows=r[[2, 0, 1]]), jit=ON)[1]) == 0
    assert _defer(capi.jit_value_key(_c1(fixtures, rows=r[[0, 2, 1]]), jit=ON)[1]) == 1
    # two spheres: the first; above the row-shading form's three rows as well
    s2 = r[2].copy()
    s2[1:5] = (3.9, 3.6, 1.4, 0.8)
    assert _defer(capi.jit_value_key(_c1(fixtures, rows=np.stack([r[1], r[2], s2])), jit=ON)[1]) == 1
    k4, d4 = capi.jit_value_key(_c1(fixtures, rows=np.stack([r[0], r[1], s2, r[2]])), jit=ON)
    assert _defer(d4) == 2 and "SAIL_JIT_ROWSHADE" not in d4
    assert k4 != capi.jit_value_key(_c1(fixtures, rows=np.stack([r[0], r[1], s2, r[2]])), jit=OFF)[0]
    # the room and pre-cull forms have no value kernel, so no deferral
    for name in ("C3", "C4"):
        s = fixtures["scenes"][name]
        assert capi.jit_value_key(s, jit=ON) == (None, "")
        assert "ROWDEFER" not in capi.jit_value_key(s, jit=ON, value=False)[1]


# ---- the moving-away reject ---------------------------------------------------------------------------------------------
KEPS, KMAX = np.float32(1e-5), np.float32(1e5)


def _edge_values():
    f = np.float32
    tiny = np.array([1, 2, 3, 0x7fffff, 0x800000, 0x800001], np.uint32).view(np.float32)  # subnormals, 2^-126 and its neighbour
    vals = [0.0, -0.0, f(2.0) ** f(-126), f(2.0) ** f(126), f(2.0) ** f(-75), f(2.0) ** f(75), np.inf, np.nan,
            1.0, 0.5, 2.0, 1e-5, 1e5, 3.4028235e38, *tiny]
    return np.array(vals, np.float32)


def _operands(n=3_000_000):
    """(a, b, cc): a >= 0 (a sum of squares); random triples over many magnitudes and both signs, every combination of the
    edge values, and cc within an ulp of 0 beside random a and b"""
    rng = np.random.default_rng(20240917)

    def wide(k):
        return (rng.standard_normal(k) * np.exp2(rng.integers(-40, 40, k))).astype(np.float32)

    a, b, cc = np.abs(wide(n)), wide(n), wide(n)
    k = n // 3  # the operands of real rays: a near 1, b and cc of the scene's size
    a[:k] = (1.0 + rng.standard_normal(k) * 1e-6).astype(np.float32)
    b[:k] = (rng.standard_normal(k) * 10).astype(np.float32)
    cc[:k] = (rng.standard_normal(k) * 30).astype(np.float32)
    e = _edge_values()
    ea, eb, ec = (g.reshape(-1) for g in np.meshgrid(np.abs(e), np.concatenate([e, -e]), np.concatenate([e, -e]), indexing="ij"))
    ulp = np.array([0, 1, 2, 0x80000000, 0x80000001, 0x80000002], np.uint32).view(np.float32)
    m = 200_000
    ua, ub, uc = np.abs(wide(m)), np.abs(wide(m)), ulp[rng.integers(0, len(ulp), m)]
    return (np.concatenate([a, ea, ua]), np.concatenate([b, eb, ub]), np.concatenate([cc, ec, uc]))


def _inline_sphere_t(a, b, cc):
    """sphereT from the discriminant to the root choice, as the kernel computes it, in numpy float32.

    Scope: f32 operations rounded to nearest one at a time (no contraction), subnormals kept; sqrtf_ is the IEEE square
    root and fdiv(x, y) = x * float32(1 / y) with a correctly rounded reciprocal (sail_math.h), which numpy's float32 sqrt
    and divide are. Not emulated: the head (a, b, cc are the inputs), and what follows the root choice -- the
    t >= kMaxDistance test and the slab test can only turn a t into a miss, never a miss or a NaN into a hit.
    Returns (rejected: discrim < 0, missed: t2 < kEps, t: the chosen root where neither)."""
    f = np.float32
    with np.errstate(all="ignore"):
        discrim = b * b - f(4.0) * a * cc
        rejected = discrim < 0
        root = np.sqrt(discrim)
        q = np.where(b < 0, f(-0.5) * (b - root), f(-0.5) * (b + root)).astype(np.float32)
        t0 = q * (f(1.0) / a)
        t1 = cc * (f(1.0) / q)
        swap = t0 > t1
        t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)
        missed = t1 < KEPS
        t = np.where(t0 < KEPS, t1, t0)
    assert discrim.dtype == q.dtype == t.dtype == np.float32
    return rejected, missed, t


def test_a_ray_that_starts_outside_and_moves_away_cannot_hit():
    """The deferring sweep drops a candidate with b > 0 and cc > 0 without running the tail. Claim: the inline sphereT
    gives such a ray no t that the sweep's `t < best` accepts. Where the roots are numbers it returns the miss at its
    t2 < kEps test: q = -0.5 (b + root) <= -0, so both roots are <= -0. Where an operand is infinite or a product
    underflows, a root can be NaN (q = -0 with a = 0 gives -0 * inf; b = inf gives inf - inf for the discriminant): then
    either t2 is still below kEps, or the chosen t is that NaN, which fails every compare the sweep and the resolve make
    (t < best, t == best). Never a number at or above kEps."""
    a, b, cc = _operands()
    assert a.dtype == b.dtype == cc.dtype == np.float32 and len(a) > 3_000_000
    rejected, missed, t = _inline_sphere_t(a, b, cc)
    away = (b > 0) & (cc > 0)
    cand = away & ~rejected  # what the reject takes out of the candidates
    assert int(cand.sum()) > 300_000 and int((cand & ~np.isfinite(t)).sum()) > 0  # both kinds are in the sample
    wins = cand & ~missed & ~np.isnan(t)
    print(f"moving away: {int(away.sum())} of {len(a)}; candidates among them {int(cand.sum())}, "
          f"missed at t2 < kEps {int((cand & missed).sum())}, NaN t {int((cand & ~missed & np.isnan(t)).sum())}, other {int(wins.sum())}")
    assert not wins.any(), (a[wins][:5], b[wins][:5], cc[wins][:5], t[wins][:5])
    # with finite, normal-range operands there is no NaN case at all: the plain claim
    plain = cand & np.isfinite(a) & np.isfinite(b) & np.isfinite(cc) & (a >= np.float32(2.0) ** np.float32(-60)) & \
        (a <= np.float32(2.0) ** np.float32(60)) & (np.abs(b) <= np.float32(2.0) ** np.float32(60)) & \
        (np.abs(b) >= np.float32(2.0) ** np.float32(-60)) & (cc <= np.float32(2.0) ** np.float32(60))
    assert int(plain.sum()) > 200_000 and missed[plain].all()
    # and the test is not vacuous: rays that move towards the sphere from outside do hit
    towards = (b < 0) & (cc > 0) & ~rejected & ~missed & (t >= KEPS)
    assert int(towards.sum()) > 100_000
