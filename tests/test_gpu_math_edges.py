"""The math spec at its class and range edges: sail_math.h (through sail_math_kernel) vs oracle/ref_math.h. Needs an MI355X.

tests/test_gpu_parity.py::test_math_spec_bit_exact probes the middle of each function's domain. This file feeds the
inputs at which sail_math.h branches: the 2^20 switch of the sin/cos/tan reduction and its 1e15 limit, the
wave-uniform range guard of rcp_rn, every class branch of powf_, results in the f32 subnormal range, and the functions
the first test never calls (expf_, to_int, fract_, clamp_(x, -1, 1)). The bar is the same: capi.math_probe equals
oracle.math bit for bit, NaN == NaN.

The probe launches 256-thread blocks, so elements 64m .. 64m+63 of an array are one wavefront: where the wave's
composition matters the inputs are built in aligned runs of 64. Every builder asserts that its input holds what it
claims before anything runs on the device.
"""
import numpy as np
import pytest

import oracle
from sail_amd import capi

pytestmark = pytest.mark.gpu

MAX_N = 1 << 18
FLT_MAX = np.float32(3.4028234663852886e38)
P20 = 0x49800000       # 2^20
B_LO = 0x00800000      # 2^-126: the smallest divisor of rcp_rn's Newton path
B_HI = 0x7E800000      # 2^126: the largest
SIGN = 0x80000000


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def f32(bits):
    return np.ascontiguousarray(np.asarray(bits, dtype=np.uint64).astype(np.uint32)).view(np.float32)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def around(bits, n=64, both_signs=True):
    """the float with these (positive) bits and the n floats on either side of it, then the same negated"""
    b = np.arange(bits - n, bits + n + 1, dtype=np.uint64)
    return f32(np.concatenate([b, b | SIGN]) if both_signs else b)


def raw_bits(rng, n):
    return f32(rng.integers(0, 1 << 32, n, dtype=np.uint64))


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def waves(x):
    assert x.size % 64 == 0
    return x.reshape(-1, 64)


class Compare:
    """runs the segments of one function, prints every count, and fails at the end with all the mismatches"""

    def __init__(self, fn, raw=False):
        self.fn, self.raw, self.n, self.bad = fn, raw, 0, []

    def run(self, what, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32).ravel()
        assert 0 < x.size <= MAX_N and y.size == x.size
        got = capi.math_probe(self.fn, x, y)
        want = oracle.math(self.fn, x, y)
        same = u32(got) == u32(want)
        if not self.raw:
            same |= np.isnan(got) & np.isnan(want)
        miss = np.flatnonzero(~same)
        self.n += x.size
        print(f"fn {self.fn} {what}: {x.size} inputs, {miss.size} mismatches")
        if miss.size:
            i = miss[:4]
            self.bad.append(f"{what}: {miss.size} of {x.size}, e.g. i={i.tolist()} x={[hex(v) for v in u32(x)[i]]} "
                            f"y={[hex(v) for v in u32(y)[i]]} gpu={[hex(v) for v in u32(got)[i]]} "
                            f"cpu={[hex(v) for v in u32(want)[i]]}")

    def done(self):
        print(f"fn {self.fn}: {self.n} inputs compared in all")
        assert not self.bad, f"fn {self.fn}: " + "; ".join(self.bad)


# ---- sin / cos / tan: the f32 reduction below 2^20, reduce_pio2 (f64) from there, NaN from 1e15 -----------------------
def quadrant_f64(x):
    """reduce_pio2's k mod 4 (two's complement) for |x| in [2^20, 1e15)"""
    k = np.floor(x.astype(np.float64) * 0.6366197723675814 + 0.5)
    return k.astype(np.int64) & 3


def trig_segments():
    rng = np.random.default_rng(2000)
    seg = {}
    x = around(P20)
    assert (np.abs(x) < 2.0 ** 20).sum() == 128 and (np.abs(x) > 2.0 ** 20).sum() == 128 and (np.abs(x) == 2.0 ** 20).sum() == 2
    seg["2^20 and 64 neighbours a side"] = x

    x = (log_uniform(rng, 2.0 ** 20, 1e15, 1 << 16) * signs(rng, 1 << 16)).astype(np.float32)
    x = np.clip(x, -np.float32(1e15), np.float32(1e15))          # RN(1e15) is below 1e15
    a = np.abs(x.astype(np.float64))
    assert ((a >= 2.0 ** 20) & (a < 1e15)).all() and (a > 1e14).any() and (a < 2.0 ** 21).any()
    for s in (x[x > 0], x[x < 0]):
        assert set(np.unique(quadrant_f64(s))) == {0, 1, 2, 3}
    seg["log-uniform [2^20, 1e15)"] = x

    x = around(int(u32(np.float32(1e15))[0]))
    a = np.abs(x.astype(np.float64))
    assert (a < 1e15).sum() == 130 and (a >= 1e15).sum() == 128     # RN(1e15) itself reduces, its successor is NaN
    seg["floats adjacent to 1e15"] = x

    big = (log_uniform(rng, 1e15, float(FLT_MAX), 4096) * signs(rng, 4096)).astype(np.float32)
    sub = f32(np.concatenate([[1, 2, 0x007FFFFF, 0x00400000], rng.integers(1, 0x00800000, 60)]))
    x = np.concatenate([big, np.array([FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32),
                        f32([0xFFC00000, 0x7F800001]), sub, -sub])
    assert np.isinf(x).sum() == 2 and np.isnan(x).sum() == 3 and (u32(x) == SIGN).any() and (u32(x) == 0).any()
    assert (np.abs(x) == FLT_MAX).sum() == 2 and ((x != 0) & (np.abs(x) < 2.0 ** -126)).sum() == 128
    seg["up to FLT_MAX, inf, NaN, zeros, subnormals"] = x

    # RN(k pi/2): the reduced argument cancels to a few ulps; every quadrant, both signs, both sides of 2^20
    k = np.concatenate([np.arange(1, (1 << 15) + 1), rng.integers(1 << 15, (1 << 22) + 1, (1 << 15) - 66),
                        np.arange(667540, 667604), [(1 << 22) - 1, 1 << 22]]).astype(np.float64)
    k = np.concatenate([k, -k])
    x = (k * (np.pi / 2)).astype(np.float32)
    assert k.size == 1 << 17 and np.abs(k).max() == 2.0 ** 22
    ki = k.astype(np.int64)
    for side in (np.abs(x) < 2.0 ** 20, np.abs(x) >= 2.0 ** 20):
        for sg in (k > 0, k < 0):
            assert set(np.unique(ki[side & sg] & 3)) == {0, 1, 2, 3}
    far = np.abs(x) >= 2.0 ** 20
    assert (quadrant_f64(x[far]) == (ki[far] & 3)).all()           # the f64 path really lands in quadrant k mod 4
    seg["RN(k pi/2), |k| <= 2^22"] = x

    # divergent waves: lanes below 2^20 (the hash RNG's range) beside lanes on the f64 path
    nw = 256
    small = (rng.uniform(1e4, 1e6, (nw, 64)) * signs(rng, (nw, 64))).astype(np.float32)
    large = (log_uniform(rng, 2.0 ** 20, 1e12, (nw, 64)) * signs(rng, (nw, 64))).astype(np.float32)
    pick = rng.random((nw, 64)) < 0.5
    lane = (np.arange(nw) * 5 + 3) % 64
    pick[:86] = False
    pick[np.arange(86), lane[:86]] = True                          # one lane of the wave on the f64 path
    pick[86:172] = True
    pick[np.arange(86, 172), lane[86:172]] = False                 # one lane of the wave on the f32 path
    x = np.where(pick, large, small)
    on64 = np.abs(x) >= 2.0 ** 20
    assert (on64.sum(axis=1) >= 1).all() and (on64.sum(axis=1) <= 63).all()
    assert (on64[:86].sum(axis=1) == 1).all() and (on64[86:172].sum(axis=1) == 63).all()
    assert len(set(np.argmax(on64[:86], axis=1))) == 64
    seg["waves mixing both reductions"] = x
    return seg


def tan_extra():
    k = np.arange(1, 1 << 13, 2, dtype=np.float64)                 # the f32 nearest the poles
    x = np.concatenate([(k * (np.pi / 2)).astype(np.float32), (-k * (np.pi / 2)).astype(np.float32),
                        np.array([0.0, -0.0], np.float32)])
    assert (u32(x) == 0).any() and (u32(x) == SIGN).any()
    assert (np.abs(np.cos(x[:-2].astype(np.float64))) < 2e-3).all()
    return x


@pytest.mark.parametrize("fn", [0, 1, 2])
def test_trig_reductions(gpu, fn):
    c = Compare(fn)
    for what, x in trig_segments().items():
        c.run(what, x)
    if fn == 2:
        c.run("zeros and the f32 nearest odd multiples of pi/2", tan_extra())
    c.done()


# ---- rcp_rn (fn 14) and the GLSL divide a * rcp_rn(b) (fn 11): the wave-uniform range guard ----------------------------
def in_range_divisors(rng, n):
    b = rng.integers(B_LO, B_HI + 1, n, dtype=np.uint64)
    return f32(b | (rng.integers(0, 2, n, dtype=np.uint64) << 31))


def out_of_range(x):
    a = np.abs(x)
    return ~((a >= np.float32(2.0 ** -126)) & (a <= np.float32(2.0 ** 126)))


OUT_CLASSES = {
    "+0": lambda rng, n: f32(np.zeros(n)),
    "-0": lambda rng, n: f32(np.full(n, SIGN)),
    "subnormal": lambda rng, n: f32(rng.integers(1, B_LO - 1, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << 31)),
    "predecessor of 2^-126": lambda rng, n: f32((B_LO - 1) | ((np.arange(n, dtype=np.uint64) & 1) << 31)),
    "successor of 2^126": lambda rng, n: f32((B_HI + 1) | ((np.arange(n, dtype=np.uint64) & 1) << 31)),
    "+inf": lambda rng, n: f32(np.full(n, 0x7F800000)),
    "-inf": lambda rng, n: f32(np.full(n, 0xFF800000)),
    "NaN": lambda rng, n: f32(np.resize(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA55555], np.uint64), n)),
}


def divisor_segments():
    rng = np.random.default_rng(2014)
    seg = {}
    # waves wholly on the Newton path, the exact bounds and their in-range neighbours at varying lanes
    nw = 320
    b = waves(in_range_divisors(rng, nw * 64)).copy()
    edge = f32([B_LO, B_LO | SIGN, B_HI, B_HI | SIGN, B_LO + 1, (B_LO + 1) | SIGN, B_HI - 1, (B_HI - 1) | SIGN])
    for m in range(128):
        b[m, (m * 7 + 1) % 64] = edge[m % 8]
    b[128, :8] = edge                                              # and all of them in one wave
    tail = in_range_divisors(rng, 37)                              # a partial last wave
    tail[5], tail[36] = edge[0], edge[3]
    x = np.concatenate([b.ravel(), tail])
    assert x.size % 64 == 37 and not out_of_range(x).any()
    assert all((u32(x) == v).sum() >= 16 for v in u32(edge))
    seg["in range"] = x

    for name, make in OUT_CLASSES.items():
        nw = 16
        b = waves(in_range_divisors(rng, nw * 64)).copy()
        lane = (np.arange(nw) * 13 + 5) % 64                       # 16 different lanes, first and last included below
        lane[0], lane[1] = 0, 63
        b[np.arange(nw), lane] = make(rng, nw)
        tail = in_range_divisors(rng, 21)
        tail[20] = make(rng, 1)[0]
        x = np.concatenate([b.ravel(), tail])
        o = out_of_range(x)
        assert (waves(o[:nw * 64]).sum(axis=1) == 1).all() and o[nw * 64:].sum() == 1 and len(set(lane)) == nw
        seg["one lane " + name] = x
    assert np.isnan(seg["one lane NaN"]).sum() == 17 and (seg["one lane predecessor of 2^-126"] != 0).all()
    return seg


def test_rcp_wave_guard(gpu):
    c = Compare(14)
    for what, x in divisor_segments().items():
        c.run(what, x)
    c.done()


def test_glsl_divide_wave_guard(gpu):
    """a * rcp_rn(b) over the same divisors: raw numerators, and numerators that put the product in the subnormal range
    and past FLT_MAX"""
    rng = np.random.default_rng(2011)
    c = Compare(11)
    for what, b in divisor_segments().items():
        n = b.size
        bd = np.where(out_of_range(b), np.float32(1.0), b).astype(np.float64)
        target = np.where(np.arange(n) % 2 == 0, log_uniform(rng, 2.0 ** -151, 2.0 ** -125, n), log_uniform(rng, 2.0 ** 126, 2.0 ** 130, n))
        with np.errstate(over="ignore"):
            a = (target * bd * signs(rng, n)).astype(np.float32)
        third = np.arange(n) % 3 == 0
        a[third] = raw_bits(rng, n)[third]
        if what == "in range":
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                prod = np.abs(a.astype(np.float64) * (np.float32(1.0) / b).astype(np.float64))
            fin = np.isfinite(a)
            assert ((prod > 0) & (prod < 2.0 ** -126) & fin).sum() >= 1000, "products in the f32 subnormal range"
            assert ((prod > float(FLT_MAX) * (1 + 2.0 ** -24)) & fin).sum() >= 1000, "products that overflow"
        c.run(what, a, b)
    c.done()


# ---- the IEEE divide (fn 8) --------------------------------------------------------------------------------------------
SPECIAL = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 0.5, 2.0, -1e-30], np.float32),
                          np.array([1e-42, -1e-42, FLT_MAX, -FLT_MAX], np.float32), f32([1, B_LO])])


def test_ieee_divide_classes(gpu):
    rng = np.random.default_rng(2008)
    assert ((SPECIAL != 0) & (np.abs(SPECIAL) < 2.0 ** -126)).sum() == 3 and (np.abs(SPECIAL) == FLT_MAX).sum() == 2
    xs, ys = np.meshgrid(SPECIAL, SPECIAL)
    c = Compare(8)
    c.run("special-value meshgrid", xs.ravel(), ys.ravel())
    c.run("raw bit patterns", raw_bits(rng, 1 << 17), raw_bits(rng, 1 << 17))
    c.done()


# ---- powf_ ---------------------------------------------------------------------------------------------------------
def test_pow_classes_and_ranges(gpu):
    rng = np.random.default_rng(2005)
    c = Compare(5)
    xv = np.concatenate([np.array([np.nan, 0.0, -0.0, 1.0, -1.0, -2.5, 0.5, 2.0, 10.0, np.inf, -np.inf, 1e-42, -1e-42,
                                   FLT_MAX, -FLT_MAX], np.float32), f32([0xFFC00000, 0x7F800001, 1, B_LO])])
    yv = np.concatenate([np.array([np.nan, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, 3.0, -3.0, 40.0, -40.0, np.inf, -np.inf,
                                   1e-42, -1e-42, FLT_MAX, -FLT_MAX], np.float32),
                         f32([0x7F800001]), np.float32(1.0) / np.array([2.2, 1.8], np.float32)])
    xs, ys = [a.ravel() for a in np.meshgrid(xv, yv)]
    nn = ~np.isnan(xs) & ~np.isnan(ys)
    for cls in (np.isnan(xs) & ~np.isnan(ys), ~np.isnan(xs) & np.isnan(ys), np.isnan(xs) & np.isnan(ys),
                (ys == 0) & np.isnan(xs), (ys == 0) & (xs < 0), (ys == 0) & np.isinf(xs), (u32(ys) == SIGN) & (xs < 0),
                nn & (xs < 0) & (ys != 0), nn & (xs == -np.inf) & (ys != 0),
                (u32(xs) == 0) & (ys > 0), (u32(xs) == 0) & (ys < 0), (u32(xs) == SIGN) & (ys > 0), (u32(xs) == SIGN) & (ys < 0),
                (xs == 0) & (ys == np.inf), (xs == 0) & (ys == -np.inf),
                (xs == np.inf) & (ys == np.inf), (xs == np.inf) & (ys == -np.inf),
                (xs == 1) & np.isinf(ys), (xs > 0) & (xs < 2.0 ** -126) & nn & (ys != 0)):
        assert cls.any()
    c.run("class meshgrid", xs, ys)

    x = f32(rng.integers(1, B_LO, 1 << 12, dtype=np.uint64))
    assert ((x > 0) & (x < 2.0 ** -126)).all()
    c.run("subnormal x", x, rng.uniform(-3, 3, x.size).astype(np.float32))

    x = (10.0 ** rng.uniform(-30, 30, 1 << 14)).astype(np.float32)
    y = rng.uniform(-60, 60, x.size).astype(np.float32)
    lg = y.astype(np.float64) * np.log2(x.astype(np.float64))
    assert (lg > 129).sum() > 1000 and (lg < -151).sum() > 1000 and ((lg > -126) & (lg < 128)).sum() > 1000
    c.run("overflow and underflow", x, y)

    x = rng.uniform(9, 11, 1 << 14).astype(np.float32)
    y = rng.uniform(-45, -37.9, x.size).astype(np.float32)
    x[::2], y[::2] = np.float32(1.0) / x[::2], -y[::2]              # the same range through log2(x) < 0, y > 0
    lg = y.astype(np.float64) * np.log2(x.astype(np.float64))
    assert ((lg > -149) & (lg < -126.01)).sum() >= 1000, "results in the f32 subnormal range"
    assert (lg < -150.5).any() and (lg > -126).any()
    c.run("subnormal results", x, y)

    # the gamma filter's call: pixel values of any non-negative pattern (subnormal, huge, inf, NaN) to 1/2.2 and 1/1.8
    for g in (2.2, 1.8):
        y1 = np.float32(1.0) / np.float32(g)
        x = f32(np.concatenate([np.arange(0, 1 << 31, 1 << 15, dtype=np.uint64), rng.integers(0, 1 << 31, 1 << 16, dtype=np.uint64),
                                [0, B_LO - 1, B_LO, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000]]))
        assert not np.signbit(x).any() and np.isnan(x).any() and np.isinf(x).any() and ((x > 0) & (x < 2.0 ** -126)).any()
        c.run(f"raw non-negative x, y = 1/{g}", x, np.full(x.size, y1, np.float32))
    c.done()


# ---- expf_ (fn 13): the wavelet filter's weights ---------------------------------------------------------------------
def test_exp_ranges_and_classes(gpu):
    rng = np.random.default_rng(2013)
    c = Compare(13)
    x = np.concatenate([np.linspace(-110, 90, 1 << 17), rng.uniform(-110, 90, 1 << 16)]).astype(np.float32)
    e = x.astype(np.float64) * np.log2(np.e)
    assert ((e > -149) & (e < -126.01)).sum() >= 1000 and (e < -151).any() and (e > 128.01).any() and (np.abs(e) < 100).any()
    c.run("[-110, 90] dense", x)
    x = np.concatenate([np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, FLT_MAX, -FLT_MAX, 1e-42, -1e-42, 88.72284, -87.33655,
                                  -103.2789, -103.97208], np.float32), f32([0xFFC00000, 0x7F800001, 1, SIGN | 1])])
    assert np.isinf(x).sum() == 2 and np.isnan(x).sum() == 3 and (u32(x) == SIGN).any() and (u32(x) == 0).any()
    c.run("classes", x)
    c.run("raw bit patterns", raw_bits(rng, 1 << 16))
    c.done()


# ---- acosf_ --------------------------------------------------------------------------------------------------------
def test_acos_edges(gpu):
    rng = np.random.default_rng(2004)
    c = Compare(4)
    x = np.concatenate([around(0x3F800000), around(0x3F000000)])   # +-1 and +-0.5 with 64 neighbours a side
    a = np.abs(x)
    assert (a == 1).sum() == 2 and (a > 1).sum() == 128 and ((a < 1) & (a > 0.9)).sum() == 128
    assert (a == 0.5).sum() == 2 and ((a > 0.5) & (a < 0.6)).sum() == 128 and (a < 0.5).sum() == 128
    c.run("+-1, +-0.5 and neighbours", x)
    sub = f32(np.concatenate([[1, B_LO - 1], rng.integers(1, B_LO, 62)]))
    x = np.concatenate([np.array([0.0, -0.0, 1.5, -1.5, 2.0, -2.0, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], np.float32),
                        f32([0xFFC00000, 0x7F800001, B_LO, B_LO | SIGN]), sub, -sub])
    assert (u32(x) == SIGN).any() and (u32(x) == 0).any() and np.isinf(x).sum() == 2 and np.isnan(x).sum() == 3
    assert ((x != 0) & (np.abs(x) < 2.0 ** -126)).sum() == 128 and (np.abs(x) > 1).sum() == 8
    c.run("zeros, subnormals, |x| > 1, inf, NaN", x)
    c.run("raw bit patterns", raw_bits(rng, 1 << 16))
    c.done()


# ---- atan2f_ -------------------------------------------------------------------------------------------------------
def test_atan2_classes(gpu):
    rng = np.random.default_rng(2003)
    c = Compare(3)
    sp = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-42, -1e-42, FLT_MAX, -FLT_MAX, 0.5, -3.0],
                                  np.float32), f32([1, SIGN | 1, B_LO, 0x7F800001])])
    assert ((sp != 0) & (np.abs(sp) < 2.0 ** -126)).sum() == 4 and (np.abs(sp) == FLT_MAX).sum() == 2
    xs, ys = [a.ravel() for a in np.meshgrid(sp, sp)]
    c.run("special-value meshgrid", xs, ys)

    n = 1 << 12
    v = np.abs(raw_bits(rng, n))
    v = v[np.isfinite(v)]
    x, y = v * signs(rng, v.size).astype(np.float32), v * signs(rng, v.size).astype(np.float32)
    assert (np.abs(x) == np.abs(y)).all() and (x != y).any() and (x == y).any() and ((v > 0) & (v < 2.0 ** -126)).any()
    c.run("|y| == |x|", x, y)

    big = log_uniform(rng, 2.0 ** 60, 2.0 ** 127, n)
    small = (big * log_uniform(rng, 2.0 ** -148, 2.0 ** -127, n)).astype(np.float32)
    big = big.astype(np.float32)
    q = small / big                                                 # f32: the quotient atan2f_ forms
    assert ((q > 0) & (q < 2.0 ** -126)).sum() >= 1000 and (small >= 2.0 ** -126).all()
    sb, ss = signs(rng, n).astype(np.float32), signs(rng, n).astype(np.float32)
    c.run("subnormal quotient y / x", big * sb, small * ss)        # probe arguments are (x, y): atan2f_(y, x)
    c.run("subnormal quotient x / y", small * ss, big * sb)
    c.done()


# ---- to_int (fn 16), fract_ (fn 17), clamp_(x, -1, 1) (fn 18) ---------------------------------------------------------
def int_like_inputs():
    rng = np.random.default_rng(2016)
    k = np.arange(-1000, 1001, dtype=np.float32)
    x = np.concatenate([around(0x4F000000),                        # +-2^31 and 64 neighbours a side
                        around(0x3F800000), around(0x4B000000), around(0x4B800000),   # 1, 2^23, 2^24
                        k + np.float32(0.5), k, -rng.random(4096).astype(np.float32),
                        np.array([0.0, -0.0, -1e-10, -1e-42, 1e-42, 0.99999994, -0.99999994, np.inf, -np.inf, np.nan, FLT_MAX,
                                  -FLT_MAX, 2147483520.0, -2147483904.0, 4294967296.0], np.float32),
                        f32([0xFFC00000, 0x7F800001, 0xFF800001, 1, SIGN | 1])])
    a = np.abs(x)
    assert (a == 2.0 ** 31).sum() == 2 and (a > 2.0 ** 31).sum() >= 130 and ((a < 2.0 ** 31) & (a > 2.0 ** 30)).sum() >= 128
    af = a[np.isfinite(x)]
    assert (u32(x) == SIGN).any() and ((x < 0) & (x > -1)).sum() > 4000 and (af - np.floor(af) == 0.5).sum() >= 2001
    return {"+-2^31, integers, half-integers, negative fractions, classes": x, "raw bit patterns": raw_bits(rng, 1 << 17)}


@pytest.mark.parametrize("fn", [9, 10, 12])
def test_min_max_clamp01_signalling_nan(gpu, fn):
    """min, max and clamp(x, 0, 1) drop a signalling NaN as they drop a quiet one (the v_med3_f32 form of clamp returned
    hi for one until clamp_ canonicalized its argument: fn 18 below found it)"""
    rng = np.random.default_rng(2009)
    x, y = raw_bits(rng, 1 << 16), raw_bits(rng, 1 << 16)
    snan = f32(np.resize(np.array([0x7F800001, 0xFF800001, 0x7FA55555, 0xFFBFFFFF], np.uint64), 256))
    x[:256], y[256:512] = snan, snan
    y[:128] = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, np.inf, -np.inf], np.float32).repeat(16)
    sig = lambda v: np.isnan(v) & ((u32(v) & 0x00400000) == 0)
    assert sig(x).sum() >= 256 and sig(y).sum() >= 256 and (sig(x) & ~np.isnan(y)).sum() >= 128
    c = Compare(fn)
    c.run("raw bit patterns and signalling NaNs", x, y)
    c.done()


@pytest.mark.parametrize("fn", [16, 17, 18])
def test_to_int_fract_clamp(gpu, fn):
    c = Compare(fn, raw=(fn == 16))
    for what, x in int_like_inputs().items():
        c.run(what, x)
    c.done()
