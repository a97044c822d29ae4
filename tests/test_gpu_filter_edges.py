"""sail_filter_kernel at its edges vs the CPU oracle's display filters. Needs an MI355X.

tests/test_gpu_parity.py::test_filter_bit_exact runs the filters over one rendered 45x37 frame with window radii 1.5..3
(LDS halos 4 and 5). Here the accumulators are chosen (Context.load, no scene) so that the kernel meets what a render
rarely gives it: frames smaller than a workgroup and than the halo (the REPEAT wrap wraps more than once), every halo
from 2 to 8 and the global path beyond, negative, anisotropic and NaN radii, both accumulation modes, texels that are
NaN, +-inf, -0, huge or subnormal, counts that are 0 or NaN, and the RGBA8 quantisation of all of these. The wavelet,
normal and position filters run over renders in which most (N1S) or all (N0) texels miss the scene and carry a NaN
position.

The oracle filters a mean image built on the host by the kernel's stated rule (SUM: rgb / (w > 0 ? w : 1), MIX: rgb);
the f32 output must match bit for bit (NaN == NaN) and the RGBA8 output floor(clamp(v, 0, 1) * 255 + 0.5) with the
spec's clamp (NaN -> 0, +inf -> 255, -inf -> 0).
"""
import numpy as np
import pytest

import oracle
from sail_amd import capi

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (3, 2), (16, 16), (17, 33), (40, 9)]   # W, H
TABLES = ["box", "triangle", "mitchell", "sinc", "gaussian"]
POINT_KINDS = [(capi.FILTER_COLOR, 2.2), (capi.FILTER_GAMMA, 2.2), (capi.FILTER_GAMMA, 1.8), (capi.FILTER_TONEMAPPING, 2.2)]
# sail_filter stages 16 + 2 * halo texels a side, halo = ceil(0.875 r) + 2 for r = max(|rx|, |ry|), up to halo 8
RADII = [(0.0, 0.0),          # halo 2
         (6.5, 1.0),          # halo 8, anisotropic
         (6.857, 6.857),      # halo 8: the last radius staged in LDS
         (6.86, 6.86),        # halo 9 -> the global path
         (7.0, 7.0), (40.0, 40.0),
         (-2.0, 3.0),
         (float("nan"), 1.0),                      # halo 3: see halo() below
         (float("nan"), float("nan"))]             # no radius at all -> the global path
MIX_RADII = [(2.0, 2.0), (7.0, 7.0)]


def halo(rx, ry):
    """sail_filter's rule, restated: fmaxf drops a NaN operand, so (NaN, 1) stages the halo of radius 1 and the NaN
    reaches the kernel in the tap coordinates only (every tap then reads NaN-weighted texels)"""
    r = np.fmax(np.abs(np.float32(rx)), np.abs(np.float32(ry)))
    h = int(np.ceil(np.float32(0.875) * r)) + 2 if r == r else 99
    return h if h <= 8 else 0


assert [halo(*r) for r in RADII] == [2, 8, 8, 0, 0, 0, 5, 3, 0] and [halo(*r) for r in MIX_RADII] == [4, 0]


@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bit_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def roomy(W, H):
    return W * H >= 256


def accumulator(W, H):
    """random non-negative sums with per-texel counts 1..8; where the frame has room, a 16x16 tile spanning 2^+-20 and
    one texel each of NaN, +inf, -inf, -0, 3e38, 1e-42, a count of 0 and a NaN count (clustered in the last three rows)"""
    rng = np.random.default_rng(1000 * W + H)
    cnt = rng.integers(1, 9, (H, W)).astype(np.float32)
    A = np.zeros((H, W, 4), np.float32)
    A[..., :3] = rng.uniform(0.0, 1.5, (H, W, 3)).astype(np.float32) * cnt[..., None]
    A[..., 3] = cnt
    if W >= 16 and H >= 16:
        tx, ty = min(1, W - 16), min(9, H - 16)                   # straddles workgroups where the frame allows
        A[ty:ty + 16, tx:tx + 16, :3] = (2.0 ** rng.uniform(-20, 20, (16, 16, 3))).astype(np.float32)
    if roomy(W, H):
        y, x = H - 1, W - 1                                       # +inf and 3e38 keep finite right / lower neighbours:
        A[y, x, :3] = np.nan                                      # a NaN in the bilinear footprint would turn them NaN
        A[y, x - 2, :3] = -np.inf
        A[y - 1, x, :3] = -0.0
        A[y - 1, x - 1, :3] = 1e-42
        A[y - 1, x - 3, 3] = 0.0
        A[y - 1, x - 4, 3] = np.nan
        A[y - 2, x - 2, :3] = np.inf
        A[y - 2, x - 4, :3] = 3e38
        v = A[..., :3]
        assert np.isnan(v).sum() == 3 and (v == np.inf).sum() == 3 and (v == -np.inf).sum() == 3
        assert (v.view(np.uint32) == 0x80000000).sum() == 3 and (v == np.float32(3e38)).sum() == 3
        assert (v == np.float32(1e-42)).sum() == 3 and (A[..., 3] == 0).sum() == 1 and np.isnan(A[..., 3]).sum() == 1
    return A


def mean_image(A, mix):
    """the kernel's texel rule: SUM divides each texel by its own count (IEEE; 0, negative and NaN counts divide by 1)"""
    m = A.copy()
    if not mix:
        w = A[..., 3:4]
        with np.errstate(over="ignore", invalid="ignore"):
            m[..., :3] = A[..., :3] / np.where(w > 0, w, np.float32(1.0))
    m[..., 3] = 1.0
    return m


def rgba8(want):
    c = oracle.math(12, want[..., :3].ravel())                    # the spec clamp: NaN -> 0
    with np.errstate(invalid="ignore"):
        return np.floor(c * np.float32(255.0) + np.float32(0.5)).astype(np.uint8).reshape(want.shape[:2] + (3,))


class Frame:
    """one context holding a chosen accumulator; compare() runs one filter on both sides and notes any mismatch"""

    def __init__(self, W, H, mix=False):
        self.W, self.H, self.mix = W, H, mix
        A = accumulator(W, H)
        self.mean = mean_image(A, mix)
        self.ctx = capi.Context(W, H)
        if mix:
            self.ctx.set_accum_mode(capi.ACCUM_MIX)
        self.ctx.load({"k": 8, "parts": [A]})
        self.bad, self.n = [], 0

    def compare(self, what, kind, w=None, r=(0.0, 0.0), gamma=2.2):
        got, got8 = self.ctx.filter(kind, w, r[0], r[1], gamma, want_u8=True)
        want = oracle.filter_image(self.mean, kind, w, r[0], r[1], gamma)
        fin = np.isfinite(want[..., :3]).all(axis=-1)
        if roomy(self.W, self.H) and not (kind == capi.FILTER_WINDOW and r[0] != r[0]):
            assert fin.any() and not fin.all(), f"{what}: the expected image must hold finite and non-finite texels"
        elif kind == capi.FILTER_WINDOW and r[0] != r[0]:
            assert np.isnan(want[..., :3]).all()
        same = bit_equal(got, want)
        same8 = (got8[..., :3] == rgba8(want)) & (got8[..., 3:4] == 255)
        self.n += fin.size
        print(f"{self.W}x{self.H} {'MIX' if self.mix else 'SUM'} {what}: {fin.size} texels ({int(fin.sum())} finite), "
              f"{int((~same).sum())} f32 and {int((~same8).sum())} RGBA8 channel mismatches")
        if not same.all():
            y, x, c = [int(v[0]) for v in np.nonzero(~same)]
            self.bad.append(f"{what}: {int((~same).sum())} f32 channels, e.g. ({x}, {y})[{c}] gpu {got[y, x, c]!r} cpu {want[y, x, c]!r}")
        if not same8.all():
            y, x, c = [int(v[0]) for v in np.nonzero(~same8)]
            self.bad.append(f"{what}: {int((~same8).sum())} RGBA8 channels, e.g. ({x}, {y})[{c}] gpu {got8[y, x, c]} for {want[y, x, c]!r}")

    def done(self):
        self.ctx.close()
        print(f"{self.W}x{self.H}: {self.n} texels compared in all")
        assert not self.bad, f"{self.W}x{self.H} {'MIX' if self.mix else 'SUM'}: " + "; ".join(self.bad)


def weights(fixtures, name):
    return np.array([float(x) for x in fixtures["filters"][name]["weight_text"]], dtype=np.float32)


def kind_name(kind, gamma):
    return {capi.FILTER_COLOR: "color", capi.FILTER_GAMMA: f"gamma {gamma}", capi.FILTER_TONEMAPPING: "tonemapping"}[kind]


@pytest.mark.parametrize("W,H", FRAMES)
def test_point_filters_sum(gpu, W, H):
    f = Frame(W, H)
    try:
        for kind, gamma in POINT_KINDS:
            f.compare(kind_name(kind, gamma), kind, gamma=gamma)
    finally:
        f.done()


@pytest.mark.parametrize("fname", TABLES)
@pytest.mark.parametrize("W,H", FRAMES)
def test_window_filter_sum(gpu, fixtures, W, H, fname):
    f = Frame(W, H)
    try:
        for r in RADII:
            f.compare(f"window {fname} r={r}", capi.FILTER_WINDOW, weights(fixtures, fname), r)
    finally:
        f.done()


def test_filters_mix(gpu, fixtures):
    """accumMode != 0: the texels are running means and are not divided (their fourth channel is ignored)"""
    f = Frame(17, 33, mix=True)
    try:
        assert not np.array_equal(f.mean[..., :3], mean_image(accumulator(17, 33), False)[..., :3], equal_nan=True)
        for kind, gamma in POINT_KINDS:
            f.compare(kind_name(kind, gamma), kind, gamma=gamma)
        for fname in TABLES:
            for r in MIX_RADII:
                f.compare(f"window {fname} r={r}", capi.FILTER_WINDOW, weights(fixtures, fname), r)
    finally:
        f.done()


# ---- wavelet / normal / position over frames whose texels mostly (N1S) or all (N0) miss the scene -----------------------
@pytest.mark.parametrize("name,W,H", [("N1S", 33, 17), ("N0", 24, 16)])
def test_aov_filters_over_missed_texels(gpu, fixtures, name, W, H):
    sc = fixtures["scenes"][name]
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), W, H, 0, 3)
    ctx = capi.Context(W, H, flags=capi.FLAG_AOV)
    bad = []
    try:
        ctx.set_scene_dict(sc)
        ctx.render_schedule(inv, seeds, sc["eye"], 3)
        mean, nrm, pos = ctx.readback(aov=True)
        miss = np.isnan(pos[..., :3]).any(axis=-1)
        print(f"{name} {W}x{H}: {int(miss.sum())} of {miss.size} texels carry a NaN position")
        if name == "N0":
            assert miss.all()
        else:
            assert miss.any() and np.isfinite(pos[..., :3]).all(axis=-1).any()
        for kind, r in [(capi.FILTER_WAVELET, (2.0, 2.0)), (capi.FILTER_WAVELET, (3.5, 1.25)),
                        (capi.FILTER_NORMAL, (0.0, 0.0)), (capi.FILTER_POSITION, (0.0, 0.0))]:
            got, got8 = ctx.filter(kind, None, r[0], r[1], 2.2, want_u8=True)
            want = oracle.filter_aov(mean, nrm, pos, kind, r[0], r[1])
            same = bit_equal(got, want)
            same8 = (got8[..., :3] == rgba8(want)) & (got8[..., 3:4] == 255)
            print(f"{name} {W}x{H} kind {kind} r={r}: {miss.size} texels ({int(np.isnan(want).any(axis=-1).sum())} with a NaN), "
                  f"{int((~same).sum())} f32 and {int((~same8).sum())} RGBA8 channel mismatches")
            if not (same.all() and same8.all()):
                bad.append(f"kind {kind} r={r}: {int((~same).sum())} f32, {int((~same8).sum())} RGBA8 channels")
    finally:
        ctx.close()
    assert not bad, f"{name} {W}x{H}: " + "; ".join(bad)
