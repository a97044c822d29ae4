"""The 3x3 variance prefilter and the a-trous passes of include/sail_hip.h (sail_denoise; sail_temporal_filter runs the
same passes) in numpy float32, one operation at a time, the tap loops in the stated order and vectorised over pixels: what
tests/test_gpu_denoise.py's and tests/temporal_filter_ref.py's references share. Written from the header, not from the
kernels. Every operation is an IEEE f32 one (the weights are rational, no exp), so the device's maps must equal these bit
for bit."""
import numpy as np

F = np.float32


def lum(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3)


def shifted(a, dy, dx, fill):
    """(a[y + dy, x + dx] with `fill` outside the frame, mask of the taps inside it)"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    if abs(dy) < H and abs(dx) < W:
        dst = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
        src = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
        out[dst] = a[src]
        inside[dst] = True
    return out, inside


def prefilter(v0):
    """the 3x3 prefilter of the raw variance: taps outside the frame or not finite are skipped"""
    shape = v0.shape
    acc, wsum = np.zeros(shape, F), np.zeros(shape, F)
    g = (F(0.25), F(0.125), F(0.0625))
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, inside = shifted(v0, dy, dx, F(np.nan))
                ok = inside & np.isfinite(vq)
                w = g[abs(dy) + abs(dx)]
                acc = np.where(ok, acc + w * vq, acc)
                wsum = np.where(ok, wsum + w, wsum)
        v = np.where(wsum > F(0), acc / wsum, F(0)).astype(F)
    assert v.dtype == F
    return v


def atrous(c, v, nd, x, iterations=4, sigma_l=1.0, sigma_x=0.2):
    """the a-trous passes, steps 1, 2, 4, ..., over (c, v) with the guides nd (decoded normal) and x (position)"""
    sl, sx = F(sigma_l), F(sigma_x)
    kk = (F(0.375), F(0.25), F(0.0625))
    with np.errstate(all="ignore"):
        for it in range(iterations):
            s = 1 << it
            den = (sl * sl) * v + F(1e-8)
            sxs = (sx * F(s)) * (sx * F(s))
            lp = lum(c)
            acc, vacc, wsum = np.zeros_like(c), np.zeros_like(v), np.zeros_like(v)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, inside = shifted(c, s * dy, s * dx, F(0))
                    if not inside.any():
                        continue
                    vq, _ = shifted(v, s * dy, s * dx, F(0))
                    kw = kk[abs(dy)] * kk[abs(dx)]
                    if dy == 0 and dx == 0:
                        w = np.full(v.shape, kw, F)
                    else:
                        nq, _ = shifted(nd, s * dy, s * dx, F(0))
                        xq, _ = shifted(x, s * dy, s * dx, F(0))
                        d = np.fmax((nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2], F(0))
                        for _ in range(6):
                            d = d * d
                        t = x - xq
                        dx2 = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
                        wx = F(1) / (F(1) + dx2 / sxs)
                        dq = lp - lum(cq)
                        wl = F(1) / (F(1) + (dq * dq) / den)
                        w = ((kw * d) * wx) * wl
                    ok = inside & (w > F(0)) & np.isfinite(cq).all(axis=-1) & np.isfinite(vq)
                    acc = np.where(ok[..., None], acc + w[..., None] * cq, acc)
                    vacc = np.where(ok, vacc + (w * w) * vq, vacc)
                    wsum = np.where(ok, wsum + w, wsum)
            upd = wsum > F(0)
            c = np.where(upd[..., None], acc / wsum[..., None], c).astype(F)
            v = np.where(upd, vacc / (wsum * wsum), v).astype(F)
    assert c.dtype == F and v.dtype == F
    return c, v
