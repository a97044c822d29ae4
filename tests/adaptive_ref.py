"""numpy restatement of the adaptive-sampling rules of include/sail_hip.h (sail_plan_adaptive, sail_render_adaptive), shared
by the host and the GPU tests. Everything here is computed from a *uniform* render's data, never from the masked code."""
import numpy as np


def tiles64(W, H):
    return (W + 63) // 64, (H + 63) // 64


def tile_pixels(W, H):
    """(tilesY, tilesX) in-frame pixels of each 64x64 tile"""
    tx, ty = tiles64(W, H)
    w = np.minimum(64, W - 64 * np.arange(tx))
    h = np.minimum(64, H - 64 * np.arange(ty))
    return (h[:, None] * w[None, :]).astype(np.int64)


def tile_slices(W, H):
    """[(t, slice y, slice x)] of every 64x64 tile, t = ty * tilesX + tx, row 0 = bottom (the frame arrays' row 0)"""
    tx, ty = tiles64(W, H)
    return [(j * tx + i, slice(j * 64, min(H, j * 64 + 64)), slice(i * 64, min(W, i * 64 + 64)))
            for j in range(ty) for i in range(tx)]


def e64(tile_err16, W, H):
    """per 64x64 tile: sum of (double) err16 * px / sum of px over its in-frame 16x16 tiles, rows outer, in index order"""
    e16 = np.asarray(tile_err16, np.float32).reshape((H + 15) // 16, (W + 15) // 16)
    tx, ty = tiles64(W, H)
    out = np.zeros((ty, tx))
    for j in range(ty):
        for i in range(tx):
            s = p = 0.0
            for v in range(j * 4, min(j * 4 + 4, e16.shape[0])):
                for u in range(i * 4, min(i * 4 + 4, e16.shape[1])):
                    px = min(16, W - u * 16) * min(16, H - v * 16)
                    s += float(e16[v, u]) * px
                    p += px
            out[j, i] = s / p
    return out


def plan(W, H, tile_err16, target, dilate, prev=None):
    """(active, e64): active = prev and (noisy or (dilate and a noisy neighbour)), noisy = not (e64 <= target)"""
    e = e64(tile_err16, W, H)
    noisy = ~(e <= target)
    keep = noisy.copy()
    if dilate:
        ty, tx = noisy.shape
        pad = np.zeros((ty + 2, tx + 2), bool)
        pad[1:-1, 1:-1] = noisy
        for dj in range(3):
            for di in range(3):
                keep |= pad[dj:dj + ty, di:di + tx]
    prev = np.ones_like(keep) if prev is None else np.asarray(prev).reshape(keep.shape) != 0
    return (prev & keep).astype(np.uint8), e


def freeze_schedule(W, H, looks, tile_err_by_look, target, dilate, start=None):
    """The driver's outcome from a uniform run: looks = the sample indices of the looks, tile_err_by_look[j] the uniform
    tile_err map of look j (j >= 1; look 0 only marks). An active tile's (P, S) pair is the uniform one, so its error is;
    a frozen tile was not noisy when it froze and reads the same bits ever after, so it stays not noisy.
    Returns (freeze look index per tile, or len(looks) - 1 for tiles active to the end; final active; pixel_samples)."""
    tx, ty = tiles64(W, H)
    px = tile_pixels(W, H)
    active = np.ones((ty, tx), np.uint8) if start is None else (np.asarray(start).reshape(ty, tx) != 0).astype(np.uint8)
    frozen_at = np.full((ty, tx), -1)
    frozen_at[active == 0] = 0
    pixel_samples, k = 0, 0
    last = 0
    for j, kj in enumerate(looks):
        if not active.any():
            break
        pixel_samples += int(px[active != 0].sum()) * (kj - k)
        k = kj
        last = j
        if j == 0:
            continue
        err = np.where(np.repeat(np.repeat(active, 4, 0), 4, 1)[:(H + 15) // 16, :(W + 15) // 16] != 0,
                       np.asarray(tile_err_by_look[j], np.float32), np.float32(0))  # frozen tiles: not noisy
        nxt, _ = plan(W, H, err, target, dilate, active)
        frozen_at[(active != 0) & (nxt == 0)] = j
        active = nxt
    frozen_at[active != 0] = last
    return frozen_at, active, pixel_samples
