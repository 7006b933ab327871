"""numpy restatement of the GIF export's delta stage (csrc/gif_delta.hip, gsdd_amd.gif.delta_frames; the rule: include/gsdd.h), on top of
tests/gif_ref.py: per pixel `shown`, the RGB it displays, walked over the frames.  Plain module (not a conftest).  Integer arithmetic
behind the uint8 rule, so every comparison is equality."""
import numpy as np

import gif_ref

MAX_TOLERANCE = 3 * 255 * 255


def transparent_of(n_colors):
    """(G,) -> (G,) int32: the group's free index n_colors[g], or -1 when all 256 are taken"""
    n = np.asarray(n_colors, dtype=np.int32)
    return np.where(n < 256, n, -1).astype(np.int32)


def delta(levels, indices, palette, n_colors, per_frame=False, tolerance=0):
    """levels (B, T, H, W, 3) uint8 (the uint8 rule of the clips, no dither offset), indices (B, T, H, W) uint8, palette (G, 256, 3+),
    n_colors (G,) -> (out (B, T, H, W) uint8, rects (B, T, 4) int32, changed (B, T) uint32, transparent (G,) int32, displayed
    (B, T, H, W, 3) uint8: what a viewer shows after each frame)"""
    B, T, H, W = indices.shape
    transparent = transparent_of(n_colors)
    out = np.empty((B, T, H, W), dtype=np.uint8)
    rects = np.empty((B, T, 4), dtype=np.int32)
    changed = np.empty((B, T), dtype=np.uint32)
    displayed = np.empty((B, T, H, W, 3), dtype=np.uint8)
    for b in range(B):
        shown = np.zeros((H, W, 3), dtype=np.int64)
        for t in range(T):
            g = b * T + t if per_frame else b
            tr = int(transparent[g])
            idx = indices[b, t]
            c = np.asarray(palette[g])[:, :3].astype(np.int64)[idx]
            if t == 0:
                unchanged = np.zeros((H, W), dtype=bool)
            else:
                unchanged = np.all(c == shown, axis=-1)
                if tolerance > 0 and tr >= 0:
                    d2 = ((levels[b, t].astype(np.int64) - shown) ** 2).sum(-1)
                    unchanged |= d2 <= tolerance
            out[b, t] = np.where(unchanged & (tr >= 0), np.uint8(tr & 255), idx)
            shown = np.where(unchanged[..., None], shown, c)
            ys, xs = np.nonzero(~unchanged)
            rects[b, t] = (xs.min(), ys.min(), xs.max(), ys.max()) if xs.size else (W, H, -1, -1)
            changed[b, t] = xs.size
            displayed[b, t] = shown
    return out, rects, changed, transparent, displayed


def decode_displayed(out, rects, palette, transparent, per_frame_tables=False):
    """what a GIF viewer shows for one clip written from (out (T, H, W), rects (T, 4), palette (1 or T, 256, 3), transparent (1 or T,))
    with disposal 1: inside each rectangle every index other than the transparent one paints its colour -> (T, H, W, 3) uint8"""
    T, H, W = out.shape
    canvas = np.zeros((H, W, 3), dtype=np.uint8)
    frames = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        p = t if per_frame_tables else 0
        x0, y0, x1, y1 = (int(v) for v in rects[t])
        if x1 < 0:
            x0 = y0 = x1 = y1 = 0
        idx = out[t, y0:y1 + 1, x0:x1 + 1]
        rgb = np.asarray(palette[p])[:, :3][idx]
        region = canvas[y0:y1 + 1, x0:x1 + 1]
        canvas[y0:y1 + 1, x0:x1 + 1] = np.where((idx != int(transparent[p]))[..., None], rgb, region)
        frames[t] = canvas
    return frames


def moving_square_levels(T=8, HW=32, square=8, noise=0, seed=0):
    """(1, T, HW, HW, 3) uint8: a constant background (90, 140, 200) and a `square` x `square` block of (230, 60, 30) that moves three
    pixels right and two down a frame; with `noise`, uniform integer noise of +-noise levels on every channel"""
    v = np.empty((1, T, HW, HW, 3), dtype=np.int64)
    v[:] = (90, 140, 200)
    for t in range(T):
        v[0, t, 2 + 2 * t:2 + 2 * t + square, 1 + 3 * t:1 + 3 * t + square] = (230, 60, 30)
    if noise:
        v = v + np.random.default_rng(seed).integers(-noise, noise + 1, v.shape)
    return np.clip(v, 0, 255).astype(np.uint8)
