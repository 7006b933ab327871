"""numpy restatement of the GIF export's stages behind the median cut (csrc/gif_refine.hip, gsdd_amd.gif): one Lloyd assignment pass
with its squared error, the refinement that strings N + 1 of them together and keeps the best palette, and Floyd-Steinberg error
diffusion.  On top of tests/gif_ref.py and a plain module like it: integer arithmetic throughout, so every comparison is equality."""
import numpy as np

import gif_ref


def nearest(px, pal):
    """px (P, 3), pal (n, 3) integers, n > 0 -> (index (P,), squared distance (P,)): the first of the smallest distances"""
    d = ((px[:, None, :].astype(np.int64) - pal[None].astype(np.int64)) ** 2).sum(-1)
    idx = np.argmin(d, axis=1)                             # (argmin returns the first minimum)
    return idx, d[np.arange(px.shape[0]), idx]


def palette_sums(levels, palette, n_colors, per_frame=False):
    """levels (B, T, H, W, 3) uint8, palette (G, 256, 3+) uint8, n_colors (G,) -> (sums (G, 256, 4) uint32: count and R, G, B sums of
    the pixels nearest to each of the first n_colors entries, sse (G,) uint64: their total squared distance); zeros with n_colors <= 0"""
    grp = gif_ref.groups_of(levels, per_frame)
    sums = np.zeros((grp.shape[0], 256, 4), dtype=np.int64)
    sse = np.zeros(grp.shape[0], dtype=np.uint64)
    for g, px in enumerate(grp):
        n = min(int(n_colors[g]), 256)
        if n <= 0:
            continue
        idx, d = nearest(px, np.asarray(palette[g])[:n, :3])
        sums[g, :, 0] = np.bincount(idx, minlength=256)
        for c in range(3):
            sums[g, :, 1 + c] = np.bincount(idx, weights=px[:, c].astype(np.float64), minlength=256).astype(np.int64)
        sse[g] = int(d.sum())
    assert sums.max() < 2 ** 32
    return sums.astype(np.uint32), sse


def next_palette(palette, sums):
    """the rounded mean (2*sum + count) // (2*count) of each entry's pixels; an entry with no pixel keeps its colour"""
    s = sums.astype(np.int64)
    count = s[..., :1]
    return np.where(count > 0, (2 * s[..., 1:] + count) // np.maximum(2 * count, 1), np.asarray(palette)[..., :3]).astype(np.uint8)


def select(errors):
    """errors (N + 1, G) -> (G,): per group the pass of the smallest error, the earliest on ties"""
    return np.argmin(np.asarray(errors), axis=0)


def refine(levels, palette, n_colors, passes, per_frame=False):
    """-> (palette (G, 256, 3) uint8, errors (passes + 1, G) uint64): p_0 = palette, p_{k+1} = next_palette(p_k); errors[k] is p_k's;
    the result is per group the p_k that `select` picks"""
    pals, errors = [np.ascontiguousarray(np.asarray(palette)[..., :3])], []
    for k in range(passes + 1):
        sums, sse = palette_sums(levels, pals[-1], n_colors, per_frame)
        errors.append(sse)
        if k < passes:
            pals.append(next_palette(pals[-1], sums))
    errors = np.stack(errors)
    pick = select(errors)
    return np.stack([pals[k][g] for g, k in enumerate(pick)]), errors


def diffuse(levels, palette, n_colors, per_frame=False):
    """Floyd-Steinberg per frame -> (B, T, H, W) uint8.  Every frame starts with no error and errors outside the frame are 0; pixels
    left to right, rows top to bottom; per channel acc = 7 e(y,x-1) + 3 e(y-1,x+1) + 5 e(y-1,x) + e(y-1,x-1),
    target = clamp(level + ((acc + 8) >> 4), 0, 255) with an arithmetic shift; the index is the nearest entry of target (the lowest on
    ties), e(y,x) = target - palette[index]; index 0 everywhere with n_colors <= 0"""
    B, T, H, W, _ = levels.shape
    out = np.zeros((B, T, H, W), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            g = b * T + t if per_frame else b
            n = min(int(n_colors[g]), 256)
            if n <= 0:
                continue
            pal = np.asarray(palette[g])[:n, :3].astype(np.int64)
            lv = levels[b, t].astype(np.int64)
            e = np.zeros((H + 1, W + 2, 3), dtype=np.int64)        # e[y + 1, x + 1]: a border of zeros above, left and right
            for y in range(H):
                for x in range(W):
                    acc = 7 * e[y + 1, x] + 3 * e[y, x + 2] + 5 * e[y, x + 1] + e[y, x]
                    target = np.clip(lv[y, x] + ((acc + 8) >> 4), 0, 255)
                    d = ((pal - target) ** 2).sum(-1)
                    i = int(np.argmin(d))
                    out[b, t, y, x] = i
                    e[y + 1, x + 1] = target - pal[i]
    return out


def block_mean_rms(shown, levels, block=4):
    """RMS over blocks and channels of the difference of the block x block means of (B, T, H, W, 3) images: what dither is for"""
    def means(a):
        B, T, H, W, C = a.shape
        return a.astype(np.float64).reshape(B, T, H // block, block, W // block, block, C).mean(axis=(3, 5))
    return float(np.sqrt(np.mean((means(shown) - means(levels)) ** 2)))
