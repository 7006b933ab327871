"""numpy restatement of the GIF export's quantiser (csrc/gif.hip, csrc/gif_host.hpp, gsdd_amd.gif.quantize_clips), stage by stage: the
uint8 rule, the 15-bit bins, the median cut, the box means, the Bayer offset and the nearest palette index with lowest-index ties.
Plain module (not a conftest): the host tests check the library's median cut and the restatement's quality against it, the GPU tests
use it as the exact reference of every kernel.  Everything behind the uint8 rule is integer arithmetic, so every comparison is
equality."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
BINS = 32768


def clips_from_levels(levels):
    """uint8 levels (B, T, H, W, 3) -> ImageNet-normalised float32 clips (B, 3, T, H, W) whose uint8 levels are `levels`: built from
    the middle of each level's interval, ((u + 0.5) / 255 - mean) / std, so that no value sits on a truncation boundary."""
    u = np.asarray(levels).astype(np.float64)
    x = ((u + 0.5) / 255.0 - MEAN.astype(np.float64)) / STD.astype(np.float64)
    return np.ascontiguousarray(np.moveaxis(x, -1, 1).astype(np.float32))


def levels_of(clips):
    """the evaluator's uint8 rule on float32 clips (B, 3, T, H, W) -> (B, T, H, W, 3) uint8: v = (x*std + mean)*255 in fp32 in that
    order, clamped to [0, 255] with NaN -> 0, truncated"""
    x = np.moveaxis(np.asarray(clips, dtype=np.float32), 1, -1)
    v = (x * STD + MEAN) * np.float32(255.0)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(v), np.float32(0), np.clip(np.trunc(v), 0, 255))
    return v.astype(np.uint8)


def groups_of(levels, per_frame):
    """(B, T, H, W, 3) -> (G, P, 3): one row of pixels per group, in the order (t, y, x)"""
    B, T, H, W, _ = levels.shape
    return levels.reshape(B * T, H * W, 3) if per_frame else levels.reshape(B, T * H * W, 3)


def bins_of(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)


def histogram(levels, per_frame=False):
    grp = groups_of(levels, per_frame)
    return np.stack([np.bincount(bins_of(g), minlength=BINS) for g in grp]).astype(np.uint32)


def median_cut(hist, colors):
    """-> (box_of_bin (32768,) uint8, number of boxes).  The rules of gsdd_gif_median_cut, on sets of bins."""
    hist = np.asarray(hist).astype(np.int64)
    coords = np.stack([(np.arange(BINS) >> 10) & 31, (np.arange(BINS) >> 5) & 31, np.arange(BINS) & 31], axis=1)
    occupied = np.flatnonzero(hist)
    box_of_bin = np.full(BINS, 255, dtype=np.uint8)
    if occupied.size == 0:
        return box_of_bin, 0
    boxes = [occupied]
    while len(boxes) < colors:
        counts = [int(hist[b].sum()) if b.size > 1 else -1 for b in boxes]
        pick = int(np.argmax(counts))                      # (the first of equal maxima: the lowest index)
        if counts[pick] < 0:
            break
        b = boxes[pick]
        c = coords[b]
        extent = c.max(axis=0) - c.min(axis=0)
        axis = int(np.argmax(extent))                      # (R before G before B on ties)
        lo, hi = int(c[:, axis].min()), int(c[:, axis].max())
        plane = np.zeros(32, dtype=np.int64)
        np.add.at(plane, c[:, axis], hist[b])
        cum = np.cumsum(plane[lo:hi + 1])
        cut = lo + int(np.argmax(2 * cum >= counts[pick]))
        if cut >= hi:
            cut = hi - 1
        boxes[pick] = b[c[:, axis] <= cut]
        boxes.append(b[c[:, axis] > cut])
    for i, b in enumerate(boxes):
        box_of_bin[b] = i
    return box_of_bin, len(boxes)


def box_sums(levels, box_of_bin, per_frame=False):
    """box_of_bin (G, 32768) -> (G, 256, 4) uint32: count and R, G, B sums per box"""
    grp = groups_of(levels, per_frame)
    out = np.zeros((grp.shape[0], 256, 4), dtype=np.int64)
    for g, px in enumerate(grp):
        box = box_of_bin[g][bins_of(px)].astype(np.int64)
        out[g, :, 0] = np.bincount(box, minlength=256)
        for c in range(3):
            out[g, :, 1 + c] = np.bincount(box, weights=px[:, c].astype(np.float64), minlength=256).astype(np.int64)
    assert out.max() < 2 ** 32
    return out.astype(np.uint32)


def palette_of(sums):
    """(G, 256, 4) -> (G, 256, 3) uint8: the rounded mean (2*sum + count) // (2*count), zeros for an empty box"""
    s = sums.astype(np.int64)
    count = s[..., :1]
    return np.where(count > 0, (2 * s[..., 1:] + count) // np.maximum(2 * count, 1), 0).astype(np.uint8)


def bayer(x, y):
    """M(x, y) of the 8 x 8 Bayer matrix, 0 .. 63"""
    m = 0
    for i in range(3):
        m = m + (((((x >> i) ^ (y >> i)) & 1) << (2 * (2 - i) + 1)) | (((y >> i) & 1) << (2 * (2 - i))))
    return m


def dither_offsets(H, W, dither):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((bayer(x & 7, y & 7) * dither) >> 6) - (dither >> 1)


def map_indices(levels, palette, n_colors, per_frame=False, dither=0):
    """palette (G, 256, 3+) uint8, n_colors (G,) -> (B, T, H, W) uint8: the lowest index of the smallest squared distance among the
    first n_colors entries (index 0 when n_colors is 0)"""
    B, T, H, W, _ = levels.shape
    px = levels.astype(np.int64)
    if dither:
        px = np.clip(px + dither_offsets(H, W, dither)[None, None, :, :, None], 0, 255)
    out = np.zeros((B, T, H, W), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            g = b * T + t if per_frame else b
            n = int(n_colors[g])
            if n <= 0:
                continue
            pal = np.asarray(palette[g])[:n, :3].astype(np.int64)
            d = ((px[b, t][:, :, None, :] - pal[None, None]) ** 2).sum(-1)
            out[b, t] = np.argmin(d, axis=-1)              # (argmin returns the first minimum)
    return out


def quantize(clips, colors=256, palette="clip", dither=0):
    """gsdd_amd.gif.quantize_clips on float32 numpy clips -> (indices (B, T, H, W), palette (G, 256, 3), n_colors (G,))"""
    per_frame = palette == "frame"
    levels = levels_of(clips)
    hist = histogram(levels, per_frame)
    cuts = [median_cut(h, colors) for h in hist]
    box = np.stack([c[0] for c in cuts])
    n = np.array([c[1] for c in cuts], dtype=np.int32)
    pal = palette_of(box_sums(levels, box, per_frame))
    return map_indices(levels, pal, n, per_frame, dither), pal, n


def reconstruct(indices, palette, per_frame=False):
    """(B, T, H, W) indices -> (B, T, H, W, 3) uint8 colours"""
    B, T = indices.shape[:2]
    out = np.empty(indices.shape + (3,), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            out[b, t] = np.asarray(palette[b * T + t if per_frame else b])[:, :3][indices[b, t]]
    return out


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def synthetic_levels(noise=False):
    """the 4 x 32 x 32 test clip R = (8x + 10t) % 256, G = 8y % 256, B = (4(x + y) + 30t) % 256 as (1, 4, 32, 32, 3) uint8; with
    `noise`, plus normal noise of mean 0 and sigma 25 (numpy's default_rng(0)), rounded and clipped"""
    t, y, x = np.meshgrid(np.arange(4), np.arange(32), np.arange(32), indexing="ij")
    v = np.stack([(8 * x + 10 * t) % 256, (8 * y) % 256, (4 * (x + y) + 30 * t) % 256], axis=-1).astype(np.float64)
    if noise:
        v = np.clip(np.rint(v + np.random.default_rng(0).normal(0.0, 25.0, v.shape)), 0, 255)
    return v.astype(np.uint8)[None]
