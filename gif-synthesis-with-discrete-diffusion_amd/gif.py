"""Sampled clips as GIF files: colour quantisation on the device, median cut and the GIF89a / LZW writer in the library's host code.

    clips (B, 3, T, H, W), ImageNet-normalised fp32 on the device (what the decoder returns)
      -> gsdd_gif_histogram          15-bit colour histogram per group (a clip, or a frame with palette="frame")
      -> one device-to-host copy     G x 128 KB
      -> gsdd_gif_median_cut         (host, integer, deterministic) bin -> box table per group
      -> gsdd_gif_box_sums           count and R, G, B sums per box; the palette is the rounded mean, formed with integer torch ops
      -> gsdd_gif_palette_sums       (refine = N > 0) N + 1 Lloyd assignment passes; the palette of smallest squared error is kept
      -> gsdd_gif_map                nearest palette entry per pixel (optional ordered dither), or
         gsdd_gif_diffuse            (dither = "fs") Floyd-Steinberg error diffusion within each frame
      -> gsdd_gif_delta              (optimize) per pixel the transparent index where the displayed colour stays; a box per frame
      -> gsdd_gif_encode             (host) GIF89a file; gsdd_gif_encode_delta writes the delta frames

Every stage is integer arithmetic behind one fp32 step (the evaluator's uint8 rule), so the indices, the palette and the file's bytes
are exactly reproducible; tests/gif_ref.py, tests/gif_refine_ref.py and tests/gif_delta_ref.py restate all of it in numpy.

The way back is probe_gif / read_gif at the end of this file: a GIF file -> uint8 frames (T, H, W, 3) on the device.

Synchronisation: quantize_clips synchronises ONCE, for the histogram the host's median cut reads (encode_gif / write_gifs copy the
indices to the host as well, which is the point of them).  Rendering happens outside the sampling loop and must stay outside any
captured graph: none of this can be recorded."""
import contextlib
import math
import os

import numpy as np
import torch

from . import ops
from ._lib import GsddError


def _check_quantize(colors, palette, dither, refine):
    """the argument checks of quantize_clips, before any device call"""
    if palette not in ("clip", "frame"):
        raise GsddError(f'quantize_clips: palette is "clip" or "frame", got {palette!r}')
    if not isinstance(colors, int) or isinstance(colors, bool) or not 2 <= colors <= 256:
        raise GsddError(f"quantize_clips: colors is an integer in 2 .. 256, got {colors!r}")
    if dither != "fs" and (not isinstance(dither, int) or isinstance(dither, bool) or not 0 <= dither <= 64):
        raise GsddError(f'quantize_clips: dither is an integer amplitude in 0 .. 64 or "fs", got {dither!r}')
    if not isinstance(refine, int) or isinstance(refine, bool) or not 0 <= refine <= 32:
        raise GsddError(f"quantize_clips: refine is an integer number of passes in 0 .. 32, got {refine!r}")


def select_palette(palettes, errors):
    """palettes: N + 1 tensors (G, 256, C), errors: N + 1 tensors (G,) -> per group the palette of the smallest error, the earliest on
    ties (a later one replaces the choice only when strictly better); torch.where on the tensors' device, no synchronisation"""
    best, best_err = palettes[0], errors[0]
    for pal, err in zip(palettes[1:], errors[1:]):
        better = err < best_err
        best = torch.where(better[:, None, None], pal, best)
        best_err = torch.where(better, err, best_err)
    return best


def refine_palette(clips, pal4, n_colors, passes, per_frame=False):
    """Lloyd passes from pal4 (G, 256, 4) uint8 = p_0: `passes` + 1 gsdd_gif_palette_sums launches give the errors of p_0 .. p_N,
    p_{k+1} being the rounded mean (2*sum + count) // (2*count) of the pixels nearest to each entry of p_k (an entry with none keeps its
    colour).  Rounding a centroid can raise the error, so the result is per group the p_k of smallest error, the earliest on ties:
    never worse than p_0.  -> (palette (G, 256, 4) uint8, errors (passes + 1, G) int64); integer torch ops on the device, no
    synchronisation."""
    palettes, errors = [pal4], []
    for k in range(passes + 1):
        sums, sse = ops.gif_palette_sums(clips, palettes[-1], n_colors, per_frame)
        errors.append(sse)
        if k < passes:
            sums = sums.to(torch.int64) & 0xFFFFFFFF
            count = sums[..., :1]
            mean = (2 * sums[..., 1:] + count) // (2 * count).clamp(min=1)
            nxt = palettes[-1].clone()
            nxt[..., :3] = torch.where(count > 0, mean.to(torch.uint8), nxt[..., :3])
            palettes.append(nxt)
    return select_palette(palettes, errors).contiguous(), torch.stack(errors)


def quantize_clips(clips, colors=256, palette="clip", dither=0, refine=0):
    """clips (B, 3, T, H, W) -> (indices (B, T, H, W) uint8 on the device, palette (G, 256, 3) uint8 on the device, n_colors (G,) int32
    on the device).  G = B with palette="clip" (one palette per clip), B*T with palette="frame" (one per frame, group b*T + t).
    colors: at most this many palette entries, 2 .. 256; entries behind n_colors[g] are zeros.  refine: k-means passes from the
    median cut's palette, 0 .. 32 (refine_palette; n_colors does not change).  dither: ordered-dither amplitude 0 .. 64, 0 = off, or
    "fs": Floyd-Steinberg error diffusion within each frame (gsdd_gif_diffuse)."""
    _check_quantize(colors, palette, dither, refine)
    per_frame = palette == "frame"
    clips = clips.contiguous() if torch.is_tensor(clips) else clips
    hist = ops.gif_histogram(clips, per_frame)
    hist_host = hist.cpu().numpy().view(np.uint32)                     # the one synchronisation
    G = hist_host.shape[0]
    box = np.empty((G, ops.GIF_BINS), dtype=np.uint8)
    n = np.empty(G, dtype=np.int32)
    for g in range(G):
        box[g], n[g] = ops.gif_median_cut(hist_host[g], colors)
    dev = clips.device
    sums = ops.gif_box_sums(clips, torch.from_numpy(box).to(dev), per_frame).to(torch.int64) & 0xFFFFFFFF
    count = sums[..., :1]
    mean = (2 * sums[..., 1:] + count) // (2 * count).clamp(min=1)     # rounded mean; an empty box gives 0
    pal4 = torch.zeros((G, 256, 4), dtype=torch.uint8, device=dev)
    pal4[..., :3] = mean.to(torch.uint8)
    n_dev = torch.from_numpy(n).to(dev)
    if refine:
        pal4, _ = refine_palette(clips, pal4, n_dev, refine, per_frame)
    indices = ops.gif_diffuse(clips, pal4, n_dev, per_frame) if dither == "fs" else ops.gif_map(clips, pal4, n_dev, per_frame, dither)
    return indices, pal4[..., :3].contiguous(), n_dev


def palette_error(clips, palette, n_colors, palette_mode="clip"):
    """-> sse (G,) int64 on the device: the squared distance of every pixel of a group to its nearest palette entry (no dither), summed
    over the group.  palette (G, 256, 3) as quantize_clips returns it, or (G, 256, 4)."""
    if palette_mode not in ("clip", "frame"):
        raise GsddError(f'palette_error: palette_mode is "clip" or "frame", got {palette_mode!r}')
    if not torch.is_tensor(palette) or palette.dim() != 3 or palette.shape[-1] not in (3, 4):
        raise GsddError("palette_error: palette must be uint8 (G, 256, 3) or (G, 256, 4)")
    if palette.shape[-1] == 3:
        palette = torch.cat([palette, torch.zeros_like(palette[..., :1])], dim=-1)
    clips = clips.contiguous() if torch.is_tensor(clips) else clips
    return ops.gif_palette_sums(clips, palette.contiguous(), n_colors, palette_mode == "frame")[1]


def psnr_from_sse(sse, values):
    """the PSNR in dB of a squared error `sse` summed over `values` uint8 values (3 per pixel); inf for sse = 0"""
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 ** 2 * values / float(sse))


def delay_centiseconds(fps):
    """round(100 / fps), the GIF's per-frame delay; an fps that rounds to 0 (or to more than 65535) is an error"""
    if not fps > 0:
        raise GsddError(f"fps must be positive, got {fps!r}")
    delay = int(round(100.0 / fps))
    if not 1 <= delay <= 65535:
        raise GsddError(f"fps = {fps!r} gives a delay of {delay} centiseconds: a GIF holds 1 .. 65535")
    return delay


def delta_frames(clips, indices, palette, n_colors, palette_mode="clip", tolerance=0):
    """The delta stage behind quantize_clips (gsdd_gif_delta; the rule: include/gsdd.h): -> (out (B, T, H, W) uint8: `indices` with the
    group's free index n_colors[g] wherever a pixel keeps the colour it shows -- or, with tolerance > 0 (a squared RGB distance, at most
    195075), shows a colour within the tolerance of its level --, rects (B, T, 4) int32: the bounding box x0, y0, x1, y1 of each frame's
    changed pixels, (W, H, -1, -1) for none, changed (B, T) int32: their number, transparent (G,) int32: n_colors[g], or -1 for a group
    of 256 colours, whose frames are cropped only).  All on the device, no synchronisation.  palette (G, 256, 3) as quantize_clips
    returns it, or (G, 256, 4)."""
    if palette_mode not in ("clip", "frame"):
        raise GsddError(f'delta_frames: palette_mode is "clip" or "frame", got {palette_mode!r}')
    if not torch.is_tensor(palette) or palette.dim() != 3 or palette.shape[-1] not in (3, 4):
        raise GsddError("delta_frames: palette must be uint8 (G, 256, 3) or (G, 256, 4)")
    if palette.shape[-1] == 3:
        palette = torch.cat([palette, torch.zeros_like(palette[..., :1])], dim=-1)
    clips = clips.contiguous() if torch.is_tensor(clips) else clips
    out, rects, changed = ops.gif_delta(clips, indices, palette.contiguous(), n_colors, palette_mode == "frame", tolerance)
    return out, rects, changed, torch.where(n_colors < 256, n_colors, torch.full_like(n_colors, -1))


def encode_gif(indices, palette, n_colors, fps=5, loop=0, rects=None, transparent=None):
    """One clip -> the bytes of a GIF89a file.  indices (T, H, W) uint8; palette (256, 3) with n_colors an int or a 1-element tensor (a
    global colour table) or palette (T, 256, 3) with n_colors (T,) (one local table per frame); tensors on any device, or numpy.
    rects (T, 4) and transparent (an int, or one per table), both or neither: one clip's delta frames (delta_frames) are written as
    sub-images with a transparent index (gsdd_gif_encode_delta)."""
    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if (rects is None) != (transparent is None):
        raise GsddError("encode_gif: rects and transparent come together (delta_frames returns both)")
    idx, pal = host(indices), host(palette)
    if pal.ndim == 2:
        pal = pal[None]
    n = np.asarray(host(n_colors), dtype=np.int32).reshape(-1)
    if rects is None:
        data, _ = ops.gif_encode(idx, pal, n, delay_centiseconds(fps), loop)
    else:
        data, _ = ops.gif_encode_delta(idx, pal, n, host(rects), np.asarray(host(transparent), dtype=np.int32).reshape(-1),
                                       delay_centiseconds(fps), loop)
    return data


def write_gifs(clips, paths, fps=5, loop=0, optimize=False, tolerance=0, **quantize_kwargs):
    """Quantise clips (B, 3, T, H, W) and write clip b to paths[b] (directories are created).  -> (indices, palette, n_colors) of
    quantize_clips.  optimize: write delta frames (delta_frames) -- the same pictures in a smaller file; tolerance > 0 (with optimize
    only) also keeps a pixel whose level is within that squared RGB distance of what it shows.  A group needs a free palette index for
    transparency: `colors` stays as given, and a group that took all 256 gets cropping only (colors=255 leaves one free)."""
    paths = list(paths)
    if not torch.is_tensor(clips) or clips.dim() != 5 or len(paths) != clips.shape[0]:
        raise GsddError("write_gifs: one path per clip of (B, 3, T, H, W)")
    if tolerance != 0 and not optimize:
        raise GsddError("write_gifs: tolerance needs optimize=True")
    delay_centiseconds(fps)
    indices, palette, n_colors = quantize_clips(clips, **quantize_kwargs)
    B, T = indices.shape[:2]
    pal, n = palette.cpu().numpy(), n_colors.cpu().numpy()
    per_frame = quantize_kwargs.get("palette", "clip") == "frame"
    if optimize:
        out, rects, _, transparent = delta_frames(clips, indices, palette, n_colors, "frame" if per_frame else "clip", tolerance)
        idx, rects, transparent = out.cpu().numpy(), rects.cpu().numpy(), transparent.cpu().numpy()
    else:
        idx = indices.cpu().numpy()
    for b, path in enumerate(paths):
        rows = slice(b * T, (b + 1) * T) if per_frame else slice(b, b + 1)
        if optimize:
            data, _ = ops.gif_encode_delta(idx[b], pal[rows], n[rows], rects[b], transparent[rows], delay_centiseconds(fps), loop)
        else:
            data, _ = ops.gif_encode(idx[b], pal[rows], n[rows], delay_centiseconds(fps), loop)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    return indices, palette, n_colors


# ----------------------------------------------------------------------------- reading
# The way back: the host walks the file and decodes the LZW streams (gsdd_gif_decode, the serial part), the device composites the
# frame rectangles onto the canvas -- transparency, disposal -- and expands the indices to RGB (gsdd_gif_compose).  What crosses to
# the device is one byte per DRAWN pixel and the small tables, not three bytes per canvas pixel per frame.
def _gif_file(what, path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        return path_or_bytes, "<bytes>"
    try:
        with open(path_or_bytes, "rb") as f:
            return f.read(), os.fspath(path_or_bytes)
    except (OSError, TypeError) as e:
        raise GsddError(f"{what}: cannot read {path_or_bytes!r}: {e}")


def probe_gif(path_or_bytes):
    """A GIF's block structure, without decoding it -> dict of width, height, frames, palettes (colour tables), raster_bytes (the sum
    of the frame rectangles' areas), loop (-1: no loop extension), global_table, version (87 / 89)."""
    data, name = _gif_file("probe_gif", path_or_bytes)
    try:
        return ops.gif_probe(data)
    except GsddError as e:
        raise GsddError(f"probe_gif: {name}: {e}")


def read_gif(path_or_bytes, device, frames=None, matte=(0, 0, 0), stream=None):
    """-> (uint8 (T, H, W, 3) on the device -- what data.preprocess takes --, the delays of the returned frames in centiseconds, info
    of probe_gif).  frames: the frame numbers to return, non-decreasing, repeats allowed (a short clip padded with its last frame);
    default: every frame.  matte: the (R, G, B) of pixels nothing has drawn yet and of disposal 2.  A host decode, one host-to-device
    copy each of the index rasters and of the tables, one launch; no device-to-host copy, no synchronisation."""
    device = torch.device(device)
    if device.type != "cuda":
        raise GsddError("read_gif: the compositor runs on a ROCm device (no CPU fallback)")
    data, name = _gif_file("read_gif", path_or_bytes)
    try:
        table, delays, palettes, raster, info = ops.gif_decode(data)
    except GsddError as e:
        raise GsddError(f"read_gif: {name}: {e}")
    F = info["frames"]
    try:
        select = np.arange(F, dtype=np.int32) if frames is None else np.asarray(list(frames), dtype=np.int64).astype(np.int32)
    except (TypeError, ValueError, OverflowError):
        raise GsddError(f"read_gif: frames is a list of frame numbers, got {frames!r}")
    if select.ndim != 1 or select.size < 1 or select.min() < 0 or select.max() >= F or np.any(np.diff(select) < 0):
        raise GsddError(f"read_gif: {name}: frames must be a non-empty non-decreasing list within 0 .. {F - 1}, got {frames!r}")
    # the tables travel as one buffer: palettes | frame table | select (each a multiple of four bytes)
    parts = (palettes.reshape(-1), table.reshape(-1).view(np.uint8), select.view(np.uint8))
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        raster_dev = torch.from_numpy(raster).to(device)
        tables_dev = torch.from_numpy(np.concatenate(parts)).to(device)
    a, b = parts[0].size, parts[0].size + parts[1].size
    out = ops.gif_compose(raster_dev, tables_dev[a:b].view(torch.int32).view(F, 8), tables_dev[:a].view(-1, 256, 4), info["width"],
                          info["height"], select, matte, stream=stream, select_dev=tables_dev[b:].view(torch.int32))
    return out, [int(delays[f]) for f in select], info
