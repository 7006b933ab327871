#!/usr/bin/env python3
"""Time of the GIF export (gsdd_amd.gif) on 16 clips of 16 frames of 128 x 128 -- ImageNet-normalised floats (16, 3, 16, 128, 128) as
the decoder returns them; a moving colour ramp with sigma-5 noise, so that neighbouring pixels share bins as video does -- per stage:
the three kernels (histogram, box sums, map without and with dither) with HIP events around each call, the whole quantize_clips (its
device-to-host copy, the host's median cuts and the palette included) and the host's encode of the 16 files by the wall clock.
Beside them, in the same run, the host baseline the export replaces: PIL's quantize(MEDIANCUT) per frame and save of the same clips
from their uint8 frames (the copy to the host not counted).  The stages behind the median cut the same way: one assignment pass of
the palette refinement (gsdd_gif_palette_sums), quantize_clips(refine=8) whole, the error diffusion (gsdd_gif_diffuse), and the path
users had for it, PIL's quantize(palette=..., dither=FLOYDSTEINBERG) per frame on the host with the same palettes; the PSNR before and
after the refinement comes from gif.palette_error.  The delta stage (gsdd_gif_delta, write_gifs(optimize=True)) last: its launch at
tolerance 0 and 48 with HIP events, and the host's encode of the 16 files from whole frames and from delta frames with their bytes --
on the clips above, where everything moves, and on a second set, the same ramp held still outside a moving 32 x 32 window with sigma-2
noise; both quantised to 255 colours, so that every clip has a free index for the transparent pixels.  Warm-up first, the cases in
alternating rounds (a drift of the clocks hits all alike), the median over the rounds reported with the spread; a round that takes longer than the time limit ends the run with
an error instead of hanging on.  usage: bench_gif.py [out.csv]"""
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from gsdd_amd import gif, ops

ROUNDS, WARMUP, ITERS, STEP_LIMIT_S = 7, 2, 5, 120.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters, events=True):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.monotonic()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    wall = time.monotonic() - t0
    if wall > STEP_LIMIT_S:
        raise SystemExit(f"bench_gif: {iters} calls took more than {STEP_LIMIT_S:.0f} s; giving up")
    return (e0.elapsed_time(e1) if events else wall * 1e3) / iters


def make_levels(B, T, HW):
    g = torch.Generator().manual_seed(0)
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(HW), torch.arange(HW), indexing="ij")
    base = torch.stack([(2 * x + 10 * t) % 256, (2 * y) % 256, ((x + y) + 30 * t) % 256], dim=-1).float()      # (T, H, W, 3)
    shift = torch.arange(B).view(B, 1, 1, 1, 1) * 9.0
    v = (base[None] + shift) % 256 + torch.randn((B, T, HW, HW, 3), generator=g) * 5.0
    return v.round().clamp(0, 255).to(torch.uint8)


def make_still_levels(B, T, HW, window=32):
    """the ramp of frame 0 held still, the moving ramp inside a window that travels six pixels right and four down a frame; sigma-2 noise"""
    g = torch.Generator().manual_seed(1)
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(HW), torch.arange(HW), indexing="ij")
    inside = (x >= 6 * t) & (x < 6 * t + window) & (y >= 4 * t) & (y < 4 * t + window)
    tt = torch.where(inside, t, torch.zeros_like(t))
    base = torch.stack([(2 * x + 10 * tt) % 256, (2 * y) % 256, ((x + y) + 30 * tt) % 256], dim=-1).float()
    shift = torch.arange(B).view(B, 1, 1, 1, 1) * 9.0
    v = (base[None] + shift) % 256 + torch.randn((B, T, HW, HW, 3), generator=g) * 2.0
    return v.round().clamp(0, 255).to(torch.uint8)


def to_clips(levels):
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    return (((levels.double() + 0.5) / 255 - mean) / std).permute(0, 4, 1, 2, 3).float().contiguous().cuda()


def delta_cases(tag, clips, B):
    """-> (cases of the delta stage on `clips` quantised to 255 colours, {name: bytes of the 16 files})"""
    idx, pal, n = gif.quantize_clips(clips, colors=255)
    pal4 = torch.cat([pal, torch.zeros_like(pal[..., :1])], dim=-1).contiguous()
    bufs = (torch.empty_like(idx), torch.empty(idx.shape[:2] + (4,), dtype=torch.int32, device="cuda"),
            torch.empty(idx.shape[:2], dtype=torch.int32, device="cuda"))
    pal_h, n_h = pal.cpu().numpy(), n.cpu().numpy()
    host = {None: (idx.cpu().numpy(), None, None)}
    for tol in (0, 48):
        out, rects, _, transparent = gif.delta_frames(clips, idx, pal, n, tolerance=tol)
        host[tol] = (out.cpu().numpy(), rects.cpu().numpy(), transparent.cpu().numpy())

    def encode_all(tol):
        px, rects, tr = host[tol]
        if tol is None:
            return [ops.gif_encode(px[b], pal_h[b:b + 1], n_h[b:b + 1], 20, 0)[0] for b in range(B)]
        return [ops.gif_encode_delta(px[b], pal_h[b:b + 1], n_h[b:b + 1], rects[b], tr[b:b + 1], 20, 0)[0] for b in range(B)]
    cases = [(f"{tag}delta_tol0", lambda: ops.gif_delta(clips, idx, pal4, n, False, 0, *bufs), True),
             (f"{tag}delta_tol48", lambda: ops.gif_delta(clips, idx, pal4, n, False, 48, *bufs), True),
             (f"{tag}encode_255_colours_16_files_host_wall", lambda: encode_all(None), False),
             (f"{tag}encode_delta_tol0_16_files_host_wall", lambda: encode_all(0), False),
             (f"{tag}encode_delta_tol48_16_files_host_wall", lambda: encode_all(48), False)]
    return cases, {str(tol): sum(len(d) for d in encode_all(tol)) for tol in (None, 0, 48)}


def main():
    B, T, HW = 16, 16, 128
    levels = make_levels(B, T, HW)
    clips = to_clips(levels)
    idx, pal, n = gif.quantize_clips(clips)
    hist = ops.gif_histogram(clips)
    box = torch.from_numpy(np.stack([ops.gif_median_cut(h, 256)[0] for h in hist.cpu().numpy().view(np.uint32)])).cuda()
    pal4 = torch.cat([pal, torch.zeros_like(pal[..., :1])], dim=-1).contiguous()
    sums = torch.empty((B, 256, 4), dtype=torch.int32, device="cuda")
    sse = torch.empty((B,), dtype=torch.int64, device="cuda")
    _, pal_refined, _ = gif.quantize_clips(clips, refine=8)
    values = 3 * T * HW * HW
    psnr = [[gif.psnr_from_sse(int(e), values) for e in gif.palette_error(clips, p, n).cpu()] for p in (pal, pal_refined)]
    out = torch.empty((B, T, HW, HW), dtype=torch.uint8, device="cuda")
    idx_h, pal_h, n_h = idx.cpu().numpy(), pal.cpu().numpy(), n.cpu().numpy()
    frames_h = levels.numpy()

    def encode_all():
        return [ops.gif_encode(idx_h[b], pal_h[b:b + 1], n_h[b:b + 1], 20, 0)[0] for b in range(B)]

    def pil_all():
        sizes = []
        for b in range(B):
            fr = [Image.fromarray(f, "RGB").quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE) for f in frames_h[b]]
            buf = io.BytesIO()
            fr[0].save(buf, format="GIF", save_all=True, append_images=fr[1:], duration=200, loop=0)
            sizes.append(buf.tell())
        return sizes

    def pil_fs_all():
        for b in range(B):
            ref = Image.new("P", (1, 1))
            ref.putpalette(pal_h[b].reshape(-1).tolist())
            for f in frames_h[b]:
                Image.fromarray(f, "RGB").quantize(palette=ref, dither=Image.Dither.FLOYDSTEINBERG)

    cases = [("histogram", lambda: ops.gif_histogram(clips, out=hist), True),
             ("box_sums", lambda: ops.gif_box_sums(clips, box, out=sums), True),
             ("map", lambda: ops.gif_map(clips, pal4, n, out=out), True),
             ("map_dither32", lambda: ops.gif_map(clips, pal4, n, dither=32, out=out), True),
             ("palette_sums", lambda: ops.gif_palette_sums(clips, pal4, n, out=sums, sse_out=sse), True),
             ("diffuse", lambda: ops.gif_diffuse(clips, pal4, n, out=out), True),
             ("quantize_clips_wall", lambda: gif.quantize_clips(clips), False),
             ("quantize_clips_refine8_wall", lambda: gif.quantize_clips(clips, refine=8), False),
             ("quantize_clips_refine8_fs_wall", lambda: gif.quantize_clips(clips, refine=8, dither="fs"), False),
             ("pil_floyd_steinberg_256_frames_host_wall", pil_fs_all, False),
             ("encode_16_files_host_wall", encode_all, False),
             ("pil_mediancut_save_16_files_host_wall", pil_all, False)]
    moving, moving_bytes = delta_cases("", clips, B)
    still, still_bytes = delta_cases("still_", to_clips(make_still_levels(B, T, HW)), B)
    cases += moving + still
    for _, fn, ev in cases:
        timed(fn, WARMUP, ev)
    ms = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, ev in cases:
            ms[name].append(timed(fn, ITERS if ev else 1, ev))
    ours, theirs = sum(len(d) for d in encode_all()), sum(pil_all())
    lines = ["case,clips,frames,rounds,iters_per_round,ms_per_call_median,ms_per_call_min,ms_per_call_max"]
    for name, _, ev in cases:
        v = ms[name]
        lines.append(f"{name},{B},{B * T},{ROUNDS},{ITERS if ev else 1},{statistics.median(v):.4f},{min(v):.4f},{max(v):.4f}")
    lines.append(f"# bytes of the 16 files: {ours} (one palette per clip, no frame differencing) vs PIL {theirs} (one palette per frame, frame differencing)")
    lines.append(f"# PSNR of the 16 clips against their uint8 frames, median cut -> refine=8: mean {statistics.mean(psnr[0]):.2f} -> "
                 f"{statistics.mean(psnr[1]):.2f} dB, least gain {min(b - a for a, b in zip(*psnr)):.2f} dB")
    for what, sizes in (("everything moves", moving_bytes), ("still outside a moving 32 x 32 window", still_bytes)):
        lines.append(f"# bytes of the 16 files at 255 colours, {what}: whole frames {sizes['None']}, delta frames {sizes['0']}, "
                     f"delta frames with tolerance 48 {sizes['48']}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
