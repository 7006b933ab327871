#!/usr/bin/env python3
"""Time of the GIF import (gsdd_amd.gif.read_gif) on 16 GIFs of 16 frames of 128 x 128: the files tools/bench_gif.py's clips give
through write_gifs (full frames, one palette per clip); the same clips written by PIL with optimize=True from palette images that
share the clip's palette (every pixel of these clips moves, so PIL keeps full frames and adds transparency and local tables); and the
same again with everything outside the middle 96 x 96 held still, so that PIL crops later frames to a sub-rectangle.  Per set of 16 files:
  decode_host      gsdd_gif_probe + gsdd_gif_decode of every file, by the wall clock
  compose          gsdd_gif_compose of every file's tables (already on the device), HIP events around the 16 launches
  read_preprocess  the whole batch: read_gif -> preprocess per file, stacked, by the wall clock (synchronised at the end)
  pil_preprocess   the path users have today, in the same run: PIL ImageSequence -> convert("RGB") -> numpy stack -> .to(device) ->
                   preprocess per file, stacked
Warm-up first, the cases in alternating rounds (a drift of the clocks hits all alike), the median over the rounds reported with the
range; a round that takes longer than the time limit ends the run with an error instead of hanging on.
usage: bench_gif_read.py [out.csv]"""
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageSequence

from bench_gif import make_levels
from gsdd_amd import gif, ops
from gsdd_amd.data import preprocess

ROUNDS, WARMUP, STEP_LIMIT_S = 7, 2, 120.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
R = 128


def timed(fn, events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.monotonic()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    wall = time.monotonic() - t0
    if wall > STEP_LIMIT_S:
        raise SystemExit(f"bench_gif_read: a call took more than {STEP_LIMIT_S:.0f} s; giving up")
    return e0.elapsed_time(e1) if events else wall * 1e3


def main():
    B, T, HW = 16, 16, 128
    levels = make_levels(B, T, HW)
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    clips = (((levels.double() + 0.5) / 255 - mean) / std).permute(0, 4, 1, 2, 3).float().contiguous().cuda()
    idx, pal, n = gif.quantize_clips(clips)
    idx_h, pal_h, n_h = idx.cpu().numpy(), pal.cpu().numpy(), n.cpu().numpy()
    ours = [ops.gif_encode(idx_h[b], pal_h[b:b + 1], n_h[b:b + 1], 20, 0)[0] for b in range(B)]

    def pil_files(indices):
        out = []
        for b in range(B):
            frames = []
            for t in range(T):
                im = Image.fromarray(indices[b, t], "P")
                im.putpalette(pal_h[b].tobytes())
                frames.append(im)
            buf = io.BytesIO()
            frames[0].save(buf, format="GIF", save_all=True, append_images=frames[1:], optimize=True, duration=200, loop=0)
            out.append(buf.getvalue())
        return out

    pils = pil_files(idx_h)                                # every pixel of these clips moves: full frames, transparency, local tables
    still = idx_h.copy()                                   # ... with a border that stands still: frames cropped to the middle 96 x 96
    still[:, 1:] = idx_h[:, :1]
    still[:, :, 16:112, 16:112] = idx_h[:, :, 16:112, 16:112]
    borders = pil_files(still)
    sets = {"own": ours, "pil_optimized": pils, "pil_optimized_still_border": borders}
    dev = torch.device("cuda")
    cases = []
    for tag, files in sets.items():
        decoded = [ops.gif_decode(d) for d in files]
        on_dev = [(torch.from_numpy(r).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev), i) for f, _, p, r, i in decoded]
        outs = [torch.empty((i["frames"], i["height"], i["width"], 3), dtype=torch.uint8, device=dev) for *_, i in on_dev]
        sels = [torch.arange(i["frames"], dtype=torch.int32, device=dev) for *_, i in on_dev]

        def decode_all(files=files):
            return [ops.gif_decode(d) for d in files]

        def compose_all(on_dev=on_dev, outs=outs, sels=sels):
            for (r, f, p, i), o, s in zip(on_dev, outs, sels):
                ops.gif_compose(r, f, p, i["width"], i["height"], range(i["frames"]), out=o, select_dev=s)

        def read_all(files=files):
            return torch.stack([preprocess(gif.read_gif(d, dev)[0], R) for d in files])

        def pil_all(files=files):
            out = []
            for d in files:
                frames = np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(d)))])
                out.append(preprocess(torch.from_numpy(frames).to(dev), R))
            return torch.stack(out)

        a, b = read_all(), pil_all()
        if not torch.equal(a, b):
            raise SystemExit(f"bench_gif_read: {tag}: read_gif and PIL disagree")
        raster = sum(i["raster_bytes"] for *_, i in on_dev)
        cases += [(f"{tag}_decode_host", decode_all, False, raster), (f"{tag}_compose", compose_all, True, raster),
                  (f"{tag}_read_preprocess", read_all, False, raster), (f"{tag}_pil_preprocess", pil_all, False, raster)]
    for _, fn, ev, _ in cases:
        for _ in range(WARMUP):
            timed(fn, ev)
    ms = {name: [] for name, *_ in cases}
    for _ in range(ROUNDS):
        for name, fn, ev, _ in cases:
            ms[name].append(timed(fn, ev))
    lines = ["case,files,frames,raster_bytes,file_bytes,rounds,ms_per_16_files_median,ms_min,ms_max"]
    for name, _, _, raster in cases:
        v = ms[name]
        size = sum(len(d) for d in sets[max((t for t in sets if name.startswith(t)), key=len)])
        lines.append(f"{name},{B},{B * T},{raster},{size},{ROUNDS},{statistics.median(v):.4f},{min(v):.4f},{max(v):.4f}")
    lines.append(f"# canvas bytes a full-frame copy moves: {B * T * HW * HW * 3}; gsdd {ops.lib().gsdd_version()}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
