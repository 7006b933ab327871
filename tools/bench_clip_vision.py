#!/usr/bin/env python3
"""Time of one call of the native CLIP image tower (gsdd_amd.vision.ClipVisionTower) at ViT-B/32's shape -- 224 x 224 in patches of 32,
50 positions, width 768, 12 heads, 12 layers, 3072 inner, projection 512 -- on random weights: `forward` on 256 frames of 128 x 128
(16 clips of 16 frames, ImageNet-normalised floats as the decoder returns them; the frame-patch kernel included), and `forward_pixels`
on the same 256 frames already at 224 (the tower without the resize).  HIP events around each call, warm-up first, the two cases in
alternating rounds (a drift of the clocks hits both alike), the median over the rounds reported with the spread; a round that takes
longer than the time limit ends the run with an error instead of hanging on.  usage: bench_clip_vision.py [out.csv]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gsdd_amd.vision import ClipVisionTower

ROUNDS, WARMUP, ITERS, STEP_LIMIT_S = 7, 3, 5, 60.0


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.monotonic()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    if time.monotonic() - t0 > STEP_LIMIT_S:
        raise SystemExit(f"bench_clip_vision: {iters} calls took more than {STEP_LIMIT_S:.0f} s; giving up")
    return e0.elapsed_time(e1) / iters


def main():
    C, H, NL, I, E, R, P, B, T, HW = 768, 12, 12, 3072, 512, 224, 32, 16, 16, 128
    S = (R // P) ** 2 + 1
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g) * 0.02
    layers = [{"wqkv": r(3 * C, C), "bqkv": r(3 * C), "wo": r(C, C), "bo": r(C), "g1": 1 + r(C), "be1": r(C), "g2": 1 + r(C), "be2": r(C),
               "w1": r(I, C), "b1": r(I), "w2": r(C, I), "b2": r(C)} for _ in range(NL)]
    tower = ClipVisionTower(r(C, 3, P, P), r(C), r(S, C), 1 + r(C), r(C), layers, 1 + r(C), r(C), r(E, C), H).cuda()
    clips = torch.randn((B, 3, T, HW, HW), generator=g).cuda()
    pixels = torch.randn((B * T, 3, R, R), generator=g).cuda()
    cases = [("forward_256x128px", lambda: tower(clips)), ("forward_pixels_256x224px", lambda: tower.forward_pixels(pixels))]
    for _, fn in cases:
        timed(fn, WARMUP)
    ms = {name: [] for name, _ in cases}
    for _ in range(ROUNDS):
        for name, fn in cases:
            ms[name].append(timed(fn, ITERS))
    lines = ["case,frames,rounds,iters_per_round,ms_per_call_median,ms_per_call_min,ms_per_call_max"]
    for name, _ in cases:
        v = ms[name]
        lines.append(f"{name},{B * T},{ROUNDS},{ITERS},{statistics.median(v):.4f},{min(v):.4f},{max(v):.4f}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
