#!/usr/bin/env python3
"""Time of the paired video metrics (gsdd_amd.metrics.paired_frame_metrics, csrc/paired_metrics.hip) on 16 clips of 16 frames of
128 x 128: a moving colour ramp with sigma-5 noise against the same ramp with fresh noise, both as ImageNet-normalised floats
(16, 3, 16, 128, 128), the form the decoder and the datamodule hand the evaluator.  Rows: the kernel alone (gsdd_paired_metrics into a
caller's partials, with SSIM and for the squared error alone), ops.paired_metrics (+ the two sums over the tiles), the whole
paired_frame_metrics call (+ the copies to the host; wall clock, it synchronises), and in the same run the path users had: the
levels by the evaluator's rule in torch, SSIM through five fp32 depthwise conv2d with the same 11 x 11 window on the GPU (the one-pass
form every torch SSIM package uses) and PSNR from a torch expression.  The two paths are compared before anything is timed: equal
squared errors, SSIM within 1e-3 (the torch path's one-pass fp32 moments are worth no more).  HIP events, warm-up first, the cases in
alternating rounds, the median over the rounds with the spread.  usage: bench_paired_metrics.py [out.csv]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gsdd_amd import lib, metrics, ops
from gsdd_amd._lib import check, ptr, stream_ptr

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
        raise SystemExit(f"bench_paired_metrics: {iters} calls took more than {STEP_LIMIT_S:.0f} s; giving up")
    return (e0.elapsed_time(e1) if events else wall * 1e3) / iters


def make_clips(B, T, HW, seed):
    g = torch.Generator().manual_seed(seed)
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(HW), torch.arange(HW), indexing="ij")
    base = torch.stack([(2 * x + 10 * t) % 256, (2 * y) % 256, ((x + y) + 30 * t) % 256], dim=-1).float()
    shift = torch.arange(B).view(B, 1, 1, 1, 1) * 9.0
    levels = ((base[None] + shift) % 256 + torch.randn((B, T, HW, HW, 3), generator=g) * 5.0).round().clamp(0, 255)
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    return (((levels.double() + 0.5) / 255 - mean) / std).permute(0, 4, 1, 2, 3).float().contiguous().cuda()


def torch_path(window):
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1, 1)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2

    def levels(x):
        return ((x * std + mean) * 255.0).nan_to_num(0.0).trunc().clamp(0.0, 255.0)

    def run(pred, target):
        """-> (sse (B, T, 3) fp64, ssim (B, T, 3) fp32, psnr (B, T) fp64) on the device"""
        a, b = levels(pred), levels(target)                                              # (B, 3, T, H, W) fp32, integer valued
        d = (a - b).double()
        sse = (d * d).sum(dim=(3, 4)).permute(0, 2, 1)
        psnr = 10.0 * torch.log10(255.0 ** 2 * 3 * a.shape[3] * a.shape[4] / sse.sum(dim=-1))
        B, _, T, H, W = a.shape
        pa, pb = a.reshape(B * 3 * T, 1, H, W), b.reshape(B * 3 * T, 1, H, W)
        conv = lambda x: torch.nn.functional.conv2d(x, window)                           # noqa: E731
        mu_a, mu_b = conv(pa), conv(pb)
        var_a, var_b, cov = conv(pa * pa) - mu_a * mu_a, conv(pb * pb) - mu_b * mu_b, conv(pa * pb) - mu_a * mu_b
        s = (2 * mu_a * mu_b + c1) * (2 * cov + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
        return sse, s.mean(dim=(1, 2, 3)).view(B, 3, T).permute(0, 2, 1), psnr
    return run


def main():
    B, T, HW = 16, 16, 128
    pred, target = make_clips(B, T, HW, 0), make_clips(B, T, HW, 1)
    i = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(i - 5.0) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).float()
    users = torch_path(torch.outer(g, g)[None, None].cuda())
    partials = torch.zeros((B * T * 3, ops.paired_metrics_tiles(HW, HW), 2), dtype=torch.int32, device="cuda")
    L = lib()

    def kernel(want_ssim):
        check(L.gsdd_paired_metrics(ptr(pred), 0, ptr(target), 0, B, T, HW, HW, want_ssim, ptr(partials), stream_ptr()))

    # the two paths agree before anything is timed
    ours = metrics.paired_frame_metrics(pred, target)
    sse, ssim, psnr = (v.cpu() for v in users(pred, target))
    if not torch.equal(ours["sse"], sse.round().long()):
        raise SystemExit("bench_paired_metrics: the torch path's squared errors are not the kernel's")
    ssim_diff = float((ours["ssim"] - ssim.double().mean(dim=-1)).abs().max())
    psnr_diff = float((ours["psnr"] - psnr).abs().max())
    if ssim_diff > 1e-3 or psnr_diff > 1e-9:
        raise SystemExit(f"bench_paired_metrics: the paths disagree: SSIM by {ssim_diff:.3e}, PSNR by {psnr_diff:.3e}")

    cases = [("kernel_sse_ssim", lambda: kernel(1), True),
             ("kernel_sse_only", lambda: kernel(0), True),
             ("ops_paired_metrics", lambda: ops.paired_metrics(pred, target, partials=partials), True),
             ("paired_frame_metrics_wall", lambda: metrics.paired_frame_metrics(pred, target), False),
             ("psnr_wall", lambda: metrics.psnr(pred, target), False),
             ("torch_fp32_conv2d_ssim_and_psnr", lambda: users(pred, target), True),
             ("torch_fp32_conv2d_ssim_and_psnr_wall", lambda: [v.cpu() for v in users(pred, target)], False)]
    for _, fn, ev in cases:
        timed(fn, WARMUP, ev)
    ms = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, ev in cases:
            ms[name].append(timed(fn, ITERS if ev else 1, ev))
    lines = ["case,clips,frames,rounds,iters_per_round,ms_per_call_median,ms_per_call_min,ms_per_call_max"]
    for name, _, ev in cases:
        v = ms[name]
        lines.append(f"{name},{B},{B * T},{ROUNDS},{ITERS if ev else 1},{statistics.median(v):.4f},{min(v):.4f},{max(v):.4f}")
    lines.append(f"# the two paths on these clips: squared errors equal; frame SSIM differs by at most {ssim_diff:.3e} (the torch path is "
                 f"one-pass fp32), frame PSNR by {psnr_diff:.3e} dB; mean PSNR {float(ours['psnr'].mean()):.3f} dB, mean SSIM "
                 f"{float(ours['ssim'].mean()):.6f}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
