#!/usr/bin/env python3
"""Time of LPIPS (gsdd_amd.lpips.Lpips, csrc/lpips.hip) on 16 clips of 16 frames of 128 x 128, both nets, on seeded weights (He-scaled
normal convolutions, biases 0.1 N(0, 1), lin weights uniform in [0, 1)): a moving colour ramp with sigma-5 noise against the same ramp
with fresh noise, both as ImageNet-normalised floats (16, 3, 16, 128, 128).  Rows per net: the whole forward (HIP events, and by the wall
clock with its copy to the host), and in the same run the path users would have had: the same rule in fp32 through torch's own GPU
convolutions and pools.  The two are compared before anything is timed (every frame within 1e-4 of the value, relative).  Then the two
kernels that are LPIPS's own, alone, with the bytes they must move and the rate that makes: the stem operand of all 256 frames of one
clip set, and the distance head on random features of every tap's shape for the 256 frame pairs.  HIP events, warm-up first, the cases
in alternating rounds, the median over the rounds with the spread.  usage: bench_lpips.py [out.csv]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from gsdd_amd import lpips as lp
from gsdd_amd import ops
from gsdd_amd._lib import check, lib, ptr, stream_ptr

ROUNDS, WARMUP, ITERS, STEP_LIMIT_S = 7, 1, 3, 240.0
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
        raise SystemExit(f"bench_lpips: {iters} calls took more than {STEP_LIMIT_S:.0f} s; giving up")
    return (e0.elapsed_time(e1) if events else wall * 1e3) / iters


def make_clips(B, T, HW, seed):
    g = torch.Generator().manual_seed(seed)
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(HW), torch.arange(HW), indexing="ij")
    base = torch.stack([(2 * x + 10 * t) % 256, (2 * y) % 256, ((x + y) + 30 * t) % 256], dim=-1).float()
    shift = torch.arange(B).view(B, 1, 1, 1, 1) * 9.0
    levels = ((base[None] + shift) % 256 + torch.randn((B, T, HW, HW, 3), generator=g) * 5.0).round().clamp(0, 255)
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    return (((levels.double() + 0.5) / 255 - mean) / std).permute(0, 4, 1, 2, 3).float().contiguous().cuda()


def seeded_weights(net, seed=0):
    g = torch.Generator().manual_seed(seed)
    convs = []
    for lay in lp.NETS[net]["layers"]:
        if lay["op"] == "conv":
            fan = lay["cin"] * lay["k"] ** 2
            convs.append((torch.randn((lay["cout"], lay["cin"], lay["k"], lay["k"]), generator=g) * (2.0 / fan) ** 0.5,
                          0.1 * torch.randn((lay["cout"],), generator=g)))
    return convs, [torch.rand((c,), generator=g) for c in lp.tap_channels(net)]


def torch_path(net, convs, lins):
    """the rule in fp32 on the GPU through torch's convolutions: (B, 3, T, H, W) floats x 2 -> (B, T) fp32 on the device"""
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1, 1)
    table = lp.stem_table().cuda()
    convs = [(w.cuda(), b.cuda()) for w, b in convs]
    lins = [v.cuda().view(1, -1, 1, 1) for v in lins]

    def stem(x):
        lv = ((x * std + mean) * 255.0).nan_to_num(0.0).trunc().clamp(0.0, 255.0).long()             # (B, 3, T, H, W)
        B, _, T, H, W = lv.shape
        return torch.stack([table[c][lv[:, c]] for c in range(3)], dim=2).view(B * T, 3, H, W)

    def run(pred, target):
        h = torch.cat([stem(pred), stem(target)])
        n, conv, tap, total = h.shape[0] // 2, 0, 0, 0.0
        for lay in lp.NETS[net]["layers"]:
            if lay["op"] == "pool":
                h = F.max_pool2d(h, lay["k"], lay["stride"])
                continue
            h = F.relu(F.conv2d(h, *convs[conv], stride=lay["stride"], padding=lay["pad"]))
            conv += 1
            if lay["tap"]:
                u = h / (torch.sqrt((h * h).sum(dim=1, keepdim=True)) + 1e-10)
                total = total + ((u[:n] - u[n:]) ** 2 * lins[tap]).sum(dim=1).mean(dim=(1, 2))
                tap += 1
        return total.view(pred.shape[0], pred.shape[2])
    return run


def main():
    B, T, HW = 16, 16, 128
    n = B * T
    pred, target = make_clips(B, T, HW, 0), make_clips(B, T, HW, 1)
    L = lib()
    lines = ["case,net,frame_pairs,rounds,iters_per_round,ms_per_call_median,ms_per_call_min,ms_per_call_max,bytes_moved,GB_per_s"]
    notes = []

    def run_cases(net, cases):
        for _, fn, ev, _ in cases:
            timed(fn, WARMUP, ev)
        ms = {name: [] for name, _, _, _ in cases}
        for _ in range(ROUNDS):
            for name, fn, ev, _ in cases:
                ms[name].append(timed(fn, ITERS if ev else 1, ev))
        for name, _, ev, nbytes in cases:
            v = ms[name]
            med = statistics.median(v)
            rate = f"{nbytes / med / 1e6:.1f}" if nbytes else ""
            lines.append(f"{name},{net},{n},{ROUNDS},{ITERS if ev else 1},{med:.4f},{min(v):.4f},{max(v):.4f},{nbytes or ''},{rate}")
            print(lines[-1], flush=True)

    for net in ("alex", "vgg"):
        convs, lins = seeded_weights(net)
        scorer = lp.Lpips(net, convs, lins).cuda()
        users = torch_path(net, convs, lins)
        # the two paths agree before anything is timed
        ours = scorer(pred, target)["lpips"]
        theirs = users(pred, target).double().cpu()
        rel = float(((ours - theirs).abs() / ours).max())
        if not rel <= 1e-4:
            raise SystemExit(f"bench_lpips: {net}: the torch path disagrees by {rel:.3e} of the value")
        notes.append(f"# {net}: the two paths on these clips differ by at most {rel:.3e} of a frame's value (the torch path is fp32 "
                     f"throughout); mean LPIPS {float(ours.mean()):.6f}; {scorer.chunk_frames(HW, HW)} frame pairs a chunk")
        print(notes[-1], flush=True)
        run_cases(net, [("lpips_forward", lambda: scorer(pred, target), True, 0),
                        ("lpips_forward_wall", lambda: scorer(pred, target), False, 0),
                        ("torch_fp32_gpu_convolutions", lambda: users(pred, target), True, 0),
                        ("torch_fp32_gpu_convolutions_wall", lambda: users(pred, target).cpu(), False, 0)])
        # the two kernels alone
        padw = lp.NETS[net]["layers"][0]["pad"]
        rows = torch.zeros((n, HW, HW + 2 * padw, 4), dtype=torch.float32, device="cuda")
        stem_bytes = n * HW * HW * 3 * 4 + rows.numel() * 4
        cases = [("kernel_stem_rows", lambda: check(L.gsdd_lpips_stem_rows(ptr(pred), 0, B, T, HW, HW, 0, n, padw, ptr(scorer.table), ptr(rows),
                                                                           stream_ptr())), True, stem_bytes)]
        sizes = [s for s, lay in zip(lp.feature_sizes(net, HW, HW), lp.NETS[net]["layers"]) if lay["op"] == "conv" and lay["tap"]]
        keep = []
        for k, ((h, w), c) in enumerate(zip(sizes, lp.tap_channels(net))):
            P = h * w
            feat = torch.rand((2 * n * P, c), device="cuda")
            partials = torch.zeros((n, ops.lpips_distance_slots(P, c)), dtype=torch.float64, device="cuda")
            keep.append((feat, partials))
            cases.append((f"kernel_layer_distance_tap{k}_P{P}_C{c}",
                          lambda feat=feat, partials=partials, P=P, c=c, k=k: check(L.gsdd_lpips_layer_distance(
                              ptr(feat), ptr(scorer.lin[k]), n, P, c, ptr(partials), stream_ptr())), True, feat.numel() * 4))
        run_cases(net, cases)
        del keep, cases, rows
        torch.cuda.empty_cache()
    lines += notes
    print("\n".join(notes))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
