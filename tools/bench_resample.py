#!/usr/bin/env python3
"""RePaint's resampling jumps at the bench.py shape (bs 16, 16x16x16 token grid, K = 4096, 19 layers, guided with distinct embeddings,
two sampler lanes), 25 % of the positions known (the first 4 of 16 latent frames), on the MI355X.  Not the headline (bench.py is).

Part 1, chains: the plain known chain (100 steps) against resample_jump 10 / resample_times 2 (190 steps + 9 jumps), warmed up once
each, then alternated --repeats rounds; HIP events on the caller's stream bracket the sampler.  One CSV row per timed call with
ms per op (steps + jumps) and ms per step (the call's time over its reverse steps: a jump costs a hundredth of a step, so this is the
figure to hold against the plain chain's); the printed spread is (max - min) / median of ms per step over a variant's rounds.

Part 2, kernels: gsdd_d3pm_forward_jump alone (a third of the inputs [MASK], from-level 39, jump 10, no hold mask) next to the plain
guided step kernel on the same positions, in this same process: at 65,536 positions (the batch) and at 32,768 (one lane's launch),
--iters launches each after a warm-up, one HIP event pair per launch: launch_median_ms / launch_min_ms.  Event timings include the
gap between the two event records and the launch, a noticeable share of a 0.1 ms kernel; the kernels' own durations come from running
this part under a kernel trace (rocprofv3 --kernel-trace --stats -- python3 tools/bench_resample.py out.csv --parts kernel, then
tools/summarize_trace.py: profiles/rG_resample_kernel_trace.csv).
CSV columns: chain rows fill ms, ms_per_op, ms_per_step; kernel rows fill launch_median_ms, launch_min_ms (ops = launches timed).
usage: bench_resample.py [out.csv] [--repeats 2] [--iters 20] [--mode renoise]   (default out: profiles/rG_resample.csv)"""
import argparse
import csv
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (importing runs nothing: bench.main() sits behind __main__)
import gsdd_amd  # noqa: E402
from gsdd_amd import ops  # noqa: E402
from gsdd_amd.d3pm import SCHED_ORDER, frame_mask, jump_table, resample_plan, sample_plan  # noqa: E402


def chains(args, device, rows):
    shape = argparse.Namespace(grid=[16, 16, 16], codes=4096, layers=19, diffusion_steps=100)
    dm, vq, L = bench.build_models(shape, device)
    B, T = args.batch, dm.num_timesteps
    texts = ["synthetic"] * B
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).to(device)
    cf_cond = torch.zeros(B, 1, 512, device=device)
    content = torch.randint(0, shape.codes, (B, L), generator=g).to(device)
    mask = frame_mask(shape.grid, 4).to(device)
    dm.sample_lanes = 2
    variants = {"known_plain": ({}, sample_plan(T).draws), "jump10_times2": (dict(resample_jump=10, resample_times=2), resample_plan(T, 10, 2).draws)}
    n_steps = {"known_plain": sample_plan(T).n_steps, "jump10_times2": resample_plan(T, 10, 2).n_steps}

    def one(name):
        kw, n_ops = variants[name]
        dm.set_noise(1234, 0)
        cur = torch.cuda.current_stream()
        ev = [ops.Event(), ops.Event()]
        ev[0].record(cur)
        tok = dm.sample(texts, None, cond, cf_cond, content_token=content, filter_ratio=0, known_mask=mask, known_mode=args.mode, **kw)["content_token"]
        ev[1].record(cur)
        torch.cuda.synchronize()
        assert dm._last_lanes == 2 and dm.noise_stream == n_ops, (dm._last_lanes, dm.noise_stream)
        assert int(tok.min()) >= 0 and int(tok.max()) < shape.codes and bool(torch.equal(tok[:, mask], content[:, mask]))
        return ev[0].elapsed_ms(ev[1])

    for name in variants:
        one(name)
    for r in range(args.repeats):
        for name in variants:
            ms = one(name)
            rows.append({"part": "chain", "variant": name, "positions": B * L, "round": r, "ops": variants[name][1], "ms": round(ms, 3),
                         "ms_per_op": round(ms / variants[name][1], 4), "ms_per_step": round(ms / n_steps[name], 4),
                         "launch_median_ms": "", "launch_min_ms": ""})
            print(rows[-1])
    for name in variants:
        per = [r_["ms_per_step"] for r_ in rows if r_["part"] == "chain" and r_["variant"] == name]
        print(f"{name:14s} ms/step median {statistics.median(per):.4f}  spread {(max(per) - min(per)) / statistics.median(per):.2%} over {len(per)} rounds")
    del dm, vq
    torch.cuda.empty_cache()


def kernels(args, device, rows):
    from oracle import d3pm as od
    K, T, L = 4096, 100, 4096
    for B in (16, 8):
        g = torch.Generator(device="cuda").manual_seed(0)
        lc = torch.randn(B * L, K, device="cuda", generator=g) * 3.0
        lu = lc + torch.randn(B * L, K, device="cuda", generator=g)
        tok = torch.randint(0, K, (B, L), device="cuda", generator=g)
        tok[:, ::3] = K
        out = torch.empty_like(tok)
        sd = od.schedule_buffers(T, K)
        sched = [sd[n].cuda() for n in SCHED_ORDER]
        t = torch.full((B,), 39, dtype=torch.int64, device="cuda")
        sid = torch.zeros(1, dtype=torch.int64, device="cuda")
        table = jump_table(T, K, 10).cuda()
        calls = {"d3pm_step_plain": lambda: ops.d3pm_step(lc, lu, tok, out, sched, t, sid, K=K, T=T, guidance=2.0, seed=1),
                 "d3pm_forward_jump": lambda: ops.d3pm_forward_jump(tok, out, table, t, sid, K=K, T=T, jump=10, seed=1)}
        for name, call in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            rows.append({"part": "kernel", "variant": name, "positions": B * L, "round": "", "ops": args.iters,
                         "ms": "", "ms_per_op": "", "ms_per_step": "", "launch_median_ms": round(statistics.median(ms), 4),
                         "launch_min_ms": round(min(ms), 4)})
            print(rows[-1])
        del lc, lu
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "rG_resample.csv"))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--mode", default="renoise", choices=["renoise", "hold"])
    ap.add_argument("--parts", nargs="+", default=["kernel", "chain"], choices=["kernel", "chain"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a ROCm device")
    device = torch.device("cuda", 0)
    gsdd_amd.lib()
    rows = []
    if "kernel" in args.parts:
        kernels(args, device, rows)
    if "chain" in args.parts:
        chains(args, device, rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    print(f"wrote {args.out}: {len(rows)} rows, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
