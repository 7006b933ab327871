#!/usr/bin/env python3
"""Composed guidance at the bench.py shape (bs 16, 16x16x16 token grid, K = 4096, 19 layers, two sampler lanes) on the MI355X, N = 1, 2, 3
conditions.  Not the headline (bench.py is).

Part 1, kernel: gsdd_d3pm_compose alone at 65,536 positions (the batch) and 32,768 (one lane's launch), next to the unguided
gsdd_d3pm_step (logits_u = NULL: one row read per position) in this same process -- --iters launches each after a warm-up, one HIP
event pair per launch: launch_median_ms / launch_min_ms, and GB/s of the median over the launch's algorithmic traffic
((N + 2) B L K 4 bytes for the compose launch: N + 1 rows read, one written; B L K 4 for the step).  Event timings include the gap
between the event records and the launch.

Part 2, chain: a whole composed sample() at N = 2 and 3 (compose_embeds lists at least one extra condition, so N = 1 has no chain; 100
steps, N + 1 stacked denoiser copies per step) next to the guided two-way call of the
same run, warmed up once each, then alternated --repeats rounds; HIP events on the caller's stream bracket the sampler.  videos_per_s
is the batch over the call's time; vs_guided_scaled holds it against the guided call's rate scaled by 2 / (N + 1) denoiser rows (1.0:
the composed call costs what its denoiser rows cost).
usage: bench_compose.py [out.csv] [--repeats 2] [--iters 20] [--parts kernel chain]   (default out: profiles/rY_compose.csv)"""
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
from gsdd_amd.d3pm import SCHED_ORDER  # noqa: E402

COLS = ["part", "variant", "n_cond", "positions", "round", "ms", "videos_per_s", "vs_guided_scaled", "launch_median_ms", "launch_min_ms", "gb_per_s"]
WEIGHTS = {1: [2.0], 2: [1.5, -0.5], 3: [1.0, 0.75, -0.25]}


def row(**kw):
    return {c: kw.get(c, "") for c in COLS}


def timed(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def kernels(args, device, rows):
    from oracle import d3pm as od
    K, T, L = 4096, 100, 4096
    for B in (16, 8):
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = torch.randn(4 * B * L, K, device="cuda", generator=g) * 3.0
        out = torch.empty(B * L, K, device="cuda")
        tok = torch.randint(0, K, (B, L), device="cuda", generator=g)
        tok[:, ::3] = K
        tok_out = torch.empty_like(tok)
        sd = od.schedule_buffers(T, K)
        sched = [sd[n].cuda() for n in SCHED_ORDER]
        t = torch.full((B,), 39, dtype=torch.int64, device="cuda")
        sid = torch.zeros(1, dtype=torch.int64, device="cuda")
        row_bytes = B * L * K * 4
        calls = {("d3pm_step_unguided", 0): (lambda: ops.d3pm_step(logits[:B * L], None, tok, tok_out, sched, t, sid, K=K, T=T, guidance=1.0, seed=1),
                                             row_bytes)}
        for N in (1, 2, 3):
            w = torch.tensor([WEIGHTS[N]], device="cuda").expand(B, N).contiguous()
            calls[("d3pm_compose", N)] = (lambda N=N, w=w: ops.d3pm_compose(logits[:(N + 1) * B * L], w, n_cond=N, B=B, L=L, K=K, out=out),
                                          (N + 2) * row_bytes)
        for (name, N), (call, nbytes) in calls.items():
            med, lo = timed(call, args.iters)
            rows.append(row(part="kernel", variant=name, n_cond=N, positions=B * L, launch_median_ms=round(med, 4), launch_min_ms=round(lo, 4),
                            gb_per_s=round(nbytes / med / 1e6, 1)))
            print(rows[-1])
        del logits, out
        torch.cuda.empty_cache()


def chains(args, device, rows):
    shape = argparse.Namespace(grid=[16, 16, 16], codes=4096, layers=19, diffusion_steps=100)
    dm, vq, L = bench.build_models(shape, device)
    B, T = args.batch, dm.num_timesteps
    texts = ["synthetic"] * B
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).to(device)
    extra = [torch.randn(B, 1, 512, generator=g).to(device) for _ in range(2)]
    cf_cond = torch.zeros(B, 1, 512, device=device)
    dm.sample_lanes = 2
    variants = {0: {}}
    variants.update({N: dict(compose_embeds=extra[:N - 1], compose_weights=WEIGHTS[N]) for N in (2, 3)})

    def one(N):
        dm.set_noise(1234, 0)
        cur = torch.cuda.current_stream()
        ev = [ops.Event(), ops.Event()]
        ev[0].record(cur)
        tok = dm.sample(texts, None, cond, cf_cond, filter_ratio=0, **variants[N])["content_token"]
        ev[1].record(cur)
        torch.cuda.synchronize()
        assert dm._last_lanes == 2 and dm.noise_stream == T and int(tok.min()) >= 0 and int(tok.max()) < shape.codes
        return ev[0].elapsed_ms(ev[1])

    for N in variants:
        one(N)
    for r in range(args.repeats):
        for N in variants:
            ms = one(N)
            rows.append(row(part="chain", variant="composed" if N else "guided", n_cond=N or 1, positions=B * L, round=r, ms=round(ms, 2),
                            videos_per_s=round(B / ms * 1e3, 4)))
    guided = statistics.median(r_["videos_per_s"] for r_ in rows if r_["part"] == "chain" and r_["variant"] == "guided")
    for r_ in rows:
        if r_["part"] == "chain":
            r_["vs_guided_scaled"] = round(r_["videos_per_s"] / (guided * 2 / (r_["n_cond"] + 1)), 4)
            print(r_)
    del dm, vq
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "rY_compose.csv"))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parts", nargs="+", default=["kernel", "chain"], choices=["kernel", "chain"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose.py needs a ROCm device")
    device = torch.device("cuda", 0)
    gsdd_amd.lib()
    rows = []
    if "kernel" in args.parts:
        kernels(args, device, rows)
    if "chain" in args.parts:
        chains(args, device, rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w = csv.DictWriter(f, fieldnames=COLS, lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    print(f"wrote {args.out}: {len(rows)} rows, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
