#!/usr/bin/env python3
"""The reverse-step kernels with and without top-r truncation at the bench shape: B * L = 65536 positions, K = 4096, guided (distinct
conditional / unconditional logits), no test hooks.  Launches gsdd_d3pm_step (plain, t = 50, masked and unmasked x_t mixed) and
gsdd_d3pm_purity_step (rule 2, prior_weight 0: one pass; prior_weight 1: score pass + draw pass), each with trunc_rate off and 0.86,
--iters times after a warm-up, bracketed by HIP events.  One CSV row per variant: kernel, prior_weight, trunc_rate, iters, median ms
and min ms per call.  A library whose ops take no trunc_rate (an earlier revision) runs the untruncated variants only.
Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_truncation.py` the per-kernel times separate d3pm_step_kernel /
d3pm_step_trunc_kernel / d3pm_purity_kernel / d3pm_purity_trunc_kernel.  Not the headline (bench.py is).
usage: bench_truncation.py [out.csv] [--iters 10] [--sigma 3]   (default out: profiles/r9_truncation_kernels.csv)"""
import argparse
import csv
import inspect
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gsdd_amd  # noqa: E402
from gsdd_amd import ops  # noqa: E402
from gsdd_amd.d3pm import SCHED_ORDER  # noqa: E402
from oracle import d3pm as od  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "r9_truncation_kernels.csv"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=3.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_truncation.py needs a ROCm device")
    dev = torch.device("cuda", 0)
    B, L, K, T = 16, 4096, 4096, 100
    g = torch.Generator(device=dev).manual_seed(7)
    lc = torch.randn(B * L, K, generator=g, device=dev) * args.sigma
    lu = lc + torch.randn(B * L, K, generator=g, device=dev)
    xt = torch.randint(0, K, (B, L), generator=g, device=dev)
    xt[:, ::2] = K
    out = torch.empty_like(xt)
    sd = od.schedule_buffers(T, K)
    sched = [sd[n].to(dev) for n in SCHED_ORDER]
    t = torch.full((B,), 50, dtype=torch.int64, device=dev)
    sid = torch.zeros((1,), dtype=torch.int64, device=dev)
    score = torch.empty((B, L), device=dev)
    smax = torch.empty((B,), device=dev)
    cand = torch.empty_like(xt)
    rates = [None] + ([0.86] if "trunc_rate" in inspect.signature(ops.d3pm_step).parameters else [])

    def step(rate):
        kw = {} if rate is None else {"trunc_rate": rate}
        ops.d3pm_step(lc, lu, xt, out, sched, t, sid, K=K, T=T, guidance=2.0, seed=1, **kw)

    def purity(weight):
        def f(rate):
            kw = {} if rate is None else {"trunc_rate": rate}
            ops.d3pm_purity_step(lc, lu, score, smax, cand, sid, K=K, guidance=2.0, prior_rule=2, prior_weight=weight, seed=1, **kw)
        return f

    rows = []
    for name, weight, fn in (("d3pm_step", "", step), ("d3pm_purity_step", 0.0, purity(0.0)), ("d3pm_purity_step", 1.0, purity(1.0))):
        for rate in rates:
            fn(rate)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.iters):
                e0, e1 = ops.Event(), ops.Event()
                cur = torch.cuda.current_stream()
                e0.record(cur)
                fn(rate)
                e1.record(cur)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_ms(e1))
            rows.append({"kernel": name, "prior_weight": weight, "trunc_rate": "" if rate is None else rate, "positions": B * L, "K": K,
                         "iters": args.iters, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)})
            print(rows[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    print(f"wrote {args.out}: {len(rows)} variants, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
