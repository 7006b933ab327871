#!/usr/bin/env python3
"""Per-call time of the step kernel with known positions (gsdd_step_desc.known) at the production class width, on the MI355X.

65,536 positions (B 16 x L 4096: 16 latent frames of 16 x 16), K = 4096, guided with distinct logits of sigma 3, no hooks.  Variants:
the plain launch; an all-False mask (the masked family with nothing to skip); 25 % known (the first 4 of 16 frames) and 50 % known
(the first 8), each in both modes.  Every variant runs --iters times after a warm-up, bracketed by HIP events.  One CSV row per
variant: variant, known share, mode, iters, median ms and min ms per call, and the logit bytes the unknown positions read.  A library
whose ops.d3pm_step takes no `known` (an earlier revision) runs the plain variant only.
usage: python3 tools/bench_known.py [--iters 20] [--out profiles/r10_known_kernels.csv]"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10_known_kernels.csv"))
    args = ap.parse_args()
    gsdd_amd.lib()
    B, L, K, T, frames = 16, 4096, 4096, 100, 16
    g = torch.Generator(device="cuda").manual_seed(0)
    lc = torch.randn(B * L, K, device="cuda", generator=g) * 3.0
    lu = lc + torch.randn(B * L, K, device="cuda", generator=g)
    tok = torch.randint(0, K, (B, L), device="cuda", generator=g)
    tok[:, ::3] = K
    x_known = torch.randint(0, K, (B, L), device="cuda", generator=g)
    out = torch.empty_like(tok)
    sd = od.schedule_buffers(T, K)
    sched = [sd[n].cuda() for n in SCHED_ORDER]
    t = torch.full((B,), 50, dtype=torch.int64, device="cuda")
    sid = torch.zeros(1, dtype=torch.int64, device="cuda")

    def mask(k):
        m = torch.zeros(B, frames, L // frames, dtype=torch.uint8, device="cuda")
        m[:, :k] = 1
        return m.view(B, L).contiguous()
    variants = [("plain", None, None)]
    if "known" in inspect.signature(ops.d3pm_step).parameters:
        variants += [("all_false_mask", 0, 0)] + [(f"{25 * k // 4}pct_{name}", k, code) for k in (4, 8) for name, code in (("renoise", 0), ("hold", 1))]
    rows = []
    for name, k, code in variants:
        kw = {} if k is None else {"known": mask(k), "x_known": x_known, "known_mode": code}
        call = lambda: ops.d3pm_step(lc, lu, tok, out, sched, t, sid, K=K, T=T, guidance=2.0, seed=1, **kw)
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
        share = 0.0 if k is None else k / frames
        rows.append({"variant": name, "known_share": share, "known_mode": "" if code is None or k == 0 else ("renoise", "hold")[code],
                     "positions": B * L, "K": K, "iters": args.iters, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                     "logit_MB_read": round((1 - share) * B * L * 2 * K * 4 / 1e6, 1)})
        print(rows[-1])
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    print(f"wrote {args.out}: {len(rows)} variants, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
