#!/usr/bin/env python3
"""What the condition lengths cost and save in the cross-attention kernels, at the training shape (bs 16, L = 4096, H = 16, Te = 22).

Launch mode (default): the sampler's kernel, the training forward and the backward (its three kernels), in rounds of three variants --
`old` (the entry points without lengths), `len22` (every length Te) and `len7` (every length 7) -- each variant WARM + ITERS launches per
round, the rounds repeated REPEATS times so that the trace itself shows its run-to-run spread.  Meant to run under a kernel trace with no
counters:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_cross_len.py
Summary mode: `bench_cross_len.py --summarize DIR [out.csv]` reads DIR's *kernel_trace.csv, orders every kernel's dispatches by start time,
deals them to (round, variant) by position (old and new entry points launch the same kernels, so the name cannot tell them apart), drops
the warm launches and prints kernel, variant, round, launches, median / min / max microseconds."""
import csv
import glob
import os
import statistics
import sys

VARIANTS = ("old", "len22", "len7")
KERNELS = ("d3pm_cross_attention_kernel", "cross_train_fwd_kernel", "cross_bwd_dq_kernel", "cross_bwd_dkv_kernel", "cross_bwd_reduce_kernel")
B, L, TE, H = 16, 4096, 22, 16
WARM, ITERS, REPEATS = 3, 50, 2


def launch():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gsdd_amd
    from gsdd_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    M = B * L
    q = torch.randn(H, M, 4, generator=g, device="cuda")
    kc, vc = (torch.randn(B * TE, 4 * H, generator=g, device="cuda") for _ in range(2))
    dO = torch.randn(M, 4 * H, generator=g, device="cuda")
    out, lse = torch.empty(M, 4 * H, device="cuda"), torch.empty(H * M, device="cuda")
    ws = ops.d3pm_cross_attention_bwd_workspace(B, L, TE, H, "cuda")
    dq, dkc, dvc = torch.empty(H, M, 4, device="cuda"), torch.empty(B * TE, 4 * H, device="cuda"), torch.empty(B * TE, 4 * H, device="cuda")
    lens = {"old": None, "len22": torch.full((B,), TE, dtype=torch.int32, device="cuda"),
            "len7": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    for _ in range(REPEATS):
        for v in VARIANTS:
            for _ in range(WARM + ITERS):
                ops.d3pm_cross_attention(q, kc, vc, B, L, TE, H, out, cond_len=lens[v])
                ops.d3pm_cross_attention_train(q, kc, vc, B, L, TE, H, out, lse, cond_len=lens[v])
                ops.d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, TE, H, ws, dq=dq, dkc=dkc, dvc=dvc, cond_len=lens[v])
            torch.cuda.synchronize()
    print(f"bench_cross_len: {REPEATS} rounds x {len(VARIANTS)} variants x {WARM + ITERS} launches of {len(KERNELS)} kernels "
          f"(gsdd {gsdd_amd.lib().gsdd_version()})")


def summarize(root, out=None):
    files = [root] if os.path.isfile(root) else glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    by_kernel = {k: [] for k in KERNELS}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("gsdd::", "")
            if name in by_kernel:
                by_kernel[name].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    per = WARM + ITERS
    lines = ["kernel,variant,round,launches,median_us,min_us,max_us"]
    for k, rows in by_kernel.items():
        rows.sort()
        if len(rows) != REPEATS * len(VARIANTS) * per:
            raise SystemExit(f"{k}: {len(rows)} dispatches in the trace, expected {REPEATS * len(VARIANTS) * per}")
        for rnd in range(REPEATS):
            for i, v in enumerate(VARIANTS):
                first = (rnd * len(VARIANTS) + i) * per
                us = [d for _, d in rows[first + WARM:first + per]]
                lines.append(f"{k},{v},{rnd},{len(us)},{statistics.median(us):.2f},{min(us):.2f},{max(us):.2f}")
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        launch()
