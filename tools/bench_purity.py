#!/usr/bin/env python3
"""Plain sample() against purity-prior sampling (prior_rule 2, prior_weight r in {0, 1}) at the bench.py shape -- bs 16, 16x16x16 token
grid (L = 4096) with the reference's T = 100 reveal list rescaled to 4096 tokens (scaled_n_sample) -- and at L = 1024 (4x16x16) with the
list as the reference carries it.  K = 4096, 19 layers, guided with distinct conditional / unconditional embeddings, two sampler lanes,
VQ-VAE decode included.  Both purity variants make 100 denoiser evaluations per call (99 purity calls and the step at t = 0), as plain
sampling does: what differs is the purity kernels' work per call.  Not the headline (bench.py is).

Every variant is warmed up once, then the variants run alternately within this one process, --repeats rounds.  HIP events on the
caller's stream bracket the sampler (the lanes join it before it returns) and the decode.  One CSV row per timed call:
  L, variant, prior_weight, calls, round, sample_ms, decode_ms, call_ms, ms_per_call (sample_ms / calls), videos_per_s
Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_purity.py` the per-kernel times give the purity step's cost against the
plain step kernel's (d3pm_purity_kernel / purity_smax_kernel / purity_select_kernel / advance_plan_kernel against d3pm_step_kernel).
usage: bench_purity.py [out.csv] [--repeats 3] [--lengths 4096 1024]   (default out: profiles/r8_purity.csv)"""
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
from gsdd_amd.d3pm import purity_plan, reference_n_sample, scaled_n_sample  # noqa: E402

GRIDS = {4096: [16, 16, 16], 1024: [4, 16, 16]}
VARIANTS = [("sample", 0, 0.0), ("purity", 2, 0.0), ("purity", 2, 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "r8_purity.csv"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lengths", type=int, nargs="+", default=[4096, 1024], choices=sorted(GRIDS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_purity.py needs a ROCm device")
    device = torch.device("cuda", 0)
    B = args.batch
    texts = ["synthetic"] * B
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).to(device)          # as bench.py: the condition differs from the unconditional one
    cf_cond = torch.zeros(B, 1, 512, device=device)
    rows = []
    for L in args.lengths:
        shape = argparse.Namespace(grid=GRIDS[L], codes=4096, layers=19, diffusion_steps=100)
        dm, vq, L_built = bench.build_models(shape, device)
        assert L_built == L
        dm.sample_lanes = 2
        T = dm.num_timesteps
        n_sample = scaled_n_sample(reference_n_sample(T), L)
        n_calls = len(purity_plan(n_sample, dm.prior_ps, T))

        def one(rule, weight):
            dm.prior_rule, dm.prior_weight, dm.n_sample = rule, weight, n_sample
            dm.set_noise(1234, 0)
            cur = torch.cuda.current_stream()
            ev = [ops.Event() for _ in range(3)]
            ev[0].record(cur)
            tok = dm.sample(texts, None, cond, cf_cond, content_token=None, filter_ratio=0)["content_token"]
            ev[1].record(cur)
            clips = vq.decode(tok.view(B, *shape.grid))
            ev[2].record(cur)
            torch.cuda.synchronize()
            want_stream = 2 * (n_calls - 1) + 1 if rule else T
            assert dm._last_lanes == 2 and dm.noise_stream == want_stream, (dm._last_lanes, dm.noise_stream)
            assert int(tok.min()) >= 0 and int(tok.max()) < shape.codes and bool(torch.isfinite(clips).all())
            return ev[0].elapsed_ms(ev[1]), ev[1].elapsed_ms(ev[2])

        for _, rule, weight in VARIANTS:                    # warm-up of every variant (graph capture, workspaces, packed weights)
            one(rule, weight)
        for r in range(args.repeats):
            for name, rule, weight in VARIANTS:
                sample_ms, decode_ms = one(rule, weight)
                calls = n_calls if rule else T
                call = sample_ms + decode_ms
                rows.append({"L": L, "variant": name, "prior_weight": "" if not rule else weight, "calls": calls, "round": r,
                             "sample_ms": round(sample_ms, 3), "decode_ms": round(decode_ms, 3), "call_ms": round(call, 3),
                             "ms_per_call": round(sample_ms / calls, 4), "videos_per_s": round(B / call * 1e3, 4)})
        del dm, vq
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    for L in args.lengths:
        base = statistics.median(r_["videos_per_s"] for r_ in rows if r_["L"] == L and r_["variant"] == "sample")
        for name, rule, weight in VARIANTS:
            mine = [r_ for r_ in rows if r_["L"] == L and r_["variant"] == name and r_["prior_weight"] == ("" if not rule else weight)]
            vps = statistics.median(r_["videos_per_s"] for r_ in mine)
            print(f"L {L:4d}  {name if not rule else f'purity rule 2 r={weight:g}':20s} calls {mine[0]['calls']:3d}  videos/s {vps:7.3f} "
                  f"(x{vps / base:.2f})  ms/call {statistics.median(r_['ms_per_call'] for r_ in mine):7.3f}")
    print(f"wrote {args.out}: {len(rows)} timed calls, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
