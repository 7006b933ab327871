#!/usr/bin/env python3
"""sample() against sample_fast(skip_step=s) at the bench.py shape: bs 16, 16x16x16 token grid (L = 4096), K = 4096, 19 layers, guided
with distinct conditional / unconditional embeddings, two sampler lanes, VQ-VAE decode included.  Not the headline (bench.py is).

Every variant is warmed up once, then the variants run alternately within this one process, --repeats rounds.  HIP events on the
caller's stream bracket the sampler (the lanes join it before it returns) and the decode.  One CSV row per timed call:
  variant, skip_step, steps_per_call, round, sample_ms, decode_ms, call_ms, ms_per_step (sample_ms / steps), videos_per_s
usage: bench_sample_fast.py [out.csv] [--skips 1 3 9] [--repeats 3]   (default out: profiles/r6_sample_fast.csv)"""
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
from gsdd_amd.d3pm import sample_plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "r6_sample_fast.csv"))
    ap.add_argument("--skips", type=int, nargs="+", default=[1, 3, 9])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_fast.py needs a ROCm device")
    device = torch.device("cuda", 0)
    shape = argparse.Namespace(grid=[16, 16, 16], codes=4096, layers=19, diffusion_steps=100)
    dm, vq, L = bench.build_models(shape, device)
    B = args.batch
    texts = ["synthetic"] * B
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).to(device)          # as bench.py: the condition differs from the unconditional one
    cf_cond = torch.zeros(B, 1, 512, device=device)
    dm.sample_lanes = 2
    T = dm.num_timesteps

    def run(skip):
        if skip is None:
            return dm.sample(texts, None, cond, cf_cond, content_token=None, filter_ratio=0)
        return dm.sample_fast(texts, None, cond, content_token=None, filter_ratio=0, skip_step=skip, cf_condition_embed=cf_cond)

    variants = [None] + list(args.skips)
    steps = {s: sample_plan(T, skip_step=s or 0).n_steps for s in variants}

    def one(skip):
        dm.set_noise(1234, 0)
        cur = torch.cuda.current_stream()
        ev = [ops.Event() for _ in range(3)]
        ev[0].record(cur)
        tok = run(skip)["content_token"]
        ev[1].record(cur)
        clips = vq.decode(tok.view(B, *shape.grid))
        ev[2].record(cur)
        torch.cuda.synchronize()
        assert dm._last_lanes == 2 and dm.noise_stream == steps[skip], (dm._last_lanes, dm.noise_stream)
        assert int(tok.min()) >= 0 and int(tok.max()) < shape.codes and bool(torch.isfinite(clips).all())
        return ev[0].elapsed_ms(ev[1]), ev[1].elapsed_ms(ev[2])

    for s in variants:                                  # warm-up of every shape (graph capture, workspaces, packed weights)
        one(s)
    rows = []
    for r in range(args.repeats):
        for s in variants:
            sample_ms, decode_ms = one(s)
            call = sample_ms + decode_ms
            rows.append({"variant": "sample" if s is None else "sample_fast", "skip_step": "" if s is None else s,
                         "steps_per_call": steps[s], "round": r, "sample_ms": round(sample_ms, 3), "decode_ms": round(decode_ms, 3),
                         "call_ms": round(call, 3), "ms_per_step": round(sample_ms / steps[s], 4),
                         "videos_per_s": round(B / call * 1e3, 4)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w.writeheader()
        w.writerows(rows)
    base = statistics.median(r_["videos_per_s"] for r_ in rows if r_["variant"] == "sample")
    for s in variants:
        mine = [r_ for r_ in rows if r_["steps_per_call"] == steps[s] and (r_["skip_step"] == ("" if s is None else s))]
        vps = statistics.median(r_["videos_per_s"] for r_ in mine)
        print(f"{'sample' if s is None else f'sample_fast s={s}':18s} steps {steps[s]:3d}  "
              f"videos/s {vps:7.3f} (x{vps / base:.2f})  ms/step {statistics.median(r_['ms_per_step'] for r_ in mine):7.3f}  "
              f"decode ms {statistics.median(r_['decode_ms'] for r_ in mine):7.2f}")
    print(f"wrote {args.out}: {len(rows)} timed calls, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
