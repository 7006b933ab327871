#!/usr/bin/env python3
"""Long clips at the bench.py shape (bs 16, 16x16x16 token grid, K = 4096, 19 layers, guided with distinct embeddings, two sampler
lanes) on the MI355X: n = 40 latent frames with overlap k = 4, so W = 3 windows.  Not the headline (bench.py is).

Three things are timed in the same process, warmed up once each and then alternated --repeats rounds; HIP events on the caller's
stream bracket each call:
  sample_long     the rollout as one program (DiffusionTransformer.sample_long)
  manual_chain    the chain of sample() calls it is defined against: sample(), then twice sample(content_token = the last k frames in
                  front, known_mask = frame_mask(grid, k)), the frames assembled on the device with torch indexing
  decode_long     VQVAE.decode_long of the long grid, against
  decode_windows  W plain decode() calls of the same windows (no merge)
Before anything is timed the two samplers' tokens are compared (they must be equal).  One CSV row per timed call; the printed summary
is median and (min ... max) per variant, and the spread (max - min) / median.
usage: bench_sample_long.py [out.csv] [--repeats 3] [--frames 40] [--overlap 4]   (default out: profiles/rX_sample_long.csv)"""
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
from gsdd_amd.d3pm import frame_mask, long_plan, sample_plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "rX_sample_long.csv"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--overlap", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_long.py needs a ROCm device")
    device = torch.device("cuda", 0)
    gsdd_amd.lib()
    shape = argparse.Namespace(grid=[16, 16, 16], codes=4096, layers=19, diffusion_steps=100)
    dm, vq, L = bench.build_models(shape, device)
    B, T, n, k = args.batch, dm.num_timesteps, args.frames, args.overlap
    F, hw = shape.grid[0], shape.grid[1] * shape.grid[2]
    s = F - k
    plan = long_plan(F, n, k, sample_plan(T))
    W = plan.windows
    texts = ["synthetic"] * B
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).to(device)
    cf_cond = torch.zeros(B, 1, 512, device=device)
    mask = frame_mask(shape.grid, k).to(device)
    dm.sample_lanes = 2
    pad = torch.zeros((B, s * hw), dtype=torch.int64, device=device)

    def sample_long():
        dm.set_noise(1234, 0)
        return dm.sample_long(texts, None, cond, cf_cond, latent_shape=shape.grid, n_frames=n, overlap=k)["content_token"]

    def manual_chain():
        dm.set_noise(1234, 0)
        grid = torch.full((B, n * hw), shape.codes, dtype=torch.int64, device=device)
        tok = dm.sample(texts, None, cond, cf_cond, filter_ratio=0)["content_token"]
        grid[:, :F * hw] = tok
        for w in range(1, W):
            tok = dm.sample(texts, None, cond, cf_cond, content_token=torch.cat([tok[:, s * hw:], pad], 1), filter_ratio=0,
                            known_mask=mask)["content_token"]
            own = plan.owned(w)
            grid[:, own.start * hw:own.stop * hw] = tok[:, k * hw:(k + len(own)) * hw]
        return grid

    state = {}

    def decode_long():
        return vq.decode_long(state["grid"], k)

    def decode_windows():
        out = None
        for w in range(W):
            idx = torch.arange(w * s, w * s + F, device=device).clamp_(max=n - 1)
            out = vq.decode(state["grid"].index_select(1, idx))
        return out

    def timed(fn):
        cur = torch.cuda.current_stream()
        ev = [ops.Event(), ops.Event()]
        ev[0].record(cur)
        res = fn()
        ev[1].record(cur)
        torch.cuda.synchronize()
        return ev[0].elapsed_ms(ev[1]), res

    a, b = sample_long(), manual_chain()
    torch.cuda.synchronize()
    assert bool(torch.equal(a, b)), f"{int((a != b).sum())} tokens of the rollout differ from the manual chain"
    assert dm._last_lanes == 2 and int(a.min()) >= 0 and int(a.max()) < shape.codes
    state["grid"] = a.view(B, n, *shape.grid[1:])
    variants = {"sample_long": sample_long, "manual_chain": manual_chain, "decode_long": decode_long, "decode_windows": decode_windows}
    for fn in (decode_long, decode_windows):
        fn()
    rows = []
    for r in range(args.repeats):
        for name, fn in variants.items():
            ms, _ = timed(fn)
            rows.append({"variant": name, "batch": B, "frames": n, "overlap": k, "windows": W, "round": r, "ms": round(ms, 3)})
            print(rows[-1])
    for name in variants:
        ms = [r_["ms"] for r_ in rows if r_["variant"] == name]
        med = statistics.median(ms)
        print(f"{name:15s} median {med:10.3f} ms  ({min(ms):.3f} ... {max(ms):.3f})  spread {(max(ms) - min(ms)) / med:.2%} over {len(ms)} rounds")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        w_ = csv.DictWriter(f, fieldnames=list(rows[0]), lineterminator="\n")
        w_.writeheader()
        w_.writerows(rows)
    print(f"wrote {args.out}: {len(rows)} rows, gsdd {gsdd_amd.lib().gsdd_version()}")


if __name__ == "__main__":
    main()
