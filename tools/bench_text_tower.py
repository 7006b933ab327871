#!/usr/bin/env python3
"""Time of one call of the native CLIP text tower (gsdd_amd.text.ClipTextTower) at ViT-B/32's text shape -- width 512, 8 heads, 12 layers,
2048 inner, 49408 tokens, projection 512 -- on random weights: a batch of 64 captions tokenised by the reference's recipe (start + up to
20 + end, ids zero-padded to 77), with the context trimmed to the longest caption (what forward does) and untrimmed (77 positions).
HIP events around the call, host work (end-of-text positions, the ids' upload) included.  usage: bench_text_tower.py [out.csv]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gsdd_amd.text import ClipTextTower


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    C, H, NL, I, V, P, B = 512, 8, 12, 2048, 49408, 512, 64
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g) * 0.02
    layers = [{"wqkv": r(3 * C, C), "bqkv": r(3 * C), "wo": r(C, C), "bo": r(C), "g1": 1 + r(C), "be1": r(C), "g2": 1 + r(C), "be2": r(C),
               "w1": r(I, C), "b1": r(I), "w2": r(C, I), "b2": r(C)} for _ in range(NL)]
    tower = ClipTextTower(r(V, C), r(77, C), layers, 1 + r(C), r(C), r(P, C), H).cuda()
    ids = torch.zeros((B, 77), dtype=torch.int64)
    lengths = torch.randint(4, 23, (B,), generator=g)
    lengths[0] = 22
    for b, n in enumerate(lengths.tolist()):
        ids[b, 0], ids[b, n - 1] = V - 2, V - 1
        ids[b, 1:n - 1] = torch.randint(1, V - 2, (n - 2,), generator=g)
    rows = [("trimmed_22_of_77", timeit(lambda: tower(ids))), ("untrimmed_77", timeit(lambda: tower(ids, trim=False)))]
    lines = ["case,batch,ms_per_call"] + [f"{name},{B},{ms:.4f}" for name, ms in rows]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
