#!/usr/bin/env python3
"""Time one D3PM training step (config C4 per-rank shape: bs 16, 16x16x16 tokens, 19 layers, K = 4096) on the HIP path.
usage: bench_train.py [B [steps]] [--cond-tokens N] [--cond-drop P] [--optim]
  --optim           the optimiser stage on: clip (max_grad_norm 1), AdamW (weight_decay 0.045, betas (0.9, 0.96)), averaged weights
                    (ema_decay 0.99), non-finite guard, 5000-step warm-up -- three launches in place of the one Adam launch
  --cond-tokens N   N condition tokens per clip (default 1: the pooled text embedding)
  --cond-drop P     classifier-free training: a second trainer on the same weights with cond_drop_prob = P and learnable_cf (condition
                    dropout, learned null embedding) is stepped in alternation with the plain one; both medians are printed"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsdd_amd  # noqa: E402
from gsdd_amd.d3pm_train import D3PMTrainer  # noqa: E402


def main():
    Te = 1
    if "--cond-tokens" in sys.argv:
        i = sys.argv.index("--cond-tokens")
        Te = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    p_drop = None
    if "--cond-drop" in sys.argv:
        i = sys.argv.index("--cond-drop")
        p_drop = float(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    optim = {}
    if "--optim" in sys.argv:
        sys.argv.remove("--optim")
        from gsdd_amd.d3pm_train import linear_warmup
        optim = dict(max_grad_norm=1.0, weight_decay=0.045, betas=(0.9, 0.96), ema_decay=0.99, skip_nonfinite=True,
                     lr_schedule=linear_warmup(1e-4, 5000))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    L, K = 4096, 4096
    torch.manual_seed(0)
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=K, spatial_size=[64, 64], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=19, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                        content_spatial_size=[64, 64], condition_dim=512, diffusion_step=100)
    dm = gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", auxiliary_loss_weight=5e-4,
                                       adaptive_auxiliary_loss=True, guidance_scale=2, content_seq_len=L).cuda()
    trainer = D3PMTrainer(dm, lr=1e-4, **optim)
    if p_drop is not None:
        import copy
        dm_cf = copy.deepcopy(dm)
        dm_cf.cond_drop_prob, dm_cf.learnable_cf = p_drop, True
        trainer_cf = D3PMTrainer(dm_cf, lr=1e-4)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, K, (B, L), generator=g).cuda()
    cond = torch.zeros(B, 1, 512).cuda() if Te == 1 else torch.randn(B, Te, 512, generator=g).cuda()
    losses = []
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    times = []
    hosts = []
    times_cf = []
    for i in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = trainer.step(tok, cond)
        host = time.perf_counter() - t0                     # python has enqueued the whole step
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        hosts.append(host * 1e3)
        losses.append(float(loss[0]))
        times.append(dt * 1e3)
        norm = f"  grad norm {float(trainer.last_grad_norm):.4f}" if optim else ""
        print(f"step {i}: loss {losses[-1]:.4f}  {dt * 1e3:.1f} ms  ({B / dt:.1f} samples/s)  mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB{norm}")
        if p_drop is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss_cf = trainer_cf.step(tok, cond)
            torch.cuda.synchronize()
            times_cf.append((time.perf_counter() - t0) * 1e3)
            print(f"step {i}, cond_drop_prob {p_drop}: loss {float(loss_cf[0]):.4f}  {times_cf[-1]:.1f} ms")
    if steps > 4 and p_drop is not None:
        tail = sorted(times_cf[3:])             # (steps 0-1 run launch by launch, step 2 captures)
        print(f"cond_drop_prob {p_drop}, learnable_cf: median of steps 3..{steps - 1}: {tail[len(tail) // 2]:.2f} ms  (min {tail[0]:.2f}, max {tail[-1]:.2f})")
        tail = sorted(times[3:])
        print(f"cond_drop_prob 0: median of steps 3..{steps - 1}: {tail[len(tail) // 2]:.2f} ms  (min {tail[0]:.2f}, max {tail[-1]:.2f})")
    if steps > 4:
        tail = sorted(times[2:])
        print(f"median of steps 2..{steps - 1}: {tail[len(tail) // 2]:.2f} ms  (min {tail[0]:.2f}); host enqueue time median "
              f"{sorted(hosts[2:])[len(hosts[2:]) // 2]:.2f} ms")
    if optim:
        print(f"optimiser stage: {trainer._adam.n_blocks} table blocks, last gradient norm {float(trainer.last_grad_norm):.4f}, "
              f"skipped steps {trainer.skipped_steps}, captures {trainer.captures}")


if __name__ == "__main__":
    main()
