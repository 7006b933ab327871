"""Writes tests/golden/clip_text_small.npz: a small seeded CLIP text tower built by transformers.CLIPTextModelWithProjection, a batch
of id rows, and the library's own outputs on them.

Tower: hidden 128, 2 heads (d = 64), 2 layers, intermediate 128, projection 32, vocabulary 64, 77 positions, QuickGELU,
torch.manual_seed(SEED).  A randomly initialised tower is bland (near-uniform attention, tiny biases), so it is perturbed: q / k
weights x 8, every bias ~ N(0, 0.1), LayerNorm gains jittered by 0.2, embeddings x 10.
Rows: lengths [2, 3, 16, 17, 22, 33, 64, 77] (start id 62, random ids in [1, 62), end id 63, zero padding to 77).
Stored: the state dict (sd/...), ids, want = the library's output with the tower in fp64, ref_fp32_err = max |fp32 library output -
want| on the same rows: the yardstick of the native tower's tolerance (4 x ref_fp32_err, tests/test_gpu_text_tower.py).

With SEED = 0 and transformers 5.15: ref_fp32_err = 6.05e-6, max |want| = 2.94 (the script prints both).  Faults injected into the
fp64 restatement (tests/text_tower_ref.py) move the outputs of EVERY one of these rows by at least: no causal mask 1.1, mask off by one
8.6e-3, missing q scale 7.0e-4, plain sigmoid instead of sigmoid(1.702 x) 0.14 -- the smallest is 29 x the bound of 2.4e-5.  If SEED or
the perturbation changes, re-measure those four figures and update this paragraph.

usage: python tests/golden/make_golden_clip_text.py"""
import os

import numpy as np
import torch
import transformers

SEED = 0
LENGTHS = [2, 3, 16, 17, 22, 33, 64, 77]
CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=128, projection_dim=32, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=77, hidden_act="quick_gelu", bos_token_id=62, eos_token_id=63, pad_token_id=0)


def build_tower():
    torch.manual_seed(SEED)
    m = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**CFG)).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_proj.weight", "k_proj.weight")):
                p.mul_(8.0)
            elif "layer_norm" in name and name.endswith(".weight"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "embedding" in name:
                p.mul_(10.0)
    return m


def build_ids():
    g = torch.Generator().manual_seed(SEED + 2)
    ids = torch.zeros((len(LENGTHS), 77), dtype=torch.int64)
    for r, n in enumerate(LENGTHS):
        ids[r, 0] = CFG["bos_token_id"]
        ids[r, 1:n - 1] = torch.randint(1, 62, (n - 2,), generator=g)
        ids[r, n - 1] = CFG["eos_token_id"]
    return ids


def main():
    m = build_tower()
    ids = build_ids()
    with torch.no_grad():
        got32 = m(input_ids=ids).text_embeds.double()
        want = m.double()(input_ids=ids).text_embeds
    m.float()
    err = (got32 - want).abs().max().item()
    out = {"sd/" + k: v.detach().float().numpy() for k, v in m.state_dict().items() if v.is_floating_point()}
    out.update(ids=ids.numpy(), want=want.numpy(), ref_fp32_err=np.float64(err), cfg_n_head=np.int64(CFG["num_attention_heads"]),
               cfg_seed=np.int64(SEED))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_text_small.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, ref_fp32_err {err:.3e}, max |want| {want.abs().max().item():.3f}")


if __name__ == "__main__":
    main()
