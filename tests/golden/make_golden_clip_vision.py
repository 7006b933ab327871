"""Writes tests/golden/clip_vision_small.npz: a small seeded CLIP image tower built by transformers.CLIPVisionModelWithProjection, six
pixel frames, and the library's own outputs on them.

Tower: hidden 128, 2 heads (d = 64), 2 layers, intermediate 128, projection 32, image 56, patch 8, QuickGELU,
torch.manual_seed(SEED): 7 x 7 patches + the class token = 50 positions, ViT-B/32's own sequence length, so the fourth 16-key tile
of the attention holds two real keys and fourteen that must be masked.  A randomly initialised tower is bland (near-uniform
attention, tiny biases), so it is perturbed much as the text fixture is: q / k weights x QK_SCALE = 4, every bias ~ N(0, 0.1), LayerNorm gains
jittered by 0.2, embeddings (class, patch, position) x 10.  (The text fixture's x 8 on q / k makes every softmax row here so peaked that
the fourteen zero-score keys of an unmasked tail carry a probability of 1e-8 and the fault would pass unseen: at x 8 it moves the
outputs by 2.8e-8, at x 4 by the figures below.  Peaked rows are the attention-alone GPU test's business.)
Frames: six of N(0, 1) pixels rounded to multiples of 1 / 32 and clamped to +- 127 / 32, (6, 3, 56, 56), taken as already
CLIP-normalised; stored as int8 `pixels_x32` (pixel = value / 32 exactly), which keeps the file under the 1 MiB a committed file may have.
Stored: the state dict (sd/...), pixels_x32, want = the library's image_embeds with the tower in fp64, ref_fp32_err = max |fp32 library
output - want| on the same frames: the yardstick of the native tower's tolerance (4 x ref_fp32_err, tests/test_gpu_clip_vision.py).

With SEED = 0 and transformers 5.15: ref_fp32_err = 2.20e-6, max |want| = 3.05 (the script prints both), so the bound is 8.8e-6.  Faults
injected into the fp64 restatement (tests/clip_vision_ref.py) move the outputs of EVERY one of the six frames by at least: tail keys of
the last 16-key tile unmasked 2.4e-3, tail mask off by one (key 49 masked too) 3.8e-3, the causal mask left on 1.2, class token behind
the patches 0.68, patch elements in the order [py][px][c] 1.06, no pre-LayerNorm 0.50 -- the smallest is 269 x the bound.  The resize
fault (Keys' a = -0.5 in place of -0.75) is measured on the frame-patch test's own inputs (tests/clip_vision_ref.py make_clips): it
moves the patch rows by 0.30 (16 -> 56), 0.36 (128 -> 224) and 0.34 (37 -> 64) against bounds of 2.6e-5, 2.1e-4 and 6.1e-6, and by
nothing where H = R.  tests/test_clip_vision_host.py asserts the factor of 10 on all of them; if SEED, QK_SCALE or the perturbation
changes, re-measure these figures and update this paragraph.

usage: python tests/golden/make_golden_clip_vision.py"""
import os

import numpy as np
import torch
import transformers

SEED = 0
N_FRAMES = 6
QK_SCALE = 4.0
CFG = dict(hidden_size=128, intermediate_size=128, projection_dim=32, num_hidden_layers=2, num_attention_heads=2, image_size=56,
           patch_size=8, hidden_act="quick_gelu")


def build_tower():
    torch.manual_seed(SEED)
    m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**CFG)).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_proj.weight", "k_proj.weight")):
                p.mul_(QK_SCALE)
            elif ("layer_norm" in name or "layrnorm" in name or "layernorm" in name) and name.endswith(".weight"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "embedding" in name:
                p.mul_(10.0)
    return m


def build_pixels():
    """-> int8 (6, 3, 56, 56): 32 x the pixel values."""
    x = torch.randn((N_FRAMES, 3, CFG["image_size"], CFG["image_size"]), generator=torch.Generator().manual_seed(SEED + 2))
    return torch.round(x * 32).clamp(-127, 127).to(torch.int8)


def main():
    m = build_tower()
    pixels_x32 = build_pixels()
    pixels = pixels_x32.float() / 32
    with torch.no_grad():
        got32 = m(pixel_values=pixels).image_embeds.double()
        want = m.double()(pixel_values=pixels.double()).image_embeds
    m.float()
    err = (got32 - want).abs().max().item()
    out = {"sd/" + k: v.detach().float().numpy() for k, v in m.state_dict().items() if v.is_floating_point()}
    out.update(pixels_x32=pixels_x32.numpy(), want=want.numpy(), ref_fp32_err=np.float64(err), cfg_n_head=np.int64(CFG["num_attention_heads"]),
               cfg_image_size=np.int64(CFG["image_size"]), cfg_patch_size=np.int64(CFG["patch_size"]), cfg_seed=np.int64(SEED))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_vision_small.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, ref_fp32_err {err:.3e}, max |want| {want.abs().max().item():.3f}")


if __name__ == "__main__":
    main()
